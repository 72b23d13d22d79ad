// mcq_api.hip -- host side of libmcq.so: the C ABI declared in include/mcq.h.
//
// The handle owns one HIP stream and the per-batch device workspace ("slabs": band matrices, factor, vectors) on one
// device; it is grown on demand and reused across calls.  One process per GPU creates one handle (bench.py,
// engine.py); a multi-GPU job is N such processes, each solving a contiguous shard of the batch.
#include <hip/hip_runtime.h>

#include <dlfcn.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <thread>
#include <vector>

#include "mcq_kernels.h"

static thread_local std::string g_err;

// A compute stream and the device workspace ("slabs") of the solver launches on it.  The handle has two: [0] serves every entry; [1] is the
// SECOND compute stream -- the step entries (mcq_solve_host_pipelined, mcq_solve_device_stream) run their odd steps on it with its own slabs, the
// sliced entries (mcq_solve_device, mcq_solve_host, mcq_solve_batch) their odd slices over rows of workspace 0: the tail of one launch overlaps the
// start of the next.  What only [0] has stays in the handle: state2 and the warm start, the small Goldfarb-Idnani pool, the event timing.
struct Workspace {
    hipStream_t stream = nullptr;       // [0]: created with the handle; [1]: on first use (ensure_streams)
    double *L = nullptr, *vec = nullptr, *Z = nullptr;
    signed char* state = nullptr;
    double* kbig = nullptr;             // overflow slots of the curvature-row working set (MCQ_KBIG_SLOTS x MCQ_KBIG_SLOT doubles)
    int* slot_flags = nullptr;          // [MCQ_SLOT_FLAGS] = overflow slots | full Goldfarb-Idnani slots | small ones: 0 free / 1 taken, claimed and released by the workgroups (never reset by the host)
    double* gi = nullptr;               // FULL slots of the Goldfarb-Idnani path (mcq_gi.inc): gi_slots x MCQ_GI_SLOT_DOUBLES(gi_nmax, gi_nmax)
    int gi_slots = 0, gi_nmax = 0;      // ([1]: gi_nmax is the ring size the workspace was sized for, with or without slots)
    size_t elems = 0, batch = 0;        // batch * nmax, and the batch, the slabs are sized for
    long long bytes = 0;                // of mcq_workspace_bytes.  [0]: the slabs (its pools are counted in gi_bytes / gis_bytes); [1]: slabs and slots
};

// One set of device buffers a uniform or padded batch is staged in.  The handle has two: [0] serves every host-buffer entry, [1] is the second
// slot of mcq_solve_host_pipelined.
struct Staging {
    double *ref = nullptr, *nv = nullptr, *sc = nullptr, *alpha = nullptr, *curv = nullptr;
    int* status = nullptr;
    size_t elems = 0, batch = 0;
};

// A grow-only device buffer of the handle, reused from call to call (grow(), below HIP_TRY).
struct Scratch {
    void* p = nullptr;
    size_t bytes = 0;
};

// One sliced mcq_solve_device call -- or several over the very same buffers -- whose slices nothing has joined yet: what each slice writes
// (alpha, curv_error, status, info: its own rows), what the call reads (reftrack, normvec, scaling: whole), the end of its latest launch per stream.
struct Range {
    const char *lo = nullptr, *hi = nullptr;        // [lo, hi); empty where the caller passed no such array
    bool meets(const Range& o) const { return lo < o.hi && o.lo < hi; }
    bool operator==(const Range& o) const { return lo == o.lo && hi == o.hi; }
};
struct SliceCall {
    Range wr[2][4], rd[3];
    hipEvent_t end[2] = {nullptr, nullptr};         // created on first use, kept with the slot
};
#define MCQ_SLICE_CALLS 16
// the sliced mcq_solve_device calls whose two streams have not been joined since (solve_device_sliced)
struct Slices {
    SliceCall call[MCQ_SLICE_CALLS];
    int count = 0;
    int batch = 0, n = 0;               // the shape of the calls in call[]: the same split and the same workspace rows per slice
    bool fast_ok = false;               // nothing but sliced calls has been enqueued on the handle since the last full join
    hipEvent_t last1 = nullptr;         // (two names for events of call[], not owned)  end of the latest slice on ws[1].stream; != nullptr: ws[0].stream has not waited for it yet
    hipEvent_t time1 = nullptr;         // != nullptr: the last timed launch was a sliced call, and this is the end of its slice on ws[1].stream
    hipEvent_t join = nullptr;          // fork_second: ws[1].stream behind ws[0].stream
};

// The copies of the host-buffer entries that run beside the kernels: a stream each way, created on first use (ensure_streams)
struct CopyPipe {
    hipStream_t in = nullptr, out = nullptr;
    hipEvent_t up[2] = {}, done[2] = {}, down[2] = {};      // mcq_solve_host_pipelined: one triple per staging slot
    hipEvent_t slice[16] = {};          // mcq_solve_host / mcq_solve_batch in slices: upload [k] / kernel [8 + k] done, per slice
};

struct mcq_handle {
    int device = 0;
    Workspace ws[2];
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};      // launches on ws[0] only, like timing_valid and span_launches
    bool timing_valid = false;
    hipEvent_t ev_back = nullptr;                   // join_second: ws[0].stream behind ws[1].stream
    hipEvent_t ev_span[2] = {nullptr, nullptr};     // mcq_timing_begin / mcq_timing_end: a span of launches on the compute stream
    int span_launches = 0;
    bool span_open = false;
    signed char* state2 = nullptr;     // working sets carried through the IQP glue (warm start of the next pass)
    bool state2_valid = false;
    int state2_batch = 0, state2_nmax = 0;   // the layout mcq_relinearise_device wrote state2 with: a warm start is honoured only for it
    Staging stage[2];
    // what exists once, allocated and freed with stage[0]
    double *d_kb = nullptr, *d_wv = nullptr;
    int* d_n = nullptr;
    mcq_info* d_info = nullptr;
    void* pin = nullptr;                             // pinned host staging (packing of the host-buffer entries)
    size_t pin_bytes = 0;
    bool poison = false;    // MCQ_POISON=1 (debugging aid): every workspace / staging allocation is filled with 0xFF bytes (NaN as a
                            // double), so that a read of memory nothing has written shows up as a wrong result on every box instead of
                            // on the rare one whose recycled memory happens to hold garbage
    bool smem_attr_set = false;
    Scratch vel;                        // profiles of mcq_vel_profile_device*, [2 nmax][batch] (the lap doubled) or [nmax][batch] (unclosed rows)
    Scratch bound;                      // mcq_bound_dists_device: samples [tracks][2][nbmax][2], raw boundaries, running sums, side statuses
    Scratch fit;                        // mcq_spline_fit_device: running sums, closed points, parameters, the per-track work area
    Scratch spl;                        // mcq_spline_approx_device: first guesses, closest parameters, distances, sides [tracks][nmax + 1] each, sample counts
    Scratch ends;                       // per-problem ring / open-chain records of mcq_solve_batch_ends (device)
    Scratch fgen;                       // mcq_points_in_path_device / mcq_friction_gen_device: polygons, kept vertices, contours, their counts
    Scratch fgen_pts;                   // mcq_friction_gen_device: the grid points' flags and the blocks' counts (sized after the boundaries' launch)
    Scratch mintime;                    // mcq_mintime_eval_device: the intervals' times and energies [batch][nmax] each, where the caller takes none
    Scratch mtstep;                     // mcq_mintime_step_device: the factor and the residual vectors (mcq_mintime_step_bytes per problem)
    Scratch iqp;                        // mcq_iqp_device: its bookkeeping per track; mcq_iqp_batch: its trace, buf and rounds as well (iqp_layout)
    Scratch iqp_set;                    // mcq_iqp_batch: the second set of the double buffer, ring and normals (iqp_set_layout)
    mcq_iqp_round_cb iqp_cb = nullptr;  // mcq_iqp_set_round_callback
    void* iqp_cb_user = nullptr;
    void* comm = nullptr;               // ncclComm_t of mcq_comm_init (RCCL, loaded with dlopen)
    int comm_rank = 0, comm_world = 0;
    hipStream_t comm_stream = nullptr;  // the gathers run here: ordered behind the solves by an event, overlapping the NEXT solve
    hipEvent_t comm_ready = nullptr, comm_t0[4] = {nullptr, nullptr, nullptr, nullptr}, comm_done[4] = {nullptr, nullptr, nullptr, nullptr};
    unsigned comm_seq = 0;              // gathers enqueued so far (event ring index)
    long long gi_bytes = 0;             // ws[0]'s full slots
    size_t gi_none_nmax = 0;           // > 0: no full slot could be had for rings of this many waypoints (beyond the byte cap, or hipMalloc said no) -- not tried again
    double* gis = nullptr;              // SMALL slots (MCQ_ALG_GI: one per resident workgroup): gis_slots x MCQ_GI_SLOT_DOUBLES(gis_nmax, gi_small_qcap(gis_nmax))
    int gis_slots = 0, gis_nmax = 0;
    long long gis_bytes = 0;
    double* d_org = nullptr;            // per-track origins of the fp32 row entries, [batch][2]
    CopyPipe cp;
    int last_upload_direct = 0;         // the last host-buffer batch went up without the packing pass (mcq_last_upload_was_direct)
    int cus = 256;                      // compute units of the device (mcq_create); the MI355X's where the runtime does not say
    Slices sl;
    hipEvent_t ev_span1 = nullptr;      // mcq_timing_end: the span's end on ws[1].stream
    bool stream_given = false;          // mcq_stream has handed ws[0].stream out: the caller may enqueue on it what the handle does not see
};

// ws[0].stream BEHIND EVERYTHING the handle has enqueued: the one stream every entry but the sliced mcq_solve_device works on.  A pending slice
// on ws[1].stream is waited for first (on the device; nothing pending: no call at all), and the next sliced call joins both ways before it
// launches, because what the caller of this function enqueues is not in its record.  The step and slice entries, which run on ws[1].stream by
// design, end with it drained or joined (join_second).  Only solve_device_sliced, join_second, the comm stream's waits, mcq_timing_end and
// creation / destruction take the raw streams.
static hipStream_t compute_stream(mcq_handle* h)
{
    if (h->sl.last1) {
        if (hipStreamWaitEvent(h->ws[0].stream, h->sl.last1, 0) != hipSuccess) (void)hipStreamSynchronize(h->ws[1].stream);
        h->sl.last1 = nullptr;
    }
    h->sl.fast_ok = false;
    return h->ws[0].stream;
}

// ---- the one error path of the HIP calls ----------------------------------------------------------------------------------------
// the message callers and tests match on: "<expr> failed: <hip error> (<file>:<line>)"
static int hip_failed(const char* expr, hipError_t e, const char* file, int line)
{
    char buf[512];
    snprintf(buf, sizeof(buf), "%s failed: %s (%s:%d)", expr, hipGetErrorString(e), file, line);
    g_err = buf;
    return MCQ_E_DEVICE;
}

// every stream the handle has created is drained: copies from / into the caller's buffers (or the pinned staging) may still be queued on any of them
static void drain(mcq_handle* h)
{
    for (hipStream_t st : {h->cp.in, h->ws[0].stream, h->ws[1].stream, h->cp.out, h->comm_stream})
        if (st) (void)hipStreamSynchronize(st);
}

// HIP_TRY returns only: the device-resident, asynchronous entries and the allocations, which leave nothing queued on the caller's host memory.
// HIP_TRY_DRAIN(expr), in a function with the handle `h`: the host-buffer entries, whose caller may free or reuse its buffers on return.
#define HIP_TRY(expr)                                                                             \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess) return hip_failed(#expr, e_, __FILE__, __LINE__);                   \
    } while (0)
#define HIP_TRY_DRAIN(expr)                                                                       \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess) { drain(h); return hip_failed(#expr, e_, __FILE__, __LINE__); }     \
    } while (0)

// The streams and events beyond ws[0].stream come into being HERE, on the first call that needs them and in this order (the runtime hands
// out hardware queues at creation; no other order has been measured with the comm stream present).
enum { COPY_STREAMS = 1, SECOND_STREAM = 2, SLICE_EVENTS = 4, STEP_EVENTS = 8 };
static int ensure_streams(mcq_handle* h, int what)
{
    CopyPipe& c = h->cp;
    if ((what & COPY_STREAMS) && !c.in) { HIP_TRY(hipStreamCreate(&c.in)); HIP_TRY(hipStreamCreate(&c.out)); }
    if ((what & SECOND_STREAM) && !h->ws[1].stream) HIP_TRY(hipStreamCreate(&h->ws[1].stream));
    if (what & SLICE_EVENTS) for (hipEvent_t& e : c.slice) if (!e) HIP_TRY(hipEventCreate(&e));
    if ((what & STEP_EVENTS) && !c.up[0]) {
        for (int k = 0; k < 2; ++k) { HIP_TRY(hipEventCreate(&c.up[k])); HIP_TRY(hipEventCreate(&c.done[k])); HIP_TRY(hipEventCreate(&c.down[k])); }
    }
    return 0;
}

// ws[1].stream behind ws[0].stream as it stands now -- and, through compute_stream, ws[0].stream behind the last slice on ws[1].stream
static int fork_second(mcq_handle* h)
{
    if (!h->sl.join) HIP_TRY(hipEventCreate(&h->sl.join));
    HIP_TRY(hipEventRecord(h->sl.join, compute_stream(h)));
    HIP_TRY(hipStreamWaitEvent(h->ws[1].stream, h->sl.join, 0));
    return 0;
}

// ws[0].stream behind ws[1].stream as it stands now: mcq_sync, a later call on the handle or a caller holding mcq_stream() sees both done
static int join_second(mcq_handle* h)
{
    if (!h->ev_back) HIP_TRY(hipEventCreate(&h->ev_back));
    HIP_TRY(hipEventRecord(h->ev_back, h->ws[1].stream));
    HIP_TRY(hipStreamWaitEvent(compute_stream(h), h->ev_back, 0));
    return 0;
}

// s holds at least `bytes` afterwards.  A launch in flight on the handle's stream may still read the old buffer: it is waited for before the free.
// A refused allocation leaves the record empty.
static int grow(mcq_handle* h, Scratch& s, size_t bytes)
{
    if (bytes <= s.bytes) return 0;
    HIP_TRY(hipStreamSynchronize(compute_stream(h)));
    (void)hipFree(s.p);
    s = Scratch();
    HIP_TRY(hipMalloc(&s.p, bytes));
    s.bytes = bytes;
    return 0;
}

// The regions of one Scratch buffer, stated once: a *_layout function below adds them in their order from the shapes alone, the entry grows
// the buffer to `bytes` and takes the pointers with at(), the regions numbered from 0 in the order of the comment above their layout function.
// A region's bytes are rounded up to `pad` (8: a double may follow ints).
struct Arena {
    size_t off[10], align[10], n = 0, bytes = 0;
    template <class T> Arena& add(size_t count, size_t pad = 8)
    {
        off[n] = bytes;
        align[n++] = alignof(T);
        bytes += (count * sizeof(T) + pad - 1) / pad * pad;
        return *this;
    }
    template <class T> T* at(void* base, int region) const { return (T*)((char*)base + off[region]); }
};

extern "C" const char* mcq_last_error(void) { return g_err.c_str(); }

extern "C" void mcq_default_opts(mcq_opts* o)
{
    if (!o) return;
    o->algorithm = MCQ_ALG_DEFAULT;
    o->max_ipm_iter = 60;
    o->max_as_iter = 60;
    o->refine_steps = 2;
    o->check_kappa = 1;
    o->objective = MCQ_OBJ_MIN_CURV;
    o->warm_start = 0;
}

static mcq_opts resolve_opts(const mcq_opts* in)
{
    mcq_opts o;
    mcq_default_opts(&o);
    if (in) {
        o.algorithm = in->algorithm == MCQ_ALG_GI ? MCQ_ALG_GI : MCQ_ALG_DEFAULT;    // (the field was `band_e` until round 4: 0 / 32 mean the default)
        if (in->max_ipm_iter > 0) o.max_ipm_iter = in->max_ipm_iter;
        if (in->max_as_iter > 0) o.max_as_iter = in->max_as_iter;
        if (in->refine_steps >= 0) o.refine_steps = in->refine_steps;
        o.check_kappa = in->check_kappa >= 0 ? 1 : 0;   // 0 (a zero-initialised struct) and 1: carried; < 0: skipped
        o.objective = in->objective == MCQ_OBJ_SHORTEST_PATH ? MCQ_OBJ_SHORTEST_PATH : MCQ_OBJ_MIN_CURV;
        o.warm_start = in->warm_start;
    }
    return o;
}

extern "C" void mcq_destroy(mcq_handle* h);
extern "C" int mcq_comm_destroy(mcq_handle* h);

extern "C" int mcq_create(int device_id, mcq_handle** out)
{
    if (!out) { g_err = "mcq_create: out is NULL"; return MCQ_E_ARG; }
    *out = nullptr;
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device_id < 0 || device_id >= ndev) { g_err = "mcq_create: no such device"; return MCQ_E_DEVICE; }
    HIP_TRY(hipSetDevice(device_id));
    mcq_handle* h = new mcq_handle();
    h->device = device_id;
    {
        const char* e = getenv("MCQ_POISON");
        h->poison = e && e[0] == '1';
    }
#ifdef __HIPCC__        // (the tests' interpreter build -- g++, every stream synchronous -- has no device to ask)
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device_id) == hipSuccess && cus > 0) h->cus = cus;
        else (void)hipGetLastError();
    }
#endif
    hipError_t e = hipStreamCreate(&h->ws[0].stream);
    for (int k = 0; k < 5 && e == hipSuccess; ++k) e = hipEventCreate(&h->ev[k]);
    if (e != hipSuccess) {
        g_err = std::string("mcq_create: ") + hipGetErrorString(e);
        mcq_destroy(h);         // releases whatever was created
        return MCQ_E_DEVICE;
    }
    *out = h;
    return 0;
}

static void free_workspace(mcq_handle* h, int which)
{
    Workspace& w = h->ws[which];
    (void)hipFree(w.L); (void)hipFree(w.vec); (void)hipFree(w.Z); (void)hipFree(w.state); (void)hipFree(w.kbig);
    (void)hipFree(w.slot_flags); (void)hipFree(w.gi);
    const Workspace old = w;
    w = Workspace();
    w.stream = old.stream;
    if (which == 0) {
        w.bytes = old.bytes;            // (kept until the next successful growth, as ever: docs/NOTEBOOK.md, "Host API")
        (void)hipFree(h->state2); (void)hipFree(h->gis);
        h->state2 = nullptr;
        h->gis = nullptr;
        h->gis_slots = h->gis_nmax = 0;
        h->gi_bytes = h->gis_bytes = 0;
        h->state2_valid = false;
    }
}

// stage[0] takes what exists once with it: the per-problem scalars, records and origins
static void free_staging(mcq_handle* h, int which)
{
    Staging& s = h->stage[which];
    (void)hipFree(s.ref); (void)hipFree(s.nv); (void)hipFree(s.sc); (void)hipFree(s.alpha); (void)hipFree(s.curv); (void)hipFree(s.status);
    s = Staging();
    if (which == 0) {
        (void)hipFree(h->d_kb); (void)hipFree(h->d_wv); (void)hipFree(h->d_n); (void)hipFree(h->d_info);
        h->d_kb = h->d_wv = nullptr;
        h->d_n = nullptr;
        h->d_info = nullptr;
        (void)hipFree(h->d_org);
        h->d_org = nullptr;
    }
}

extern "C" void mcq_destroy(mcq_handle* h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->ws[0].stream) (void)hipStreamSynchronize(h->ws[0].stream);
    if (h->cp.in) (void)hipStreamSynchronize(h->cp.in);
    if (h->cp.out) (void)hipStreamSynchronize(h->cp.out);
    (void)mcq_comm_destroy(h);
    if (h->ws[1].stream) (void)hipStreamSynchronize(h->ws[1].stream);
    for (int k = 0; k < 2; ++k) { free_workspace(h, k); free_staging(h, k); }
    if (h->ws[1].stream) (void)hipStreamDestroy(h->ws[1].stream);
    for (hipEvent_t* set : {h->cp.up, h->cp.done, h->cp.down}) for (int k = 0; k < 2; ++k) if (set[k]) (void)hipEventDestroy(set[k]);
    for (hipEvent_t e : h->cp.slice) if (e) (void)hipEventDestroy(e);
    if (h->cp.in) (void)hipStreamDestroy(h->cp.in);
    if (h->cp.out) (void)hipStreamDestroy(h->cp.out);
    for (Scratch* s : {&h->vel, &h->bound, &h->fit, &h->spl, &h->ends, &h->fgen, &h->fgen_pts, &h->mintime, &h->mtstep, &h->iqp, &h->iqp_set}) (void)hipFree(s->p);
    if (h->pin) (void)hipHostFree(h->pin);
    for (int k = 0; k < 5; ++k) if (h->ev[k]) (void)hipEventDestroy(h->ev[k]);
    for (int k = 0; k < 2; ++k) if (h->ev_span[k]) (void)hipEventDestroy(h->ev_span[k]);
    for (SliceCall& c : h->sl.call) for (hipEvent_t e : c.end) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : {h->sl.join, h->ev_back, h->ev_span1}) if (e) (void)hipEventDestroy(e);
    if (h->ws[0].stream) (void)hipStreamDestroy(h->ws[0].stream);
    delete h;
}

// Goldfarb-Idnani slots (mcq_gi.inc).  Two pools:
//   FULL slots  -- a working set holds at most nmax independent constraints: nmax x nmax (Q) + nmax x nmax (R) doubles (64 MB at nmax = 2000).  The
//                  fallback's pool: as many as $MCQ_GI_BYTES (16 GB) hold, at most MCQ_GI_FULL_MAX = 512 (256 at nmax = 2000: a sweep over tight curvature
//                  bounds can send hundreds of problems of one launch down this path), never more than the batch.  A rare path must not cost the
//                  common one its launch: a slot beyond the byte cap (rings above ~32 000 waypoints) or a refused hipMalloc leaves the handle
//                  WITHOUT the pool -- the kernel then returns what its own phases left (MCQ_ITER_CAP, ...), as in round 4; not tried again for
//                  rings that long.
//   SMALL slots -- round 6, mcq_opts.algorithm = MCQ_ALG_GI (every problem takes the path: one slot per resident workgroup): working sets of up to
//                  gi_small_qcap(nmax) = nmax / 8 constraints (rounded up to 64, at least 128), what the path's working sets measure on every workload
//                  here (62 .. 100 active rows at nmax = 2000); 4.6 MB at nmax = 2000, 2.4 GB for 512 of them (round 5: full slots,
//                  33 GB).  A problem that outgrows its small slot moves into a full one in place (gi_grow, mcq_gi.inc).
static size_t gi_small_qcap(size_t nmax)
{
    const size_t q = std::max<size_t>(128, ((nmax / 8 + 63) / 64) * 64);
    return std::min(q, nmax);
}

static size_t gi_byte_cap()
{
    if (const char* e = getenv("MCQ_GI_BYTES")) { const long long v = atoll(e); if (v >= 0) return (size_t)v; }
    return (size_t)16 << 30;       // (288 GB of HBM: round 6 measured the 600-large-ring stress at 75 s with 4 GB of full slots and 44 s with 48 GB)
}

// hipMalloc of `slots` items of `per` bytes, halving the count until the allocation succeeds; returns the count had (0: none)
static int alloc_slots(double** out, int slots, size_t per)
{
    *out = nullptr;
    while (slots >= 1) {
        if (hipMalloc((void**)out, (size_t)slots * per) == hipSuccess) return slots;
        (void)hipGetLastError();        // (an out-of-memory is not sticky, but it stays in the last-error slot)
        *out = nullptr;
        slots /= 2;
    }
    return 0;
}

// the full pool of workspace 0, regrown on its own
static void ensure_gi(mcq_handle* h, size_t batch, size_t nmax)
{
    Workspace& w = h->ws[0];
    if (h->gi_none_nmax && nmax >= h->gi_none_nmax) return;
    const size_t cap_bytes = gi_byte_cap();
    int want = MCQ_GI_FULL_MAX;
    if (const char* e = getenv("MCQ_GI_SLOTS")) want = std::min(std::max(atoi(e), 1), MCQ_GI_FULL_MAX);
    const size_t per = MCQ_GI_SLOT_DOUBLES(nmax, nmax) * sizeof(double);
    int slots = (int)std::min<size_t>((size_t)want, cap_bytes / per);
    slots = (int)std::min<size_t>((size_t)slots, std::max<size_t>(batch, 1));
    if (w.gi && (size_t)w.gi_nmax >= nmax && w.gi_slots >= slots) return;
    nmax = std::max(nmax, (size_t)w.gi_nmax);
    const size_t per2 = MCQ_GI_SLOT_DOUBLES(nmax, nmax) * sizeof(double);
    slots = std::max(slots, w.gi_slots);
    slots = (int)std::min<size_t>((size_t)slots, cap_bytes / per2);
    (void)hipStreamSynchronize(compute_stream(h));
    (void)hipFree(w.gi);
    w.gi = nullptr;
    w.gi_slots = w.gi_nmax = 0;
    h->gi_bytes = 0;
    slots = alloc_slots(&w.gi, slots, per2);
    if (slots < 1) { h->gi_none_nmax = nmax; return; }
    if (h->poison) (void)hipMemsetAsync(w.gi, 0xff, (size_t)slots * per2, compute_stream(h));
    w.gi_slots = slots;
    w.gi_nmax = (int)nmax;
    h->gi_bytes = (long long)((size_t)slots * per2);
}

// the small pool of MCQ_ALG_GI; an error only if the handle ends up with no slot of either kind (the caller asked for this path by name)
static int ensure_gi_small(mcq_handle* h, size_t batch, size_t nmax)
{
    int slots = (int)std::min<size_t>(std::max<size_t>(batch, 1), MCQ_GI_SLOTS_MAX);
    if (!(h->gis && (size_t)h->gis_nmax >= nmax && h->gis_slots >= slots)) {
        nmax = std::max(nmax, (size_t)h->gis_nmax);
        slots = std::max(slots, h->gis_slots);
        const size_t per = MCQ_GI_SLOT_DOUBLES(nmax, gi_small_qcap(nmax)) * sizeof(double);
        const size_t cap_bytes = std::max(gi_byte_cap(), (size_t)8 << 30);
        slots = (int)std::min<size_t>((size_t)slots, cap_bytes / per);
        (void)hipStreamSynchronize(compute_stream(h));
        (void)hipFree(h->gis);
        h->gis = nullptr;
        h->gis_slots = h->gis_nmax = 0;
        h->gis_bytes = 0;
        slots = alloc_slots(&h->gis, slots, per);
        if (slots >= 1) {
            if (h->poison) (void)hipMemsetAsync(h->gis, 0xff, (size_t)slots * per, compute_stream(h));
            h->gis_slots = slots;
            h->gis_nmax = (int)nmax;
            h->gis_bytes = (long long)((size_t)slots * per);
        }
    }
    if (!h->gis && !h->ws[0].gi) { g_err = "MCQ_ALG_GI: no device memory for a Goldfarb-Idnani slot at this ring size"; return MCQ_E_DEVICE; }
    return 0;
}

// Workspace `which`, grown to batch x nmax.  The two differ in what the handle keeps once: workspace 0 carries state2 (two state bytes per
// element in its byte count against one) and regrows its full Goldfarb-Idnani pool on its own, counted apart (ensure_gi); workspace 1 -- the
// second compute stream, created here -- takes half of workspace 0's full slots when it is sized, counted with its slabs, and is sized anew
// for longer rings than those slots hold.
static int ensure_workspace(mcq_handle* h, int which, size_t batch, size_t nmax)
{
    Workspace& w = h->ws[which];
    if (int rc = ensure_streams(h, which == 1 ? SECOND_STREAM : 0)) return rc;
    const size_t elems = batch * nmax;
    if (elems <= w.elems && batch <= w.batch && (which == 0 || (size_t)w.gi_nmax >= nmax)) {
        if (which == 0) ensure_gi(h, batch, nmax);
        return 0;
    }
    HIP_TRY(hipStreamSynchronize(which == 0 ? compute_stream(h) : w.stream));
    free_workspace(h, which);
    const size_t l_bytes = elems * MCQ_LLD * sizeof(double), vec_bytes = elems * MCQ_NVEC * sizeof(double),
                 z_bytes = (elems + batch * (size_t)MCQ_KMAX * MCQ_KMAX) * sizeof(double),
                 kbig_bytes = (size_t)MCQ_KBIG_SLOTS * MCQ_KBIG_SLOT * sizeof(double);
    HIP_TRY(hipMalloc((void**)&w.L, l_bytes));
    HIP_TRY(hipMalloc((void**)&w.vec, vec_bytes));
    HIP_TRY(hipMalloc((void**)&w.Z, z_bytes));
    HIP_TRY(hipMalloc((void**)&w.state, elems));
    if (which == 0) HIP_TRY(hipMalloc((void**)&h->state2, elems));
    HIP_TRY(hipMalloc((void**)&w.kbig, kbig_bytes));
    HIP_TRY(hipMalloc((void**)&w.slot_flags, MCQ_SLOT_FLAGS * sizeof(int)));
    HIP_TRY(hipMemsetAsync(w.slot_flags, 0, MCQ_SLOT_FLAGS * sizeof(int), w.stream));
    size_t slot_bytes = 0;
    if (which == 0) ensure_gi(h, batch, nmax);
    else {
        // half the first workspace's full slots (none where it has none: the kernel then returns what its own phases left)
        const Workspace& w0 = h->ws[0];
        const size_t per = MCQ_GI_SLOT_DOUBLES(nmax, nmax) * sizeof(double);
        const int slots = w0.gi && (size_t)w0.gi_nmax >= nmax ? alloc_slots(&w.gi, std::max(1, w0.gi_slots / 2), per) : 0;
        slot_bytes = (size_t)slots * per;
        if (h->poison && w.gi) HIP_TRY(hipMemsetAsync(w.gi, 0xff, slot_bytes, w.stream));
        w.gi_slots = slots;
        w.gi_nmax = (int)nmax;
    }
    HIP_TRY(hipMemsetAsync(w.state, 0, elems, w.stream));
    if (which == 0) HIP_TRY(hipMemsetAsync(h->state2, 0, elems, w.stream));
    if (h->poison) {
        HIP_TRY(hipMemsetAsync(w.L, 0xff, l_bytes, w.stream));
        HIP_TRY(hipMemsetAsync(w.vec, 0xff, vec_bytes, w.stream));
        HIP_TRY(hipMemsetAsync(w.Z, 0xff, z_bytes, w.stream));
        HIP_TRY(hipMemsetAsync(w.kbig, 0xff, kbig_bytes, w.stream));
    }
    w.elems = elems;
    w.batch = batch;
    w.bytes = (long long)(elems * ((MCQ_LLD + MCQ_NVEC + 1) * sizeof(double) + (which == 0 ? 2 : 1)) +
                          batch * (size_t)MCQ_KMAX * MCQ_KMAX * sizeof(double) + kbig_bytes + slot_bytes);
    return 0;
}

// Staging set `which`, grown to batch x nmax.  What exists once -- the per-problem scalars, records and origins -- comes and goes with set 0,
// which is also the only one MCQ_POISON fills.
static int ensure_staging(mcq_handle* h, int which, size_t batch, size_t nmax)
{
    Staging& s = h->stage[which];
    const size_t elems = batch * nmax;
    if (elems <= s.elems && batch <= s.batch) return 0;
    HIP_TRY(hipStreamSynchronize(compute_stream(h)));
    if (which == 1) {       // (the pipeline's copy streams: its entry has created them)
        HIP_TRY(hipStreamSynchronize(h->cp.in));
        HIP_TRY(hipStreamSynchronize(h->cp.out));
    }
    free_staging(h, which);
    HIP_TRY(hipMalloc((void**)&s.ref, elems * 4 * sizeof(double)));
    HIP_TRY(hipMalloc((void**)&s.nv, elems * 2 * sizeof(double)));
    HIP_TRY(hipMalloc((void**)&s.sc, elems * sizeof(double)));
    HIP_TRY(hipMalloc((void**)&s.alpha, elems * sizeof(double)));
    HIP_TRY(hipMalloc((void**)&s.curv, batch * sizeof(double)));
    HIP_TRY(hipMalloc((void**)&s.status, batch * sizeof(int)));
    if (which == 0) {
        HIP_TRY(hipMalloc((void**)&h->d_kb, batch * sizeof(double)));
        HIP_TRY(hipMalloc((void**)&h->d_wv, batch * sizeof(double)));
        HIP_TRY(hipMalloc((void**)&h->d_n, batch * sizeof(int)));
        HIP_TRY(hipMalloc((void**)&h->d_info, batch * sizeof(mcq_info)));
        HIP_TRY(hipMalloc((void**)&h->d_org, batch * 2 * sizeof(double)));
        if (h->poison) {
            HIP_TRY(hipMemsetAsync(s.ref, 0xff, elems * 4 * sizeof(double), compute_stream(h)));
            HIP_TRY(hipMemsetAsync(s.nv, 0xff, elems * 2 * sizeof(double), compute_stream(h)));
            HIP_TRY(hipMemsetAsync(s.sc, 0xff, elems * sizeof(double), compute_stream(h)));
            HIP_TRY(hipMemsetAsync(s.alpha, 0xff, elems * sizeof(double), compute_stream(h)));
        }
    }
    s.elems = elems;
    s.batch = batch;
    return 0;
}

// a uniform (n_list == nullptr) or ragged batch over these rows and result arrays; everything else of McqBatch is zero: an entry sets what is
// special to it, fill_batch the workspace, options and slots
static McqBatch make_batch(int batch, int nmax, const int* n_list, const double* ref, const double* nv, const double* sc, double* alpha,
                           double* curv_err, int* status, mcq_info* info, double kappa_bound, double w_veh)
{
    McqBatch B;
    memset(&B, 0, sizeof(B));
    B.batch = batch;
    B.n = nmax;
    B.nmax = nmax;
    B.n_list = n_list;
    B.ref = ref;
    B.nv = nv;
    B.sc = sc;
    B.alpha = alpha;
    B.curv_err = curv_err;
    B.status = status;
    B.info = info;
    B.kappa_bound = kappa_bound;
    B.w_veh = w_veh;
    return B;
}

// workspace, options and slots of a solver launch (everything of McqBatch the caller does not set)
static int fill_batch(mcq_handle* h, McqBatch& B, const mcq_opts& o, Workspace& w)
{
    B.L = w.L; B.vec = w.vec; B.Z = w.Z; B.state = w.state;
    B.max_ipm_iter = o.max_ipm_iter;
    B.max_as_iter = o.max_as_iter;
    B.refine_steps = o.refine_steps;
    B.check_kappa = o.check_kappa;
    B.objective = o.objective;
    B.poison_lds = h->poison ? 1 : 0;
    B.kbig = w.kbig;
    B.slot_flags = w.slot_flags;      // (zero between launches: the workgroups release what they claim)
    B.kbig_slots = MCQ_KBIG_SLOTS;
    B.algorithm = o.algorithm;
    // the Goldfarb-Idnani slots hold working sets of up to gi_nmax constraints on rings of up to gi_nmax waypoints (slot stride: B.nmax)
    const bool gi_path = o.objective == MCQ_OBJ_MIN_CURV && !B.prep_only;
    B.gis = nullptr;
    B.gis_slots = B.gis_qcap = 0;
    if (&w == &h->ws[0] && o.algorithm == MCQ_ALG_GI && gi_path) {
        // every problem takes the Goldfarb-Idnani path: a (small) slot per resident workgroup, so that they run side by side
        if (int rc = ensure_gi_small(h, (size_t)B.batch, (size_t)B.nmax)) return rc;
        if (h->gis && B.nmax <= h->gis_nmax) {
            B.gis = h->gis;
            B.gis_slots = h->gis_slots;
            B.gis_qcap = (int)gi_small_qcap((size_t)B.nmax);
        }
    }
    const bool gi_on = w.gi && w.gi_slots > 0 && B.nmax <= w.gi_nmax && gi_path;
    B.gi = gi_on ? w.gi : nullptr;
    B.gi_slots = gi_on ? w.gi_slots : 0;
    B.gi_qcap = B.nmax;
    // The overflow slots of the curvature-row working set (rounds 3-4) serve only where no Goldfarb-Idnani slot exists: which of more than eight
    // such problems of a launch got one depended on the order the GPU scheduled workgroups in, and so did the last bits of their results
    // (ADVICE r5).  With a Goldfarb-Idnani pool every working set beyond MCQ_KMAX rows takes THAT path -- one route per problem, whatever else
    // is in the launch.
    if (B.gi || B.gis) B.kbig_slots = 0;
    return 0;
}

// ---- every solve: prepare, enqueue_solve, note_solve.  The warm start, the event timing and the launch count of a span
// are workspace 0's: a launch on workspace 1 (mcq_solve_host_pipelined's and mcq_solve_device_stream's odd steps) neither reads nor touches them.
// A warm start applies only with the working sets mcq_relinearise_device carried over for exactly this batch layout.
static bool warm_applies(const mcq_handle* h, const mcq_opts& o, int batch, int nmax)
{
    return o.warm_start > 0 && h->state2_valid && h->state2_batch == batch && h->state2_nmax == nmax;
}

static bool shortest_path(const McqBatch& B) { return B.objective == MCQ_OBJ_SHORTEST_PATH && !B.prep_only; }

// B ready for enqueue_solve on workspace w: fill_batch, the warm start (workspace 0's, spent by the solve that may take it), the shortest
// path's conditions
static int prepare(mcq_handle* h, McqBatch& B, const mcq_opts& o, Workspace& w)
{
    const bool first = &w == &h->ws[0];
    if (int rc = fill_batch(h, B, o, w)) return rc;
    B.warm = first && !B.prep_only && warm_applies(h, o, B.batch, B.nmax) ? h->state2 : nullptr;
    if (!B.prep_only && first) h->state2_valid = false;
    if (shortest_path(B) && !B.nv) { g_err = "shortest-path objective: normvec is required"; return MCQ_E_ARG; }
    if (shortest_path(B)) B.check_kappa = 0;
    return 0;
}

// THE enqueue of the solver's kernels: problems [b0, b1) of the prepared B on `st`, between the events of mcq_last_timing where `timed`.  The
// shortest path's assembly and prep_only are launches over the whole batch: such a B goes in one piece.
static int enqueue_solve(mcq_handle* h, const McqBatch& B, hipStream_t st, int b0, int b1, bool timed)
{
    if (b1 == b0) return 0;            // (an empty slice; a grid of 0 workgroups is a launch error)
    if (timed) HIP_TRY(hipEventRecord(h->ev[0], st));
    if (B.prep_only) {
        hipLaunchKernelGGL(mcq_assemble_kernel, dim3(B.batch), dim3(256), 0, st, B);
        HIP_TRY(hipGetLastError());
        return 0;
    }
    // (minimum curvature has no assembly launch: the solver kernel assembles its problem itself -- assemble_problem() -- since round 4)
    if (shortest_path(B)) {
        hipLaunchKernelGGL(mcq_assemble_sp_kernel, dim3(B.batch), dim3(256), 0, st, B);
        HIP_TRY(hipGetLastError());
    }
    if (timed) HIP_TRY(hipEventRecord(h->ev[1], st));
    if (timed) HIP_TRY(hipEventRecord(h->ev[2], st));
    McqBatch S = B;
    S.pb0 = b0;
    hipLaunchKernelGGL(mcq_solve_kernel, dim3(b1 - b0), dim3(256), 0, st, S);
    HIP_TRY(hipGetLastError());
    if (timed) HIP_TRY(hipEventRecord(h->ev[3], st));
    if (timed) HIP_TRY(hipEventRecord(h->ev[4], st));
    return 0;
}

// What a solve leaves for mcq_last_timing and an open span: once per launch on workspace 0 and once per sliced call, whatever its route.
// timed: ev[0..4] lie around it; end1: a sliced mcq_solve_device's end on ws[1].stream, which the timing runs to where it is the later one.
static void note_solve(mcq_handle* h, const McqBatch& B, bool timed, hipEvent_t end1)
{
    h->timing_valid = timed;
    h->sl.time1 = end1;
    if (h->span_open && !shortest_path(B)) ++h->span_launches;  // (a shortest-path launch has never been counted: docs/NOTEBOOK.md, "Host API")
}

static int launch(mcq_handle* h, McqBatch& B, const mcq_opts& o, Workspace& w)
{
    const bool first = &w == &h->ws[0];
    hipStream_t st = first ? compute_stream(h) : w.stream;
    if (int rc = prepare(h, B, o, w)) return rc;
    if (int rc = enqueue_solve(h, B, st, 0, B.batch, first)) return rc;
    if (first && !B.prep_only) note_solve(h, B, true, nullptr);
    return 0;
}
static int launch(mcq_handle* h, McqBatch& B, const mcq_opts& o) { return launch(h, B, o, h->ws[0]); }

// ---- mcq_solve_device in TWO SLICES, ordered slice by slice -----------------------------------------------------------------------------
// A launch of more workgroups than the device holds at once ends with its slowest slot: 1024 problems on 512 slots take ~10.3 ms for ~9.4 ms of
// mean load, and the next call's launch, in the same stream, may not start in between (docs/NOTEBOOK.md R6.3).  So problems [0, b) go as one
// launch on ws[0].stream and [b, batch) as one on ws[1].stream, both over their own rows of workspace 0 (McqBatch.pb0, as mcq_solve_host's
// slices), and a LATER call's slice j is ordered behind this call's slice j only -- by stream order: while the stragglers of one launch finish,
// the other stream's launch fills the slots they have left.  Results are bitwise those of the one launch: the problems are independent.
//
// What keeps this correct is the record h->sl.call[] of the sliced calls since the last FULL JOIN (each stream waits for the other's last event).
// A call may skip the join only if it has the record's shape -- the same split, the same workspace rows per slice -- and, by interval checks
// on addresses, touches nothing the OTHER stream of a recorded call may still be working on (slice_conflict).  Everything else joins first,
// which is always correct and merely forfeits the overlap: another shape, an overlap, a full record, anything enqueued through compute_stream()
// in between.  Calls over the very same buffers share one entry (the later call's events stand for both, by stream order), so a loop over one
// set of buffers, or over two in turn, never fills the record; entries whose launches have ended make room when a new one is needed.
// THE routing rule (DESIGN.md section 7 has the table and the reasons): the slices a solve of this shape gets from an entry of this kind;
// 1 = the one launch.  Shared conditions first, then the kind's threshold and knobs.
enum EntryKind { ENTRY_DEVICE, ENTRY_HOST };
static int slices_for(const mcq_handle* h, EntryKind kind, int batch, int nmax, const mcq_opts& o)
{
    if (o.objective != MCQ_OBJ_MIN_CURV || o.algorithm == MCQ_ALG_GI || warm_applies(h, o, batch, nmax)) return 1;
    if (kind == ENTRY_DEVICE) {
        // More than one residency round (two workgroups per CU): a batch the device holds at once has no tail to fill, and an isolated call of
        // exactly 512 problems on 256 CUs takes 5.79 ms as two launches of 256 against 5.46 ms as one (docs/NOTEBOOK.md)
        int slice_min = 2 * h->cus + 1;
        if (const char* e = getenv("MCQ_DEVICE_SLICE_MIN")) slice_min = std::max(atoi(e), 2);      // (the tests slice batches of two to eight)
        // two slices, split (batch + 1) / 2; not on a handle whose stream the caller holds (mcq_stream).  $MCQ_DEVICE_ONE_LAUNCH=1: the A/B knob
        const char* one = getenv("MCQ_DEVICE_ONE_LAUNCH");
        return batch < slice_min || h->stream_given || (one && one[0] == '1') ? 1 : 2;
    }
    int slice_min = 512;           // ($MCQ_HOST_SLICE_MIN: the tests slice a batch of eleven)
    if (const char* e = getenv("MCQ_HOST_SLICE_MIN")) slice_min = std::max(atoi(e), 4);
    int nsl = 2;                   // (one per compute stream; more make a heavy-tailed batch wait slice by slice: docs/NOTEBOOK.md R6.5)
    if (const char* e = getenv("MCQ_HOST_SLICES")) nsl = std::min(std::max(atoi(e), 2), 8);
    nsl = std::min(nsl, batch);        // (a slice per problem at most: eight slices of a batch of four to seven had empty ones)
    return nsl > 1 && batch >= slice_min && !getenv("MCQ_HOST_ONE_LAUNCH") ? nsl : 1;          // ($MCQ_HOST_ONE_LAUNCH: the A/B knob)
}
// the host entries' split: slice or chunk k of `parts` begins at this problem
static int split_at(int batch, int k, int parts) { return (int)((long long)batch * k / parts); }

static Range rows_of(const void* p, size_t r0, size_t r1, size_t row_bytes)
{
    Range r;
    if (p) { r.lo = (const char*)p + r0 * row_bytes; r.hi = (const char*)p + r1 * row_bytes; }
    return r;
}

// what the two slices [0, b) and [b, batch) of B write, and what the call reads
static void slice_ranges(const McqBatch& B, int b, SliceCall& c)
{
    const size_t n = (size_t)B.nmax, bt = (size_t)B.batch;
    for (int j = 0; j < 2; ++j) {
        const size_t r0 = j ? (size_t)b : 0, r1 = j ? bt : (size_t)b;
        c.wr[j][0] = rows_of(B.alpha, r0, r1, n * sizeof(double));
        c.wr[j][1] = rows_of(B.curv_err, r0, r1, sizeof(double));
        c.wr[j][2] = rows_of(B.status, r0, r1, sizeof(int));
        c.wr[j][3] = rows_of(B.info, r0, r1, sizeof(mcq_info));
    }
    c.rd[0] = rows_of(B.ref, 0, bt, n * 4 * sizeof(double));
    c.rd[1] = rows_of(B.nv, 0, bt, n * 2 * sizeof(double));
    c.rd[2] = rows_of(B.sc, 0, bt, n * sizeof(double));
}

// May slice j of the new call `c` run while slice 1 - j of the recorded call `old` does?  Not if it writes what that one writes, and -- the
// reads are kept whole, not per slice -- not if either call reads what the other writes.  (Slice j behind `old`'s slice j: stream order.)
static bool slice_conflict(const SliceCall& c, const SliceCall& old)
{
    for (int j = 0; j < 2; ++j)
        for (const Range& w : c.wr[j]) {
            for (const Range& ow : old.wr[1 - j]) if (w.meets(ow)) return true;
            for (const Range& r : old.rd) if (w.meets(r)) return true;
        }
    for (const Range& r : c.rd)
        for (int j = 0; j < 2; ++j)
            for (const Range& ow : old.wr[j]) if (r.meets(ow)) return true;
    return false;
}

static bool same_buffers(const SliceCall& a, const SliceCall& b)
{
    for (int j = 0; j < 2; ++j) for (int k = 0; k < 4; ++k) if (!(a.wr[j][k] == b.wr[j][k])) return false;
    for (int k = 0; k < 3; ++k) if (!(a.rd[k] == b.rd[k])) return false;
    return true;
}

// (the tests' interpreter build has no hipEventQuery; its streams are synchronous: whatever was enqueued has ended)
static bool event_done(hipEvent_t e)
{
#ifdef __HIPCC__
    const hipError_t q = hipEventQuery(e);
    if (q != hipSuccess) (void)hipGetLastError();       // (hipErrorNotReady is no error of the handle's)
    return q == hipSuccess;
#else
    (void)e;
    return true;
#endif
}

static int solve_device_sliced(mcq_handle* h, McqBatch& B, const mcq_opts& o)
{
    if (int rc = ensure_streams(h, SECOND_STREAM)) return rc;
    if (int rc = prepare(h, B, o, h->ws[0])) return rc;
    const int b = (B.batch + 1) / 2;
    SliceCall c;
    slice_ranges(B, b, c);
    bool join = !h->sl.fast_ok || B.batch != h->sl.batch || B.nmax != h->sl.n;
    for (int k = 0; k < h->sl.count && !join; ++k) join = slice_conflict(c, h->sl.call[k]);
    int slot = -1;
    for (int k = 0; k < h->sl.count && !join && slot < 0; ++k) if (same_buffers(c, h->sl.call[k])) slot = k;
    if (!join && slot < 0 && h->sl.count == MCQ_SLICE_CALLS) {
        // room: the entries whose launches have ended on both streams go (their events stay with their slots)
        int kept = 0;
        for (int k = 0; k < h->sl.count; ++k)
            if (!(event_done(h->sl.call[k].end[0]) && event_done(h->sl.call[k].end[1]))) std::swap(h->sl.call[kept++], h->sl.call[k]);
        h->sl.count = kept;
        join = kept == MCQ_SLICE_CALLS;
    }
    hipStream_t s0 = h->ws[0].stream, s1 = h->ws[1].stream;
    if (join) {
        // the full join: ws[0].stream behind the last slice on ws[1].stream, ws[1].stream behind ws[0].stream as it is now
        if (int rc = fork_second(h)) return rc;
        h->sl.count = 0;
        h->sl.batch = B.batch;
        h->sl.n = B.nmax;
        h->sl.fast_ok = true;
    }
    if (slot < 0 || join) slot = h->sl.count++;
    SliceCall& e = h->sl.call[slot];
    for (int j = 0; j < 2; ++j) if (!e.end[j]) HIP_TRY(hipEventCreate(&e.end[j]));
    c.end[0] = e.end[0];
    c.end[1] = e.end[1];
    e = c;
    if (getenv("MCQ_DEVICE_SLICE_TRACE")) fprintf(stderr, "mcq_solve_device: two slices, %s, %d in the record\n", join ? "joined" : "overlapped", h->sl.count);
    // slice 0 carries the event timing of a launch: mcq_last_timing reads slice 1's end next to it
    if (int rc = enqueue_solve(h, B, s0, 0, b, true)) return rc;
    HIP_TRY(hipEventRecord(e.end[0], s0));
    if (int rc = enqueue_solve(h, B, s1, b, B.batch, false)) return rc;
    HIP_TRY(hipEventRecord(e.end[1], s1));
    h->sl.last1 = e.end[1];
    note_solve(h, B, true, e.end[1]);           // one per CALL: span / launches stays the average device time per step
    return 0;
}

extern "C" int mcq_solve_device(mcq_handle* h, int batch, int n, const double* reftrack, const double* normvec,
                                const double* scaling, double kappa_bound, double w_veh, const mcq_opts* opts,
                                double* alpha_out, double* curv_err_out, int* status_out, mcq_info* info_out)
{
    if (!h || batch <= 0 || n <= 0 || !reftrack || !alpha_out || !curv_err_out || !status_out) {
        g_err = "mcq_solve_device: bad argument";
        return MCQ_E_ARG;
    }
    HIP_TRY(hipSetDevice(h->device));
    const mcq_opts o = resolve_opts(opts);
    int rc = ensure_workspace(h, 0, (size_t)batch, (size_t)n);
    if (rc) return rc;
    McqBatch B = make_batch(batch, n, nullptr, reftrack, normvec, scaling, alpha_out, curv_err_out, status_out, info_out, kappa_bound, w_veh);
    if (slices_for(h, ENTRY_DEVICE, batch, n, o) == 1) {
        if (getenv("MCQ_DEVICE_SLICE_TRACE")) fprintf(stderr, "mcq_solve_device: one launch\n");
        return launch(h, B, o);
    }
    return solve_device_sliced(h, B, o);
}

// grid of the streaming conversions: four values per work-item, 4096 workgroups at most
static dim3 convert_grid(size_t count)
{
    const size_t blocks = (count / 4 + 255) / 256;
    return dim3((unsigned)(blocks < 4096 ? blocks + 1 : 4096));
}

static int widen_launch(mcq_handle* h, const float* src, double* dst, size_t count)
{
    hipLaunchKernelGGL(mcq_widen_kernel, convert_grid(count), dim3(256), 0, compute_stream(h), src, dst, count);
    HIP_TRY(hipGetLastError());
    return 0;
}

static int narrow_launch(mcq_handle* h, const double* src, float* dst, size_t count)
{
    hipLaunchKernelGGL(mcq_narrow_kernel, convert_grid(count), dim3(256), 0, compute_stream(h), src, dst, count);
    HIP_TRY(hipGetLastError());
    return 0;
}

// fp32 at the boundary, fp64 inside (BASELINE config 5): the float rows are widened into the handle's staging buffers, the
// fp64 engine runs unchanged, alpha is narrowed on the way out.  The conversions stream 28 + 12 bytes per waypoint next
// to the ~93 KB per waypoint the solver moves: not measurable.
extern "C" int mcq_solve_device_f32(mcq_handle* h, int batch, int n, const float* reftrack, const float* normvec,
                                    const float* scaling, double kappa_bound, double w_veh, const mcq_opts* opts,
                                    float* alpha_out, double* curv_err_out, int* status_out, mcq_info* info_out)
{
    if (!h || batch <= 0 || n <= 0 || !reftrack || !alpha_out || !curv_err_out || !status_out) {
        g_err = "mcq_solve_device_f32: bad argument";
        return MCQ_E_ARG;
    }
    HIP_TRY(hipSetDevice(h->device));
    const mcq_opts o = resolve_opts(opts);
    int rc = ensure_workspace(h, 0, (size_t)batch, (size_t)n);
    if (rc) return rc;
    rc = ensure_staging(h, 0, (size_t)batch, (size_t)n);
    if (rc) return rc;
    const size_t elems = (size_t)batch * n;
    const Staging& s = h->stage[0];
    rc = widen_launch(h, reftrack, s.ref, elems * 4);
    if (rc) return rc;
    if (normvec) { rc = widen_launch(h, normvec, s.nv, elems * 2); if (rc) return rc; }
    if (scaling) { rc = widen_launch(h, scaling, s.sc, elems); if (rc) return rc; }
    McqBatch B = make_batch(batch, n, nullptr, s.ref, normvec ? s.nv : nullptr, scaling ? s.sc : nullptr, s.alpha, curv_err_out, status_out, info_out,
                            kappa_bound, w_veh);
    rc = launch(h, B, o);
    if (rc) return rc;
    return narrow_launch(h, s.alpha, alpha_out, elems);
}

// one wave per track (mcq_widen_rows_kernel): fp64 rows [x, y, w_r, w_l] from float rows in either layout
static int widen_rows_launch(mcq_handle* h, int batch, int n, int layout, const float* d_rows, const double* d_origin, double* d_out)
{
    hipLaunchKernelGGL(mcq_widen_rows_kernel, dim3((unsigned)batch), dim3(64), 0, compute_stream(h), d_rows, d_origin, d_out, n, layout);
    HIP_TRY(hipGetLastError());
    return 0;
}

// fp32 rows in either layout (include/mcq.h: MCQ_F32_ABSOLUTE / MCQ_F32_INCREMENTS), device-resident: the rows are rebuilt as fp64
// [x, y, w_r, w_l] in the handle's staging buffer (mcq_widen_rows_kernel: running sums in fp64, closure defect spread over the
// ring), normals and scalings are derived on the device, alpha is narrowed on the way out.
static int solve_f32_rows(mcq_handle* h, int batch, int n, int layout, const float* d_rows, const double* d_origin, double kappa_bound,
                          double w_veh, const mcq_opts& o, float* d_alpha_out, double* curv_err_out, int* status_out, mcq_info* info_out)
{
    const size_t elems = (size_t)batch * n;
    int rc = widen_rows_launch(h, batch, n, layout, d_rows, d_origin, h->stage[0].ref);
    if (rc) return rc;
    McqBatch B = make_batch(batch, n, nullptr, h->stage[0].ref, nullptr, nullptr, h->stage[0].alpha, curv_err_out, status_out, info_out, kappa_bound, w_veh);
    rc = launch(h, B, o);
    if (rc) return rc;
    return narrow_launch(h, h->stage[0].alpha, d_alpha_out, elems);
}

extern "C" int mcq_solve_device_f32_rows(mcq_handle* h, int batch, int n, int layout, const float* reftrack, const double* origin,
                                         double kappa_bound, double w_veh, const mcq_opts* opts, float* alpha_out,
                                         double* curv_err_out, int* status_out, mcq_info* info_out)
{
    if (!h || batch <= 0 || n <= 0 || !reftrack || !alpha_out || !curv_err_out || !status_out ||
        (layout != MCQ_F32_ABSOLUTE && layout != MCQ_F32_INCREMENTS)) {
        g_err = "mcq_solve_device_f32_rows: bad argument";
        return MCQ_E_ARG;
    }
    HIP_TRY(hipSetDevice(h->device));
    const mcq_opts o = resolve_opts(opts);
    int rc = ensure_workspace(h, 0, (size_t)batch, (size_t)n);
    if (rc) return rc;
    rc = ensure_staging(h, 0, (size_t)batch, (size_t)n);
    if (rc) return rc;
    return solve_f32_rows(h, batch, n, layout, reftrack, origin, kappa_bound, w_veh, o, alpha_out, curv_err_out, status_out, info_out);
}

// The pieces of the fp32 boundary on their own (include/mcq.h): the launches of the entries above through the same helpers.
extern "C" int mcq_f32_rows_device(mcq_handle* h, int batch, int n, int layout, const float* reftrack, const double* origin, double* reftrack_out)
{
    if (!h || batch <= 0 || n <= 0 || !reftrack || !reftrack_out || (layout != MCQ_F32_ABSOLUTE && layout != MCQ_F32_INCREMENTS)) {
        g_err = "mcq_f32_rows_device: bad argument";
        return MCQ_E_ARG;
    }
    HIP_TRY(hipSetDevice(h->device));
    return widen_rows_launch(h, batch, n, layout, reftrack, origin, reftrack_out);
}

extern "C" int mcq_f32_widen_device(mcq_handle* h, size_t count, const float* src, double* dst)
{
    if (!h || count == 0 || !src || !dst) {
        g_err = "mcq_f32_widen_device: bad argument";
        return MCQ_E_ARG;
    }
    HIP_TRY(hipSetDevice(h->device));
    return widen_launch(h, src, dst, count);
}

extern "C" int mcq_f32_narrow_device(mcq_handle* h, size_t count, const double* src, float* dst)
{
    if (!h || count == 0 || !src || !dst) {
        g_err = "mcq_f32_narrow_device: bad argument";
        return MCQ_E_ARG;
    }
    HIP_TRY(hipSetDevice(h->device));
    return narrow_launch(h, src, dst, count);
}

extern "C" int mcq_solve_device_ragged(mcq_handle* h, int batch, int nmax, const int* n_list, const double* reftrack,
                                       const double* normvec, const double* scaling, double kappa_bound, double w_veh,
                                       const mcq_opts* opts, double* alpha_out, double* curv_err_out, int* status_out,
                                       mcq_info* info_out)
{
    if (!h || batch <= 0 || nmax <= 0 || !n_list || !reftrack || !alpha_out || !curv_err_out || !status_out) {
        g_err = "mcq_solve_device_ragged: bad argument";
        return MCQ_E_ARG;
    }
    HIP_TRY(hipSetDevice(h->device));
    const mcq_opts o = resolve_opts(opts);
    int rc = ensure_workspace(h, 0, (size_t)batch, (size_t)nmax);
    if (rc) return rc;
    McqBatch B = make_batch(batch, nmax, n_list, reftrack, normvec, scaling, alpha_out, curv_err_out, status_out, info_out, kappa_bound, w_veh);
    return launch(h, B, o);
}

// The ragged device entry with per-problem vehicle parameters (device arrays): the shape of a vehicle-width sweep whose
// tracks are already resident (BASELINE config 4).  Either list may be NULL (the scalar applies to every problem).
extern "C" int mcq_solve_device_ragged_params(mcq_handle* h, int batch, int nmax, const int* n_list, const double* reftrack,
                                              const double* normvec, const double* scaling, double kappa_bound, double w_veh,
                                              const double* kappa_bound_list, const double* w_veh_list, const mcq_opts* opts,
                                              double* alpha_out, double* curv_err_out, int* status_out, mcq_info* info_out)
{
    if (!h || batch <= 0 || nmax <= 0 || !n_list || !reftrack || !alpha_out || !curv_err_out || !status_out) {
        g_err = "mcq_solve_device_ragged_params: bad argument";
        return MCQ_E_ARG;
    }
    HIP_TRY(hipSetDevice(h->device));
    const mcq_opts o = resolve_opts(opts);
    int rc = ensure_workspace(h, 0, (size_t)batch, (size_t)nmax);
    if (rc) return rc;
    McqBatch B = make_batch(batch, nmax, n_list, reftrack, normvec, scaling, alpha_out, curv_err_out, status_out, info_out, kappa_bound, w_veh);
    B.kappa_bound_list = kappa_bound_list;
    B.w_veh_list = w_veh_list;
    return launch(h, B, o);
}

extern "C" int mcq_prep_device(mcq_handle* h, int batch, int nmax, const int* n_list, const double* reftrack,
                               double* normvec_out, double* scaling_out, int* status_out)
{
    if (!h || batch <= 0 || nmax <= 0 || !reftrack || !status_out || (!normvec_out && !scaling_out)) {
        g_err = "mcq_prep_device: bad argument";
        return MCQ_E_ARG;
    }
    HIP_TRY(hipSetDevice(h->device));
    const mcq_opts o = resolve_opts(nullptr);
    int rc = ensure_workspace(h, 0, (size_t)batch, (size_t)nmax);
    if (rc) return rc;
    // (kappa_bound 1, w_veh 0: the bounds computed along the way are not used -- any widths are "feasible")
    McqBatch B = make_batch(batch, nmax, n_list, reftrack, nullptr, nullptr, nullptr, nullptr, status_out, nullptr, 1.0, 0.0);
    B.nv_out = normvec_out;
    B.sc_out = scaling_out;
    B.prep_only = 1;
    return launch(h, B, o);
}

extern "C" int mcq_normals_crossing_device(mcq_handle* h, int batch, int nmax, const int* n_list, const double* reftrack,
                                           const double* normvec, int horizon, int* crossing_out)
{
    if (!h || batch <= 0 || nmax <= 0 || !reftrack || !normvec || !crossing_out) {
        g_err = "mcq_normals_crossing_device: bad argument";
        return MCQ_E_ARG;
    }
    HIP_TRY(hipSetDevice(h->device));
    hipLaunchKernelGGL(mcq_normals_crossing_kernel, dim3(batch), dim3(256), 0, compute_stream(h), nmax, n_list, reftrack, normvec,
                       horizon, crossing_out);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int mcq_relinearise_device(mcq_handle* h, int batch, int nmax, const int* n_in, const double* reftrack_in,
                                      const double* normvec_in, const double* alpha, const int* live, double alpha_scale,
                                      double stepsize, double* reftrack_out, double* normvec_out, int* n_out,
                                      int* status_out)
{
    if (!h || batch <= 0 || nmax <= 0 || !n_in || !reftrack_in || !normvec_in || !alpha || !reftrack_out || !normvec_out ||
        !n_out || !status_out || !(stepsize > 0.0) || reftrack_in == reftrack_out || normvec_in == normvec_out) {
        g_err = "mcq_relinearise_device: bad argument";
        return MCQ_E_ARG;
    }
    HIP_TRY(hipSetDevice(h->device));
    int rc = ensure_workspace(h, 0, (size_t)batch, (size_t)nmax);
    if (rc) return rc;
    McqRelin R;
    memset(&R, 0, sizeof(R));
    R.batch = batch;
    R.nmax = nmax;
    R.n_in = n_in;
    R.ref_in = reftrack_in;
    R.nv_in = normvec_in;
    R.alpha = alpha;
    R.live = live;
    R.alpha_scale = alpha_scale;
    R.stepsize = stepsize;
    R.ref_out = reftrack_out;
    R.nv_out = normvec_out;
    R.n_out = n_out;
    R.status = status_out;
    R.vec = h->ws[0].vec;
    R.state_in = h->ws[0].state;          // what the last solve on this handle left (the caller solves, then re-linearises, the same batch)
    R.state_out = h->state2;
    h->state2_valid = true;
    h->state2_batch = batch;
    h->state2_nmax = nmax;
    hipLaunchKernelGGL(mcq_relinearise_kernel, dim3(batch), dim3(256), 0, compute_stream(h), R);
    HIP_TRY(hipGetLastError());
    return 0;
}

// every velocity-profile entry ends here.  The three older entries launch the closed / ggv form (closed = 1, no loc_gg);
// mcq_vel_profile_device_forms picks one of the four kernels: a launch has one form for all its variants.
static int vel_profile_launch(mcq_handle* h, int batch, int n, int nmax, const int* n_of_track, const int* track_of,
                              const double* kappa, const double* el_lengths, const double* ggv, int n_ggv,
                              const double* ax_max_machines, int n_machines, const double* drag_coeff, const double* m_veh,
                              const double* v_max, double dyn_model_exp, double* vx_out, double* lap_time_out,
                              const double* mu = nullptr, int filt_window = 0, int closed = 1, const double* loc_gg = nullptr,
                              const double* v_start = nullptr, const double* v_end = nullptr)
{
    // upstream's "either ggv and optionally mu OR loc_gg"
    const bool tables_ok = loc_gg ? (!ggv && n_ggv == 0 && !mu) : (ggv && n_ggv >= 1);
    if (!h || batch <= 0 || (!n_of_track && n < 2) || nmax < n || nmax < 2 || !kappa || !el_lengths || !tables_ok ||
        !ax_max_machines || n_machines < 1 || !drag_coeff || !m_veh || !v_max || !vx_out || !lap_time_out ||
        !(dyn_model_exp > 0.0) || (!closed && !v_start)) {
        g_err = "mcq_vel_profile_device: bad argument";
        return MCQ_E_ARG;
    }
    HIP_TRY(hipSetDevice(h->device));
    const size_t need = (size_t)(closed ? 2 : 1) * nmax * batch * sizeof(double);      // the lap doubled, or the row once
    if (int rc = grow(h, h->vel, need)) return rc;
    McqVelForms F;
    memset(&F, 0, sizeof(F));
    McqVel& V = F.V;
    V.batch = batch; V.n = n; V.nmax = nmax;
    V.n_of_track = n_of_track;
    V.track_of = track_of; V.kappa = kappa; V.el = el_lengths;
    V.ggv = ggv; V.ng = n_ggv; V.axm = ax_max_machines; V.nam = n_machines;
    V.drag = drag_coeff; V.mass = m_veh; V.vmax = v_max; V.dyn_exp = dyn_model_exp;
    V.mu = mu; V.filt_window = filt_window;
    V.scratch = (double*)h->vel.p; V.vx_out = vx_out; V.lap_time = lap_time_out;
    F.loc_gg = loc_gg; F.v_start = v_start; F.v_end = v_end;
    const dim3 grid((batch + 63) / 64), block(64);
    if (closed && !loc_gg) hipLaunchKernelGGL(mcq_vel_profile_kernel, grid, block, 0, compute_stream(h), V);
    else if (closed) hipLaunchKernelGGL(mcq_vel_profile_locgg_kernel, grid, block, 0, compute_stream(h), F);
    else if (!loc_gg) hipLaunchKernelGGL(mcq_vel_profile_open_kernel, grid, block, 0, compute_stream(h), F);
    else hipLaunchKernelGGL(mcq_vel_profile_open_locgg_kernel, grid, block, 0, compute_stream(h), F);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int mcq_vel_profile_device(mcq_handle* h, int batch, int n, int nmax, const int* track_of, const double* kappa,
                                      const double* el_lengths, const double* ggv, int n_ggv, const double* ax_max_machines,
                                      int n_machines, const double* drag_coeff, const double* m_veh, const double* v_max,
                                      double dyn_model_exp, double* vx_out, double* lap_time_out)
{
    return vel_profile_launch(h, batch, n, nmax, nullptr, track_of, kappa, el_lengths, ggv, n_ggv, ax_max_machines,
                              n_machines, drag_coeff, m_veh, v_max, dyn_model_exp, vx_out, lap_time_out);
}

extern "C" int mcq_vel_profile_device_ragged(mcq_handle* h, int batch, int nmax, const int* n_of_track, const int* track_of,
                                             const double* kappa, const double* el_lengths, const double* ggv, int n_ggv,
                                             const double* ax_max_machines, int n_machines, const double* drag_coeff,
                                             const double* m_veh, const double* v_max, double dyn_model_exp, double* vx_out,
                                             double* lap_time_out)
{
    if (!n_of_track) { g_err = "mcq_vel_profile_device_ragged: n_of_track is NULL"; return MCQ_E_ARG; }
    return vel_profile_launch(h, batch, 0, nmax, n_of_track, track_of, kappa, el_lengths, ggv, n_ggv, ax_max_machines,
                              n_machines, drag_coeff, m_veh, v_max, dyn_model_exp, vx_out, lap_time_out);
}

extern "C" int mcq_vel_profile_device_opts(mcq_handle* h, int batch, int n, int nmax, const int* n_of_track, const int* track_of,
                                           const double* kappa, const double* el_lengths, const double* ggv, int n_ggv,
                                           const double* ax_max_machines, int n_machines, const double* drag_coeff,
                                           const double* m_veh, const double* v_max, const mcq_vel_opts* opts, double* vx_out,
                                           double* lap_time_out)
{
    if (!opts) { g_err = "mcq_vel_profile_device_opts: opts is NULL"; return MCQ_E_ARG; }
    if (opts->filt_window < 0) { g_err = "mcq_vel_profile_device_opts: negative filt_window"; return MCQ_E_ARG; }
    return vel_profile_launch(h, batch, n_of_track ? 0 : n, nmax, n_of_track, track_of, kappa, el_lengths, ggv, n_ggv, ax_max_machines,
                              n_machines, drag_coeff, m_veh, v_max, opts->dyn_model_exp, vx_out, lap_time_out, opts->mu,
                              opts->filt_window);
}

extern "C" int mcq_vel_profile_device_forms(mcq_handle* h, int batch, int n, int nmax, const int* n_of_track, const int* track_of,
                                            const double* kappa, const double* el_lengths, const double* ggv, int n_ggv,
                                            const double* ax_max_machines, int n_machines, const double* drag_coeff,
                                            const double* m_veh, const double* v_max, const mcq_vel_forms* forms, double* vx_out,
                                            double* lap_time_out)
{
    if (!forms) { g_err = "mcq_vel_profile_device_forms: forms is NULL"; return MCQ_E_ARG; }
    if (forms->filt_window < 0) { g_err = "mcq_vel_profile_device_forms: negative filt_window"; return MCQ_E_ARG; }
    if (forms->loc_gg && (ggv || n_ggv != 0 || forms->mu)) {
        g_err = "mcq_vel_profile_device_forms: either ggv and optionally mu OR loc_gg, not both";
        return MCQ_E_ARG;
    }
    if (!forms->loc_gg && !ggv) { g_err = "mcq_vel_profile_device_forms: either ggv or loc_gg must be supplied"; return MCQ_E_ARG; }
    if (!forms->closed && !forms->v_start) { g_err = "mcq_vel_profile_device_forms: v_start is required when closed == 0"; return MCQ_E_ARG; }
    return vel_profile_launch(h, batch, n_of_track ? 0 : n, nmax, n_of_track, track_of, kappa, el_lengths, ggv, n_ggv, ax_max_machines,
                              n_machines, drag_coeff, m_veh, v_max, forms->dyn_model_exp, vx_out, lap_time_out, forms->mu,
                              forms->filt_window, forms->closed != 0, forms->loc_gg, forms->v_start, forms->v_end);
}

// the fields both raceline entries share (Q is zeroed by the caller, with the record it may be part of)
static void fill_race(McqRace& Q, mcq_handle* h, int batch, int nmax, const int* n_in, const double* reftrack, const double* normvec,
                      const double* alpha, double stepsize, int mmax, double* raceline_out, double* psi_out, double* kappa_out,
                      double* el_lengths_out, int* m_out, int* status_out)
{
    Q.batch = batch; Q.nmax = nmax; Q.mmax = mmax;
    Q.n_in = n_in; Q.ref = reftrack; Q.nv = normvec; Q.alpha = alpha; Q.stepsize = stepsize;
    Q.xy_out = raceline_out; Q.psi_out = psi_out; Q.kappa_out = kappa_out; Q.el_out = el_lengths_out;
    Q.m_out = m_out; Q.status = status_out;
    Q.vec = h->ws[0].vec;
}

extern "C" int mcq_raceline_device(mcq_handle* h, int batch, int nmax, const int* n_in, const double* reftrack,
                                   const double* normvec, const double* alpha, double stepsize, int mmax,
                                   double* raceline_out, double* psi_out, double* kappa_out, double* el_lengths_out,
                                   int* m_out, int* status_out)
{
    if (!h || batch <= 0 || nmax < 3 || mmax < 2 || !reftrack || !normvec || !alpha || !(stepsize > 0.0) || !kappa_out ||
        !el_lengths_out || !m_out || !status_out) {
        g_err = "mcq_raceline_device: bad argument";
        return MCQ_E_ARG;
    }
    HIP_TRY(hipSetDevice(h->device));
    int rc = ensure_workspace(h, 0, (size_t)batch, (size_t)nmax);
    if (rc) return rc;
    McqRace Q;
    memset(&Q, 0, sizeof(Q));
    fill_race(Q, h, batch, nmax, n_in, reftrack, normvec, alpha, stepsize, mmax, raceline_out, psi_out, kappa_out, el_lengths_out, m_out, status_out);
    hipLaunchKernelGGL(mcq_raceline_kernel, dim3(batch), dim3(256), 0, compute_stream(h), Q);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int mcq_raceline_device_ends(mcq_handle* h, int batch, int nmax, const int* n_in, const double* reftrack,
                                        const double* normvec, const double* alpha, const int* closed, const double* psi,
                                        double stepsize, int mmax, double* raceline_out, double* psi_out, double* kappa_out,
                                        double* el_lengths_out, int* m_out, int* status_out)
{
    if (!h || batch <= 0 || nmax < 2 || mmax < 2 || !reftrack || !normvec || !alpha || !(stepsize > 0.0) || !kappa_out ||
        !el_lengths_out || !m_out || !status_out || (!closed && !psi)) {
        g_err = "mcq_raceline_device_ends: bad argument";
        return MCQ_E_ARG;
    }
    HIP_TRY(hipSetDevice(h->device));
    int rc = ensure_workspace(h, 0, (size_t)batch, (size_t)nmax);
    if (rc) return rc;
    if (!psi) {     // legal for a launch of rings only: the flags are read back (the one blocking path of this entry)
        std::vector<int> flags((size_t)batch);
        HIP_TRY(hipStreamSynchronize(compute_stream(h)));
        HIP_TRY(hipMemcpy(flags.data(), closed, (size_t)batch * sizeof(int), hipMemcpyDeviceToHost));
        for (int k = 0; k < batch; ++k)
            if (flags[k] == 0) {
                g_err = "mcq_raceline_device_ends: psi is NULL and a row is a chain";
                return MCQ_E_ARG;
            }
    }
    McqRaceEnds E;
    memset(&E, 0, sizeof(E));
    fill_race(E.Q, h, batch, nmax, n_in, reftrack, normvec, alpha, stepsize, mmax, raceline_out, psi_out, kappa_out, el_lengths_out, m_out, status_out);
    E.closed = closed; E.psi = psi;
    hipLaunchKernelGGL(mcq_raceline_ends_kernel, dim3(batch), dim3(256), 0, compute_stream(h), E);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- the finished trajectory and check_traj's verdicts (include/mcq.h) ----------------------------------------------------------------
extern "C" int mcq_trajectory_device(mcq_handle* h, int batch, int m, int mmax, const int* m_of_track, const int* track_of,
                                     const double* raceline, const double* psi, const double* kappa, const double* el_lengths,
                                     const double* vx, int closed, const double* drag_coeff, const double* m_veh, const double* v_max,
                                     const double* ggv, int n_ggv, const double* ax_max_machines, int n_machines, double curvlim,
                                     double* traj_out, double* t_out, double* length_out, double* limits_out, int* flags_out)
{
    if (!h || batch <= 0 || mmax < 2 || (!m_of_track && (m < 2 || m > mmax)) || !raceline || !psi || !kappa || !el_lengths || !vx ||
        !drag_coeff || !m_veh || !v_max || (ggv && n_ggv < 1) || (ax_max_machines && n_machines < 1) || curvlim != curvlim ||
        !length_out || !limits_out || !flags_out) {
        g_err = "mcq_trajectory_device: bad argument";
        return MCQ_E_ARG;
    }
    HIP_TRY(hipSetDevice(h->device));
    McqTraj T;
    memset(&T, 0, sizeof(T));
    T.batch = batch; T.m = m_of_track ? 0 : m; T.mmax = mmax;
    T.m_of_track = m_of_track; T.track_of = track_of;
    T.xy = raceline; T.psi = psi; T.kappa = kappa; T.el = el_lengths; T.vx = vx;
    T.closed = closed != 0;
    T.drag = drag_coeff; T.mass = m_veh; T.vmax = v_max;
    T.ggv = ggv; T.ng = ggv ? n_ggv : 0; T.axm = ax_max_machines; T.nam = ax_max_machines ? n_machines : 0;
    T.curvlim = curvlim;
    T.traj = traj_out; T.t_out = t_out; T.length = length_out; T.limits = limits_out; T.flags = flags_out;
    hipLaunchKernelGGL(mcq_trajectory_kernel, dim3(batch), dim3(64), 0, compute_stream(h), T);
    HIP_TRY(hipGetLastError());
    return 0;
}

// bytes the boundary scratch may take ($MCQ_BOUND_BYTES, default 1 GiB)
static size_t bound_byte_cap()
{
    const char* e = getenv("MCQ_BOUND_BYTES");
    const double v = e ? atof(e) : 0.0;
    return v >= 1.0 ? (size_t)v : ((size_t)1 << 30);
}

// samples [tracks][2][nbmax][2] | raw boundaries [tracks][2][nmax][2] | running sums [tracks][2][nmax + 1] | side statuses [tracks][2]
static Arena bound_layout(size_t tracks, size_t nmax, size_t nbmax)
{
    return Arena().add<double>(2 * tracks * nbmax * 2).add<double>(2 * tracks * nmax * 2).add<double>(2 * tracks * (nmax + 1)).add<int>(2 * tracks);
}

extern "C" int mcq_bound_dists_device(mcq_handle* h, int tracks, int nmax, const int* n_list, const double* reftrack,
                                      const double* normvec, int mmax, const int* m_list, const double* raceline, const double* psi,
                                      double length_veh, double width_veh, const double* length_veh_list, const double* width_veh_list,
                                      double stepsize_bound, int mode, double* min_dists_out, double* min_dist_out, int* nb_out,
                                      double* bound_out, int* status_out)
{
    const bool len_ok = length_veh_list || (length_veh >= 0.0 && length_veh <= 1.7e308);
    const bool wid_ok = width_veh_list || (width_veh >= 0.0 && width_veh <= 1.7e308);
    if (!h || tracks <= 0 || nmax < 3 || mmax < 1 || !reftrack || !normvec || !raceline || !psi || !len_ok || !wid_ok ||
        !(stepsize_bound > 0.0) || !(stepsize_bound <= 1.7e308) || (mode != MCQ_BOUNDS_ALL && mode != MCQ_BOUNDS_FIRST_ROW) ||
        !min_dists_out || !min_dist_out || !nb_out || !status_out) {
        g_err = "mcq_bound_dists_device: bad argument";
        return MCQ_E_ARG;
    }
    HIP_TRY(hipSetDevice(h->device));
    // what the scratch holds in doubles next to the samples: they take what $MCQ_BOUND_BYTES leaves
    const size_t sides = 2 * (size_t)tracks;
    const size_t fixed = bound_layout(tracks, nmax, 0).bytes / sizeof(double);
    const size_t cap = bound_byte_cap() / sizeof(double);
    if (cap < fixed + sides * 2) {
        g_err = "mcq_bound_dists_device: the boundary scratch would exceed $MCQ_BOUND_BYTES";
        return MCQ_E_TOO_LARGE;
    }
    size_t nbmax = (cap - fixed) / (sides * 2);
    if (nbmax > MCQ_BOUND_NB_MAX) nbmax = MCQ_BOUND_NB_MAX;
    const Arena a = bound_layout(tracks, nmax, nbmax);
    if (int rc = grow(h, h->bound, a.bytes)) return rc;
    McqBound P;
    memset(&P, 0, sizeof(P));
    P.tracks = tracks; P.nmax = nmax; P.mmax = mmax; P.nbmax = (int)nbmax; P.mode = mode;
    P.n_list = n_list; P.m_list = m_list; P.ref = reftrack; P.nv = normvec; P.xy = raceline; P.psi = psi;
    P.length_veh = length_veh; P.width_veh = width_veh; P.length_list = length_veh_list; P.width_list = width_veh_list;
    P.step = stepsize_bound;
    P.samples = a.at<double>(h->bound.p, 0); P.pts = a.at<double>(h->bound.p, 1); P.cum = a.at<double>(h->bound.p, 2);
    P.side_status = a.at<int>(h->bound.p, 3);
    P.min_dists = min_dists_out; P.min_dist = min_dist_out; P.nb_out = nb_out; P.bound_out = bound_out; P.status = status_out;
    hipStream_t st = compute_stream(h);
    hipLaunchKernelGGL(mcq_bound_points_kernel, dim3(2 * tracks), dim3(256), 0, st, P);
    HIP_TRY(hipGetLastError());
    const int block = 256 * MCQ_BD_S;
    hipLaunchKernelGGL(mcq_bound_dists_kernel, dim3((mmax + block - 1) / block, tracks), dim3(256), 0, st, P);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(mcq_bound_min_kernel, dim3(tracks), dim3(256), 0, st, P);
    HIP_TRY(hipGetLastError());
    return 0;
}

// doubles per track of the fit's work area: B-splines [mimax][k + 1], residuals [mimax], two triangles [(2 k + 5) nkmax], coefficients [nkmax][2],
// jump rows [nkmax][k + 2], fpint [nkmax + 2], then the ints: intervals [mimax], nrdata [nkmax + 2], row marks [mimax]; at the end the segments'
// reduced rows [mimax][k + 1] and their right-hand sides [mimax][2]
static size_t fit_work_per(size_t mm, size_t k, size_t nk)
{
    return mm * (k + 2) + 2 * (2 * k + 5) * nk + 2 * nk + nk * (k + 2) + nk + 2 + (2 * mm + nk + 2 + 1) / 2 + 1 + mm * (k + 3);
}

// running sums [tracks][nmax + 1] | closed points [tracks][mimax][2] | parameters [tracks][mimax] | work areas [tracks][fit_work_per]
static Arena fit_layout(size_t tracks, size_t nmax, size_t mimax, size_t k, size_t nkmax)
{
    return Arena().add<double>(tracks * (nmax + 1)).add<double>(tracks * mimax * 2).add<double>(tracks * mimax).add<double>(tracks * fit_work_per(mimax, k, nkmax));
}

// FITPACK's periodic smoothing fit (include/mcq.h): one launch on the handle's stream, a workgroup per track
extern "C" int mcq_spline_fit_device(mcq_handle* h, int tracks, int nmax, const int* n_list, const double* track, double stepsize_prep, int mimax,
                                     int k, double s, int nkmax, int* nk_out, double* knots_out, double* coef_out, double* fp_out, int* ier_out,
                                     int* mi_out, double* pts_out, int* status_out)
{
    if (!h || tracks <= 0 || tracks > MCQ_SPL_MAX_TRACKS || nmax < 3 || nmax > MCQ_SPL_MAX_N || mimax < 2 || mimax > MCQ_SPL_MAX_N || !track ||
        k < 1 || k > 5 || !(s >= 0.0) || !(s <= 1.7e308) || nkmax < 2 * k + 2 || nkmax > MCQ_SPL_MAX_N + 10 || !(stepsize_prep == stepsize_prep) ||
        !nk_out || !knots_out || !coef_out || !ier_out || !status_out) {
        g_err = "mcq_spline_fit_device: bad argument";
        return MCQ_E_ARG;
    }
    HIP_TRY(hipSetDevice(h->device));
    const Arena a = fit_layout(tracks, nmax, mimax, k, nkmax);
    if (int rc = grow(h, h->fit, a.bytes)) return rc;
    McqFit P;
    memset(&P, 0, sizeof(P));
    P.tracks = tracks; P.nmax = nmax; P.mimax = mimax; P.k = k; P.nkmax = nkmax;
    P.n_list = n_list; P.track = track; P.step = stepsize_prep; P.s = s;
    P.cum = a.at<double>(h->fit.p, 0); P.pts = a.at<double>(h->fit.p, 1); P.u = a.at<double>(h->fit.p, 2); P.work = a.at<double>(h->fit.p, 3);
    P.work_per = fit_work_per(mimax, k, nkmax);
    P.nk_out = nk_out; P.knots_out = knots_out; P.coef_out = coef_out; P.fp_out = fp_out; P.ier_out = ier_out; P.mi_out = mi_out;
    P.pts_out = pts_out; P.status = status_out;
    hipLaunchKernelGGL(mcq_spline_fit_kernel, dim3(tracks), dim3(256), 0, compute_stream(h), P);
    HIP_TRY(hipGetLastError());
    return 0;
}

// first guesses | closest parameters | distances | sides, [tracks][nmax + 1] each | sample counts [tracks] (they take a double's room each)
static Arena spl_layout(size_t tracks, size_t nmax)
{
    const size_t per = tracks * (nmax + 1);
    return Arena().add<double>(per).add<double>(per).add<double>(per).add<double>(per).add<int>(2 * tracks);
}

// tph.spline_approximation behind FITPACK's fit (include/mcq.h): three launches on the handle's stream
extern "C" int mcq_spline_approx_device(mcq_handle* h, int tracks, int nmax, const int* n_list, const double* track, int k, int nkmax,
                                        const int* nk_list, const double* knots, const double* coef, double stepsize_reg, int mmax,
                                        double* reftrack_out, int* m_out, double* closest_t_out, double* dists_out, double* dev_out,
                                        int* nonmono_out, int* status_out)
{
    if (!h || tracks <= 0 || tracks > MCQ_SPL_MAX_TRACKS || nmax < 3 || nmax > MCQ_SPL_MAX_N || !track || k < 1 || k > 5 || nkmax < 2 * k + 2 || !knots || !coef || !(stepsize_reg > 0.0) ||
        !(stepsize_reg <= 1.7e308) || mmax < 3 || !reftrack_out || !m_out || !status_out) {
        g_err = "mcq_spline_approx_device: bad argument";
        return MCQ_E_ARG;
    }
    HIP_TRY(hipSetDevice(h->device));
    const Arena a = spl_layout(tracks, nmax);
    if (int rc = grow(h, h->spl, a.bytes)) return rc;
    McqSpline S;
    memset(&S, 0, sizeof(S));
    S.tracks = tracks; S.nmax = nmax; S.k = k; S.nkmax = nkmax; S.mmax = mmax;
    S.n_list = n_list; S.nk_list = nk_list; S.track = track; S.knots = knots; S.coef = coef; S.step = stepsize_reg;
    S.tguess = a.at<double>(h->spl.p, 0); S.ct = a.at<double>(h->spl.p, 1); S.dist = a.at<double>(h->spl.p, 2); S.side = a.at<double>(h->spl.p, 3);
    S.npts = a.at<int>(h->spl.p, 4);
    S.ref_out = reftrack_out; S.m_out = m_out; S.ct_out = closest_t_out; S.dist_out = dists_out; S.dev_out = dev_out;
    S.nonmono_out = nonmono_out; S.status = status_out;
    hipStream_t st = compute_stream(h);
    hipLaunchKernelGGL(mcq_spline_length_kernel, dim3(tracks), dim3(256), 0, st, S);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(mcq_spline_search_kernel, dim3((nmax + 1 + 255) / 256, tracks), dim3(256), 0, st, S);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(mcq_spline_finish_kernel, dim3(tracks), dim3(256), 0, st, S);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int mcq_min_width_device(mcq_handle* h, int batch, int nmax, const int* n_list, double* reftrack_io, double min_width,
                                    int* changed_out)
{
    if (!h || batch <= 0 || nmax <= 0 || !reftrack_io || !changed_out || !(min_width == min_width)) {
        g_err = "mcq_min_width_device: bad argument";
        return MCQ_E_ARG;
    }
    HIP_TRY(hipSetDevice(h->device));
    hipLaunchKernelGGL(mcq_min_width_kernel, dim3(batch), dim3(256), 0, compute_stream(h), nmax, n_list, reftrack_io, min_width, changed_out);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- the export tables (include/mcq.h): the spline lengths per track, then the lookup and the rows per variant; two launches on the handle's stream
extern "C" int mcq_export_device(mcq_handle* h, int tracks, int nmax, const int* n_list, const double* reftrack, const double* normvec,
                                 const double* alpha, int batch, int mmax, const int* m_of_track, const int* track_of, const double* traj,
                                 double* ltpl_out, int* idx_out, double* spline_lengths_out, double* s_ref_out, double* spline_total_out,
                                 int* status_out)
{
    if (!h || tracks <= 0 || batch <= 0 || nmax < 3 || mmax < 2 || !reftrack || !normvec || !alpha || !traj || !ltpl_out ||
        !spline_total_out || !status_out) {
        g_err = "mcq_export_device: bad argument";
        return MCQ_E_ARG;
    }
    const size_t nblk = ((size_t)nmax + MCQ_EX_ROWS) / MCQ_EX_ROWS;      // row blocks of a table of nmax + 1 rows
    if ((size_t)batch * nblk > 0x7fffffffu) {
        g_err = "mcq_export_device: more row blocks than one launch holds";
        return MCQ_E_TOO_LARGE;
    }
    HIP_TRY(hipSetDevice(h->device));
    int rc = ensure_workspace(h, 0, (size_t)tracks, (size_t)nmax);
    if (rc) return rc;
    McqExport X;
    memset(&X, 0, sizeof(X));
    X.tracks = tracks; X.nmax = nmax; X.batch = batch; X.mmax = mmax;
    X.n_list = n_list; X.ref = reftrack; X.nv = normvec; X.alpha = alpha;
    X.m_of_track = m_of_track; X.track_of = track_of; X.traj = traj;
    X.vec = h->ws[0].vec;
    X.ltpl = ltpl_out; X.idx = idx_out; X.len_out = spline_lengths_out; X.s_ref_out = s_ref_out; X.total_out = spline_total_out;
    X.status = status_out;
    hipStream_t st = compute_stream(h);
    hipLaunchKernelGGL(mcq_export_s_kernel, dim3(tracks), dim3(256), 0, st, X);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(mcq_export_rows_kernel, dim3((unsigned)((size_t)batch * nblk)), dim3(256), 0, st, X);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- friction maps (include/mcq.h): one map = one device allocation holding the index; the two entries need no temporaries of their own ----
struct mcq_fmap {
    McqFmap F;
    void* dev = nullptr;
    size_t bytes = 0;
};
#define MCQ_FMAP_MAX_BINS (1 << 22)

// NOTE: an edge is o + k * side in two roundings, here and in fric_edge (csrc/mcq_fric.inc, compiled without contraction).  This translation
// unit's host code is baseline x86-64, which has no fused multiply-add to contract to.
static inline double fmap_edge(double o, double side, int k) { return o + (double)k * side; }

static int fmap_bin(double c, double o, double side, int nb)
{
    const double t = std::floor((c - o) / side);
    int k = t >= (double)(nb - 1) ? nb - 1 : (t > 0.0 ? (int)t : 0);
    while (k > 0 && c < fmap_edge(o, side, k)) --k;                 // the quotient's rounding against the edges the kernels measure from
    while (k < nb - 1 && c > fmap_edge(o, side, k + 1)) ++k;
    return k;
}

extern "C" int mcq_fmap_create(mcq_handle* h, int cells, const double* xy_host, const double* mue_host, double bin_side, mcq_fmap** out)
{
    if (!h || cells < 1 || !xy_host || !mue_host || !out) {
        g_err = "mcq_fmap_create: bad argument";
        return MCQ_E_ARG;
    }
    *out = nullptr;
    double x0 = INFINITY, x1 = -INFINITY, y0 = INFINITY, y1 = -INFINITY;
    for (int c = 0; c < cells; ++c) {
        const double x = xy_host[2 * (size_t)c], y = xy_host[2 * (size_t)c + 1];
        if (!(std::isfinite(x) && std::isfinite(y))) {
            g_err = "mcq_fmap_create: a cell coordinate is not finite";
            return MCQ_E_ARG;
        }
        x0 = std::min(x0, x); x1 = std::max(x1, x); y0 = std::min(y0, y); y1 = std::max(y1, y);
    }
    const double wx = x1 - x0, wy = y1 - y0;
    if (!(std::isfinite(wx) && std::isfinite(wy))) {
        g_err = "mcq_fmap_create: the cells' bounding box is not finite";
        return MCQ_E_ARG;
    }
    double side = bin_side;
    if (!(side > 0.0) || !std::isfinite(side)) {        // automatic: a cell per bin on average over the box
        side = std::sqrt(wx * wy / (double)cells);
        if (!(side > 0.0) || !std::isfinite(side)) side = std::max(wx, wy) / (double)cells;     // a degenerate box: all cells on one line ...
        if (!(side > 0.0) || !std::isfinite(side)) side = 1.0;                                  // ... or at one point
    }
    // a degenerate axis has one bin; the bin count is capped by growing the side
    for (;;) {
        const double bx = std::floor(wx / side) + 1.0, by = std::floor(wy / side) + 1.0;
        if (bx * by <= (double)MCQ_FMAP_MAX_BINS) break;
        side *= 2.0;
    }
    const int nbx = (int)std::floor(wx / side) + 1, nby = (int)std::floor(wy / side) + 1;
    const size_t nb = (size_t)nbx * nby;
    // one allocation: sxy [cells][2], mue [cells], bin_start [nb + 1], sidx [cells]
    const size_t off_mue = (size_t)cells * 2 * sizeof(double), off_bs = off_mue + (size_t)cells * sizeof(double);
    const size_t off_idx = off_bs + (nb + 1) * sizeof(int), bytes = off_idx + (size_t)cells * sizeof(int);
    std::vector<double> img((bytes + 7) / 8);
    char* base = (char*)img.data();
    double* sxy = (double*)base;
    double* mue = (double*)(base + off_mue);
    int* bs = (int*)(base + off_bs);
    int* sidx = (int*)(base + off_idx);
    std::vector<int> bin_of(cells);
    for (size_t b = 0; b <= nb; ++b) bs[b] = 0;
    for (int c = 0; c < cells; ++c) {
        bin_of[c] = fmap_bin(xy_host[2 * (size_t)c + 1], y0, side, nby) * nbx + fmap_bin(xy_host[2 * (size_t)c], x0, side, nbx);
        ++bs[bin_of[c] + 1];
    }
    for (size_t b = 0; b < nb; ++b) bs[b + 1] += bs[b];
    {
        std::vector<int> fill(bs, bs + nb);
        for (int c = 0; c < cells; ++c) {       // a counting sort: within a bin the cells keep their original order
            const int at = fill[bin_of[c]]++;
            sxy[2 * (size_t)at] = xy_host[2 * (size_t)c];
            sxy[2 * (size_t)at + 1] = xy_host[2 * (size_t)c + 1];
            sidx[at] = c;
        }
    }
    memcpy(mue, mue_host, (size_t)cells * sizeof(double));
    HIP_TRY(hipSetDevice(h->device));
    mcq_fmap* m = new mcq_fmap();
    hipError_t e = hipMalloc(&m->dev, bytes);
    if (e == hipSuccess) e = hipMemcpy(m->dev, base, bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(m->dev);
        delete m;
        return hip_failed("mcq_fmap_create: hipMalloc / hipMemcpy", e, __FILE__, __LINE__);
    }
    m->bytes = bytes;
    char* d = (char*)m->dev;
    m->F.cells = cells; m->F.nbx = nbx; m->F.nby = nby;
    m->F.x0 = x0; m->F.y0 = y0; m->F.side = side;
    m->F.sxy = (const double*)d; m->F.mue = (const double*)(d + off_mue);
    m->F.bin_start = (const int*)(d + off_bs); m->F.sidx = (const int*)(d + off_idx);
    *out = m;
    return 0;
}

extern "C" int mcq_fmap_destroy(mcq_handle* h, mcq_fmap* fmap)
{
    if (!h) { g_err = "mcq_fmap_destroy: bad argument"; return MCQ_E_ARG; }
    if (!fmap) return 0;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(compute_stream(h)));      // a launch in flight may still read the map
    (void)hipFree(fmap->dev);
    delete fmap;
    return 0;
}

extern "C" int mcq_fmap_info(const mcq_fmap* fmap, int* cells, int* bins_x, int* bins_y, double* bin_side, long long* device_bytes)
{
    if (!fmap) { g_err = "mcq_fmap_info: bad argument"; return MCQ_E_ARG; }
    if (cells) *cells = fmap->F.cells;
    if (bins_x) *bins_x = fmap->F.nbx;
    if (bins_y) *bins_y = fmap->F.nby;
    if (bin_side) *bin_side = fmap->F.side;
    if (device_bytes) *device_bytes = (long long)fmap->bytes;
    return 0;
}

extern "C" int mcq_fmap_query_device(mcq_handle* h, const mcq_fmap* fmap, int count, const double* xy, double* mue_out, int* idx_out,
                                     double* dist_out)
{
    if (!h || !fmap || count < 0 || (count > 0 && (!xy || !mue_out))) {
        g_err = "mcq_fmap_query_device: bad argument";
        return MCQ_E_ARG;
    }
    if (count == 0) return 0;
    HIP_TRY(hipSetDevice(h->device));
    hipLaunchKernelGGL(mcq_fmap_query_kernel, dim3((unsigned)(((size_t)count + 255) / 256)), dim3(256), 0, compute_stream(h), fmap->F, count, xy,
                       mue_out, idx_out, dist_out);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int mcq_friction_grid_device(mcq_handle* h, const mcq_fmap* fmap, int tracks, int nmax, const int* n_list, const double* reftrack,
                                        const double* normvec, double width_opt, const double* width_list, double wheelbase_front,
                                        double wheelbase_rear, double dn, int jmax, double* n_out, int* cnt_out, double* mue_out, int* idx_out,
                                        double* w_mue_out, int* status_out)
{
    if (!h || !fmap || tracks <= 0 || nmax < 1 || !(dn > 0.0) || !std::isfinite(dn) || jmax < 1 || !reftrack || !normvec || !n_out || !cnt_out ||
        !mue_out || !status_out) {
        g_err = "mcq_friction_grid_device: bad argument";
        return MCQ_E_ARG;
    }
    const size_t nblk = ((size_t)nmax + MCQ_FG_ROWS) / MCQ_FG_ROWS;
    if ((size_t)tracks * nblk > 0x7fffffffu) {
        g_err = "mcq_friction_grid_device: more row blocks than one launch holds";
        return MCQ_E_TOO_LARGE;
    }
    HIP_TRY(hipSetDevice(h->device));
    McqFricGrid G;
    memset(&G, 0, sizeof(G));
    G.F = fmap->F;
    G.tracks = tracks; G.nmax = nmax; G.jmax = jmax;
    G.n_list = n_list; G.ref = reftrack; G.nv = normvec;
    G.width = width_opt; G.width_list = width_list; G.wbf = wheelbase_front; G.wbr = wheelbase_rear; G.dn = dn;
    G.n_out = n_out; G.cnt_out = cnt_out; G.mue_out = mue_out; G.idx_out = idx_out; G.w_out = w_mue_out; G.status = status_out;
    hipLaunchKernelGGL(mcq_friction_grid_kernel, dim3((unsigned)((size_t)tracks * nblk)), dim3(256), 0, compute_stream(h), G);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int mcq_friction_gauss_device(mcq_handle* h, int tracks, int nmax, int jmax, const double* n_out, const int* cnt_out,
                                         const double* mue_out, const int* status, int n_gauss, double rcond, double* w_gauss_out,
                                         double* center_dist_out, int* rank_out, int* sweeps_out)
{
    if (!h || tracks <= 0 || nmax < 1 || jmax < 1 || n_gauss < 1 || n_gauss > 15 || std::isnan(rcond) || !n_out || !cnt_out || !mue_out || !status ||
        !w_gauss_out || !center_dist_out) {
        g_err = "mcq_friction_gauss_device: bad argument";
        return MCQ_E_ARG;
    }
    const int N = 2 * n_gauss + 1;
    const size_t row_bytes = mcq_fgs_row_doubles(jmax, N) * sizeof(double);
    if (row_bytes > MCQ_FGS_LDS) {
        g_err = "mcq_friction_gauss_device: one row's matrix does not fit into 64 KB of LDS";
        return MCQ_E_TOO_LARGE;
    }
    const int rows_wg = (int)std::min<size_t>(MCQ_FGS_ROWS, MCQ_FGS_LDS / row_bytes);
    const size_t nblk = ((size_t)nmax + rows_wg) / rows_wg;
    if ((size_t)tracks * nblk > 0x7fffffffu) {
        g_err = "mcq_friction_gauss_device: more row blocks than one launch holds";
        return MCQ_E_TOO_LARGE;
    }
    HIP_TRY(hipSetDevice(h->device));
    McqFricGauss G;
    memset(&G, 0, sizeof(G));
    G.tracks = tracks; G.nmax = nmax; G.jmax = jmax; G.n_gauss = n_gauss; G.N = N; G.rows_wg = rows_wg; G.rcond = rcond;
    G.n = n_out; G.cnt = cnt_out; G.mue = mue_out; G.status = status;
    G.w_out = w_gauss_out; G.cd_out = center_dist_out; G.rank_out = rank_out; G.sweeps_out = sweeps_out;
    hipLaunchKernelGGL(mcq_friction_gauss_kernel, dim3((unsigned)((size_t)tracks * nblk)), dim3(64 * rows_wg), rows_wg * row_bytes, compute_stream(h), G);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int mcq_friction_model_device(mcq_handle* h, int tracks, int nmax, int qmax, const double* q, const int* qcnt, int model,
                                         const double* weights, int n_gauss, int centres, const double* center_dist, const double* n_out,
                                         const int* cnt_out, int jmax, double* mue_out)
{
    const bool gauss = model == MCQ_FRIC_GAUSS, fit = gauss && centres == MCQ_FRIC_CENTRES_FIT;
    if (!h || tracks <= 0 || nmax < 1 || qmax < 1 || !q || !weights || !mue_out || (model != MCQ_FRIC_LINEAR && !gauss) ||
        (gauss && (n_gauss < 1 || n_gauss > 15 || !center_dist || (centres != MCQ_FRIC_CENTRES_FIT && centres != MCQ_FRIC_CENTRES_MINTIME))) ||
        (fit && (!n_out || !cnt_out || jmax < 1))) {
        g_err = "mcq_friction_model_device: bad argument";
        return MCQ_E_ARG;
    }
    const size_t total = (size_t)tracks * ((size_t)nmax + 1) * qmax, nblk = (total + 255) / 256;
    if (nblk > 0x7fffffffu) {
        g_err = "mcq_friction_model_device: more positions than one launch holds";
        return MCQ_E_TOO_LARGE;
    }
    HIP_TRY(hipSetDevice(h->device));
    McqFricModel M;
    memset(&M, 0, sizeof(M));
    M.tracks = tracks; M.nmax = nmax; M.qmax = qmax; M.jmax = jmax; M.model = model; M.centres = centres; M.n_gauss = n_gauss;
    M.N = gauss ? 2 * n_gauss + 1 : 0;
    M.q = q; M.qcnt = qcnt; M.w = weights; M.cd = center_dist; M.n = n_out; M.cnt = cnt_out; M.mue_out = mue_out;
    hipLaunchKernelGGL(mcq_friction_model_kernel, dim3((unsigned)nblk), dim3(256), 0, compute_stream(h), M);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- friction map generation (include/mcq.h; csrc/mcq_fgen.inc) ----
// kept [paths][vmax][2] | contours [paths][2 vmax][2] (own: none when the caller takes them) | flags [paths][vmax] | counts [paths]
static Arena path_layout(size_t paths, size_t vmax, bool own_contours)
{
    return Arena().add<double>(paths * vmax * 2).add<double>(own_contours ? paths * vmax * 4 : 0).add<int>(paths * vmax).add<int>(paths);
}

// per track: polygons [2][2 nmax][2] | kept, the same | contours [2][4 nmax][2] | radii [2] || flags [2][2 nmax] | counts, contour counts, nx ny [2] each
static Arena fgen_layout(size_t tracks, size_t nmax)
{
    const size_t tn = tracks * nmax, t2 = tracks * 2;
    return Arena().add<double>(tn * 8).add<double>(tn * 8).add<double>(tn * 16).add<double>(t2).add<int>(tn * 4).add<int>(t2).add<int>(t2).add<int>(t2);
}

// the grid points' flags [tracks][maxblk][256] | the blocks' counts [tracks][maxblk] (one per track where there is no block)
static Arena fgen_pts_layout(size_t tracks, size_t maxblk)
{
    return Arena().add<unsigned char>(tracks * maxblk * 256).add<int>(tracks * std::max<size_t>(maxblk, 1), sizeof(int));
}

extern "C" int mcq_points_in_path_device(mcq_handle* h, int paths, int vmax, const int* v_list, const double* verts, const double* radius, int count,
                                         const double* xy, unsigned char* inside_out, int* status_out, double* contour_out, int* contour_count_out)
{
    if (!h || paths <= 0 || vmax < 1 || count < 0 || !verts || !radius || !status_out || (count > 0 && (!xy || !inside_out)) ||
        (contour_out == nullptr) != (contour_count_out == nullptr)) {
        g_err = "mcq_points_in_path_device: bad argument";
        return MCQ_E_ARG;
    }
    const size_t blocks = ((size_t)count + 255) / 256;
    if (paths > 65535) {        // (count is an int: its blocks of 256 points fit the first axis)
        g_err = "mcq_points_in_path_device: more paths than one launch holds";
        return MCQ_E_TOO_LARGE;
    }
    HIP_TRY(hipSetDevice(h->device));
    const Arena a = path_layout(paths, vmax, !contour_out);
    if (int rc = grow(h, h->fgen, a.bytes)) return rc;
    void* base = h->fgen.p;
    McqContour C;
    memset(&C, 0, sizeof(C));
    C.paths = paths; C.vmax = vmax; C.v_list = v_list; C.verts = verts; C.radius = radius; C.status = status_out;
    C.kept = a.at<double>(base, 0);
    C.cont = contour_out ? contour_out : a.at<double>(base, 1);
    C.flag = a.at<int>(base, 2);
    C.ccount = contour_count_out ? contour_count_out : a.at<int>(base, 3);
    hipStream_t st = compute_stream(h);
    hipLaunchKernelGGL(mcq_fgen_contour_kernel, dim3(paths), dim3(256), 0, st, C);
    HIP_TRY(hipGetLastError());
    if (count == 0) return 0;
    hipLaunchKernelGGL(mcq_fgen_points_kernel, dim3((unsigned)blocks, paths), dim3(256), 0, st, C, count, xy, inside_out);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int mcq_friction_gen_device(mcq_handle* h, int tracks, int nmax, const int* n_list, const double* reftrack, double cellwidth,
                                       const int* inside_right, int cmax, double* bound_r_out, double* bound_l_out, double* grid_out,
                                       int* count_out, double* cells_out, int* status_out)
{
    if (!h || tracks <= 0 || nmax < 3 || !(cellwidth > 0.0) || !std::isfinite(cellwidth) || !reftrack || !grid_out || !status_out ||
        (cells_out && (cmax < 0 || !count_out))) {
        g_err = "mcq_friction_gen_device: bad argument";
        return MCQ_E_ARG;
    }
    if (tracks > 32767) {       // (tracks lie along the second axis of the all-pairs and scatter launches)
        g_err = "mcq_friction_gen_device: more tracks than one launch holds";
        return MCQ_E_TOO_LARGE;
    }
    HIP_TRY(hipSetDevice(h->device));
    const size_t t2 = (size_t)tracks * 2;
    const Arena a = fgen_layout(tracks, nmax);
    if (int rc = grow(h, h->fgen, a.bytes)) return rc;
    void* base = h->fgen.p;
    McqFgen G;
    memset(&G, 0, sizeof(G));
    G.tracks = tracks; G.nmax = nmax; G.cmax = cells_out ? cmax : 0; G.cw = cellwidth;
    G.n_list = n_list; G.ref = reftrack; G.inside_right = inside_right;
    G.bound_r = bound_r_out; G.bound_l = bound_l_out; G.grid = grid_out; G.count = count_out; G.cells = cells_out; G.status = status_out;
    G.poly = a.at<double>(base, 0); G.cont = a.at<double>(base, 2); G.prad = a.at<double>(base, 3);
    G.pcount = a.at<int>(base, 5); G.ccount = a.at<int>(base, 6); G.rec = a.at<int>(base, 7);
    hipStream_t st = compute_stream(h);
    hipLaunchKernelGGL(mcq_fgen_bounds_kernel, dim3(tracks), dim3(256), 0, st, G);
    HIP_TRY(hipGetLastError());
    if (!count_out) return 0;       // boundaries, grids and status only
    McqContour C;
    memset(&C, 0, sizeof(C));
    C.paths = 2 * tracks; C.vmax = 2 * nmax; C.v_list = G.pcount; C.verts = G.poly; C.radius = G.prad;
    C.kept = a.at<double>(base, 1); C.flag = a.at<int>(base, 4); C.cont = G.cont; C.ccount = G.ccount;
    hipLaunchKernelGGL(mcq_fgen_contour_kernel, dim3(2 * tracks), dim3(256), 0, st, C);
    HIP_TRY(hipGetLastError());
    // the one wait: the grids' sizes decide the launches that follow
    std::vector<int> rec(t2);
    HIP_TRY(hipMemcpyAsync(rec.data(), G.rec, t2 * sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    size_t maxblk = 0;
    for (int t = 0; t < tracks; ++t) {
        const size_t items = (size_t)rec[2 * t] * (((size_t)rec[2 * t + 1] + MCQ_FGEN_PPT - 1) / MCQ_FGEN_PPT);
        maxblk = std::max(maxblk, (items + 255) / 256);
    }
    // (MCQ_FGEN_GRID bounds a track at 2^31 - 1 points: at most 2^21 blocks of 256 items, within a launch's first axis)
    const Arena ap = fgen_pts_layout(tracks, maxblk);
    if (int rc = grow(h, h->fgen_pts, ap.bytes)) return rc;
    G.maxblk = (int)maxblk;
    G.bits = ap.at<unsigned char>(h->fgen_pts.p, 0);
    G.bcount = ap.at<int>(h->fgen_pts.p, 1);
    if (maxblk > 0) {
        hipLaunchKernelGGL(mcq_fgen_mask_kernel, dim3((unsigned)maxblk, tracks), dim3(256), 0, st, G);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(mcq_fgen_scan_kernel, dim3(tracks), dim3(256), 0, st, G);
    HIP_TRY(hipGetLastError());
    if (maxblk > 0 && cells_out && cmax > 0) {
        hipLaunchKernelGGL(mcq_fgen_scatter_kernel, dim3((unsigned)maxblk, tracks), dim3(256), 0, st, G);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

// ---- the minimum-time NLP as functions of w (include/mcq.h; csrc/mcq_mintime.inc) ----
// The collocation constants [REF opt_mintime.py:143-176]: Lagrange polynomials through tau = [0, the Gauss-Legendre points of degree 3 on (0, 1)],
// D their values at 1, C their derivatives at the points, B their integrals over [0, 1].  Computed once, in long double, from the monomial
// coefficients as numpy.poly1d holds them.
static const McqMtColl& mintime_coll()
{
    static const McqMtColl coll = [] {
        McqMtColl c;
        const long double s15 = sqrtl(15.0L) / 10.0L, tau[4] = {0.0L, 0.5L - s15, 0.5L, 0.5L + s15};
        for (int j = 0; j < 4; ++j) {
            long double p[4] = {0.0L, 0.0L, 0.0L, 1.0L};       // coefficients, highest power first, of the product so far (degree grows to 3)
            int deg = 0;
            for (int r = 0; r < 4; ++r) {
                if (r == j) continue;
                long double q[4] = {0.0L, 0.0L, 0.0L, 0.0L};
                const long double den = tau[j] - tau[r];
                for (int i = 3 - deg; i < 4; ++i) {
                    q[i - 1] += p[i] / den;
                    q[i] += -tau[r] * p[i] / den;
                }
                for (int i = 0; i < 4; ++i) p[i] = q[i];
                ++deg;
            }
            c.tau[j] = (double)tau[j];
            c.D[j] = (double)(p[0] + p[1] + p[2] + p[3]);
            c.B[j] = (double)(p[0] / 4.0L + p[1] / 3.0L + p[2] / 2.0L + p[3]);
            for (int r = 0; r < 4; ++r) c.C[j][r] = (double)((3.0L * p[0] * tau[r] + 2.0L * p[1]) * tau[r] + p[2]);
        }
        return c;
    }();
    return coll;
}

static int mintime_opts_bad(const mcq_mintime_opts* o)
{
    return !o || o->pwr_behavior != 0 || (o->friction != -1 && o->friction != MCQ_FRIC_LINEAR && o->friction != MCQ_FRIC_GAUSS) ||
           (o->friction == MCQ_FRIC_GAUSS && (o->n_gauss < 1 || o->n_gauss > 15));
}

extern "C" int mcq_mintime_layout(int N, const mcq_mintime_opts* opts, mcq_mintime_dims* out)
{
    if (N < 2 || !out || mintime_opts_bad(opts) || (long long)N * 31 + 64 > 0x7fffffffLL) {
        g_err = "mcq_mintime_layout: bad argument (N >= 2, no powertrain states, friction -1 / MCQ_FRIC_LINEAR / MCQ_FRIC_GAUSS with n_gauss 1 .. 15)";
        return MCQ_E_ARG;
    }
    const int safe = opts->safe_traj ? 1 : 0, energy = opts->limit_energy ? 1 : 0;
    memset(out, 0, sizeof(*out));
    out->nw = 5 + 24 * N;
    out->ng = mcq_mt_ng(N, safe, energy);
    out->off_x = 0; out->off_u = 5; out->off_xc = 9; out->stride_w = 24;
    out->rows_first = 27 + 2 * safe; out->rows_next = 31 + 2 * safe;
    out->row_colloc = 0; out->row_cont = 15; out->row_power = 20; out->row_kamm = 21; out->row_roll = 25; out->row_pedal = 26; out->row_act = 27;
    out->row_safe = safe ? 31 : -1;
    out->row_periodic = mcq_mt_row0(N, safe);
    out->row_energy = energy ? out->row_periodic + 5 : -1;
    const McqMtColl& c = mintime_coll();
    memcpy(out->tau, c.tau, sizeof(c.tau)); memcpy(out->C, c.C, sizeof(c.C)); memcpy(out->D, c.D, sizeof(c.D)); memcpy(out->B, c.B, sizeof(c.B));
    return 0;
}

// the checks the four device entries share, and the launch record they fill further
static int mintime_record(const char* who, mcq_handle* h, const mcq_mintime_data* d, const mcq_mintime_opts* o, bool need_w, McqMintime& M)
{
    if (!h || !d || mintime_opts_bad(o) || d->batch <= 0 || d->nmax < 2 || !d->pars || !d->w_tr_right_cl || !d->w_tr_left_cl ||
        (need_w && (!d->h || !d->kappa_cl || !d->w)) || (need_w && o->friction >= 0 && !d->w_mue) ||
        (need_w && o->friction == MCQ_FRIC_GAUSS && !d->center_dist)) {
        g_err = std::string(who) + ": bad argument";
        return MCQ_E_ARG;
    }
    if (d->batch > 65535 || (long long)d->nmax * MCQ_MT_JAC_LANES + 64 * MCQ_MT_JAC_LANES > 0x7fffffffLL) {
        g_err = std::string(who) + ": more problems or intervals than one launch holds";
        return MCQ_E_TOO_LARGE;
    }
    memset(&M, 0, sizeof(M));
    M.d = *d;
    M.o = *o;
    M.c = mintime_coll();
    M.P = o->friction < 0 ? 0 : (o->friction == MCQ_FRIC_LINEAR ? 2 : 2 * o->n_gauss + 2);
    M.nwmax = 5 + 24 * d->nmax;
    M.ngmax = mcq_mt_ng(d->nmax, o->safe_traj ? 1 : 0, o->limit_energy ? 1 : 0);
    return 0;
}

extern "C" int mcq_mintime_bounds_device(mcq_handle* h, const mcq_mintime_data* data, const mcq_mintime_opts* opts, double* w0_out, double* lbw_out,
                                         double* ubw_out, double* lbg_out, double* ubg_out)
{
    McqMintime M;
    if (int rc = mintime_record("mcq_mintime_bounds_device", h, data, opts, false, M)) return rc;
    if (!w0_out || !lbw_out || !ubw_out || !lbg_out || !ubg_out) {
        g_err = "mcq_mintime_bounds_device: bad argument";
        return MCQ_E_ARG;
    }
    HIP_TRY(hipSetDevice(h->device));
    M.w0 = w0_out; M.lbw = lbw_out; M.ubw = ubw_out; M.lbg = lbg_out; M.ubg = ubg_out;
    hipLaunchKernelGGL(mcq_mintime_bounds_kernel, dim3(data->batch), dim3(256), 0, compute_stream(h), M);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int mcq_mintime_eval_device(mcq_handle* h, const mcq_mintime_data* data, const mcq_mintime_opts* opts, double* g_out, double* J_out,
                                       double* lap_time_out, double* energy_out, double* x_opt_out, double* u_opt_out, double* tf_opt_out,
                                       double* dt_opt_out, double* ax_opt_out, double* ay_opt_out, double* ec_opt_out, int* status_out)
{
    McqMintime M;
    if (int rc = mintime_record("mcq_mintime_eval_device", h, data, opts, true, M)) return rc;
    if (!g_out || !J_out || !status_out) {
        g_err = "mcq_mintime_eval_device: bad argument";
        return MCQ_E_ARG;
    }
    HIP_TRY(hipSetDevice(h->device));
    const size_t bn = (size_t)data->batch * data->nmax;
    M.dt_own = dt_opt_out; M.ec_own = ec_opt_out;
    if (!dt_opt_out || !ec_opt_out) {
        if (int rc = grow(h, h->mintime, 2 * bn * sizeof(double))) return rc;
        if (!dt_opt_out) M.dt_own = (double*)h->mintime.p;
        if (!ec_opt_out) M.ec_own = (double*)h->mintime.p + bn;
    }
    M.g = g_out; M.J = J_out; M.lap = lap_time_out; M.energy = energy_out; M.x_opt = x_opt_out; M.u_opt = u_opt_out; M.tf_opt = tf_opt_out;
    M.dt_opt = dt_opt_out; M.ax_opt = ax_opt_out; M.ay_opt = ay_opt_out; M.ec_opt = ec_opt_out; M.status = status_out;
    const unsigned per_wg = 256 / MCQ_MT_EVAL_LANES;
    hipLaunchKernelGGL(mcq_mintime_eval_kernel, dim3(((unsigned)data->nmax + per_wg - 1) / per_wg, data->batch), dim3(256), 0, compute_stream(h), M);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(mcq_mintime_sum_kernel, dim3(data->batch), dim3(256), 0, compute_stream(h), M);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int mcq_mintime_jac_device(mcq_handle* h, const mcq_mintime_data* data, const mcq_mintime_opts* opts, double* blocks_out, double* grad_J_out,
                                      double* grad_energy_out)
{
    McqMintime M;
    if (int rc = mintime_record("mcq_mintime_jac_device", h, data, opts, true, M)) return rc;
    if (!blocks_out || !grad_J_out) {
        g_err = "mcq_mintime_jac_device: bad argument";
        return MCQ_E_ARG;
    }
    HIP_TRY(hipSetDevice(h->device));
    M.blocks = blocks_out; M.grad_J = grad_J_out; M.grad_E = grad_energy_out;
    const size_t lanes = (size_t)data->nmax * MCQ_MT_JAC_LANES;
    hipLaunchKernelGGL(mcq_mintime_jac_kernel, dim3((unsigned)((lanes + 255) / 256), data->batch), dim3(256), 0, compute_stream(h), M);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int mcq_mintime_kkt_device(mcq_handle* h, const mcq_mintime_data* data, const mcq_mintime_opts* opts, const double* g, const double* blocks,
                                      const double* grad_J, const double* grad_energy, const double* lam_g, const double* lam_x, const double* lbw,
                                      const double* ubw, const double* lbg, const double* ubg, double* r_out, double* kkt_out)
{
    McqMintime M;
    if (int rc = mintime_record("mcq_mintime_kkt_device", h, data, opts, true, M)) return rc;
    if (!g || !blocks || !grad_J || (opts->limit_energy && !grad_energy) || !lam_g || !lam_x || !lbw || !ubw || !lbg || !ubg || !r_out || !kkt_out) {
        g_err = "mcq_mintime_kkt_device: bad argument";
        return MCQ_E_ARG;
    }
    HIP_TRY(hipSetDevice(h->device));
    M.g_in = g; M.blocks_in = blocks; M.grad_J_in = grad_J; M.grad_E_in = grad_energy; M.lam_g = lam_g; M.lam_x = lam_x;
    M.lbw_in = lbw; M.ubw_in = ubw; M.lbg_in = lbg; M.ubg_in = ubg; M.r = r_out; M.kkt = kkt_out;
    hipLaunchKernelGGL(mcq_mintime_kkt_kernel, dim3(data->batch), dim3(256), 0, compute_stream(h), M);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int mcq_mintime_hess_device(mcq_handle* h, const mcq_mintime_data* data, const mcq_mintime_opts* opts, const double* lam_g,
                                       const double* sigma, double* hblocks_out)
{
    McqMintime M;
    if (int rc = mintime_record("mcq_mintime_hess_device", h, data, opts, true, M)) return rc;
    if (!lam_g || !hblocks_out) {
        g_err = "mcq_mintime_hess_device: bad argument";
        return MCQ_E_ARG;
    }
    HIP_TRY(hipSetDevice(h->device));
    M.lam_g = lam_g; M.sigma = sigma; M.hblocks = hblocks_out;
    hipLaunchKernelGGL(mcq_mintime_hess_kernel, dim3((unsigned)data->nmax, data->batch), dim3(MCQ_MT_HESS_NT), 0, compute_stream(h), M);
    HIP_TRY(hipGetLastError());
    return 0;
}

// (reads n_list alone of the launch's arrays: h, kappa_cl and w may be NULL)
extern "C" int mcq_mintime_hessvec_device(mcq_handle* h, const mcq_mintime_data* data, const mcq_mintime_opts* opts, const double* hblocks,
                                          const double* v, int nvec, double* y_out)
{
    McqMintime M;
    if (int rc = mintime_record("mcq_mintime_hessvec_device", h, data, opts, false, M)) return rc;
    if (!hblocks || !v || nvec <= 0 || !y_out) {
        g_err = "mcq_mintime_hessvec_device: bad argument";
        return MCQ_E_ARG;
    }
    HIP_TRY(hipSetDevice(h->device));
    M.hblocks_in = hblocks; M.v = v; M.nvec = nvec; M.y = y_out;
    hipLaunchKernelGGL(mcq_mintime_hessvec_kernel, dim3(((unsigned)M.nwmax + 255) / 256, data->batch), dim3(256), 0, compute_stream(h), M);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- the regularised primal-dual Newton step from the resident blocks (include/mcq.h; csrc/mcq_mtstep.inc) ----
extern "C" int mcq_mintime_step_bytes(int nmax, const mcq_mintime_opts* opts, int nvec, size_t* bytes_per_problem)
{
    if (nmax < 2 || nvec <= 0 || !bytes_per_problem || mintime_opts_bad(opts) || (long long)nmax * 64 + 64 > 0x7fffffffLL) {
        g_err = "mcq_mintime_step_bytes: bad argument";
        return MCQ_E_ARG;
    }
    const int nw = 5 + 24 * nmax, ng = mcq_mt_ng(nmax, opts->safe_traj ? 1 : 0, opts->limit_energy ? 1 : 0);
    *bytes_per_problem = mcq_mts_work(nmax, nvec, nw, ng) * sizeof(double);
    return 0;
}

extern "C" long long mcq_mintime_step_workspace(mcq_handle* h) { return h ? (long long)h->mtstep.bytes : 0; }

// (reads n_list alone of the launch's arrays, as mcq_mintime_hessvec_device does)
extern "C" int mcq_mintime_step_device(mcq_handle* h, const mcq_mintime_data* data, const mcq_mintime_opts* opts, const double* hblocks,
                                       const double* blocks, const double* grad_energy, const double* dw, const double* dg, const double* rhs,
                                       int nvec, int refine, double* sol_out, double* res_out, int* inertia_out, int* status_out)
{
    McqMintime M;
    if (int rc = mintime_record("mcq_mintime_step_device", h, data, opts, false, M)) return rc;
    if (!hblocks || !blocks || (opts->limit_energy && !grad_energy) || !dw || !dg || !rhs || nvec <= 0 || refine < 0 || !sol_out || !res_out ||
        !inertia_out || !status_out) {
        g_err = "mcq_mintime_step_device: bad argument";
        return MCQ_E_ARG;
    }
    if ((long long)nvec * ((long long)M.nwmax + M.ngmax) > 0x7fffffffLL) {
        g_err = "mcq_mintime_step_device: more right-hand sides than one launch holds";
        return MCQ_E_TOO_LARGE;
    }
    HIP_TRY(hipSetDevice(h->device));
    McqMtStep S;
    memset(&S, 0, sizeof(S));
    S.batch = data->batch; S.nmax = data->nmax; S.n_list = data->n_list;
    S.safe = opts->safe_traj ? 1 : 0; S.energy = opts->limit_energy ? 1 : 0; S.nwmax = M.nwmax; S.ngmax = M.ngmax; S.nvec = nvec; S.refine = refine;
    S.hblocks = hblocks; S.blocks = blocks; S.grad_energy = grad_energy; S.dw = dw; S.dg = dg; S.rhs = rhs;
    S.sol = sol_out; S.res = res_out; S.inertia = inertia_out; S.status = status_out;
    S.work_per = mcq_mts_work(S.nmax, nvec, S.nwmax, S.ngmax);
    if (int rc = grow(h, h->mtstep, (size_t)data->batch * S.work_per * sizeof(double))) return rc;
    S.work = (double*)h->mtstep.p;
    hipLaunchKernelGGL(mcq_mintime_step_kernel, dim3(data->batch), dim3(256), 0, compute_stream(h), S);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- device memory plumbing for callers that keep data resident between calls without a second HIP runtime in the
//      process (the Python IQP driver): plain allocate / free / copy on the handle's device and stream ------------------
extern "C" int mcq_device_alloc(mcq_handle* h, size_t bytes, void** out)
{
    if (!h || !out || bytes == 0) { g_err = "mcq_device_alloc: bad argument"; return MCQ_E_ARG; }
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipMalloc(out, bytes));
    HIP_TRY(hipMemsetAsync(*out, 0, bytes, compute_stream(h)));
    return 0;
}

extern "C" int mcq_device_free(mcq_handle* h, void* ptr)
{
    if (!h) { g_err = "mcq_device_free: NULL handle"; return MCQ_E_ARG; }
    if (!ptr) return 0;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(compute_stream(h)));
    if (h->comm_stream) HIP_TRY(hipStreamSynchronize(h->comm_stream));      // (a gather in flight may read or write the buffer)
    HIP_TRY(hipFree(ptr));
    return 0;
}

extern "C" int mcq_copy_to_device(mcq_handle* h, void* dst, const void* src, size_t bytes)
{
    if (!h || !dst || !src) { g_err = "mcq_copy_to_device: bad argument"; return MCQ_E_ARG; }
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, compute_stream(h)));
    HIP_TRY(hipStreamSynchronize(compute_stream(h)));          // the host buffer may be reused on return
    return 0;
}

extern "C" int mcq_copy_to_host(mcq_handle* h, void* dst, const void* src, size_t bytes)
{
    if (!h || !dst || !src) { g_err = "mcq_copy_to_host: bad argument"; return MCQ_E_ARG; }
    HIP_TRY(hipSetDevice(h->device));
    // a gather enqueued before this copy may be writing `src` on the comm stream: the copy is ordered behind the latest one (ADVICE r4:
    // parallel.solve_sharded read its receive buffer before the gather had finished)
    if (h->comm_stream && h->comm_seq > 0) HIP_TRY(hipStreamWaitEvent(compute_stream(h), h->comm_done[(h->comm_seq - 1) & 3u], 0));
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, compute_stream(h)));
    HIP_TRY(hipStreamSynchronize(compute_stream(h)));
    return 0;
}

extern "C" int mcq_sync(mcq_handle* h)
{
    if (!h) { g_err = "mcq_sync: NULL handle"; return MCQ_E_ARG; }
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(compute_stream(h)));
    if (h->comm_stream) HIP_TRY(hipStreamSynchronize(h->comm_stream));      // gathers in flight (mcq_comm_allgather) are work of the handle too
    if (h->ws[1].stream) HIP_TRY(hipStreamSynchronize(h->ws[1].stream));
    return 0;
}

// (From here on the caller may enqueue on the stream what the handle does not see: mcq_solve_device keeps to the one launch on this handle.)
extern "C" void* mcq_stream(mcq_handle* h)
{
    if (!h) return nullptr;
    h->stream_given = true;
    return (void*)compute_stream(h);
}

extern "C" int mcq_last_timing(mcq_handle* h, float ms[5])
{
    if (!h || !ms || !h->timing_valid) { g_err = "mcq_last_timing: no timed launch"; return MCQ_E_ARG; }
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipEventSynchronize(h->ev[4]));
    HIP_TRY(hipEventElapsedTime(&ms[0], h->ev[0], h->ev[1]));      // shortest path: mcq_assemble_sp_kernel; otherwise the gap between two event records
    ms[1] = 0.0f;                                                   // (no such kernel since round 4)
    HIP_TRY(hipEventElapsedTime(&ms[2], h->ev[2], h->ev[3]));
    ms[3] = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms[4], h->ev[0], h->ev[4]));
    if (h->sl.time1) {
        // a sliced mcq_solve_device: from slice 0's start to the later of the two slices' ends (neither stream has waited for the other)
        float to1 = 0.0f;
        HIP_TRY(hipEventSynchronize(h->sl.time1));
        HIP_TRY(hipEventElapsedTime(&to1, h->ev[2], h->sl.time1));
        ms[2] = std::max(ms[2], to1);
        HIP_TRY(hipEventElapsedTime(&to1, h->ev[0], h->sl.time1));
        ms[4] = std::max(ms[4], to1);
    }
    return 0;
}

// A span of calls on the handle, timed on the device (include/mcq.h).  It begins behind everything enqueued so far, on both compute streams
// (compute_stream; the first sliced call of the span joins ws[1].stream behind the begin event), and ends with the later of the two streams.
extern "C" int mcq_timing_begin(mcq_handle* h)
{
    if (!h) { g_err = "mcq_timing_begin: NULL handle"; return MCQ_E_ARG; }
    HIP_TRY(hipSetDevice(h->device));
    for (int k = 0; k < 2; ++k) if (!h->ev_span[k]) HIP_TRY(hipEventCreate(&h->ev_span[k]));
    HIP_TRY(hipEventRecord(h->ev_span[0], compute_stream(h)));
    h->span_launches = 0;
    h->span_open = true;
    return 0;
}

extern "C" int mcq_timing_end(mcq_handle* h, float* ms_out, int* launches_out)
{
    if (!h || !ms_out || !launches_out) { g_err = "mcq_timing_end: bad argument"; return MCQ_E_ARG; }
    if (!h->span_open) { g_err = "mcq_timing_end: no span open (mcq_timing_begin)"; return MCQ_E_ARG; }
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipEventRecord(h->ev_span[1], h->ws[0].stream));
    HIP_TRY(hipEventSynchronize(h->ev_span[1]));
    HIP_TRY(hipEventElapsedTime(ms_out, h->ev_span[0], h->ev_span[1]));
    if (h->sl.last1) {         // slices pending on ws[1].stream: an end event there as well, neither stream waiting for the other
        float ms1 = 0.0f;
        if (!h->ev_span1) HIP_TRY(hipEventCreate(&h->ev_span1));
        HIP_TRY(hipEventRecord(h->ev_span1, h->ws[1].stream));
        HIP_TRY(hipEventSynchronize(h->ev_span1));
        HIP_TRY(hipEventElapsedTime(&ms1, h->ev_span[0], h->ev_span1));
        *ms_out = std::max(*ms_out, ms1);
    }
    *launches_out = h->span_launches;
    h->span_open = false;
    return 0;
}

extern "C" int mcq_last_upload_was_direct(mcq_handle* h) { return h ? h->last_upload_direct : 0; }

extern "C" long long mcq_workspace_bytes(mcq_handle* h) { return h ? h->ws[0].bytes + h->gi_bytes + h->gis_bytes + h->ws[1].bytes : 0; }

static int ensure_pin(mcq_handle* h, size_t bytes)
{
    if (bytes <= h->pin_bytes) return 0;
    HIP_TRY(hipStreamSynchronize(compute_stream(h)));
    if (h->pin) (void)hipHostFree(h->pin);
    h->pin = nullptr;
    h->pin_bytes = 0;
    HIP_TRY(hipHostMalloc(&h->pin, bytes, hipHostMallocDefault));
    if (h->poison) memset(h->pin, 0xff, bytes);
    h->pin_bytes = bytes;
    return 0;
}

// fn(t, i0, i1) for the nthreads sub-ranges [i0, i1) of [lo, hi): sub-range 0 on the caller, the others on threads of their own -- and those no
// thread could be had for on the caller as well, behind its own.  Returns when all are done.
template <class F> static void fan_out(int lo, int hi, int nthreads, F fn)
{
    auto run = [=](int t) { fn(t, lo + (int)((long long)(hi - lo) * t / nthreads), lo + (int)((long long)(hi - lo) * (t + 1) / nthreads)); };
    std::vector<std::thread> th;
    int taken = 1;          // sub-ranges 0 .. taken - 1 have a thread (0: this one)
    try {
        for (; taken < nthreads; ++taken) th.emplace_back(run, taken);
    } catch (...) {}
    run(0);
    for (int t = taken; t < nthreads; ++t) run(t);
    for (auto& t : th) t.join();
}

// host-side time stamps of one call on stderr, where the environment names `env` ($MCQ_PIPE_TRACE, $MCQ_IQP_TRACE): fmt takes `what`, then
// the ms since the record was made
struct Stamps {
    bool on;
    struct timespec t0;
    explicit Stamps(const char* env) : on(getenv(env) != nullptr) { clock_gettime(CLOCK_MONOTONIC, &t0); }
    template <class T> void at(const char* fmt, T what) const
    {
        if (!on) return;
        struct timespec t1;
        clock_gettime(CLOCK_MONOTONIC, &t1);
        fprintf(stderr, fmt, what, (t1.tv_sec - t0.tv_sec) * 1e3 + (t1.tv_nsec - t0.tv_nsec) * 1e-6);
    }
};

// ---- the n spline scalings out of the dense matrix the reference passes (include/mcq.h); host code, no GPU ----------------------------------
// closed: calc_splines' closed system through n waypoints, [4n][4n]; open: its open system, [4(n-1)][4(n-1)] with 12 n - 15 non-zeros, whose
// last block holds the two heading rows and whose s_out ends in two ones.
static int les_scalings(const double* A, int n, double* s_out, int check, bool closed)
{
    const char* name = closed ? "mcq_les_scalings" : "mcq_les_scalings_open";
    if (!A || !s_out || n < 3) { g_err = std::string(name) + ": bad argument"; return MCQ_E_ARG; }
    const int ns = closed ? n : n - 1;          // splines
    const size_t m = (size_t)4 * ns;
    for (int i = 0; i + 1 < ns; ++i) s_out[i] = -A[((size_t)4 * i + 2) * m + 4 * i + 5];
    if (closed) s_out[n - 1] = A[(m - 2) * m + 1];
    else s_out[n - 2] = s_out[n - 1] = 1.0;
    if (!check) return 0;
    // Row by row: the entries the system has in that row, at their values (the closed system's wrap-around rows carry the
    // opposite sign), and NOTHING else -- a row's non-zeros are counted while it streams through.
    // one thread per 16 MB of matrix, 32 at most (512 MB at n = 2000: 3.4 ms on 8 threads of the bench host, memory-bound); $MCQ_PACK_THREADS overrides
    int nthreads = (int)std::min<size_t>(32, std::max<size_t>(1, (m * m * sizeof(double)) >> 24));
    if (const char* e = getenv("MCQ_PACK_THREADS")) nthreads = atoi(e);
    const int hw = (int)std::thread::hardware_concurrency();
    if (hw > 0 && nthreads > hw) nthreads = hw;
    if (nthreads > ns) nthreads = ns;
    if (nthreads < 1) nthreads = 1;
    std::vector<long long> bad((size_t)nthreads, -1);          // first offending (row * m + column) of a thread's blocks
    auto rel = [](double a, double b) { return fabs(a - b) <= 1e-12 * fabs(b); };
    fan_out(0, ns, nthreads, [&](int t, int i0, int i1) {
        for (int i = i0; i < i1 && bad[t] < 0; ++i) {
            const size_t j = (size_t)4 * i;
            const bool last = i == ns - 1;
            const double s = last && !closed ? 1.0 : s_out[i];
            if (!(s > 0.0) || !std::isfinite(s)) { bad[t] = (long long)((j + 2) * m + (last ? 1 : j + 5)); break; }
            for (int r = 0; r < 4; ++r) {
                const double* row = A + (j + r) * m;
                size_t nz = 0;
                for (size_t c = 0; c < m; ++c) nz += row[c] != 0.0;
                bool ok;
                if (r == 0) ok = nz == 1 && row[j] == 1.0;
                else if (r == 1) ok = nz == 4 && row[j] == 1.0 && row[j + 1] == 1.0 && row[j + 2] == 1.0 && row[j + 3] == 1.0;
                else if (r == 2 && !last) ok = nz == 4 && row[j + 1] == 1.0 && row[j + 2] == 2.0 && row[j + 3] == 3.0 && row[j + 5] == -s;
                else if (r == 2) ok = closed ? nz == 4 && row[j + 1] == -1.0 && row[j + 2] == -2.0 && row[j + 3] == -3.0 && row[1] == s
                                             : nz == 1 && row[1] == 1.0;                                        // heading at the start
                else if (!last) ok = nz == 3 && row[j + 2] == 2.0 && row[j + 3] == 6.0 && rel(-row[j + 6], 2.0 * s * s);
                else ok = nz == 3 && (closed ? row[j + 2] == -2.0 && row[j + 3] == -6.0 && rel(row[2], 2.0 * s * s)
                                             : row[j + 1] == 1.0 && row[j + 2] == 2.0 && row[j + 3] == 3.0);    // ... at the end
                if (!ok) { bad[t] = (long long)((j + r) * m); break; }
            }
        }
    });
    for (int t = 0; t < nthreads; ++t) {
        if (bad[t] >= 0) {
            char buf[160];
            snprintf(buf, sizeof buf, "%s: row %lld of A does not have the structure of calc_splines' %s-spline system", name, bad[t] / (long long)m,
                     closed ? "closed" : "open");
            g_err = buf;
            return MCQ_E_ARG;
        }
    }
    return 0;
}

extern "C" int mcq_les_scalings(const double* A, int n, double* s_out, int check) { return les_scalings(A, n, s_out, check, true); }

extern "C" int mcq_les_scalings_open(const double* A, int n, double* s_out, int check) { return les_scalings(A, n, s_out, check, false); }

extern "C" int mcq_host_alloc(mcq_handle* h, size_t bytes, void** out)
{
    if (!h || !out || bytes == 0) { g_err = "mcq_host_alloc: bad argument"; return MCQ_E_ARG; }
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipHostMalloc(out, bytes, hipHostMallocDefault));
    return 0;
}

extern "C" int mcq_host_free(mcq_handle* h, void* ptr)
{
    if (!h) { g_err = "mcq_host_free: NULL handle"; return MCQ_E_ARG; }
    if (!ptr) return 0;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(compute_stream(h)));
    HIP_TRY(hipHostFree(ptr));
    return 0;
}

// rows [row0, row0 + rows) of n waypoints each, from the host arrays ref / nv / sc (whole, [batch][n][*]; nv, sc: or nullptr) into staging set s
static int upload_rows(mcq_handle* h, const Staging& s, const double* ref, const double* nv, const double* sc, size_t row0, size_t rows, size_t n,
                       hipStream_t st)
{
    const size_t off = row0 * n, cnt = rows * n;
    HIP_TRY_DRAIN(hipMemcpyAsync(s.ref + off * 4, ref + off * 4, cnt * 4 * sizeof(double), hipMemcpyHostToDevice, st));
    if (nv) HIP_TRY_DRAIN(hipMemcpyAsync(s.nv + off * 2, nv + off * 2, cnt * 2 * sizeof(double), hipMemcpyHostToDevice, st));
    if (sc) HIP_TRY_DRAIN(hipMemcpyAsync(s.sc + off, sc + off, cnt * sizeof(double), hipMemcpyHostToDevice, st));
    return 0;
}

// Slice k = problems b0 .. b1 - 1 of B, whose uploads have just been queued on h->cp.in: its kernel behind them on the slice's compute stream,
// its rows of alpha (B.nmax each) behind the kernel on h->cp.out into alpha_host ([batch][nmax], the caller's array or the pinned staging).
static int launch_slice(mcq_handle* h, const McqBatch& B, int k, int b0, int b1, double* alpha_host)
{
    HIP_TRY_DRAIN(hipEventRecord(h->cp.slice[k], h->cp.in));
    hipStream_t st = h->ws[k & 1].stream;          // the handle's two, in turn (a stream per slice was slower: docs/NOTEBOOK.md R6.5)
    HIP_TRY_DRAIN(hipStreamWaitEvent(st, h->cp.slice[k], 0));
    if (int rc = enqueue_solve(h, B, st, b0, b1, false)) { drain(h); return rc; }
    HIP_TRY_DRAIN(hipEventRecord(h->cp.slice[8 + k], st));
    HIP_TRY_DRAIN(hipStreamWaitEvent(h->cp.out, h->cp.slice[8 + k], 0));
    const size_t off = (size_t)b0 * B.nmax, cnt = (size_t)(b1 - b0) * B.nmax;
    HIP_TRY_DRAIN(hipMemcpyAsync(alpha_host + off, B.alpha + off, cnt * sizeof(double), hipMemcpyDeviceToHost, h->cp.out));
    return 0;
}

// The results of a host-buffer batch, from staging set 0 to the host on `st`: alpha_bytes of alpha (alpha_dst == nullptr: it went down slice by
// slice), curv_error, status, and the info records where the caller wants them.
static int download_results(mcq_handle* h, hipStream_t st, int batch, void* alpha_dst, const void* alpha_src, size_t alpha_bytes,
                            double* curv_err_dst, int* status_dst, mcq_info* info_dst)
{
    if (alpha_dst) HIP_TRY_DRAIN(hipMemcpyAsync(alpha_dst, alpha_src, alpha_bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY_DRAIN(hipMemcpyAsync(curv_err_dst, h->stage[0].curv, batch * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY_DRAIN(hipMemcpyAsync(status_dst, h->stage[0].status, batch * sizeof(int), hipMemcpyDeviceToHost, st));
    if (info_dst) HIP_TRY_DRAIN(hipMemcpyAsync(info_dst, h->d_info, batch * sizeof(mcq_info), hipMemcpyDeviceToHost, st));
    return 0;
}

// ---- how a host batch goes up: per-problem buffers through the handle's pinned staging ([batch][nmax][*]) or straight from where they lie ----
// What the entry states, then what plan_upload decides once per call; the loop over chunks [b0, b1) of problems (upload_chunk) is the caller's.
struct Upload {
    const mcq_problem* probs;   // nullptr: a UNIFORM batch (mcq_solve_host) -- ref / nv / sc are the caller's arrays, read as they lie, one chunk
    int batch;
    size_t nmax;
    bool any_sc, with_nv;
    double *ref, *nv, *sc, *alpha, *kb, *wv;       // the pinned block: ref | nv | sc | alpha | kb | wv | info | n   (then the entry's extra bytes)
    mcq_info* info;
    int* n;
    bool direct;                // no packing pass: strided copies from the caller's page-locked arrays
    int nthreads, nchunks;      // of the packing pass where the entry does not slice (a direct batch: one chunk)
    void* extra;                // the entry's extra bytes, 8-byte aligned
};

// the per-problem scalars of a ragged host batch, through the pinned block to the device on `up`
static int upload_scalars(mcq_handle* h, const Upload& U, hipStream_t up)
{
    if (!U.probs) return 0;         // (a uniform batch: its scalars are arguments of the launch)
    for (int b = 0; b < U.batch; ++b) { U.kb[b] = U.probs[b].kappa_bound; U.wv[b] = U.probs[b].w_veh; U.n[b] = U.probs[b].n; }
    HIP_TRY_DRAIN(hipMemcpyAsync(h->d_kb, U.kb, U.batch * sizeof(double), hipMemcpyHostToDevice, up));
    HIP_TRY_DRAIN(hipMemcpyAsync(h->d_wv, U.wv, U.batch * sizeof(double), hipMemcpyHostToDevice, up));
    HIP_TRY_DRAIN(hipMemcpyAsync(h->d_n, U.n, U.batch * sizeof(int), hipMemcpyHostToDevice, up));
    return 0;
}

// lays out the pinned block and decides how the batch goes up; enqueues nothing
static int plan_upload(mcq_handle* h, Upload& U, size_t extra_bytes)
{
    const mcq_problem* probs = U.probs;
    const int batch = U.batch;
    const bool with_nv = U.with_nv;
    const size_t elems = (size_t)batch * U.nmax;
    const size_t bytes = elems * (4 + 2 + 1 + 1) * sizeof(double) + (size_t)batch * (2 * sizeof(double) + sizeof(int) + sizeof(mcq_info)) + 64 + extra_bytes;
    if (int rc = ensure_pin(h, bytes)) return rc;
    U.ref = (double*)h->pin;
    U.nv = U.ref + elems * 4;
    U.sc = U.nv + elems * 2;
    U.alpha = U.sc + elems;
    U.kb = U.alpha + elems;
    U.wv = U.kb + batch;
    U.info = (mcq_info*)(U.wv + batch);
    U.n = (int*)(U.info + batch);
    U.extra = (char*)h->pin + ((size_t)((char*)(U.n + batch) - (char*)h->pin) + 7) / 8 * 8;       // (within the 64 bytes of slack)
    // ---- no packing at all (round 6): a UNIFORM batch that lies in the caller's memory as one contiguous, page-locked block per array (what
    //      engine.py hands over for stacked arrays from mcq_host_alloc) goes to the device straight from there -- one strided copy per array
    //      (rows of n waypoints into rows of nmax) instead of a 115 MB memcpy into the staging first: that memcpy was 4-6 ms of a 36-42 ms
    //      mcq_iqp_batch call and the part of it that differs from host to host.  $MCQ_PACK_ALWAYS=1: the packing pass (A/B knob). ----
    const int n0 = probs[0].n;
    bool direct = batch >= 2 && n0 > 0 && !getenv("MCQ_PACK_ALWAYS");
    for (int b = 1; b < batch && direct; ++b) {
        direct = probs[b].n == n0 && probs[b].reftrack == probs[0].reftrack + (size_t)b * n0 * 4
                 && (!with_nv || probs[b].normvec == probs[0].normvec + (size_t)b * n0 * 2)
                 && (probs[0].scaling ? probs[b].scaling == probs[0].scaling + (size_t)b * n0 : probs[b].scaling == nullptr);
    }
    auto pinned = [](const void* p) {
        hipPointerAttribute_t a;
        if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
        return a.type == hipMemoryTypeHost;
    };
    U.direct = direct && pinned(probs[0].reftrack) && (!with_nv || pinned(probs[0].normvec)) && (!probs[0].scaling || pinned(probs[0].scaling));
    h->last_upload_direct = U.direct ? 1 : 0;
    // A large batch (the 1024 N = 2000 tracks of the bench: 115 MB) is packed in four chunks of tracks by several host threads, and a
    // chunk's uploads are queued as soon as it is packed: one thread copies at ~10 GB/s -- 11 ms, a quarter of the whole mcq_iqp_batch
    // call -- and the DMA of chunk k runs while chunk k + 1 is packed.  $MCQ_PACK_THREADS: threads (default 8 for batches above 8 MB; 1 = the single loop).
    const size_t row_doubles = 4 + (with_nv ? 2 : 0) + (U.any_sc ? 1 : 0);
    const size_t payload = elems * row_doubles * sizeof(double);
    const char* pt = getenv("MCQ_PACK_THREADS");
    const bool forced = pt && *pt;          // (asked for explicitly: whatever the size of the batch -- the tests pack six small tracks on three threads)
    int nthreads = forced ? atoi(pt) : (payload > ((size_t)8 << 20) && batch >= 16 ? 8 : 1);
    const int hw = (int)std::thread::hardware_concurrency();
    if (hw > 0 && nthreads > hw) nthreads = hw;
    if (nthreads > batch) nthreads = batch;
    if (nthreads < 1) nthreads = 1;
    U.nthreads = nthreads;
    U.nchunks = U.direct ? 1 : std::min(batch, (forced && nthreads > 1) || (payload > ((size_t)32 << 20) && batch >= 16) ? 4 : 1);
    return 0;
}

// problems [b0, b1) of the batch into staging set 0 on `up`: straight from the caller's arrays, or packed into the pinned block (by the plan's
// threads; the padding behind a track's n waypoints is never read by a kernel: no need to clear it) and copied from there
static int upload_chunk(mcq_handle* h, const Upload& U, int b0, int b1, hipStream_t up)
{
    const Staging& s = h->stage[0];
    const mcq_problem* probs = U.probs;
    const size_t nmax = U.nmax;
    if (U.direct) {
        const size_t w = (size_t)probs[0].n * sizeof(double), pitch = nmax * sizeof(double), rows = (size_t)(b1 - b0);
        HIP_TRY_DRAIN(hipMemcpy2DAsync(s.ref + (size_t)b0 * nmax * 4, pitch * 4, probs[b0].reftrack, w * 4, w * 4, rows, hipMemcpyHostToDevice, up));
        if (U.with_nv) HIP_TRY_DRAIN(hipMemcpy2DAsync(s.nv + (size_t)b0 * nmax * 2, pitch * 2, probs[b0].normvec, w * 2, w * 2, rows, hipMemcpyHostToDevice, up));
        if (U.any_sc) HIP_TRY_DRAIN(hipMemcpy2DAsync(s.sc + (size_t)b0 * nmax, pitch, probs[b0].scaling, w, w, rows, hipMemcpyHostToDevice, up));
        return 0;
    }
    if (probs) fan_out(b0, b1, U.nthreads, [&](int, int r0, int r1) {
        for (int b = r0; b < r1; ++b) {
            const size_t n = (size_t)probs[b].n;
            memcpy(U.ref + (size_t)b * nmax * 4, probs[b].reftrack, n * 4 * sizeof(double));
            if (U.with_nv) memcpy(U.nv + (size_t)b * nmax * 2, probs[b].normvec, n * 2 * sizeof(double));
            if (U.any_sc) {
                if (probs[b].scaling) memcpy(U.sc + (size_t)b * nmax, probs[b].scaling, n * sizeof(double));
                else for (size_t q = 0; q < n; ++q) U.sc[(size_t)b * nmax + q] = 1.0;
            }
        }
    });
    return upload_rows(h, s, U.ref, U.with_nv ? U.nv : nullptr, U.any_sc ? U.sc : nullptr, (size_t)b0, (size_t)(b1 - b0), nmax, up);
}

// the whole batch on the compute stream, for the one launch behind it (mcq_solve_batch unsliced, mcq_iqp_batch)
static int upload_batch(mcq_handle* h, const Upload& U)
{
    hipStream_t up = compute_stream(h);
    if (U.direct) { if (int rc = upload_scalars(h, U, up)) return rc; }        // (a direct batch's scalars have always gone first)
    for (int k = 0; k < U.nchunks; ++k)
        if (int rc = upload_chunk(h, U, split_at(U.batch, k, U.nchunks), split_at(U.batch, k + 1, U.nchunks), up)) return rc;
    if (!U.direct) { if (int rc = upload_scalars(h, U, up)) return rc; }       // (a packed batch's follow the rows)
    return 0;
}

// A host-buffer batch through staging set 0, in slices or as one launch (slices_for): U says how its rows go up, alpha comes back into
// alpha_host ([batch][nmax]: the caller's array or the pinned staging), the small arrays into the caller's.  Returns with all of it done.
// In SLICES the upload (and packing) of slice k + 1 and the download of slice k - 1 run while slice k's kernel does -- a copy stream each way,
// the kernels on the two compute streams in turn, all on disjoint rows of the ONE workspace (McqBatch.pb0): bitwise the one launch.  No
// event timing then: no pair of events spans the slices' kernels.
static int solve_staged(mcq_handle* h, McqBatch& B, const mcq_opts& o, const Upload& U, double* alpha_host, double* curv_out, int* status_out,
                        mcq_info* info_host)
{
    const int batch = B.batch, nsl = slices_for(h, ENTRY_HOST, batch, B.nmax, o);
    if (nsl == 1) {
        if (int rc = upload_batch(h, U)) return rc;
        if (int rc = launch(h, B, o)) { drain(h); return rc; }
        hipStream_t st = compute_stream(h);
        if (int rc = download_results(h, st, batch, alpha_host, B.alpha, (size_t)batch * B.nmax * sizeof(double), curv_out, status_out, info_host)) return rc;
        HIP_TRY(hipStreamSynchronize(st));
        return 0;
    }
    if (int rc = ensure_streams(h, COPY_STREAMS | SECOND_STREAM | SLICE_EVENTS)) return rc;
    HIP_TRY(hipStreamSynchronize(compute_stream(h)));          // whatever ran before on the handle is done with the staging buffers and the workspace
    HIP_TRY(hipStreamSynchronize(h->ws[1].stream));
    if (int rc = prepare(h, B, o, h->ws[0])) return rc;
    int rc = upload_scalars(h, U, h->cp.in);                   // the slices' kernels read the per-problem scalars: first
    for (int k = 0; k < nsl && !rc; ++k) {
        const int b0 = split_at(batch, k, nsl), b1 = split_at(batch, k + 1, nsl);
        rc = upload_chunk(h, U, b0, b1, h->cp.in);
        if (!rc) rc = launch_slice(h, B, k, b0, b1, alpha_host);
    }
    if (rc) { drain(h); return rc; }
    // (cp.out is behind every slice's kernel now: the small arrays follow the last slice's alpha)
    if ((rc = download_results(h, h->cp.out, batch, nullptr, nullptr, 0, curv_out, status_out, info_host))) return rc;
    HIP_TRY_DRAIN(hipStreamSynchronize(h->cp.out));
    HIP_TRY_DRAIN(hipStreamSynchronize(compute_stream(h)));
    HIP_TRY_DRAIN(hipStreamSynchronize(h->ws[1].stream));
    note_solve(h, B, false, nullptr);
    return 0;
}

extern "C" int mcq_solve_host(mcq_handle* h, int batch, int n, const double* reftrack, const double* normvec,
                              const double* scaling, double kappa_bound, double w_veh, const mcq_opts* opts, double* alpha_out,
                              double* curv_err_out, int* status_out, mcq_info* info_out)
{
    if (!h || batch <= 0 || n <= 0 || !reftrack || !alpha_out || !curv_err_out || !status_out) {
        g_err = "mcq_solve_host: bad argument";
        return MCQ_E_ARG;
    }
    HIP_TRY(hipSetDevice(h->device));
    const mcq_opts o = resolve_opts(opts);
    int rc = ensure_workspace(h, 0, (size_t)batch, (size_t)n);
    if (rc) return rc;
    rc = ensure_staging(h, 0, (size_t)batch, (size_t)n);
    if (rc) return rc;
    const Staging& s = h->stage[0];
    McqBatch B = make_batch(batch, n, nullptr, s.ref, normvec ? s.nv : nullptr, scaling ? s.sc : nullptr, s.alpha, s.curv, s.status,
                            info_out ? h->d_info : nullptr, kappa_bound, w_veh);
    // uniform: the caller's arrays as they lie, read only (nothing is packed into them), one chunk
    Upload U = {nullptr, batch, (size_t)n, scaling != nullptr, normvec != nullptr, const_cast<double*>(reftrack), const_cast<double*>(normvec),
                const_cast<double*>(scaling)};
    U.nchunks = 1;
    return solve_staged(h, B, o, U, alpha_out, curv_err_out, status_out, info_out);
}

// Host-buffer fp32 entry (mcq_solve_batch_f32): float rows in, float alpha out -- half the PCIe bytes of the
// fp64 entry.  The float rows land in the staging buffer of the (unused) normals -- batch * n * 2 doubles = batch * n * 4 floats --,
// the float alpha in the one of the scalings; the fp64 rows are rebuilt next to them (solve_f32_rows).
extern "C" int mcq_solve_batch_f32(mcq_handle* h, int batch, int n, int layout, const float* reftrack, const double* origin,
                                   double kappa_bound, double w_veh, const mcq_opts* opts, float* alpha_out, double* curv_err_out,
                                   int* status_out, mcq_info* info_out)
{
    if (!h || batch <= 0 || n <= 0 || !reftrack || !alpha_out || !curv_err_out || !status_out ||
        (layout != MCQ_F32_ABSOLUTE && layout != MCQ_F32_INCREMENTS)) {
        g_err = "mcq_solve_batch_f32: bad argument";
        return MCQ_E_ARG;
    }
    HIP_TRY(hipSetDevice(h->device));
    const mcq_opts o = resolve_opts(opts);
    int rc = ensure_workspace(h, 0, (size_t)batch, (size_t)n);
    if (rc) return rc;
    rc = ensure_staging(h, 0, (size_t)batch, (size_t)n);
    if (rc) return rc;
    const size_t elems = (size_t)batch * n;
    hipStream_t st = compute_stream(h);
    float* d_rows = (float*)h->stage[0].nv;
    float* d_al32 = (float*)h->stage[0].sc;
    HIP_TRY_DRAIN(hipMemcpyAsync(d_rows, reftrack, elems * 4 * sizeof(float), hipMemcpyHostToDevice, st));
    if (origin) HIP_TRY_DRAIN(hipMemcpyAsync(h->d_org, origin, (size_t)batch * 2 * sizeof(double), hipMemcpyHostToDevice, st));
    rc = solve_f32_rows(h, batch, n, layout, d_rows, origin ? h->d_org : nullptr, kappa_bound, w_veh, o, d_al32, h->stage[0].curv, h->stage[0].status,
                        info_out ? h->d_info : nullptr);
    if (rc) { drain(h); return rc; }
    rc = download_results(h, st, batch, alpha_out, d_al32, elems * sizeof(float), curv_err_out, status_out, info_out);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

// ---- a stream of uniform host batches with the PCIe behind the kernels (include/mcq.h) ------------------------------------------
// What the two step entries (mcq_solve_host_pipelined, mcq_solve_device_stream) share.  Kernels of odd steps on the second compute stream /
// workspace ($MCQ_PIPE_ONE_STREAM: the A/B knob); MCQ_ALG_GI stays on one stream: its slots (one per resident workgroup) belong to the first
// workspace (the second one's few slots made odd steps run ~32 problems at a time)
static bool two_step_streams(int steps, const mcq_opts& o) { return steps > 1 && !getenv("MCQ_PIPE_ONE_STREAM") && o.algorithm != MCQ_ALG_GI; }

static int check_step_list(const char* who, int steps, const double* const* reftrack, double* const* alpha_out, double* const* curv_err_out,
                           int* const* status_out)
{
    for (int k = 0; k < steps; ++k)
        if (!reftrack[k] || !alpha_out[k] || !curv_err_out[k] || !status_out[k]) { g_err = std::string(who) + ": NULL buffer in step list"; return MCQ_E_ARG; }
    return 0;
}

extern "C" int mcq_solve_host_pipelined(mcq_handle* h, int steps, int batch, int n, const double* const* reftrack,
                                        const double* const* normvec, const double* const* scaling, double kappa_bound, double w_veh,
                                        const mcq_opts* opts, double* const* alpha_out, double* const* curv_err_out,
                                        int* const* status_out)
{
    if (!h || steps <= 0 || batch <= 0 || n <= 0 || !reftrack || !alpha_out || !curv_err_out || !status_out) {
        g_err = "mcq_solve_host_pipelined: bad argument";
        return MCQ_E_ARG;
    }
    if (int rc = check_step_list("mcq_solve_host_pipelined", steps, reftrack, alpha_out, curv_err_out, status_out)) return rc;
    HIP_TRY(hipSetDevice(h->device));
    const mcq_opts o = resolve_opts(opts);
    int rc = ensure_workspace(h, 0, (size_t)batch, (size_t)n);
    if (rc) return rc;
    rc = ensure_staging(h, 0, (size_t)batch, (size_t)n);
    if (rc) return rc;
    rc = ensure_streams(h, COPY_STREAMS | STEP_EVENTS);
    if (rc) return rc;
    rc = ensure_staging(h, 1, (size_t)batch, (size_t)n);
    if (rc) return rc;
    // curv_error / status of every step land in PINNED memory of the handle and reach the caller's arrays at the end: a device-to-host copy into
    // pageable memory -- what these two small arrays usually are -- blocks the host until the step's kernels have finished, i.e. the host could
    // not enqueue step k + 1 before step k was over (round 5: this was the 0.5 ms per step that rounds 3-4 reported as "not hidden")
    rc = ensure_pin(h, (size_t)steps * batch * (sizeof(double) + sizeof(int)));
    if (rc) return rc;
    double* pin_cu = (double*)h->pin;
    int* pin_st = (int*)(pin_cu + (size_t)steps * batch);
    const bool two = two_step_streams(steps, o);
    if (two) { rc = ensure_workspace(h, 1, (size_t)batch, (size_t)n); if (rc) return rc; }
    HIP_TRY(hipStreamSynchronize(compute_stream(h)));          // whatever ran before on the handle's stream is done with the staging buffers
    const size_t elems = (size_t)batch * n;
    // Order of the host's enqueues: upload(0); then per step  kernels(k), upload(k + 1), download(k).  The copies of both directions
    // drain through one in-order copy queue of the runtime (rocprofv3 --memory-copy-trace, round 3: with download(k) enqueued ahead
    // of upload(k + 1) the upload sat behind it, i.e. behind the kernels of step k, and nothing overlapped): the upload of the NEXT
    // step therefore goes in first -- it only depends on kernels two steps back -- and runs while step k computes.
    auto upload = [&](int k) -> int {
        const int s = k & 1;
        // the kernels of step k - 2 were the last readers of this slot's rows
        if (k >= 2) HIP_TRY_DRAIN(hipStreamWaitEvent(h->cp.in, h->cp.done[s], 0));
        if (int rc2 = upload_rows(h, h->stage[s], reftrack[k], normvec ? normvec[k] : nullptr, scaling ? scaling[k] : nullptr, 0, (size_t)batch,
                                  (size_t)n, h->cp.in)) return rc2;
        HIP_TRY_DRAIN(hipEventRecord(h->cp.up[s], h->cp.in));
        return 0;
    };
    rc = upload(0);
    if (rc) return rc;
    const Stamps ts("MCQ_PIPE_TRACE");
    for (int k = 0; k < steps; ++k) {
        const int s = k & 1;
        const Staging& S = h->stage[s];
        ts.at("pipe: step %d enqueued from %.3f ms\n", k);
        const double* nv_k = normvec ? normvec[k] : nullptr;
        const double* sc_k = scaling ? scaling[k] : nullptr;
        // kernels of step k: after its upload, and after the download of step k - 2 has left the slot's result buffers
        // (slot s's kernels always run on compute stream s: step k - 2, the last user of this slot's workspace and buffers, precedes in stream order)
        Workspace& w = h->ws[two ? s : 0];
        HIP_TRY_DRAIN(hipStreamWaitEvent(w.stream, h->cp.up[s], 0));
        if (k >= 2) HIP_TRY_DRAIN(hipStreamWaitEvent(w.stream, h->cp.down[s], 0));
        McqBatch B = make_batch(batch, n, nullptr, S.ref, nv_k ? S.nv : nullptr, sc_k ? S.sc : nullptr, S.alpha, S.curv, S.status, nullptr,
                                kappa_bound, w_veh);
        rc = launch(h, B, o, w);
        if (rc) { drain(h); return rc; }
        HIP_TRY_DRAIN(hipEventRecord(h->cp.done[s], w.stream));
        if (k + 1 < steps) { rc = upload(k + 1); if (rc) return rc; }
        // download of step k
        HIP_TRY_DRAIN(hipStreamWaitEvent(h->cp.out, h->cp.done[s], 0));
        HIP_TRY_DRAIN(hipMemcpyAsync(alpha_out[k], S.alpha, elems * sizeof(double), hipMemcpyDeviceToHost, h->cp.out));
        HIP_TRY_DRAIN(hipMemcpyAsync(pin_cu + (size_t)k * batch, S.curv, batch * sizeof(double), hipMemcpyDeviceToHost, h->cp.out));
        HIP_TRY_DRAIN(hipMemcpyAsync(pin_st + (size_t)k * batch, S.status, batch * sizeof(int), hipMemcpyDeviceToHost, h->cp.out));
        HIP_TRY_DRAIN(hipEventRecord(h->cp.down[s], h->cp.out));
    }
    HIP_TRY_DRAIN(hipStreamSynchronize(h->cp.in));
    HIP_TRY_DRAIN(hipStreamSynchronize(compute_stream(h)));
    if (two) HIP_TRY_DRAIN(hipStreamSynchronize(h->ws[1].stream));
    HIP_TRY_DRAIN(hipStreamSynchronize(h->cp.out));
    for (int k = 0; k < steps; ++k) {
        memcpy(curv_err_out[k], pin_cu + (size_t)k * batch, batch * sizeof(double));
        memcpy(status_out[k], pin_st + (size_t)k * batch, batch * sizeof(int));
    }
    return 0;
}

// mcq_solve_batch and mcq_solve_batch_ends: d_ends = the device copy of the per-problem mcq_ends records, or nullptr (all rings)
static int solve_batch_impl(mcq_handle* h, const mcq_problem* probs, const mcq_ends* d_ends, int batch, const mcq_opts* opts,
                            double* alpha_out, double* curv_err_out, int* status_out, mcq_info* info_out)
{
    if (!h || !probs || batch <= 0 || !alpha_out || !curv_err_out || !status_out) {
        g_err = "mcq_solve_batch: bad argument";
        return MCQ_E_ARG;
    }
    HIP_TRY(hipSetDevice(h->device));
    const mcq_opts o = resolve_opts(opts);
    size_t nmax = 3;
    bool any_sc = false;
    for (int b = 0; b < batch; ++b) {
        if (!probs[b].reftrack || probs[b].n < 0 || (probs[b].normvec == nullptr) != (probs[0].normvec == nullptr)) {
            g_err = "mcq_solve_batch: problem with NULL buffers (normvec must be given for all problems or for none)";
            return MCQ_E_ARG;
        }
        if ((size_t)probs[b].n > nmax) nmax = (size_t)probs[b].n;
        if (probs[b].scaling) any_sc = true;
    }
    int rc = ensure_workspace(h, 0, (size_t)batch, nmax);
    if (rc) return rc;
    rc = ensure_staging(h, 0, (size_t)batch, nmax);
    if (rc) return rc;
    const Staging& s = h->stage[0];
    const bool with_nv = probs[0].normvec != nullptr;       // none given: normals (and scalings) are derived on the device
    Upload P = {probs, batch, nmax, any_sc, with_nv};
    McqBatch B = make_batch(batch, (int)nmax, h->d_n, s.ref, with_nv ? s.nv : nullptr, any_sc ? s.sc : nullptr, s.alpha, s.curv, s.status, h->d_info,
                            0.0, 0.0);
    B.kappa_bound_list = h->d_kb;
    B.w_veh_list = h->d_wv;
    B.ends = d_ends;
    rc = plan_upload(h, P, 0);
    if (rc) return rc;
    rc = solve_staged(h, B, o, P, P.alpha, curv_err_out, status_out, P.info);
    if (rc) return rc;
    // the padded rows of the pinned staging, back to back into the caller's array
    size_t off = 0;
    for (int b = 0; b < batch; ++b) {
        const size_t n = (size_t)probs[b].n;
        memcpy(alpha_out + off, P.alpha + (size_t)b * nmax, n * sizeof(double));
        off += n;
        if (info_out) info_out[b] = P.info[b];
    }
    return 0;
}

extern "C" int mcq_solve_batch(mcq_handle* h, const mcq_problem* probs, int batch, const mcq_opts* opts,
                               double* alpha_out, double* curv_err_out, int* status_out, mcq_info* info_out)
{
    return solve_batch_impl(h, probs, nullptr, batch, opts, alpha_out, curv_err_out, status_out, info_out);
}

// ---- rings and open chains in one batch (include/mcq.h): the records go up once, the solver kernel reads its problem's -----------------------
extern "C" int mcq_solve_batch_ends(mcq_handle* h, const mcq_problem* probs, const mcq_ends* ends, int batch, const mcq_opts* opts,
                                    double* alpha_out, double* curv_err_out, int* status_out, mcq_info* info_out)
{
    if (!ends) return mcq_solve_batch(h, probs, batch, opts, alpha_out, curv_err_out, status_out, info_out);
    if (!h || !probs || batch <= 0 || !alpha_out || !curv_err_out || !status_out) {
        g_err = "mcq_solve_batch_ends: bad argument";
        return MCQ_E_ARG;
    }
    const mcq_opts o = resolve_opts(opts);
    for (int b = 0; b < batch; ++b) {
        if (ends[b].closed) continue;
        if (!probs[b].normvec) { g_err = "mcq_solve_batch_ends: an open chain needs normvec"; return MCQ_E_ARG; }
        if (o.objective != MCQ_OBJ_MIN_CURV) { g_err = "mcq_solve_batch_ends: open chains have the minimum-curvature objective only"; return MCQ_E_ARG; }
    }
    HIP_TRY(hipSetDevice(h->device));
    if (int rc = grow(h, h->ends, (size_t)batch * sizeof(mcq_ends))) return rc;
    // ordered before every launch of the solve (and the copy streams of its slices) by the synchronisation: the caller's array is pageable
    HIP_TRY(hipMemcpyAsync(h->ends.p, ends, (size_t)batch * sizeof(mcq_ends), hipMemcpyHostToDevice, compute_stream(h)));
    HIP_TRY(hipStreamSynchronize(compute_stream(h)));
    return solve_batch_impl(h, probs, (const mcq_ends*)h->ends.p, batch, opts, alpha_out, curv_err_out, status_out, info_out);
}

// ---- a stream of RESIDENT uniform batches on the handle's two compute streams (include/mcq.h) ---------------------------------------------
extern "C" int mcq_solve_device_stream(mcq_handle* h, int steps, int batch, int n, const double* const* reftrack, const double* const* normvec,
                                       const double* const* scaling, double kappa_bound, double w_veh, const mcq_opts* opts,
                                       double* const* alpha_out, double* const* curv_err_out, int* const* status_out)
{
    if (!h || steps <= 0 || batch <= 0 || n <= 0 || !reftrack || !alpha_out || !curv_err_out || !status_out) {
        g_err = "mcq_solve_device_stream: bad argument";
        return MCQ_E_ARG;
    }
    if (int rc = check_step_list("mcq_solve_device_stream", steps, reftrack, alpha_out, curv_err_out, status_out)) return rc;
    HIP_TRY(hipSetDevice(h->device));
    const mcq_opts o = resolve_opts(opts);
    int rc = ensure_workspace(h, 0, (size_t)batch, (size_t)n);
    if (rc) return rc;
    const bool two = two_step_streams(steps, o);
    if (two) { rc = ensure_workspace(h, 1, (size_t)batch, (size_t)n); if (rc) return rc; }
    // the second stream starts behind whatever the caller has enqueued on the first (uploads of the inputs, an earlier call)
    if (two) { rc = fork_second(h); if (rc) return rc; }
    for (int k = 0; k < steps; ++k) {
        const double* nv_k = normvec ? normvec[k] : nullptr;
        McqBatch B = make_batch(batch, n, nullptr, reftrack[k], nv_k, (scaling && nv_k) ? scaling[k] : nullptr, alpha_out[k], curv_err_out[k],
                                status_out[k], nullptr, kappa_bound, w_veh);
        rc = launch(h, B, o, h->ws[two ? (k & 1) : 0]);
        if (rc) { drain(h); return rc; }
    }
    // the handle's first stream ends behind the second one, now and not lazily: mcq_sync, a later call on the handle or a caller holding
    // mcq_stream() sees every step done
    return two ? join_second(h) : 0;
}

// ---- tph.iqp_handler as one call (include/mcq.h) ---------------------------------------------------------------------------------
extern "C" int mcq_iqp_set_round_callback(mcq_handle* h, mcq_iqp_round_cb cb, void* user)
{
    if (!h) { g_err = "mcq_iqp_set_round_callback: NULL handle"; return MCQ_E_ARG; }
    h->iqp_cb = cb;
    h->iqp_cb_user = cb ? user : nullptr;
    return 0;
}

// h->iqp.  mcq_iqp_device's bookkeeping: live | n of the other set | glue status | pass status | final n (= n_io on return) | live count [1] |
// the pass's curvature errors; what mcq_iqp_batch hands it as its outputs: trace [batch][MCQ_IQP_TRACE] | buf | rounds.  [batch] each.
enum { IQP_LIVE, IQP_N_OTHER, IQP_GLUE_STATUS, IQP_PASS_STATUS, IQP_FINAL_N, IQP_LIVE_COUNT, IQP_PASS_CURV, IQP_TRACE, IQP_BUF, IQP_ROUNDS };
static Arena iqp_layout(size_t batch)
{
    Arena a;
    for (int k = IQP_LIVE; k <= IQP_FINAL_N; ++k) a.add<int>(batch);
    return a.add<int>(1).add<double>(batch).add<double>(batch * MCQ_IQP_TRACE).add<int>(batch).add<int>(batch);
}

// h->iqp_set, the second set of mcq_iqp_batch's double buffer: ring [batch][nmax][4] | normals [batch][nmax][2] ...
static Arena iqp_set_layout(size_t elems) { return Arena().add<double>(elems * 4).add<double>(elems * 2); }
// ... and the extra bytes of its pinned block: room for that set on the host, then buf [batch] as the host reads it
static Arena iqp_pin_layout(size_t elems, size_t batch) { return iqp_set_layout(elems).add<int>(batch); }

// One run of mcq_iqp_device: what its pieces share.  The regions of h->iqp the kernels' records take read-only are here once more, writable.
struct IqpRun {
    int batch, nmax, iters_min, max_rounds;
    double kappa_bound, w_veh, stepsize;
    const double* scaling;              // the first pass's (the re-spline of passes 2+ uses unit ones, as upstream)
    double* alpha;
    mcq_opts o;
    bool warm, timed;                   // warm: passes 2+ start from the carried working sets
    mcq_iqp_stats* stats;
    int *glue_status, *pass_status;
    double* pass_curv;
    int* n_set[2];                      // the two sets: [0] the caller's a (n_io doubles as its sizes), [1] its b and the arena's sizes
    double *ref_set[2], *nv_set[2];
    McqIqpStep S;
    int cur, rounds, n_live;            // the set the next pass reads; rounds run; tracks still iterating, as last read back
};

// `count` elements of each of two device arrays into host vectors on the compute stream, waited for.  The vectors are the caller's locals: a
// failure drains before it returns.
template <class A, class B> static int fetch(mcq_handle* h, int count, const A* d_a, std::vector<A>& a, const B* d_b, std::vector<B>& b)
{
    a.resize((size_t)count);
    b.resize((size_t)count);
    HIP_TRY_DRAIN(hipMemcpyAsync(a.data(), d_a, count * sizeof(A), hipMemcpyDeviceToHost, compute_stream(h)));
    HIP_TRY_DRAIN(hipMemcpyAsync(b.data(), d_b, count * sizeof(B), hipMemcpyDeviceToHost, compute_stream(h)));
    HIP_TRY_DRAIN(hipStreamSynchronize(compute_stream(h)));
    return 0;
}

// the tracks still iterating, as the bookkeeping counted them (into the run record: mcq_iqp_device drains where a piece fails)
static int iqp_read_live(mcq_handle* h, IqpRun& R)
{
    HIP_TRY(hipMemcpyAsync(&R.n_live, R.S.live_count, sizeof(int), hipMemcpyDeviceToHost, compute_stream(h)));
    HIP_TRY(hipStreamSynchronize(compute_stream(h)));
    return 0;
}

// every track starts live (a track with n == 0 ends in its first, empty pass: status MCQ_BAD_INPUT, rounds_out 1), every output cleared
static int iqp_begin(mcq_handle* h, IqpRun& R)
{
    const size_t ints = (size_t)R.batch * sizeof(int);
    const std::vector<int> ones((size_t)R.batch, 1);
    HIP_TRY_DRAIN(hipMemcpyAsync(R.S.live, ones.data(), ints, hipMemcpyHostToDevice, compute_stream(h)));
    HIP_TRY_DRAIN(hipMemsetAsync(R.S.final_rounds, 0, ints, compute_stream(h)));
    HIP_TRY_DRAIN(hipMemsetAsync(R.S.final_buf, 0, ints, compute_stream(h)));
    HIP_TRY_DRAIN(hipStreamSynchronize(compute_stream(h)));      // `ones` goes out of scope
    if (R.S.curv_trace) HIP_TRY(hipMemsetAsync(R.S.curv_trace, 0, (size_t)R.batch * MCQ_IQP_TRACE * sizeof(double), compute_stream(h)));
    if (R.stats) { R.stats->rounds = 0; R.stats->qp_solves = 0; for (int k = 0; k < 16; ++k) { R.stats->solver_ms[k] = 0.f; R.stats->fallbacks[k] = 0; } }
    // the final ring sizes are collected in a scratch array and moved to n_io at the end
    HIP_TRY(hipMemsetAsync(R.S.final_n, 0, ints, compute_stream(h)));
    return 0;
}

// ---- The first iters_min rounds as ONE launch.  A track's rounds depend on nothing but its own previous round, and no track can end before
//      round iters_min, so nothing has to come back to the host in between; but launched round by round, every round ends with its slowest
//      track -- a warm start that falls back to the cold path takes 8.7 ms where the median track takes 3 -- and the next round's launch
//      waits for it with most compute units idle (third pass of the 1024 ovals: 6.5 ms of mean load, 11.5 ms of launch; neither another cap
//      of the exchange nor the pass before says which tracks those will be: docs/NOTEBOOK.md R5.7).  In mcq_iqp_rounds_kernel every
//      workgroup takes its track through those rounds on its own -- the bodies of the solver, bookkeeping and glue kernels between workgroup
//      barriers, the same arrays --: nobody waits for anybody.  Results bitwise those of iqp_round, which takes over after round iters_min
//      (and runs everything when per-round data must reach the host: timed statistics, the print_debug callback; $MCQ_IQP_FUSED=0: always). ----
static int iqp_fused(mcq_handle* h, IqpRun& R)
{
    const int ra = std::min(R.iters_min, R.max_rounds);
    McqIqpRounds F;
    memset(&F, 0, sizeof(F));
    F.B = make_batch(R.batch, R.nmax, nullptr, nullptr, nullptr, nullptr, R.alpha, R.pass_curv, R.pass_status, nullptr, R.kappa_bound, R.w_veh);
    if (int rc = fill_batch(h, F.B, R.o, h->ws[0])) return rc;
    F.R.batch = R.batch; F.R.nmax = R.nmax; F.R.alpha = R.alpha; F.R.live = R.S.live; F.R.stepsize = R.stepsize; F.R.status = R.glue_status;
    F.R.vec = h->ws[0].vec; F.R.state_in = h->ws[0].state; F.R.state_out = h->state2;
    F.S = R.S;
    for (int q = 0; q < 2; ++q) { F.n_set[q] = R.n_set[q]; F.ref_set[q] = R.ref_set[q]; F.nv_set[q] = R.nv_set[q]; }
    F.sc = R.scaling;
    F.warm = R.warm ? h->state2 : nullptr;
    F.rounds = ra;
    HIP_TRY(hipMemsetAsync(R.S.live_count, 0, sizeof(int), compute_stream(h)));
    hipLaunchKernelGGL(mcq_iqp_rounds_kernel, dim3((unsigned)R.batch), dim3(256), 0, compute_stream(h), F);
    HIP_TRY(hipGetLastError());
    // (iqp_round may go on from the working sets the last round's glue carried over)
    h->state2_valid = true;
    h->state2_batch = R.batch;
    h->state2_nmax = R.nmax;
    R.cur = ra & 1;
    R.rounds = ra;
    return iqp_read_live(h, R);
}

// what reaches the host after a round's QP pass: the timed statistics (a failed read-back leaves the round's count at 0) and print_debug's
// callback -- the pass's curvature errors and who ran it, before the termination test decides
static int iqp_report(mcq_handle* h, const IqpRun& R, int it)
{
    std::vector<int> lv;
    if (R.timed && it <= 16) {
        float ms[5];
        if (mcq_last_timing(h, ms) == 0) R.stats->solver_ms[it - 1] = ms[4];
        std::vector<mcq_info> info;
        if (fetch(h, R.batch, h->d_info, info, R.S.live, lv) == 0)
            for (int k = 0; k < R.batch; ++k) if (lv[k] && (info[k].second_attempt & 2)) ++R.stats->fallbacks[it - 1];
    }
    if (h->iqp_cb) {
        std::vector<double> cv;
        if (int rc = fetch(h, R.batch, R.pass_curv, cv, R.S.live, lv)) return rc;
        h->iqp_cb(h->iqp_cb_user, it, R.batch, cv.data(), lv.data());
    }
    return 0;
}

// round `it` launch by launch: the QP pass, the host's reports, the bookkeeping, the glue for the tracks that go on, the bookkeeping
static int iqp_round(mcq_handle* h, IqpRun& R, int it)
{
    const int cur = R.cur;
    R.rounds = it;
    McqBatch B = make_batch(R.batch, R.nmax, R.n_set[cur], R.ref_set[cur], R.nv_set[cur], it == 1 ? R.scaling : nullptr, R.alpha, R.pass_curv,
                            R.pass_status, R.timed ? h->d_info : nullptr, R.kappa_bound, R.w_veh);
    R.o.warm_start = (R.warm && it > 1) ? 1 : 0;
    if (int rc = launch(h, B, R.o)) return rc;
    if (int rc = iqp_report(h, R, it)) return rc;
    HIP_TRY(hipMemsetAsync(R.S.live_count, 0, sizeof(int), compute_stream(h)));
    const dim3 grid((unsigned)((R.batch + 255) / 256)), block(256);
    R.S.phase = 0; R.S.round = it; R.S.cur = cur; R.S.n_ring = R.n_set[cur]; R.S.n_next = R.n_set[1 - cur];
    hipLaunchKernelGGL(mcq_iqp_step_kernel, grid, block, 0, compute_stream(h), R.S);
    HIP_TRY(hipGetLastError());
    const double scale = it < R.iters_min ? (double)it / (double)R.iters_min : 1.0;
    if (int rc = mcq_relinearise_device(h, R.batch, R.nmax, R.n_set[cur], R.ref_set[cur], R.nv_set[cur], R.alpha, R.S.live, scale, R.stepsize,
                                        R.ref_set[1 - cur], R.nv_set[1 - cur], R.n_set[1 - cur], R.glue_status)) return rc;
    R.S.phase = 1;
    hipLaunchKernelGGL(mcq_iqp_step_kernel, grid, block, 0, compute_stream(h), R.S);
    HIP_TRY(hipGetLastError());
    R.cur = 1 - cur;
    // the first iters_min - 1 rounds cannot end a healthy track: no need to look
    return (it >= R.iters_min || it == R.max_rounds) ? iqp_read_live(h, R) : 0;
}

// the final ring sizes into n_io, the run waited for; then, on the idle stream, the statistics and the statuses of the tracks the cap cut off
static int iqp_finish(mcq_handle* h, IqpRun& R)
{
    HIP_TRY(hipMemcpyAsync(R.n_set[0], R.S.final_n, (size_t)R.batch * sizeof(int), hipMemcpyDeviceToDevice, compute_stream(h)));
    HIP_TRY(hipStreamSynchronize(compute_stream(h)));
    std::vector<int> a, b;
    if (R.stats) {
        // QP passes summed over the tracks = sum of the rounds every track ran (the live count is only read back from round
        // iters_min on: counting launches x live tracks over-counted tracks that failed in an early round)
        // (a statistic: a failed read-back must not discard the run -- qp_solves = -1 then; tracks that came in empty ran no QP)
        long long solves = 0;
        if (fetch(h, R.batch, R.S.final_rounds, a, R.n_set[0], b) != 0) solves = -1;
        else for (int k = 0; k < R.batch; ++k) if (b[k] > 0) solves += a[k];
        R.stats->rounds = R.rounds;
        R.stats->qp_solves = (int)solves;
    }
    if (R.n_live > 0) {
        // tracks still iterating at max_rounds: report them (status MCQ_ITER_CAP), keep their last state
        if (int rc = fetch(h, R.batch, R.S.live, a, R.S.final_status, b)) return rc;
        for (int k = 0; k < R.batch; ++k) if (a[k] && b[k] == MCQ_OK) b[k] = MCQ_ITER_CAP;
        HIP_TRY_DRAIN(hipMemcpyAsync(R.S.final_status, b.data(), (size_t)R.batch * sizeof(int), hipMemcpyHostToDevice, compute_stream(h)));
        HIP_TRY_DRAIN(hipStreamSynchronize(compute_stream(h)));
    }
    return 0;
}

// the pieces in their order: the fused launch where nothing per round has to reach the host, the remaining rounds one by one
static int iqp_run(mcq_handle* h, IqpRun& R)
{
    if (int rc = iqp_begin(h, R)) return rc;
    int it = 1;
    const char* fe = getenv("MCQ_IQP_FUSED");
    if (!(fe && fe[0] == '0') && !R.timed && !h->iqp_cb) {
        if (int rc = iqp_fused(h, R)) return rc;
        it = R.rounds + 1;
    }
    for (; it <= R.max_rounds && R.n_live > 0; ++it)
        if (int rc = iqp_round(h, R, it)) return rc;
    return iqp_finish(h, R);
}

extern "C" int mcq_iqp_device(mcq_handle* h, int batch, int nmax, int* n_io, double* reftrack_a, double* normvec_a,
                              double* reftrack_b, double* normvec_b, const double* scaling, double kappa_bound, double w_veh,
                              double stepsize_interp, int iters_min, double curv_error_allowed, int max_rounds,
                              const mcq_opts* opts, double* alpha_out, int* buf_out, double* curv_err_out, int* status_out,
                              int* rounds_out, double* curv_trace_out, mcq_iqp_stats* stats)
{
    if (!h || batch <= 0 || nmax <= 0 || !n_io || !reftrack_a || !normvec_a || !reftrack_b || !normvec_b || !alpha_out ||
        !buf_out || !curv_err_out || !status_out || !rounds_out || !(stepsize_interp > 0.0) || iters_min < 1 || max_rounds < 1 ||
        reftrack_a == reftrack_b || normvec_a == normvec_b) {
        g_err = "mcq_iqp_device: bad argument";
        return MCQ_E_ARG;
    }
    HIP_TRY(hipSetDevice(h->device));
    const bool timed = stats && stats->timed;
    if (int rc = ensure_workspace(h, 0, (size_t)batch, (size_t)nmax)) return rc;
    const Arena a = iqp_layout((size_t)batch);
    if (int rc = grow(h, h->iqp, a.bytes)) return rc;
    if (timed) { if (int rc = ensure_staging(h, 0, (size_t)batch, (size_t)nmax)) return rc; }       // (the info records)
    void* const p = h->iqp.p;
    IqpRun R = {batch, nmax, iters_min, max_rounds, kappa_bound, w_veh, stepsize_interp, scaling, alpha_out, resolve_opts(opts),
                !(opts && opts->warm_start < 0), timed, stats, a.at<int>(p, IQP_GLUE_STATUS), a.at<int>(p, IQP_PASS_STATUS), a.at<double>(p, IQP_PASS_CURV),
                {n_io, a.at<int>(p, IQP_N_OTHER)}, {reftrack_a, reftrack_b}, {normvec_a, normvec_b}};
    R.n_live = batch;
    McqIqpStep& S = R.S;            // (zero so far, like cur and rounds)
    S.batch = batch; S.iters_min = iters_min; S.curv_allowed = curv_error_allowed;
    S.curv = R.pass_curv; S.status = R.pass_status; S.relin_status = R.glue_status;
    S.live = a.at<int>(p, IQP_LIVE); S.final_n = a.at<int>(p, IQP_FINAL_N); S.live_count = a.at<int>(p, IQP_LIVE_COUNT);
    S.final_buf = buf_out; S.final_curv = curv_err_out; S.final_status = status_out; S.final_rounds = rounds_out;
    S.curv_trace = curv_trace_out;
    const int rc = iqp_run(h, R);
    // What every way out of a run has in common: nothing of it is in flight (iqp_finish has waited; a failure may have left copies into the
    // record or launches queued), and the working sets belong to its last glue call, not to a later solve.
    if (rc) drain(h);
    h->state2_valid = false;
    return rc;
}

// The end states' rings and normals into the caller's [batch][nmax][*] arrays, buf_h saying which set holds a track's.  One set holds them all
// (the usual case: one iters_min for all, every track ends in the same round): it goes out in two copies.  Otherwise both sets go through the
// pinned block -- set 0 into the now free input block, set 1 into the extra bytes -- and from there track by track.
static int iqp_rings_down(mcq_handle* h, const Upload& P, const Arena& pin, const Stamps& ts, const double* ref_b, const double* nv_b,
                          const int* n_out, double* reftrack_out, double* normvec_out)
{
    const size_t nmax = P.nmax, elems = (size_t)P.batch * nmax;
    const int* buf_h = pin.at<int>(P.extra, 2);
    const double* d_ref[2] = {h->stage[0].ref, ref_b};
    const double* d_nv[2] = {h->stage[0].nv, nv_b};
    bool use[2] = {false, false};
    for (int b = 0; b < P.batch; ++b) use[buf_h[b] ? 1 : 0] = true;
    if (use[0] != use[1]) {
        const int q = use[1] ? 1 : 0;
        HIP_TRY_DRAIN(hipMemcpyAsync(reftrack_out, d_ref[q], elems * 4 * sizeof(double), hipMemcpyDeviceToHost, compute_stream(h)));
        HIP_TRY_DRAIN(hipMemcpyAsync(normvec_out, d_nv[q], elems * 2 * sizeof(double), hipMemcpyDeviceToHost, compute_stream(h)));
        HIP_TRY_DRAIN(hipStreamSynchronize(compute_stream(h)));
        ts.at("iqp_batch: %-28s at %.3f ms\n", "rings and normals down");
        return 0;
    }
    double* ref_h[2] = {P.ref, pin.at<double>(P.extra, 0)};
    double* nv_h[2] = {P.nv, pin.at<double>(P.extra, 1)};
    for (int q = 0; q < 2; ++q) {
        HIP_TRY_DRAIN(hipMemcpyAsync(ref_h[q], d_ref[q], elems * 4 * sizeof(double), hipMemcpyDeviceToHost, compute_stream(h)));
        HIP_TRY_DRAIN(hipMemcpyAsync(nv_h[q], d_nv[q], elems * 2 * sizeof(double), hipMemcpyDeviceToHost, compute_stream(h)));
    }
    HIP_TRY_DRAIN(hipStreamSynchronize(compute_stream(h)));
    for (int b = 0; b < P.batch; ++b) {
        const int q = buf_h[b] ? 1 : 0;
        const size_t n = n_out[b] > 0 ? (size_t)n_out[b] : 0;
        memcpy(reftrack_out + (size_t)b * nmax * 4, ref_h[q] + (size_t)b * nmax * 4, n * 4 * sizeof(double));
        memcpy(normvec_out + (size_t)b * nmax * 2, nv_h[q] + (size_t)b * nmax * 2, n * 2 * sizeof(double));
    }
    return 0;
}

extern "C" int mcq_iqp_batch(mcq_handle* h, const mcq_problem* probs, int batch, double stepsize_interp, int iters_min,
                             double curv_error_allowed, int max_rounds, const mcq_opts* opts, int nmax_out, double* alpha_out,
                             double* reftrack_out, double* normvec_out, int* n_out, double* curv_err_out, int* status_out,
                             int* rounds_out, double* curv_trace_out, mcq_iqp_stats* stats)
{
    if (!h || !probs || batch <= 0 || nmax_out < 3 || !alpha_out || !reftrack_out || !normvec_out || !n_out || !curv_err_out ||
        !status_out || !rounds_out) {
        g_err = "mcq_iqp_batch: bad argument";
        return MCQ_E_ARG;
    }
    HIP_TRY(hipSetDevice(h->device));
    const Stamps ts("MCQ_IQP_TRACE");
    const char* const line = "iqp_batch: %-28s at %.3f ms\n";
    const size_t nmax = (size_t)nmax_out, elems = (size_t)batch * nmax;
    bool any_sc = false;
    for (int b = 0; b < batch; ++b) {
        if (!probs[b].reftrack || !probs[b].normvec || probs[b].n < 0) { g_err = "mcq_iqp_batch: reftrack and normvec are required"; return MCQ_E_ARG; }
        if ((size_t)probs[b].n > nmax) { g_err = "mcq_iqp_batch: a track has more waypoints than nmax_out"; return MCQ_E_TOO_LARGE; }
        if (probs[b].kappa_bound != probs[0].kappa_bound || probs[b].w_veh != probs[0].w_veh) {
            g_err = "mcq_iqp_batch: one kappa_bound / w_veh per call";
            return MCQ_E_ARG;
        }
        if (probs[b].scaling) any_sc = true;
    }
    // buffers: grown here and kept by the handle (no allocation / hipFree -- an implicit device-wide synchronisation -- per call)
    const Arena set2 = iqp_set_layout(elems), own = iqp_layout((size_t)batch);
    if (int rc = ensure_workspace(h, 0, (size_t)batch, nmax)) return rc;
    if (int rc = ensure_staging(h, 0, (size_t)batch, nmax)) return rc;
    if (int rc = grow(h, h->iqp_set, set2.bytes)) return rc;
    if (int rc = grow(h, h->iqp, own.bytes)) return rc;
    const Staging& s = h->stage[0];
    double *ref_b = set2.at<double>(h->iqp_set.p, 0), *nv_b = set2.at<double>(h->iqp_set.p, 1);
    double* trace_d = curv_trace_out ? own.at<double>(h->iqp.p, IQP_TRACE) : nullptr;
    int *d_buf = own.at<int>(h->iqp.p, IQP_BUF), *d_rounds = own.at<int>(h->iqp.p, IQP_ROUNDS);
    ts.at(line, "checked, buffers ready");
    // plan and upload; the pinned block's extra bytes take the end states of the second set and buf
    Upload P = {probs, batch, nmax, any_sc, true};
    const Arena pin = iqp_pin_layout(elems, (size_t)batch);
    if (int rc = plan_upload(h, P, pin.bytes)) return rc;
    int* buf_h = pin.at<int>(P.extra, 2);
    if (int rc = upload_batch(h, P)) return rc;
    ts.at(line, "packed, uploads queued");
    int rc = mcq_iqp_device(h, batch, (int)nmax, h->d_n, s.ref, s.nv, ref_b, nv_b, any_sc ? s.sc : nullptr, probs[0].kappa_bound, probs[0].w_veh,
                            stepsize_interp, iters_min, curv_error_allowed, max_rounds, opts, s.alpha, d_buf, s.curv, s.status, d_rounds, trace_d, stats);
    ts.at(line, "rounds done");
    if (rc) return rc;
    // results down: alpha straight into the caller's [batch][nmax_out] array (its padding holds whatever the device buffer held)
    if (trace_d) HIP_TRY(hipMemcpy(curv_trace_out, trace_d, (size_t)batch * MCQ_IQP_TRACE * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY_DRAIN(hipMemcpyAsync(n_out, h->d_n, batch * sizeof(int), hipMemcpyDeviceToHost, compute_stream(h)));
    HIP_TRY_DRAIN(hipMemcpyAsync(buf_h, d_buf, batch * sizeof(int), hipMemcpyDeviceToHost, compute_stream(h)));
    HIP_TRY_DRAIN(hipMemcpyAsync(rounds_out, d_rounds, batch * sizeof(int), hipMemcpyDeviceToHost, compute_stream(h)));
    rc = download_results(h, compute_stream(h), batch, alpha_out, s.alpha, elems * sizeof(double), curv_err_out, status_out, nullptr);
    if (rc) return rc;
    HIP_TRY_DRAIN(hipStreamSynchronize(compute_stream(h)));
    ts.at(line, "alpha and per-track results down");
    return iqp_rings_down(h, P, pin, ts, ref_b, nv_b, n_out, reftrack_out, normvec_out);
}



// =====================================================================================================================
// The one collective of a multi-GPU job (include/mcq.h): ncclAllGather of RCCL on the handle's COMM stream, ordered behind its compute stream by an event.  RCCL is loaded with dlopen on
// first use -- libmcq.so has no link-time dependency on it, and a single-GPU process never maps its 570 MB.  Only the five entry
// points below are bound; their types are restated here (rccl.h: ncclUniqueId = 128 opaque bytes, ncclComm_t an opaque pointer,
// ncclDataType_t: ncclInt32 = 2, ncclFloat32 = 7, ncclFloat64 = 8; ncclSuccess = 0).
// =====================================================================================================================
namespace {
struct RcclId { char internal[MCQ_COMM_ID_BYTES]; };
struct Rccl {
    void* lib = nullptr;
    int (*GetUniqueId)(RcclId*) = nullptr;
    int (*CommInitRank)(void**, int, RcclId, int) = nullptr;
    int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
    std::string path;
};
Rccl g_rccl;

int rccl_load()
{
    if (g_rccl.lib) return 0;
    std::vector<std::string> cand;
    if (const char* e = getenv("MCQ_RCCL_LIB")) cand.push_back(e);
    if (const char* e = getenv("ROCM_PATH")) cand.push_back(std::string(e) + "/lib/librccl.so.1");
    cand.push_back("/opt/rocm/lib/librccl.so.1");
    cand.push_back("librccl.so.1");
    std::string tried;
    for (const std::string& p : cand) {
        void* lib = dlopen(p.c_str(), RTLD_NOW | RTLD_LOCAL);
        if (!lib) { tried += p + " (" + (dlerror() ? dlerror() : "?") + "); "; continue; }
        g_rccl.GetUniqueId = (int (*)(RcclId*))dlsym(lib, "ncclGetUniqueId");
        g_rccl.CommInitRank = (int (*)(void**, int, RcclId, int))dlsym(lib, "ncclCommInitRank");
        g_rccl.AllGather = (int (*)(const void*, void*, size_t, int, void*, hipStream_t))dlsym(lib, "ncclAllGather");
        g_rccl.CommDestroy = (int (*)(void*))dlsym(lib, "ncclCommDestroy");
        g_rccl.GetErrorString = (const char* (*)(int))dlsym(lib, "ncclGetErrorString");
        if (!g_rccl.GetUniqueId || !g_rccl.CommInitRank || !g_rccl.AllGather || !g_rccl.CommDestroy) {
            tried += p + " (symbols missing); ";
            dlclose(lib);
            continue;
        }
        g_rccl.lib = lib;
        g_rccl.path = p;
        return 0;
    }
    g_err = "mcq_comm: RCCL could not be loaded: " + tried;
    return MCQ_E_DEVICE;
}

int rccl_fail(const char* what, int rc)
{
    g_err = std::string(what) + " failed: " + (g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : "?") + " (" + g_rccl.path + ")";
    return MCQ_E_DEVICE;
}
}   // namespace

extern "C" int mcq_comm_unique_id(unsigned char id_out[MCQ_COMM_ID_BYTES])
{
    if (!id_out) { g_err = "mcq_comm_unique_id: id_out is NULL"; return MCQ_E_ARG; }
    int rc = rccl_load();
    if (rc) return rc;
    RcclId id;
    const int r = g_rccl.GetUniqueId(&id);
    if (r != 0) return rccl_fail("ncclGetUniqueId", r);
    memcpy(id_out, id.internal, MCQ_COMM_ID_BYTES);
    return 0;
}

extern "C" int mcq_comm_init(mcq_handle* h, int rank, int world, const unsigned char id[MCQ_COMM_ID_BYTES])
{
    if (!h || !id || world < 1 || rank < 0 || rank >= world) { g_err = "mcq_comm_init: bad argument"; return MCQ_E_ARG; }
    if (h->comm) { g_err = "mcq_comm_init: the handle already has a communicator"; return MCQ_E_ARG; }
    int rc = rccl_load();
    if (rc) return rc;
    HIP_TRY(hipSetDevice(h->device));
    if (!h->comm_stream) {
        HIP_TRY(hipStreamCreate(&h->comm_stream));
        HIP_TRY(hipEventCreate(&h->comm_ready));
        for (int k = 0; k < 4; ++k) { HIP_TRY(hipEventCreate(&h->comm_t0[k])); HIP_TRY(hipEventCreate(&h->comm_done[k])); }
    }
    RcclId uid;
    memcpy(uid.internal, id, MCQ_COMM_ID_BYTES);
    void* comm = nullptr;
    const int r = g_rccl.CommInitRank(&comm, world, uid, rank);
    if (r != 0) return rccl_fail("ncclCommInitRank", r);
    h->comm = comm;
    h->comm_rank = rank;
    h->comm_world = world;
    h->comm_seq = 0;
    return 0;
}

extern "C" int mcq_comm_allgather(mcq_handle* h, const void* send, void* recv, size_t count, int dtype)
{
    if (!h || !send || !recv || dtype < MCQ_DT_F64 || dtype > MCQ_DT_I32) { g_err = "mcq_comm_allgather: bad argument"; return MCQ_E_ARG; }
    if (!h->comm) { g_err = "mcq_comm_allgather: mcq_comm_init has not been called on this handle"; return MCQ_E_ARG; }
    if (count == 0) return 0;
    HIP_TRY(hipSetDevice(h->device));
    // behind everything enqueued on the handle's stream so far (the solve that filled `send`), on a stream of its own: the handle's
    // stream goes on with the next solve while the gather runs
    // (ws[0].stream is NOT pulled behind a pending slice on ws[1].stream here -- compute_stream would serialise the next sliced call behind this
    // one, and a caller gathers after every step: the comm stream waits for both slices' ends instead)
    HIP_TRY(hipEventRecord(h->comm_ready, h->ws[0].stream));
    HIP_TRY(hipStreamWaitEvent(h->comm_stream, h->comm_ready, 0));
    if (h->sl.last1) HIP_TRY(hipStreamWaitEvent(h->comm_stream, h->sl.last1, 0));
    const unsigned slot = h->comm_seq & 3u;
    HIP_TRY(hipEventRecord(h->comm_t0[slot], h->comm_stream));
    const int nccl_t = dtype == MCQ_DT_F64 ? 8 : dtype == MCQ_DT_F32 ? 7 : 2;
    const int r = g_rccl.AllGather(send, recv, count, nccl_t, h->comm, h->comm_stream);
    if (r != 0) return rccl_fail("ncclAllGather", r);
    HIP_TRY(hipEventRecord(h->comm_done[slot], h->comm_stream));
    ++h->comm_seq;
    return 0;
}

extern "C" int mcq_comm_wait(mcq_handle* h, int lag, float* ms_out)
{
    if (!h || lag < 0 || lag > 2) { g_err = "mcq_comm_wait: bad argument"; return MCQ_E_ARG; }
    if (ms_out) *ms_out = 0.0f;
    if (!h->comm || h->comm_seq <= (unsigned)lag) return 0;          // nothing (that old) in flight
    HIP_TRY(hipSetDevice(h->device));
    const unsigned slot = (h->comm_seq - 1u - (unsigned)lag) & 3u;
    HIP_TRY(hipEventSynchronize(h->comm_done[slot]));
    if (ms_out) HIP_TRY(hipEventElapsedTime(ms_out, h->comm_t0[slot], h->comm_done[slot]));
    return 0;
}

extern "C" int mcq_comm_world(mcq_handle* h, int* rank_out, int* world_out)
{
    if (!h || !h->comm) { g_err = "mcq_comm_world: no communicator"; return MCQ_E_ARG; }
    if (rank_out) *rank_out = h->comm_rank;
    if (world_out) *world_out = h->comm_world;
    return 0;
}

extern "C" int mcq_comm_destroy(mcq_handle* h)
{
    if (!h) return MCQ_E_ARG;
    int ret = 0;
    (void)hipSetDevice(h->device);
    if (h->comm) {
        if (h->ws[0].stream) (void)hipStreamSynchronize(compute_stream(h));
        if (h->comm_stream) (void)hipStreamSynchronize(h->comm_stream);
        const int r = g_rccl.CommDestroy(h->comm);
        h->comm = nullptr;
        h->comm_rank = h->comm_world = 0;
        if (r != 0) ret = rccl_fail("ncclCommDestroy", r);
    }
    if (h->comm_stream) {
        (void)hipEventDestroy(h->comm_ready);
        for (int k = 0; k < 4; ++k) { (void)hipEventDestroy(h->comm_t0[k]); (void)hipEventDestroy(h->comm_done[k]); }
        (void)hipStreamDestroy(h->comm_stream);
        h->comm_stream = nullptr;
        h->comm_ready = nullptr;
        for (int k = 0; k < 4; ++k) h->comm_t0[k] = h->comm_done[k] = nullptr;
    }
    h->comm_seq = 0;      // no gather in flight any more: mcq_copy_to_host / mcq_device_free must not wait on the destroyed events
    return ret;
}
