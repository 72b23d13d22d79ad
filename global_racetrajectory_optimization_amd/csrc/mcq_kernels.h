// mcq_kernels.h -- hand-written HIP (gfx950 / CDNA4) kernels of the minimum-curvature raceline QP engine.
//
// One workgroup == one problem (one closed reference track); the batch is the grid.  Everything is fp64.
// The maths follows SURVEY.md App. A (restating tph.opt_min_curv, call sites [REF main_globaltraj.py:264-271,
// 344-350]); DESIGN.md sections 3-5 derive the structure-exploiting form used here:
//
//   K1 mcq_assemble_kernel : [x,y,w_r,w_l] rows, normals, spline scalings  ->  box bounds, the pivots of the closed cubic-spline
//                            system (a cyclic tridiagonal matrix T: periodic pivot recurrences, mcq_tri.inc), x'', y'' (two solves
//                            with T), x', y', the curvature pre-factor, k_ref.  No matrix is formed: E = a T^-1 R Nx + b T^-1 R Ny.
//   K3 mcq_solve_kernel    : Mehrotra predictor-corrector interior point on the box QP -> active-set identification ->
//                            block-pivoting active-set iterations on the identified vertex (exact KKT point, like the
//                            Goldfarb-Idnani solver the reference uses returns) -> fp64 residual refinement through
//                            E -> curvature-row check -> opt_min_curv's curvature-error post-check.  Linear algebra: the
//                            saddle-point elimination of mcq_kkt.inc (5 x 5 blocks per waypoint; H = E'E is never formed),
//                            E and E' applied through T (mcq_tri.inc); shortest path: scalar cyclic tridiagonal (mcq_tri.inc).
//
// Global-memory workspace per problem (doubles):
//   L        [nmax][MCQ_LLD]  records of the saddle-point elimination (mcq_kkt.inc: K_AD, K_AY, K_AS, K_YV -- 65 doubles per waypoint)
//                             and three scratch vectors of the long-ring tridiagonal route (K_TS)
//   vectors  [MCQ_NVEC][nmax] see the enum below
//   Z        [nmax] + [MCQ_KMAX][MCQ_KMAX]   curvature-row path: one scratch vector, the Schur complement of the active rows
//   state    [nmax] bytes     working set
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/mcq.h"

#define MCQ_LLD 72                 /* doubles per waypoint of the L slab */
#define MCQ_NVEC 32
#define MCQ_TRI_MAXN 2048         /* rings up to this length run the tridiagonal sweeps of mcq_tri.inc in LDS (eight waypoints per thread); longer ones on workspace vectors */
#define MCQ_KMAX 120               /* active curvature rows the Schur-complement path of the active-set phase holds */
#define MCQ_KBIG 512               /* ... and of the overflow path (round 3): a problem with more of them claims one of the handle's slots, */
#define MCQ_KBIG_SLOT ((size_t)MCQ_KBIG * MCQ_KBIG + 6 * (size_t)MCQ_KBIG)   /* doubles per slot: Schur matrix, three vectors, the index / sign / pivot lists */
#define MCQ_KBIG_SLOTS 8           /* slots per handle (17 MB): problems of one launch that can take the overflow path */
#define MCQ_ZLD(nmax) ((size_t)(nmax) + (size_t)MCQ_KMAX * MCQ_KMAX)   /* doubles of the curvature-row scratch per problem: one vector + the Schur matrix */

struct McqDims {
    int n;
};
__host__ __device__ inline McqDims mcq_dims(int n)
{
    McqDims d;
    d.n = n;
    return d;
}

// Pointers into HBM carry the global address space in their type so that device functions that are not inlined still
// compile to global_load / global_store (a generic pointer would become FLAT and serialise against LDS traffic).
typedef __attribute__((address_space(1))) double gdouble;
typedef __attribute__((address_space(1))) signed char gschar;
typedef __attribute__((address_space(1))) char gchar;
typedef __attribute__((address_space(1))) int gint;
typedef __attribute__((address_space(1))) mcq_info ginfo;

// Device workspace of ONE problem (pointers into the handle's slabs).
struct McqWork {
    const gdouble* ref;   // [n][4]
    const gdouble* nv;    // [n][2]
    const gdouble* sc;    // [n] or nullptr
    gdouble* L;           // also scratch for the T^-1 rows during assembly
    gdouble* vec;         // MCQ_NVEC vectors of length nmax, see enum below
    gschar* state;        // [n] 0 free, -1 at lower bound, +1 at upper bound, 2 fixed (lo == hi)
    gdouble* Z;           // curvature-row path: [nmax] scratch vector, then the [MCQ_KMAX][MCQ_KMAX] Schur matrix / its LU factors
    gdouble* alpha;       // [n] output
    gdouble* curv_err;    // [1]
    gint* status;         // [1]
    ginfo* info;          // [1] or nullptr
};

enum {
    V_XP = 0, V_YP, V_CP, V_KREF, V_XPP, V_YPP, V_F, V_LO, V_HI, V_X, V_G, V_ZL, V_ZU, V_SIG, V_RHS, V_DXA, V_T0, V_T1,
    V_T2, V_T3, V_TL, V_TU, V_YL, V_YU, V_SK, V_EDA, V_Q, V_NX, V_NY, V_SC,   /* unit normals and spline scalings as used (given or derived) */
    V_IDL, V_TUC        /* saddle-point core: 1 / pivot and super-diagonal of the spline matrix T (mcq_tri.inc) */
};

struct McqBatch {
    int pb0;        // slice launches (round 6, mcq_solve_host): workgroup w of the launch works on problem pb0 + w of the batch's arrays
    int batch;
    int n;          // uniform-n path (n_list == nullptr) or nmax
    int nmax;
    const int* n_list;      // per-problem n (device) or nullptr
    const double* ref;      // [batch][nmax][4]
    const double* nv;       // [batch][nmax][2], or nullptr: normals AND scalings are derived from the closed distance-scaled
                            // spline through the reference line (what prep_track does with calc_splines), `sc` is ignored
    const double* sc;       // [batch][nmax] or nullptr (unit scalings)
    double* nv_out;         // optional outputs of the assembly: normals [batch][nmax][2], scalings [batch][nmax]
    double* sc_out;
    int prep_only;          // assembly kernel stops after the spline quantities (mcq_prep_device)
    double* L; double* vec; double* Z;
    signed char* state;
    double* alpha;          // [batch][nmax]
    double* curv_err; int* status; mcq_info* info;
    double kappa_bound, w_veh;
    const double* kappa_bound_list;  // per-problem overrides (device) or nullptr
    const double* w_veh_list;
    int max_ipm_iter, max_as_iter, refine_steps, check_kappa;
    const signed char* warm; // [batch][nmax] working set to start the exchange from (IQP passes 2+), or nullptr (cold: interior point)
    int poison_lds;         // MCQ_POISON=1 (debugging aid): the solver kernel starts from an LDS full of NaNs, like the workspaces
    double* kbig;           // overflow slots of the curvature-row working set (MCQ_KBIG_SLOT doubles each), kbig_slots of them;
    int* slot_flags;        // [MCQ_SLOT_FLAGS: MCQ_KBIG_SLOTS overflow slots, MCQ_GI_FULL_MAX full, MCQ_GI_SLOTS_MAX small Goldfarb-Idnani slots] 0 = free, 1 = taken: a workgroup claims a slot by compare-and-swap and releases it when it is
                            // done (zero whenever no launch is in flight: nothing for the host to reset between launches)
    int kbig_slots;
    int objective;          // MCQ_OBJ_*: shortest path = H (a cyclic tridiagonal: two vectors) and f written directly by
                            // mcq_assemble_sp_kernel, the gradient is H x + f; no curvature rows, no curvature-error post-check
    int algorithm;          // MCQ_ALG_GI: interior point and block pivoting are skipped, every problem goes through the Goldfarb-Idnani path
    double* gi;             // FULL slots of the Goldfarb-Idnani path (mcq_gi.inc), MCQ_GI_SLOT_DOUBLES(nmax, gi_qcap) doubles each: a workgroup whose
    int gi_slots, gi_qcap;  // problem needs the path claims one (and waits for one if all are taken); gi_qcap = constraints a working set can
                            // hold (= nmax: no more can be independent)
    double* gis;            // SMALL slots (round 6; MCQ_ALG_GI: one per resident workgroup), working sets of up to gis_qcap < nmax constraints --
    int gis_slots, gis_qcap; // what the observed working sets need; a problem that outgrows its small slot moves into a full one in place (gi_grow).
                            // Flags: slot_flags[kbig_slots + MCQ_GI_FULL_MAX + s]
    const mcq_ends* ends;   // [batch] (device) per-problem ring / open-chain records (include/mcq.h), or nullptr: every problem is a ring
};
static_assert(MCQ_CHAIN_MAXN == MCQ_TRI_MAXN, "open chains run the tridiagonal sweeps through LDS only");

__global__ void mcq_assemble_kernel(McqBatch B);
__global__ void mcq_assemble_sp_kernel(McqBatch B);
__global__ void mcq_solve_kernel(McqBatch B);      // saddle-point elimination (mcq_kkt.inc) / scalar cyclic tridiagonal (shortest path, mcq_tri.inc); two workgroups per CU
/* Goldfarb-Idnani dual active-set path (mcq_gi.inc): inside mcq_solve_kernel, for whatever its interior point + block pivoting did not
 * settle (iteration cap, working set beyond its arrays, ...) -- solved again from scratch by quadprog's algorithm, in an HBM slot of the handle */
#define MCQ_GI_SLOTS 8
#define MCQ_GI_FULL_MAX 512        /* full slots (working sets of up to nmax constraints) a handle holds at most (the default byte cap, 16 GB, gives 256 at nmax = 2000; $MCQ_GI_BYTES moves it) */
#define MCQ_GI_SLOTS_MAX 512       /* small slots when every problem takes the path (mcq_opts.algorithm = MCQ_ALG_GI): one per resident workgroup */
#define MCQ_SLOT_FLAGS (MCQ_KBIG_SLOTS + MCQ_GI_FULL_MAX + MCQ_GI_SLOTS_MAX)
#define MCQ_GI_SLOT_FULL 100       /* gi_solve: the working set has outgrown the slot (internal: gi_rescue moves the problem to a full slot) */
#define MCQ_GI_SLOT_DOUBLES(nm, qcap) ((size_t)(qcap) * (size_t)(nm) + (size_t)(qcap) * (size_t)(qcap) + 9 * (size_t)(qcap) + 8)

/* tph.check_normals_crossing [REF helper_funcs_glob/src/prep_track.py:57-59], one workgroup per track: crossing_out [batch] =
 * 1 / 0, or -1 where tph raises (horizon >= n) */
__global__ void mcq_normals_crossing_kernel(int nmax, const int* n_list, const double* ref_all, const double* nv_all,
                                            int horizon, int* crossing_out);

/* fp32 boundary (BASELINE config 5): float <-> double streaming conversions around the fp64 engine */
__global__ void mcq_widen_kernel(const float* src, double* dst, size_t count);
__global__ void mcq_narrow_kernel(const double* src, float* dst, size_t count);
/* float rows -> fp64 rows [x, y, w_r, w_l]: layout 0 absolute coordinates, 1 ring increments (include/mcq.h MCQ_F32_*); one wave per track */
__global__ void mcq_widen_rows_kernel(const float* rows, const double* origin, double* dst, int n, int layout);

size_t mcq_solve_lds_bytes();   /* static LDS of the solver kernel (reporting only) */

/* ---- IQP glue on the device: raceline = refline + alpha * normal, closed spline through it
 *      (unit scalings), arclength re-sampling at ~stepsize, track widths carried over, normals of the re-sampled ring.
 *      One workgroup per track; mirrors tph.create_raceline / interp_track_widths / calc_splines(use_dist_scaling=False)
 *      as iqp_handler chains them. ---- */
struct McqRelin {
    int batch, nmax;
    const int* n_in;        // [batch] waypoints of each track
    const double* ref_in;   // [batch][nmax][4]
    const double* nv_in;    // [batch][nmax][2]
    const double* alpha;    // [batch][nmax]
    const int* live;        // [batch] (0: leave this track alone) or nullptr
    double alpha_scale;     // damping of the early IQP iterations (iter / iters_min), 1 afterwards
    double stepsize;        // stepsize_interp
    double* ref_out;        // [batch][nmax][4]
    double* nv_out;         // [batch][nmax][2]
    int* n_out;             // [batch]
    int* status;            // [batch]: MCQ_OK, or MCQ_BAD_INPUT if the re-sampled ring has < 3 or > nmax points
    double* vec;            // workspace, [batch][MCQ_NVEC][nmax] (the solver's vector slab)
    const signed char* state_in;   // [batch][nmax] working set the solver left for these tracks (or nullptr)
    signed char* state_out;        // [batch][nmax] the same carried to the re-sampled rings (warm start of the next pass)
};
__global__ void mcq_relinearise_kernel(McqRelin R);

/* ---- the bookkeeping of tph.iqp_handler between the QP pass and the glue, on the device (one thread per track):
 *      phase 0 (after the QP pass of round `round`): record the state of every live track (it is the final one if the track
 *              stops here), stop it if its QP failed or if round >= iters_min and curv_error_max <= curv_allowed;
 *      phase 1 (after the glue): a live track whose re-sampled ring did not fit stops with MCQ_BAD_INPUT; tracks that stopped get
 *              n_next = 0 (the next QP pass skips them).  live_count [1] = tracks still iterating (zeroed before phase 0). ---- */
struct McqIqpStep {
    int batch, phase, round, iters_min, cur;
    double curv_allowed;
    const double* curv;         // [batch] curvature error of the pass just solved
    const int* status;          // [batch] its status
    const int* relin_status;    // [batch] status of the glue (phase 1)
    int* live;                  // [batch]
    const int* n_ring;          // [batch] ring sizes solved in this round
    int* n_next;                // [batch] ring sizes of the next round (phase 1: zeroed for stopped tracks)
    int* final_n; int* final_buf; double* final_curv; int* final_status; int* final_rounds;
    double* curv_trace;         // [batch][MCQ_IQP_TRACE] or nullptr
    int* live_count;
};
__global__ void mcq_iqp_step_kernel(McqIqpStep S);

/* ---- the first `rounds` rounds of iqp_handler as ONE launch, a workgroup per track (mcq_kernels.hip: mcq_iqp_rounds_kernel).  B: the QP pass's
 *      launch parameters (outputs, options, workspace; its ref / nv / n_list / sc / warm are not read); n_set / ref_set / nv_set: the two ring
 *      buffers (round r reads set (r - 1) & 1 and writes the other); sc: the first round's scalings or nullptr; warm: the carried working sets
 *      (= R.state_out) or nullptr (cold passes); R: the glue's parameters (its n_in / ref_in / nv_in / *_out / alpha_scale are not read);
 *      S: the bookkeeping's (phase / round / cur / n_ring / n_next are not read; live_count: zero on entry, tracks still iterating on return). ---- */
struct McqIqpRounds {
    McqBatch B;
    McqRelin R;
    McqIqpStep S;
    int* n_set[2];
    double* ref_set[2];
    double* nv_set[2];
    const double* sc;
    const signed char* warm;
    int rounds;
};
__global__ void mcq_iqp_rounds_kernel(McqIqpRounds F);

/* ---- raceline at the output resolution + heading / curvature (what main_globaltraj.py runs between the QP and the velocity
 *      profile [REF main_globaltraj.py:371-387]: tph.create_raceline + tph.calc_head_curv_an).  One workgroup per track. ---- */
struct McqRace {
    int batch, nmax, mmax;
    const int* n_in;        // [batch] waypoints of each track, or nullptr (all nmax)
    const double* ref;      // [batch][nmax][4]
    const double* nv;       // [batch][nmax][2]
    const double* alpha;    // [batch][nmax]
    double stepsize;        // stepsize_interp_after_opt
    double* xy_out;         // [batch][mmax][2] raceline_interp, or nullptr
    double* psi_out;        // [batch][mmax] heading (0 = north), or nullptr
    double* kappa_out;      // [batch][mmax]
    double* el_out;         // [batch][mmax] element lengths (closed: m of them)
    int* m_out;             // [batch] points of the interpolated raceline
    int* status;            // [batch] MCQ_OK, or MCQ_BAD_INPUT (n < 3, or the raceline needs more than mmax points)
    double* vec;            // workspace, [batch][MCQ_NVEC][nmax] (the solver's vector slab)
};
__global__ void mcq_raceline_kernel(McqRace Q);

/* ---- the same with OPEN chains among the rows (mcq_raceline_device_ends): a chain row is tph.calc_splines(path, psi_s, psi_e,
 *      use_dist_scaling=False) + calc_spline_lengths + interp_splines(incl_last_point=True) + calc_head_curv_an; el_out holds its m - 1
 *      elements and a 0.  Ring rows return the bits of mcq_raceline_kernel.  status: also MCQ_BAD_INPUT for a chain of n < 2 waypoints or a
 *      non-finite end heading. ---- */
struct McqRaceEnds {
    McqRace Q;
    const int* closed;      // [batch] != 0: a ring row; nullptr: every row is a chain
    const double* psi;      // [batch][2] (psi_s, psi_e), read for chain rows only
};
__global__ void mcq_raceline_ends_kernel(McqRaceEnds E);

/* ---- ggv velocity profile + lap time of many (track, vehicle) variants: the forward /
 *      backward quasi-steady-state sweeps of tph.calc_vel_profile (closed track, global ggv) followed by
 *      tph.calc_ax_profile / calc_t_profile, one thread per variant. ---- */
struct McqVel {
    int batch, n, nmax;
    const int* n_of_track;   // [tracks] valid entries of each kappa / el row, or nullptr (all rows: n)
    const int* track_of;     // [batch] row of kappa / el a variant uses, or nullptr (row = variant)
    const double* kappa;     // [tracks][nmax]
    const double* el;        // [tracks][nmax] element lengths (closed: n of them)
    const double* ggv;       // [batch][ng][3]  (v, ax_max, ay_max)
    int ng;
    const double* axm;       // [batch][nam][2] (v, ax_max of the machines)
    int nam;
    const double* drag;      // [batch] drag coefficient
    const double* mass;      // [batch]
    const double* vmax;      // [batch]
    double dyn_exp;
    const double* mu;        // [tracks][nmax] friction coefficient per waypoint, or nullptr (1 everywhere)
    int filt_window;         // odd width of the closed moving-average filter on the finished profile (tph.conv_filt); <= 1: none
    double* scratch;         // [2 nmax][batch]: the lap-doubled profile, variant-minor (coalesced across threads)
    double* vx_out;          // [batch][nmax]
    double* lap_time;        // [batch]
};
__global__ void mcq_vel_profile_kernel(McqVel V);

/* ---- the other forms of tph.calc_vel_profile's signature (mcq_vel_profile_device_forms): unclosed rows (n curvatures, n - 1 element
 *      lengths, a start speed and optionally an end speed; V.scratch then holds [nmax][batch]) and / or local tyre limits per waypoint
 *      in place of the ggv diagram (V.ggv / V.mu nullptr, V.ng 0).  One kernel per form: the same body as mcq_vel_profile_kernel with the
 *      form as a compile-time parameter. ---- */
struct McqVelForms {
    McqVel V;
    const double* loc_gg;    // [tracks][nmax][2] (ax_max, ay_max) per waypoint (the _locgg kernels), else unused
    const double* v_start;   // [batch] (the _open kernels), else unused
    const double* v_end;     // [batch], NaN: none for that variant, or nullptr: none at all (the _open kernels)
};
__global__ void mcq_vel_profile_open_kernel(McqVelForms F);
__global__ void mcq_vel_profile_locgg_kernel(McqVelForms F);
__global__ void mcq_vel_profile_open_locgg_kernel(McqVelForms F);

/* ---- tph.calc_ax_profile / calc_t_profile, the trajectory rows [s, x, y, psi, kappa, vx, ax] and the limit quantities of check_traj
 *      [REF main_globaltraj.py:412-421, 502-534; helper_funcs_glob/src/check_traj.py] of a batch of variants (mcq_trajectory_device).
 *      One wave per variant: the lanes form the elements' lengths, times and accelerations coalesced, lane 0 sums s and t in the order
 *      of numpy.cumsum / of the velocity kernel's lap-time loop, the limits are wave reductions of exact maxima / minima. ---- */
struct McqTraj {
    int batch, m, mmax;
    const int* m_of_track;   // [tracks] stations of each row, or nullptr (all rows: m)
    const int* track_of;     // [batch] row a variant uses, or nullptr (row = variant)
    const double* xy;        // [tracks][mmax][2]
    const double* psi;       // [tracks][mmax]
    const double* kappa;     // [tracks][mmax]
    const double* el;        // [tracks][mmax] (closed: m elements; unclosed: m - 1)
    const double* vx;        // [batch][mmax]
    int closed;
    const double* drag;      // [batch]
    const double* mass;      // [batch]
    const double* vmax;      // [batch]
    const double* ggv;       // [batch][ng][3] or nullptr
    int ng;
    const double* axm;       // [batch][nam][2] or nullptr
    int nam;
    double curvlim;
    double* traj;            // [batch][mmax][7] or nullptr
    double* t_out;           // [batch][mmax + 1] or nullptr
    double* length;          // [batch]
    double* limits;          // [batch][MCQ_TRAJ_NLIM]
    int* flags;              // [batch]
};
__global__ void mcq_trajectory_kernel(McqTraj T);

/* ---- check_traj's first block (mcq_bound_dists_device): the two boundaries p + n w_r / p - n w_l, re-sampled by interp_track's rule
 *      (mcq_bound_points_kernel, a workgroup per track and side), the minimum distance of the vehicle's four corners to every sample per
 *      station (mcq_bound_dists_kernel, grid (station blocks, tracks): the all-pairs hot path) and the minimum over a track's stations with
 *      the track's status (mcq_bound_min_kernel, a workgroup per track). ---- */
#define MCQ_BD_S 2          /* stations per thread of mcq_bound_dists_kernel: a station block is MCQ_BD_S x 256 stations */
#define MCQ_BD_TILE 256     /* boundary samples per LDS tile */
struct McqBound {
    int tracks, nmax, mmax, nbmax, mode;
    const int* n_list;       // [tracks] or nullptr (all nmax)
    const int* m_list;       // [tracks] or nullptr (all mmax)
    const double* ref;       // [tracks][nmax][4]
    const double* nv;        // [tracks][nmax][2]
    const double* xy;        // [tracks][mmax][2]
    const double* psi;       // [tracks][mmax]
    double length_veh, width_veh;
    const double* length_list;  // [tracks] or nullptr
    const double* width_list;   // [tracks] or nullptr
    double step;
    double* samples;         // scratch [tracks][2][nbmax][2]
    double* pts;             // scratch [tracks][2][nmax][2]: the raw boundaries
    double* cum;             // scratch [tracks][2][nmax + 1]: running sums of their element lengths
    int* side_status;        // scratch [tracks][2]
    double* min_dists;       // [tracks][mmax]
    double* min_dist;        // [tracks]
    int* nb_out;             // [tracks][2]
    double* bound_out;       // [tracks][2][nmax][2] or nullptr
    int* status;             // [tracks]
};
__global__ void mcq_bound_points_kernel(McqBound P);
__global__ void mcq_bound_dists_kernel(McqBound P);
__global__ void mcq_bound_min_kernel(McqBound P);

/* ---- tph.spline_approximation behind FITPACK's fit (mcq_spline_approx_device) [REF helper_funcs_glob/src/prep_track.py:39-45]: from the
 *      B-spline (knots, coefficients) of the smoothed centre line and the raw rows to the prepared rows.  Three launches:
 *      mcq_spline_length_kernel (a workgroup per track: checks, the closed raw line's running sum -> first guesses, the smoothed line's length
 *      -> the number of rows), mcq_spline_search_kernel (grid (blocks of 256 raw waypoints, tracks): scipy.optimize.fmin's one-dimensional
 *      Nelder-Mead search per waypoint, the hot path) and mcq_spline_finish_kernel (a workgroup per track: deviations, widths carried over by
 *      numpy.interp's rule, the path rows, the NaN padding).  The spline is evaluated as FITPACK's splev / fpbspl do, with the degree a
 *      compile-time parameter; knots and coefficients are staged in LDS when 3 nk <= MCQ_SPL_LDS doubles and read from HBM otherwise. ---- */
#define MCQ_SPL_LDS 3072      /* doubles of LDS for a track's knots and coefficients: nk <= 1024 knots are staged (24 KB) */
#define MCQ_SPL_MAXFUN 200    /* fmin's default budget for one variable: 200 function calls, 200 iterations */
struct McqSpline {
    int tracks, nmax, k, nkmax, mmax;
    const int* n_list;       // [tracks] or nullptr (all nmax)
    const int* nk_list;      // [tracks] or nullptr (all nkmax)
    const double* track;     // [tracks][nmax][4] raw rows, not closed
    const double* knots;     // [tracks][nkmax]
    const double* coef;      // [tracks][2][nkmax]
    double step;             // stepsize_reg
    double* tguess;          // scratch [tracks][nmax + 1]: running sums, then the first guesses
    double* ct;              // scratch [tracks][nmax + 1]: closest parameters
    double* dist;            // scratch [tracks][nmax + 1]: distances to the closest points
    double* side;            // scratch [tracks][nmax + 1]: side of the closest point (entry n is not used)
    int* npts;               // scratch [tracks]: no_points_reg_cl
    double* ref_out;         // [tracks][mmax][4]
    int* m_out;              // [tracks]
    double* ct_out;          // [tracks][nmax + 1] or nullptr
    double* dist_out;        // [tracks][nmax + 1] or nullptr
    double* dev_out;         // [tracks][2] or nullptr
    int* nonmono_out;        // [tracks] or nullptr
    int* status;             // [tracks]
};
__global__ void mcq_spline_length_kernel(McqSpline S);
__global__ void mcq_spline_search_kernel(McqSpline S);
__global__ void mcq_spline_finish_kernel(McqSpline S);

/* ---- FITPACK's periodic smoothing fit (mcq_spline_fit_device; csrc/mcq_fit.inc): one launch, a workgroup per track -- interp_track's
 *      re-sampling, the chord-length parameter, fpclos.  The triangle of the periodic system takes (2 k + 5) doubles per distinct coefficient
 *      (band k + 2, border k + 1, two right-hand sides); it lives in LDS while that is at most MCQ_FIT_LDS doubles (k = 3: n <= 565 knots) and
 *      in the handle's scratch beyond, with the same statements and the same bits. ---- */
#define MCQ_FIT_LDS 6144      /* doubles of LDS for a fit's triangle (48 KB) */
struct McqFit {
    int tracks, nmax, mimax, k, nkmax;
    const int* n_list;       // [tracks] or nullptr (all nmax)
    const double* track;     // [tracks][nmax][4] raw rows, not closed
    double step, s;          // stepsize_prep (<= 0: no re-sampling), smoothing factor
    double* cum;             // scratch [tracks][nmax + 1]: running sums of the raw line
    double* pts;             // scratch [tracks][mimax][2]: the closed points that are fitted
    double* u;               // scratch [tracks][mimax]: their parameter
    double* work;            // scratch [tracks][work_per]: B-splines, residuals, triangles, coefficients, jump rows, fpknot's tables, the segments' reduced rows
    size_t work_per;         // doubles per track
    int* nk_out;             // [tracks]
    double* knots_out;       // [tracks][nkmax]
    double* coef_out;        // [tracks][2][nkmax]
    double* fp_out;          // [tracks] or nullptr
    int* ier_out;            // [tracks]
    int* mi_out;             // [tracks] or nullptr
    double* pts_out;         // [tracks][mimax][2] or nullptr
    int* status;             // [tracks]
};
__global__ void mcq_spline_fit_kernel(McqFit P);

/* prep_track's tail [REF helper_funcs_glob/src/prep_track.py:89-98]: rows narrower than min_width grow by half the deficit on both sides. */
__global__ void mcq_min_width_kernel(int nmax, const int* n_list, double* ref_all, double min_width, int* changed_out);

/* ---- the export tables (mcq_export_device) [REF main_globaltraj.py:502-552, helper_funcs_glob/src/export_traj_ltpl.py:35-63].  Two launches:
 *      mcq_export_s_kernel (a workgroup per TRACK: the raceline's own spline lengths at the reference waypoints and their running sum -- the front
 *      half of mcq_raceline_kernel, kept in the slab's slots 6 / 7 for the second launch) and mcq_export_rows_kernel (a workgroup per variant and row block:
 *      per waypoint the nearest station of the variant's s column, then the table, a lane per output element). ---- */
#define MCQ_EX_RPT 4        /* table rows a thread of mcq_export_rows_kernel looks up */
#define MCQ_EX_ROWS (256 * MCQ_EX_RPT)      /* table rows per workgroup: every workgroup reads the variant's whole s column, so fewer, larger row
                                             * blocks read it less often (measured at config 4's shape: 4.10 ms with 256 rows, 2.47 ms with 1024; docs/NOTEBOOK.md "Export tables") */
#define MCQ_EX_TILE 1024    /* stations of the s column per LDS tile */
struct McqExport {
    int tracks, nmax, batch, mmax;
    const int* n_list;       // [tracks] or nullptr (all nmax)
    const double* ref;       // [tracks][nmax][4]
    const double* nv;        // [tracks][nmax][2]
    const double* alpha;     // [tracks][nmax]
    const int* m_of_track;   // [tracks] or nullptr (all mmax)
    const int* track_of;     // [batch] or nullptr (row = variant)
    const double* traj;      // [batch][mmax][MCQ_TRAJ_COLS]
    double* vec;             // workspace, [tracks][MCQ_NVEC][nmax] (the solver's vector slab)
    double* ltpl;            // [batch][nmax + 1][MCQ_LTPL_COLS]
    int* idx;                // [batch][nmax] or nullptr
    double* len_out;         // [tracks][nmax] or nullptr
    double* s_ref_out;       // [tracks][nmax + 1] or nullptr
    double* total_out;       // [tracks]
    int* status;             // [batch]
};
__global__ void mcq_export_s_kernel(McqExport X);
__global__ void mcq_export_rows_kernel(McqExport X);

/* ---- friction maps (mcq_fmap_create, mcq_fmap_query_device, mcq_friction_grid_device; csrc/mcq_fric.inc) [REF opt_mintime_traj/src/
 *      friction_map_interface.py, extract_friction_coeffs.py, approx_friction_map.py].  McqFmap is the device view of one map: a uniform grid of bins
 *      over the cells' bounding box in CSR form, built and uploaded once by mcq_fmap_create. ---- */
struct McqFmap {
    int cells, nbx, nby;
    double x0, y0, side;     // lower corner of the box, side of a bin: bin k of an axis starts at x0 + k * side (two roundings)
    const int* bin_start;    // [nbx * nby + 1]: bin iy * nbx + ix holds the sorted cells bin_start[.] .. bin_start[. + 1] - 1
    const double* sxy;       // [cells][2] coordinates, sorted by bin (within a bin: by original index)
    const int* sidx;         // [cells] original index of a sorted cell
    const double* mue;       // [cells] in ORIGINAL order
};
__global__ void mcq_fmap_query_kernel(McqFmap F, int count, const double* xy, double* mue_out, int* idx_out, double* dist_out);

#define MCQ_FG_ROWS 4        /* rows of a track per workgroup of mcq_friction_grid_kernel: a wave each */
struct McqFricGrid {
    McqFmap F;
    int tracks, nmax, jmax;
    const int* n_list;       // [tracks] or nullptr (all nmax)
    const double* ref;       // [tracks][nmax][4]
    const double* nv;        // [tracks][nmax][2]
    double width;            // width_opt where width_list is nullptr
    const double* width_list;   // [tracks] or nullptr
    double wbf, wbr, dn;
    double* n_out;           // [tracks][nmax + 1][jmax]
    int* cnt_out;            // [tracks][nmax + 1]
    double* mue_out;         // [tracks][4][nmax + 1][jmax]
    int* idx_out;            // [tracks][4][nmax + 1][jmax] or nullptr
    double* w_out;           // [tracks][4][nmax + 1][2] or nullptr
    int* status;             // [tracks]
};
__global__ void mcq_friction_grid_kernel(McqFricGrid G);

/* the Gaussian-basis fit on the grid kernel's outputs (mcq_friction_gauss_device) and the evaluation of either model (mcq_friction_model_device).
 * A row of the fit keeps its centred cnt x N matrix, V and its small vectors in LDS: fgs_row_doubles doubles; rows_wg rows (waves) share a workgroup. */
#define MCQ_FGS_PART 384        /* doubles of a row's exchange buffers: two buffers of three sums, or one of four wheels (64 lanes each) */
#define MCQ_FGS_ROWS 4          /* most rows per workgroup */
#define MCQ_FGS_LDS 65536       /* bytes a workgroup may take */
static inline size_t mcq_fgs_row_doubles(int jmax, int N) { return (size_t)N * ((size_t)jmax + N + 6) + MCQ_FGS_PART; }
struct McqFricGauss {
    int tracks, nmax, jmax, n_gauss, N, rows_wg;
    double rcond;            // <= 0: max(cnt, N) * DBL_EPSILON
    const double* n;         // [tracks][nmax + 1][jmax]
    const int* cnt;          // [tracks][nmax + 1]
    const double* mue;       // [tracks][4][nmax + 1][jmax]
    const int* status;       // [tracks]
    double* w_out;           // [tracks][4][nmax + 1][N + 1]
    double* cd_out;          // [tracks][nmax + 1]
    int* rank_out;           // [tracks][nmax + 1] or nullptr
    int* sweeps_out;         // [tracks][nmax + 1] or nullptr
};
__global__ void mcq_friction_gauss_kernel(McqFricGauss G);

struct McqFricModel {
    int tracks, nmax, qmax, jmax, model, centres, n_gauss, N;
    const double* q;         // [tracks][nmax + 1][qmax]
    const int* qcnt;         // [tracks][nmax + 1] or nullptr (all qmax)
    const double* w;         // [tracks][4][nmax + 1][P]
    const double* cd;        // [tracks][nmax + 1] (Gaussian model)
    const double* n;         // [tracks][nmax + 1][jmax] (MCQ_FRIC_CENTRES_FIT)
    const int* cnt;          // [tracks][nmax + 1] (MCQ_FRIC_CENTRES_FIT)
    double* mue_out;         // [tracks][4][nmax + 1][qmax]
};
__global__ void mcq_friction_model_kernel(McqFricModel M);

/* ---- friction map generation (mcq_points_in_path_device, mcq_friction_gen_device; csrc/mcq_fgen.inc) [REF main_gen_frictionmap.py,
 *      frictionmap/src/reftrack_functions.py]: matplotlib's contains_points with a radius -- agg's contour, then the crossing test -- on the
 *      reference's boundaries and grid. ---- */
#define MCQ_FGEN_TILE 512       /* contour vertices per LDS tile of the crossing test */
#define MCQ_FGEN_PPT 4          /* grid points (one x, consecutive y) per thread of mcq_fgen_mask_kernel: the edge's terms that do not depend on y are shared */
struct McqContour {
    int paths, vmax;
    const int* v_list;       // [paths] or nullptr (all vmax)
    const double* verts;     // [paths][vmax][2]
    const double* radius;    // [paths]
    double* kept;            // scratch [paths][vmax][2]: the vertices that are not within 1e-14 of their predecessor
    int* flag;               // scratch [paths][vmax]
    double* cont;            // [paths][2 vmax][2]
    int* ccount;             // [paths]
    int* status;             // [paths] or nullptr
};
__global__ void mcq_fgen_contour_kernel(McqContour C);
__global__ void mcq_fgen_points_kernel(McqContour C, int count, const double* xy, unsigned char* inside_out);

struct McqFgen {
    int tracks, nmax, cmax, maxblk;
    double cw;
    const int* n_list;       // [tracks] or nullptr (all nmax)
    const double* ref;       // [tracks][nmax][4]
    const int* inside_right; // [tracks] or nullptr (all right)
    double* bound_r;         // [tracks][nmax][2] or nullptr
    double* bound_l;
    double* grid;            // [tracks][6]
    int* count;              // [tracks]
    double* cells;           // [tracks][cmax][2] or nullptr
    int* status;             // [tracks]
    double* poly;            // scratch [tracks][2][2 nmax][2]: the polygons to test (closed: outside, inside; open: one of 2 n vertices)
    int* pcount;             // [tracks][2]
    double* prad;            // [tracks][2]
    double* cont;            // [tracks][2][4 nmax][2]: their contours (McqContour with paths = 2 tracks, vmax = 2 nmax)
    int* ccount;             // [tracks][2]
    int* rec;                // [tracks][2]: nx, ny (0 for a refused track)
    unsigned char* bits;     // [tracks][maxblk * 256]: per item the on-track flags of its MCQ_FGEN_PPT points
    int* bcount;             // [tracks][maxblk]: cells per block of 256 items, then their running sum
};
/* ---- the minimum-time NLP as functions of w (mcq_mintime_*_device; csrc/mcq_mintime.inc) [REF opt_mintime_traj/src/opt_mintime.py:143-861].
 *      Layouts: include/mcq.h.  Lane mappings: the evaluation one lane per (interval, evaluation point) -- 4 per interval, 64 intervals per workgroup;
 *      the Jacobian one lane per (interval, evaluation point, direction) -- 36 per interval, a one-tangent dual number each; the Hessian of the
 *      Lagrangian a workgroup of 192 lanes per interval, one lane per (evaluation point, unordered pair of its 9 directions) -- 180 hyper-dual
 *      evaluations; H v one lane per entry of w. ---- */
#define MCQ_MT_EVAL_LANES 4
#define MCQ_MT_JAC_LANES 36
#define MCQ_MT_HESS_NT 192
#define MCQ_MT_HESS_PAIRS 45
struct McqMtColl {
    double tau[4], C[4][4], D[4], B[4];
};
struct McqMintime {
    mcq_mintime_data d;
    mcq_mintime_opts o;
    McqMtColl c;
    int P;                   // doubles per friction row: 0, 2 or 2 n_gauss + 2
    int nwmax, ngmax;
    // evaluation
    double *g, *J, *lap, *energy, *x_opt, *u_opt, *tf_opt, *dt_opt, *ax_opt, *ay_opt, *ec_opt;
    int* status;
    double *dt_own;          // [batch][nmax]: dt_opt, or the handle's scratch where the caller takes none (the sums read it)
    double *ec_own;
    // bounds
    double *w0, *lbw, *ubw, *lbg, *ubg;
    // Jacobian
    double *blocks, *grad_J, *grad_E;
    // certificate
    const double *g_in, *blocks_in, *grad_J_in, *grad_E_in, *lam_g, *lam_x, *lbw_in, *ubw_in, *lbg_in, *ubg_in;
    double *r, *kkt;
    // Hessian of the Lagrangian (lam_g above), H v
    const double *sigma, *hblocks_in, *v;
    double *hblocks, *y;
    int nvec;
};
__host__ __device__ inline int mcq_mt_ng(int N, int safe, int energy) { return N * (27 + 2 * safe) + 4 * (N - 1) + 5 + energy; }
__host__ __device__ inline int mcq_mt_row0(int k, int safe) { return k * (27 + 2 * safe) + (k > 0 ? 4 * (k - 1) : 0); }
/* THE NLP'S MAPS, ONCE (tests/layout_check.cpp holds them to a brute-force statement).  An interval has 33 ROW SLOTS: 0 .. 26 always, 27 .. 30 (the
 * actuator rows) from k = 1 on, 31 and 32 (the safe pair) with safe_traj alone; the rows of g are the present slots in rising order, interval after
 * interval from mcq_mt_row0.  A block has 33 COLUMN SLOTS: 0 .. 28 are w[24 k ..], 29 .. 32 are U_k-1. */
#define MCQ_MT_ROWS_ALWAYS 27   // the slots below exist in every interval, each at its own number behind mcq_mt_row0: a hot loop takes them without asking
// row slot -> its offset behind mcq_mt_row0(k, safe), or -1 where the slot is absent (below slot 31 a present slot's offset is the slot itself)
__host__ __device__ inline int mcq_mt_row_off(int k, int safe, int slot)
{
    if (slot < MCQ_MT_ROWS_ALWAYS) return slot;
    if (slot < 31) return k > 0 ? slot : -1;
    return safe ? (k > 0 ? slot : slot - 4) : -1;
}
__host__ __device__ inline int mcq_mt_row_of(int k, int safe, int slot)
{
    const int off = mcq_mt_row_off(k, safe, slot);
    return off < 0 ? -1 : mcq_mt_row0(k, safe) + off;
}
// row i < mcq_mt_row0(N, safe) of g -> its interval and row slot: interval 0 has 27 + 2 safe rows, every later one 4 more
__host__ __device__ inline void mcq_mt_slot_of(int i, int safe, int* k, int* slot)
{
    const int first = 27 + 2 * safe;
    *k = i < first ? 0 : 1 + (i - first) / (first + 4);
    const int off = i - mcq_mt_row0(*k, safe);
    *slot = *k == 0 && off >= 27 ? off + 4 : off;
}
// entry i of w -> the (at most two) blocks kb and column slots cb that hold it, the block at 24 k + slot first; -1 where there is none.  X_k is also
// in block k - 1 at 24 + c.  U_k is also in the next block at 24 + c: the Jacobian's (wrap false) has a next block for k + 1 < N alone, the
// Hessian's (wrap true) is block 0 behind the last (the regularisation's cyclic term).  Nothing holds an entry past nw.
__host__ __device__ inline void mcq_mt_holders(int N, int i, bool wrap, int kb[2], int cb[2])
{
    const int k = i / 24, c = i - 24 * k;
    kb[0] = kb[1] = cb[0] = cb[1] = -1;
    if (N == 0 || i >= 5 + 24 * N) return;
    if (c < 5) {
        if (k < N) { kb[0] = k; cb[0] = c; }
        if (k >= 1) { kb[1] = k - 1; cb[1] = 24 + c; }
    } else {
        kb[0] = k; cb[0] = c;
        if (c < 9 && (wrap || k + 1 < N)) { kb[1] = k + 1 < N ? k + 1 : 0; cb[1] = 24 + c; }
    }
}
// the entry of w behind column slot `slot` of Hessian block k (slots 29 .. 32 of block 0: U_N-1; the Jacobian's block 0 has none there)
__host__ __device__ inline int mcq_mt_slot_entry(int N, int k, int slot) { return slot < 29 ? 24 * k + slot : 24 * (k > 0 ? k - 1 : N - 1) + 5 + (slot - 29); }
// a problem's own sizes: N from n_list (nmax without one), 0 -- and then nw = ng = per = 0 -- outside 2 .. nmax; per is the first periodicity row
struct McqMtSizes {
    int N, safe, energy, nw, ng, per;
};
__host__ __device__ inline int mcq_mt_intervals(const int* n_list, int nmax, int b)
{
    const int n = n_list ? n_list[b] : nmax;
    return n < 2 || n > nmax ? 0 : n;
}
__host__ __device__ inline McqMtSizes mcq_mt_sizes(const int* n_list, int nmax, int b, int safe, int energy)
{
    McqMtSizes Z;
    Z.N = mcq_mt_intervals(n_list, nmax, b);
    Z.safe = safe ? 1 : 0;
    Z.energy = energy ? 1 : 0;
    Z.nw = Z.N ? 5 + 24 * Z.N : 0;
    Z.ng = Z.N ? mcq_mt_ng(Z.N, Z.safe, Z.energy) : 0;
    Z.per = Z.N ? mcq_mt_row0(Z.N, Z.safe) : 0;
    return Z;
}
__global__ void mcq_mintime_bounds_kernel(McqMintime M);
__global__ void mcq_mintime_eval_kernel(McqMintime M);
__global__ void mcq_mintime_sum_kernel(McqMintime M);
__global__ void mcq_mintime_jac_kernel(McqMintime M);
__global__ void mcq_mintime_kkt_kernel(McqMintime M);
__global__ void mcq_mintime_hess_kernel(McqMintime M);
__global__ void mcq_mintime_hessvec_kernel(McqMintime M);
/* ---- the regularised primal-dual Newton step from the resident blocks (mcq_mintime_step_device; csrc/mcq_mtstep.inc): a workgroup per problem,
 *      a front of 94 per interval -- 57 pivots, a Schur complement of 37 passed on -- in LDS; the factor kept per interval is the front's 94 x 57
 *      panel, and once per problem the last 37 x 37; behind them one residual vector per right-hand side. ---- */
#define MCQ_MTS_PANEL (94 * 57)
#define MCQ_MTS_LAST (37 * 37)
struct McqMtStep {
    int batch, nmax;
    const int* n_list;
    int safe, energy, nwmax, ngmax, nvec, refine;
    const double *hblocks, *blocks, *grad_energy, *dw, *dg, *rhs;
    double *sol, *res;
    int *inertia, *status;
    double* work;            // [batch][work_per]
    size_t work_per;         // doubles per problem: nmax MCQ_MTS_PANEL + MCQ_MTS_LAST + nvec (nwmax + ngmax)
};
__host__ __device__ inline size_t mcq_mts_work(int nmax, int nvec, int nwmax, int ngmax)
{
    return (size_t)nmax * MCQ_MTS_PANEL + MCQ_MTS_LAST + (size_t)nvec * ((size_t)nwmax + ngmax);
}
__global__ void mcq_mintime_step_kernel(McqMtStep S);

__global__ void mcq_fgen_bounds_kernel(McqFgen G);
__global__ void mcq_fgen_mask_kernel(McqFgen G);
__global__ void mcq_fgen_scan_kernel(McqFgen G);
__global__ void mcq_fgen_scatter_kernel(McqFgen G);
