/*
 * mcq.h -- C ABI of the MI355X-native minimum-curvature raceline QP engine (libmcq.so).
 *
 * Drop-in boundary.  The reference has NO native interface for this path: it calls the
 * third-party Python functions
 *     trajectory_planning_helpers.opt_min_curv.opt_min_curv   [REF main_globaltraj.py:264-271, 344-350]
 *     trajectory_planning_helpers.iqp_handler.iqp_handler     [REF main_globaltraj.py:273-284]
 * which end in quadprog.solve_qp (C).  The entry points below are what a ctypes binding inside those two Python
 * functions binds instead (INTEGRATION.md shows the stub).  Plain pointers and sizes only; no torch / numpy types.
 *
 * One "problem" = one closed reference track (or an open chain with end headings: mcq_solve_batch_ends below):
 *     reftrack  [n][4] row-major double  = [x_m, y_m, w_tr_right_m, w_tr_left_m]   (producer [REF prep_track.py:39-45,104])
 *     normvec   [n][2] row-major double  = unit normals pointing right             (producer [REF prep_track.py:50-51])
 *     scaling   [n]    double            = s_i = l_i / l_{i+1}, the only information opt_min_curv needs from the
 *                                          dense 4n x 4n matrix `A` the reference passes [REF main_globaltraj.py:267]
 *                                          (s_i = -A[4i+2][4i+5], s_{n-1} = A[4n-2][1]); NULL => all ones
 *                                          (calc_splines(use_dist_scaling=False), the iqp_handler re-spline).
 * Result per problem: alpha[n] (lateral shift along the normal, metres; consumer [REF main_globaltraj.py:371-376]),
 * curv_error_max (the opt_min_curv post-check that iqp_handler terminates on), status.
 *
 * The QP solved is exactly the one tph hands to quadprog:
 *     minimise   1/2 a'Ha + f'a,   H = E'E,  f = MCQ_F_SCALE * E' k_ref
 *     subject to -(w_l - w_veh/2) <= a <= (w_r - w_veh/2),     |k_ref + E a| <= kappa_bound
 *
 * Ownership: caller owns every buffer passed in; the library copies to / from device memory it owns inside the
 * handle and retains no caller pointer after a call returns.  Threading: one host thread per handle at a time.
 * Errors: functions return 0 on success or a negative MCQ_E_* code (mcq_last_error() gives text); per-problem
 * outcomes are in status_out[].  The library never calls exit().
 */
#ifndef MCQ_H
#define MCQ_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MCQ_F_SCALE 2.0 /* the factor-2 quirk of tph's quadprog call -- reproduced, not fixed */

/* per-problem status (status_out[]) */
enum {
    MCQ_OK = 0,
    MCQ_INFEASIBLE = 1,      /* w_r + w_l < w_veh somewhere  -> tph raises RuntimeError("Problem not solvable, ...") */
    MCQ_NOT_PD = 2,          /* Cholesky pivot <= 0            -> quadprog raises ValueError("matrix G is not positive definite") */
    MCQ_ITER_CAP = 3,        /* iteration cap hit -- of the Goldfarb-Idnani fallback too (20 n + 2000 steps; not observed) --, or of the interior
                               * point + block pivoting on a handle that has no Goldfarb-Idnani slot for rings this long (see MCQ_ALG_GI below) */
    MCQ_BAD_INPUT = 4,       /* n < 3, non-finite input */
    MCQ_KAPPA_INFEASIBLE = 5, /* curvature rows cannot be satisfied -> quadprog raises ValueError("constraints are inconsistent, no solution") */
    MCQ_KAPPA_ACTIVE = 6,     /* box-only optimum violates a curvature row and the curvature-row phase is disabled (check_kappa < 0).
                               * (Rounds 1-4 also returned it for more active curvature rows than the working-set arrays hold -- 120 in LDS,
                               * 512 through an overflow slot; such problems now go through the Goldfarb-Idnani path, which has no limit --
                               * round 6: ALL of them, so that a problem's route and the last bits of its result do not depend on what else is in
                               * the launch.  On a handle without a Goldfarb-Idnani slot -- rings beyond the byte cap below -- the overflow slots
                               * serve as before and this status can come back for more than 512 rows.)  Also returned by that path when
                               * check_kappa < 0 and the returned point violates a curvature row. */
    MCQ_RING_OVERFLOW = 7,    /* mcq_iqp_device / mcq_iqp_batch only: the re-sampled raceline of an IQP round needs more waypoints than
                               * the buffers hold (nmax / nmax_out) -- not an input error of the QP (that stays MCQ_BAD_INPUT) */
    MCQ_KAPPA_NO_SLOT = 8,    /* returned only on a handle WITHOUT Goldfarb-Idnani slots (rings beyond the byte cap): more than eight problems of
                               * one launch with more than 120 active curvature rows each.  Everywhere else such problems are solved by the
                               * Goldfarb-Idnani path inside the same kernel, on every entry point */
    MCQ_SINGULAR = 9          /* mcq_mintime_step_device only: a pivot of the primal-dual matrix's LDL^T is zero or not finite */
};

/* library-level error codes (negative return values) */
enum {
    MCQ_E_ARG = -1,     /* NULL / out-of-range argument */
    MCQ_E_DEVICE = -2,  /* HIP runtime error (no device, launch failure, out of memory) */
    MCQ_E_TOO_LARGE = -3
};

typedef struct mcq_handle mcq_handle; /* opaque; owns device buffers + one HIP stream on one device */

typedef struct {
    int n;                  /* waypoints */
    const double* reftrack; /* [n][4] */
    const double* normvec;  /* [n][2], or NULL for every problem of a batch: derived on the device (with the scalings) */
    const double* scaling;  /* [n] or NULL */
    double kappa_bound;     /* veh_params.curvlim  [REF params/racecar.ini:49] */
    double w_veh;           /* optim_opts.width_opt [REF params/racecar.ini:72] */
} mcq_problem;

typedef struct {
    int algorithm;      /* MCQ_ALG_DEFAULT (0; any value other than MCQ_ALG_GI): interior point -> block pivoting on the identified vertex,
                         * with the Goldfarb-Idnani path below as the fallback of every problem that phase does not settle;
                         * MCQ_ALG_GI (1): EVERY problem through the engine's Goldfarb-Idnani dual active-set path (quadprog's algorithm
                         * [REF requirements.txt:3 via tph.opt_min_curv]: one constraint enters per iteration, ratio test, drops -- finite by
                         * construction; a reference mode: 8.1 k solves/s on 1024 rings of 2000 waypoints, a twelfth of the default path's rate).
                         * Memory of that path (round 6): FULL slots (2 nmax^2 doubles: a working set of up to nmax constraints) for the fallback,
                         * as many as $MCQ_GI_BYTES (default 16 GB) hold, at most 512, never more than the batch -- and NONE where one slot exceeds
                         * the cap (rings above ~32 000 waypoints) or the allocation is refused: the launch then runs without the fallback and
                         * reports what interior point + block pivoting left (MCQ_ITER_CAP ...), it does not fail; SMALL slots (working sets of up
                         * to max(128, nmax / 8) constraints, 4.6 MB at nmax = 2000) for MCQ_ALG_GI, one per resident workgroup (2.4 GB for 512),
                         * a problem that outgrows its small slot moving into a full one.  MCQ_ALG_GI without any slot to be had is MCQ_E_DEVICE.
                         * mcq_solve_host_pipelined / mcq_solve_device_stream keep MCQ_ALG_GI on ONE compute stream.  Minimum-curvature
                         * objective only.  (Until round 4 this field was `band_e`, ignored since E is applied through the spline system.) */
    int max_ipm_iter;   /* 0 => default 60 */
    int max_as_iter;    /* 0 => default 60 */
    int refine_steps;   /* fp64 residual-refinement rounds on the final active set; <0 => default 2 */
    int check_kappa;    /* curvature rows |k_ref + E a| <= kappa_bound: 0 or 1 => carried (the default: a zero-initialised mcq_opts
                         * solves the QP the reference solves); < 0 => skipped (box-only QP; a violated row is then reported as
                         * MCQ_KAPPA_ACTIVE instead of being enforced) */
    int objective;      /* MCQ_OBJ_MIN_CURV (0, default) or MCQ_OBJ_SHORTEST_PATH: the QP of tph.opt_shortest_path
                         * [REF main_globaltraj.py:286-290] on the same box rows -- H = cyclic tridiagonal
                         * (4 |n_i|^2 on the diagonal, -2 n_i.n_{i+1} beside it), f_i = 2 n_i.(2 p_i - p_{i-1} - p_{i+1}),
                         * deviations clipped at 0.001 m instead of rejected.  normvec is required; scaling, kappa_bound
                         * and the curvature rows are ignored and curv_err_out is 0. */
    int warm_start;     /* 1: start from the working sets that the preceding mcq_relinearise_device call on this handle carried
                         * over from the preceding solve of the same batch (IQP passes 2+): the exchange alone, no interior point,
                         * unless it runs out of 12 rounds (then the cold path; mcq_info.second_attempt & 2).  Ignored when no such
                         * working sets are at hand.  The result is an exact KKT vertex of the same QP either way.  Default 0.
                         * A warm start that applies takes the ONE launch in every entry that would otherwise slice the batch --
                         * mcq_solve_device, and likewise mcq_solve_host / mcq_solve_batch / mcq_solve_batch_ends, which until then
                         * sliced a batch of 512 or more and dropped the warm start silently. */
} mcq_opts;
#define MCQ_OBJ_MIN_CURV 0
#define MCQ_OBJ_SHORTEST_PATH 1
#define MCQ_ALG_DEFAULT 0
#define MCQ_ALG_GI 1

/* per-problem diagnostics (optional output) */
typedef struct {
    int ipm_iters;      /* interior-point iterations (one factorisation each) */
    int as_iters;       /* active-set (block pivoting) iterations (one factorisation each) */
    int n_active_box;   /* box rows active at the optimum */
    int n_active_kappa; /* curvature rows active at the optimum */
    double kappa_max;   /* max_i |k_ref_i + (E a)_i| at the returned a */
    double kkt_res;     /* max free-gradient magnitude relative to max |f| */
    /* device wall-clock (s_memrealtime, 100 MHz ticks) spent by this problem's workgroup in the phases of the solver
     * kernel: [0] factorisations, [1] solves, [2] gradients (E, E' through the spline system), [3] whole kernel (assembly included),
     * [4] / [5] the interior-point / the active-set phase, [7] curvature check, (rare) curvature-row phase, outputs;
     * [6] the same span as [3] in shader-clock cycles (s_memtime): [6] / [3] x 100 MHz = the clock the CU actually ran at */
    long long ticks[8];
    int refine_rounds;  /* fp64 refinement rounds run on the final working set (<= opts.refine_steps) */
    int second_attempt; /* bit 0: the active-set phase ran out of its first budget and the interior point was resumed to
                           mu = 1e-13 (degenerate / very ill-conditioned instance); bit 1: a warm start (mcq_opts.warm_start)
                           was abandoned for the cold path */
    int f32_factorisations;  /* of ipm_iters: factorisations whose records were stored as floats (the first interior-point
                                iterations, while the dual residual is far above what such records can resolve; round 4) */
    int gi_iters;       /* iterations (full + partial steps) of the Goldfarb-Idnani path, 0 if it did not run for this problem
                           (second_attempt bit 2 says that it ran, bit 3 that its final polish through the block-pivoting phase did not
                           settle and the Goldfarb-Idnani iterate itself is returned: feasible / optimal to its own 2e-9 m tolerances;
                           bits 4-7: the status the solver kernel had left for the problem -- why this path ran) */
} mcq_info;

int mcq_create(int device_id, mcq_handle** out);
void mcq_destroy(mcq_handle* h);
const char* mcq_last_error(void);
void mcq_default_opts(mcq_opts* o);

/* Host-buffer entry point == what opt_min_curv binds.  alpha_out is the concatenation of the per-problem alpha
 * vectors (sum of n over the batch); curv_err_out/status_out/info_out have `batch` entries (info_out may be NULL). */
int mcq_solve_batch(mcq_handle* h, const mcq_problem* probs, int batch, const mcq_opts* opts, double* alpha_out,
                    double* curv_err_out, int* status_out, mcq_info* info_out);

/* ---- open chains (tph.opt_min_curv(..., closed=False, psi_s, psi_e, fix_s, fix_e)) ----------------------------------------------------------
 * One record per problem of the batch.  closed != 0: the problem is a ring, solved exactly as by mcq_solve_batch (bitwise; the other fields
 * are ignored).  closed == 0: the n waypoints are an OPEN chain of n - 1 splines whose end headings are psi_s / psi_e (rad, tph convention: 0
 * points north, the heading vector is (cos(psi + pi/2), sin(psi + pi/2))).  The spline system loses the couplings between waypoint n - 1 and
 * waypoint 0 and gains the heading rows (DESIGN.md "Open chains"); E, f, the curvature rows and the curvature-error post-check follow.
 *   - scaling[n]: entries 0..n-3 are the inner joints' s_i = l_i / l_(i+1) (s_i = -A[4i+2][4i+5] of the open calc_splines matrix,
 *     mcq_les_scalings_open); entries n-2, n-1 are not read; NULL => all ones.
 *   - fix_s / fix_e pin the first / last waypoint to |alpha| <= MCQ_FIX_HALF_WIDTH (applied before the infeasibility check, like tph).
 *   - The heading rows use the UNIT heading vectors, unscaled (tph.opt_min_curv's q_x / q_y); tph.calc_splines scales its own heading rows by
 *     the first / last element length -- a quirk reproduced, not fixed (MCQ_HEADING_SCALE).
 *   - A chain needs normvec (no derived normals) and the minimum-curvature objective: MCQ_E_ARG otherwise.  A chain of more than
 *     MCQ_CHAIN_MAXN waypoints, or a non-finite psi_s / psi_e, is MCQ_BAD_INPUT for that problem.
 * Mixed batches of rings and chains are allowed; ends == NULL is exactly mcq_solve_batch. */
#define MCQ_FIX_HALF_WIDTH 0.05
#define MCQ_HEADING_SCALE 1.0   /* opt_min_curv's heading rows: unit vectors (calc_splines scales its own by el_lengths[0] / [-1]) */
#define MCQ_CHAIN_MAXN 2048
typedef struct {
    int closed;         /* != 0: ring (the other fields are ignored) */
    int fix_s, fix_e;   /* pin the first / last waypoint (chains only) */
    double psi_s, psi_e;  /* end headings (chains only) */
} mcq_ends;
int mcq_solve_batch_ends(mcq_handle* h, const mcq_problem* probs, const mcq_ends* ends, int batch, const mcq_opts* opts, double* alpha_out,
                         double* curv_err_out, int* status_out, mcq_info* info_out);

/* Device-resident entry points (uniform n, inputs already in HBM; used by bench.py, the IQP driver and the multi-GPU
 * shard path).  All pointers are DEVICE pointers on the handle's device; layouts as above with a leading batch axis:
 * reftrack [batch][n][4], normvec [batch][n][2], scaling [batch][n] or NULL, alpha_out [batch][n],
 * curv_err_out [batch], status_out [batch], info_out [batch] or NULL.  Asynchronous on the handle's stream;
 * mcq_sync() waits.  mcq_stream() returns the hipStream_t (as void*) so callers can record events on it.
 *
 * mcq_solve_device runs a batch of MORE than one residency round -- two workgroups per compute unit of the device: from 513 problems on 256
 * CUs; $MCQ_DEVICE_SLICE_MIN gives the smallest sliced batch instead -- as TWO launches: problems [0, (batch + 1) / 2) on the handle's stream, the others on its second compute stream, both
 * over their rows of the one workspace.  A later such call's slice is ordered behind this call's slice on the same stream only, so the
 * slowest problems of one launch finish while the next launch fills the slots they have left: a caller that streams batches through this
 * entry gets the overlap of mcq_solve_device_stream without listing its steps up front and without a second workspace.  The handle still
 * behaves like ONE in-order stream: every other entry, mcq_sync, the copies and mcq_stream first order the handle's stream behind a pending
 * slice, and a sliced call skips the join of its two streams only while it provably touches nothing the other stream of an earlier,
 * un-joined call may still be working on (same batch and n; its slices' output rows clear of the other slices' of those calls; neither
 * call reading what the other writes -- interval checks on addresses; a loop over one set of buffers, over two in turn, or over fresh ones
 * per call stays overlapped).  Results are bitwise those of the one launch.  One launch as before: smaller batches, a warm start that
 * applies, MCQ_OBJ_SHORTEST_PATH, MCQ_ALG_GI, a handle whose mcq_stream the caller has taken (what it enqueues there the handle cannot see),
 * and $MCQ_DEVICE_ONE_LAUNCH=1 (A/B knob).  $MCQ_DEVICE_SLICE_TRACE=1: one line per call on stderr saying which path it took.  The ragged
 * and fp32 entries below keep the one launch. */
int mcq_solve_device(mcq_handle* h, int batch, int n, const double* reftrack, const double* normvec,
                     const double* scaling, double kappa_bound, double w_veh, const mcq_opts* opts, double* alpha_out,
                     double* curv_err_out, int* status_out, mcq_info* info_out);
/* The same with per-problem sizes: n_list [batch] (device) waypoints per problem, every array strided by nmax
 * (reftrack [batch][nmax][4], ...).  This is what a batch of IQP runs needs: N changes from pass to pass and differs
 * between tracks [REF main_globaltraj.py:273-284]. */
int mcq_solve_device_ragged(mcq_handle* h, int batch, int nmax, const int* n_list, const double* reftrack,
                            const double* normvec, const double* scaling, double kappa_bound, double w_veh,
                            const mcq_opts* opts, double* alpha_out, double* curv_err_out, int* status_out,
                            mcq_info* info_out);

/* mcq_solve_device_ragged with per-problem vehicle parameters: kappa_bound_list / w_veh_list [batch] (DEVICE arrays; either may
 * be NULL, then the scalar applies to every problem) -- what mcq_problem.{kappa_bound,w_veh} are to the host-buffer entry.  The
 * shape of a vehicle-width sweep over resident tracks [REF params/racecar.ini:49,72; BASELINE config 4]. */
int mcq_solve_device_ragged_params(mcq_handle* h, int batch, int nmax, const int* n_list, const double* reftrack,
                                   const double* normvec, const double* scaling, double kappa_bound, double w_veh,
                                   const double* kappa_bound_list, const double* w_veh_list, const mcq_opts* opts,
                                   double* alpha_out, double* curv_err_out, int* status_out, mcq_info* info_out);

/* fp32 at the boundary (BASELINE config 5: 65536 tracks, alpha collected with one all-gather): as mcq_solve_device, with
 * the tracks stored as float in HBM (reftrack [batch][n][4], normvec [batch][n][2] or NULL, scaling [batch][n] or NULL) and
 * alpha_out [batch][n] written as float.  The arithmetic in between is the fp64 engine, unchanged -- cond(H) = 1e9..1e12
 * leaves no room for fp32 factors -- so the result is the exact QP solution OF THE ROUNDED INPUTS, rounded once more on
 * the way out (|alpha| < 2^3 m => 2.4e-7 m); how far the rounded inputs move the solution is a property of the QP, not of
 * the engine (measured in tests/test_gpu_parity.py).  With normvec == NULL the normals and scalings are derived in fp64 from
 * the float x, y (preferred: float normals are unit vectors only to 6e-8).  curv_err_out stays double.
 * MCQ_OBJ_SHORTEST_PATH: solved on the widened rows and normals where normvec is given (H_ii = 4 |n_i|^2 takes float normals as they
 * are); with normvec == NULL, and through mcq_solve_device_f32_rows / mcq_solve_batch_f32 below (which always derive their normals), the
 * objective is refused with MCQ_E_ARG, as on every entry without normals (tests/sp_checks.py: check_f32). */
int mcq_solve_device_f32(mcq_handle* h, int batch, int n, const float* reftrack, const float* normvec,
                         const float* scaling, double kappa_bound, double w_veh, const mcq_opts* opts, float* alpha_out,
                         double* curv_err_out, int* status_out, mcq_info* info_out);

/* fp32 rows in the layout that keeps the QP's accuracy (round 3).  The QP depends on the coordinates only through differences
 * of neighbouring waypoints (x', x'' of the closed spline), so rounding ABSOLUTE coordinates to float (ulp 1.2e-4 m at |x| = 1.9 km)
 * throws away what the 3 m steps carry: measured 2e-3 m on alpha at N = 2000.  MCQ_F32_INCREMENTS stores the ring as float
 * increments -- row i = [x_{i+1} - x_i, y_{i+1} - y_i, w_tr_right_i, w_tr_left_i], row n-1 closing the ring -- plus an optional fp64
 * origin per track (alpha does not depend on it): the device rebuilds x, y by an fp64 running sum whose closure defect (the float
 * increments do not sum to zero exactly: ~1e-5 m) is spread evenly over the n increments.  Measured: |alpha - alpha(fp64 rows)|
 * <= 5e-6 m at N = 2000, the same as rounding the two WIDTH columns alone; stated tolerance of BASELINE config 5: 1e-4 m
 * (tests/test_gpu_parity.py::test_fp32_boundary_full_size).  Normals and scalings are always derived on the device in fp64.
 * layout = MCQ_F32_ABSOLUTE takes rows [x, y, w_r, w_l] like mcq_solve_device_f32 (origin added if given). */
#define MCQ_F32_ABSOLUTE 0
#define MCQ_F32_INCREMENTS 1
/* device-resident: reftrack [batch][n][4] float, origin [batch][2] double or NULL, alpha_out [batch][n] float (DEVICE pointers) */
int mcq_solve_device_f32_rows(mcq_handle* h, int batch, int n, int layout, const float* reftrack, const double* origin,
                              double kappa_bound, double w_veh, const mcq_opts* opts, float* alpha_out, double* curv_err_out,
                              int* status_out, mcq_info* info_out);
/* host buffers (SURVEY.md section 8b's `mcq_solve_batch_f32`): the same for a uniform batch in HOST memory -- float rows in, float
 * alpha out, half the PCIe bytes of mcq_solve_host; curv_err_out / status_out / info_out (may be NULL) in host memory.  Blocking. */
int mcq_solve_batch_f32(mcq_handle* h, int batch, int n, int layout, const float* reftrack, const double* origin,
                        double kappa_bound, double w_veh, const mcq_opts* opts, float* alpha_out, double* curv_err_out,
                        int* status_out, mcq_info* info_out);

/* The pieces of the fp32 boundary on their own: the very launches the three entries above make, on DEVICE pointers, asynchronous on the
 * handle's stream.  Input and output must not overlap.  MCQ_E_ARG for a null handle or pointer (origin may be NULL), batch <= 0, n <= 0,
 * count == 0 or a layout other than the two above.
 * mcq_f32_rows_device: what mcq_solve_device_f32_rows does before its solver launch -- reftrack_out [batch][n][4] double = the rows the
 *   engine sees (x, y rebuilt or origin added per `layout`, the widths widened): input for mcq_prep_device, mcq_raceline_device,
 *   mcq_export_device.  No solver workspace is touched: any n.
 * mcq_f32_widen_device / mcq_f32_narrow_device: dst[i] = (double)src[i] (exact) / dst[i] = (float)src[i] (round to nearest even, as
 *   alpha on the way out), count values: any fp64 result at half the bytes before an all-gather. */
int mcq_f32_rows_device(mcq_handle* h, int batch, int n, int layout, const float* reftrack, const double* origin, double* reftrack_out);
int mcq_f32_widen_device(mcq_handle* h, size_t count, const float* src, double* dst);
int mcq_f32_narrow_device(mcq_handle* h, size_t count, const double* src, float* dst);

/* The front half of prep_track on the device [REF helper_funcs_glob/src/prep_track.py:48-51]: unit normals (pointing
 * right) and spline scalings s_i = l_i / l_{i+1} of the closed distance-scaled cubic spline through the reference line --
 * what tph.calc_splines(path) returns as normvec_normalized and encodes in its matrix.  reftrack [batch][nmax][4],
 * n_list [batch] or NULL (all nmax); outputs normvec_out [batch][nmax][2] and / or scaling_out [batch][nmax] (either may
 * be NULL); status_out [batch].  The solve entry points derive the same quantities themselves when they are called with
 * normvec == NULL (then `scaling` is ignored).  Asynchronous on the handle's stream. */
int mcq_prep_device(mcq_handle* h, int batch, int nmax, const int* n_list, const double* reftrack, double* normvec_out,
                    double* scaling_out, int* status_out);

/* The check prep_track runs on the normals [REF helper_funcs_glob/src/prep_track.py:57-59] -- tph.check_normals_crossing(track,
 * normvec_normalized, horizon = 10): do the normal segments [p - w_left n, p + w_right n] of two waypoints at most `horizon`
 * apart intersect?  reftrack [batch][nmax][4], normvec [batch][nmax][2], n_list [batch] or NULL (all nmax);
 * crossing_out [batch] (device) = 1 / 0, or -1 where tph raises RuntimeError (horizon >= n).  Asynchronous on the handle's
 * stream. */
int mcq_normals_crossing_device(mcq_handle* h, int batch, int nmax, const int* n_list, const double* reftrack,
                                const double* normvec, int horizon, int* crossing_out);

/* Device-side glue of tph.iqp_handler between two passes (what upstream does on the host with two dense 4N x 4N spline
 * solves per pass): raceline = refline + alpha_scale * alpha * normal; closed spline through it (unit scalings);
 * arclength re-sampling at ~stepsize (tph.create_raceline); track widths shifted by -/+ alpha and carried over linearly
 * (tph.interp_track_widths); unit normals of the closed spline through the re-sampled ring
 * (tph.calc_splines(use_dist_scaling=False)).  All pointers DEVICE pointers, arrays strided by nmax; `live` [batch] or
 * NULL selects the tracks to process; n_out [batch] receives the new waypoint counts; status_out [batch] MCQ_OK or
 * MCQ_BAD_INPUT (new ring would have < 3 or > nmax points; the IQP loop reports that as MCQ_RING_OVERFLOW).  Input and output buffers must differ.  Asynchronous on
 * the handle's stream.  Side effect inside the handle: the working sets the preceding solve left for these tracks are carried to
 * the re-sampled rings (new point -> nearer end of its old segment), for mcq_opts.warm_start of the next pass. */
int mcq_relinearise_device(mcq_handle* h, int batch, int nmax, const int* n_in, const double* reftrack_in,
                           const double* normvec_in, const double* alpha, const int* live, double alpha_scale,
                           double stepsize, double* reftrack_out, double* normvec_out, int* n_out, int* status_out);
/* ggv velocity profile and lap time of a batch of (track, vehicle) variants -- what the lap-time-matrix sweep of the
 * reference runs per cell [REF main_globaltraj.py:400-422, 460-493]: tph.calc_vel_profile (closed track, global ggv, no
 * filter, mu = 1 -- mcq_vel_profile_device_opts below takes both; every step of upstream's solver: fixed-point lateral limit over all ggv rows, sweeps gated on the acceleration-phase
 * starts and on v_max, one look-ahead round in the backward sweep) followed by calc_ax_profile / calc_t_profile (lap time as
 * the sum of 2 l / (v_a + v_b)).  One device thread per variant.  A variant whose ggv or machine table ends below its v_max
 * (tph raises RuntimeError) gets lap_time NaN and a vx_out row of NaNs (never stale buffer contents).  All pointers DEVICE pointers:
 * kappa / el_lengths [tracks][nmax] (n valid entries each), track_of [batch] (row used by a variant) or NULL (row =
 * variant), ggv [batch][n_ggv][3] (v, ax_max, ay_max), ax_max_machines [batch][n_machines][2], drag_coeff / m_veh / v_max
 * [batch]; outputs vx_out [batch][nmax], lap_time_out [batch].  Asynchronous on the handle's stream. */
int mcq_vel_profile_device(mcq_handle* h, int batch, int n, int nmax, const int* track_of, const double* kappa,
                           const double* el_lengths, const double* ggv, int n_ggv, const double* ax_max_machines,
                           int n_machines, const double* drag_coeff, const double* m_veh, const double* v_max,
                           double dyn_model_exp, double* vx_out, double* lap_time_out);

/* The same over tracks of different lengths: n_of_track [tracks] (device) = valid entries of each kappa / el_lengths row (rows
 * strided by nmax); a variant whose row has fewer than 2 or more than nmax entries gets lap_time NaN.  This is the shape of
 * BASELINE config 4's sweep: (reference track x vehicle width) racelines from mcq_raceline_device, each shared by a grid of
 * ggv / top-speed variants. */
int mcq_vel_profile_device_ragged(mcq_handle* h, int batch, int nmax, const int* n_of_track, const int* track_of,
                                  const double* kappa, const double* el_lengths, const double* ggv, int n_ggv,
                                  const double* ax_max_machines, int n_machines, const double* drag_coeff,
                                  const double* m_veh, const double* v_max, double dyn_model_exp, double* vx_out,
                                  double* lap_time_out);

/* The same two entries with the options of tph.calc_vel_profile that main_globaltraj.py reads from its parameter file
 * [REF main_globaltraj.py:400-410, params/racecar.ini:53-57: vel_calc_opts] or leaves at their defaults: dyn_model_exp; filt_window --
 * tph.conv_filt's closed moving average of that (odd) width over the finished profile, lap time from the filtered profile (0 or 1:
 * none; an even width, where tph raises RuntimeError, or one wider than the ring gives lap_time NaN); mu -- a friction coefficient per
 * waypoint, DEVICE pointer [tracks][nmax] like kappa, or NULL for 1 everywhere (tph's `mu` argument; the reference passes none).
 * n_of_track NULL: every row has n entries (mcq_vel_profile_device); otherwise n is ignored (.._ragged). */
typedef struct mcq_vel_opts {
    double dyn_model_exp;
    int filt_window;
    int reserved_;
    const double* mu;
} mcq_vel_opts;
int mcq_vel_profile_device_opts(mcq_handle* h, int batch, int n, int nmax, const int* n_of_track, const int* track_of,
                                const double* kappa, const double* el_lengths, const double* ggv, int n_ggv,
                                const double* ax_max_machines, int n_machines, const double* drag_coeff, const double* m_veh,
                                const double* v_max, const mcq_vel_opts* opts, double* vx_out, double* lap_time_out);

/* The whole signature of tph.calc_vel_profile on the device: the entry above plus its two other forms.
 *   closed == 0 -- UNCLOSED rows: a row of n curvatures has n - 1 element lengths (el_lengths keeps the layout [tracks][nmax]; entry n - 1
 *     of a row is not read).  After the lateral limit and the cut at v_max, v[0] = min(v[0], v_start); one forward sweep over the n points (the
 *     lap is not doubled); v[n-1] = min(v[n-1], v_end) where an end speed is given; one backward sweep.  v_start: DEVICE [batch], required.
 *     v_end: DEVICE [batch], or NULL (no variant has one); a NaN entry means none for that variant.  Negative v_start / v_end count as 0, as
 *     upstream.  filt_window is tph.conv_filt(closed=False): only entries w .. n-1-w, w = (filt_window - 1) / 2, are averaged, both ends
 *     keep their unfiltered values bit for bit.  lap_time_out is the time over the n - 1 elements, sum of 2 l / (v_a + v_b): +inf where
 *     v_a + v_b == 0 (two points, v_start = v_end = 0) -- the formula's own value, not an error and not a NaN.
 *     With closed != 0, v_start and v_end are not read.
 *   loc_gg -- LOCAL LIMITS: DEVICE [tracks][nmax][2] = (ax_max, ay_max) per waypoint, indexed like kappa / mu, in place of the diagram, for
 *     closed and unclosed rows.  Then ggv must be NULL, n_ggv 0 and mu NULL (upstream's "either ggv and optionally mu OR loc_gg"); anything
 *     else, and neither ggv nor loc_gg, is MCQ_E_ARG.  The lateral limit is sqrt(ay_max_i R_i) without iteration; a step takes |ax_max| and
 *     ay_max of the point it leaves, the look-ahead of the backward sweep those of the point it reaches; machine table and drag as before.
 *     Only the machine table is range-checked against v_max.
 *   dyn_model_exp, filt_window, mu: as in mcq_vel_opts.  The other arguments: as in mcq_vel_profile_device_opts.  The caller owns every
 *     buffer; the handle owns the scratch ([2 nmax][batch] doubles for closed rows, [nmax][batch] for unclosed ones, grown on demand).
 * NaN rules: lap_time NaN and a vx_out row of NaNs for a bad row length (n < 2, n > nmax), a ggv / machine table that ends below v_max, an
 *   even filter window or one wider than the row, and a non-finite v_start.
 * CAVEAT (open question): the lateral limit of the unclosed + ggv form is iterated exactly as for closed rows (first estimate from the mean
 *   mu, at most 100 rounds, 0.5 %), because the project's specification oracle/vel_ref.py does so.  Whether upstream iterates there or refines
 *   once could not be checked against the package itself; the kernel keeps that step in one place.
 * Asynchronous on the handle's stream. */
typedef struct mcq_vel_forms {
    double dyn_model_exp;
    int filt_window;
    int closed;
    const double* mu;
    const double* loc_gg;
    const double* v_start;
    const double* v_end;
} mcq_vel_forms;
int mcq_vel_profile_device_forms(mcq_handle* h, int batch, int n, int nmax, const int* n_of_track, const int* track_of,
                                 const double* kappa, const double* el_lengths, const double* ggv, int n_ggv,
                                 const double* ax_max_machines, int n_machines, const double* drag_coeff, const double* m_veh,
                                 const double* v_max, const mcq_vel_forms* forms, double* vx_out, double* lap_time_out);

/* What main_globaltraj.py runs between the QP and the velocity profile [REF main_globaltraj.py:371-387], batched on the device:
 * tph.create_raceline (raceline = refline + alpha * normal, closed cubic spline through it with unit scalings, re-sampled at
 * ~stepsize = stepsize_interp_after_opt) and tph.calc_head_curv_an (heading and curvature from the spline's derivatives).
 * Inputs strided by nmax as in mcq_solve_device_ragged (n_in [batch] or NULL: all nmax); outputs strided by mmax:
 * raceline_out [batch][mmax][2] (or NULL), psi_out [batch][mmax] (heading, 0 = north, [-pi, pi); or NULL), kappa_out and
 * el_lengths_out [batch][mmax] -- the two inputs of mcq_vel_profile_device(_ragged) --, m_out [batch] points per raceline,
 * status_out [batch] MCQ_OK or MCQ_BAD_INPUT (n < 3, or more than mmax points needed).  Asynchronous on the handle's stream. */
int mcq_raceline_device(mcq_handle* h, int batch, int nmax, const int* n_in, const double* reftrack, const double* normvec,
                        const double* alpha, double stepsize, int mmax, double* raceline_out, double* psi_out,
                        double* kappa_out, double* el_lengths_out, int* m_out, int* status_out);

/* The same with OPEN chains among the rows: the step between mcq_solve_batch_ends and mcq_vel_profile_device_forms (closed = 0).
 * closed [batch] (DEVICE): an entry != 0 is a ring row and returns the bits of mcq_raceline_device; NULL: every row is a chain.
 * psi [batch][2] (DEVICE) = (psi_s, psi_e), read for chain rows only; it must be non-NULL if any row is a chain (with psi == NULL the
 * flags are read back once, blocking, and a chain row is MCQ_E_ARG).  A chain row of n >= 2 waypoints:
 *   points    P_i = p_i + alpha_i n_i, i = 0 .. n-1; n - 1 segments, D_i = P_(i+1) - P_i;
 *   spline    tph.calc_splines(path, psi_s, psi_e, use_dist_scaling=False) with el_lengths = None: unit scalings, and the heading rows
 *             carry the UNIT vectors h = (cos(psi + pi/2), sin(psi + pi/2)) times MCQ_HEADING_SCALE -- the rows the chain solve linearised, so
 *             the raceline is the curve whose curvature the QP minimised:
 *               2 c_0 + c_1 = 3 (D_0 - h_s),  c_(i-1) + 4 c_i + c_(i+1) = 3 (D_i - D_(i-1)),  c_(n-2) + 2 c_(n-1) = 3 (h_e - D_(n-2)),
 *               b_i = D_i - (2 c_i + c_(i+1)) / 3,  d_i = (c_(i+1) - c_i) / 3  (i <= n-2);
 *   lengths   tph.calc_spline_lengths over the n - 1 segments (15 points, 14 chords), running sum in numpy.cumsum's order: total;
 *   stations  m = ceil(total / stepsize) + 1 points, all kept (tph.interp_splines, incl_last_point = True): station j <= m-2 at
 *             q_j = j * total / (m - 1), station m-1 at t = 1 of segment n-2 (the last raceline point; derivatives taken there);
 *   outputs   raceline_out / psi_out / kappa_out hold m entries; el_lengths_out [j] = q_(j+1) - q_j (j <= m-3), [m-2] = total - q_(m-2),
 *             [m-1] = 0 (written; mcq_vel_profile_device_forms with closed = 0 reads the first m - 1); m_out = m.
 * status_out: MCQ_BAD_INPUT for a chain of n < 2 (or more than nmax) waypoints, a non-finite psi_s / psi_e, or m > mmax (m_out then
 * reports the m needed, as for rings); ring rows as in mcq_raceline_device.  nmax >= 2.  Asynchronous on the handle's stream. */
int mcq_raceline_device_ends(mcq_handle* h, int batch, int nmax, const int* n_in, const double* reftrack, const double* normvec,
                             const double* alpha, const int* closed, const double* psi, double stepsize, int mmax,
                             double* raceline_out, double* psi_out, double* kappa_out, double* el_lengths_out, int* m_out,
                             int* status_out);

/* ---- the finished trajectory and check_traj's verdicts [REF main_globaltraj.py:412-421, 502-534; helper_funcs_glob/src/check_traj.py] ----
 *
 * mcq_trajectory_device: tph.calc_ax_profile, the time profile, the rows [s, x, y, psi, kappa, vx, ax] and the seven limit tests of check_traj for a
 * batch of variants.  All pointers DEVICE pointers.  raceline [tracks][mmax][2], psi / kappa / el_lengths [tracks][mmax]: the outputs of
 * mcq_raceline_device(_ends), unchanged; m_of_track [tracks] stations per row, or NULL (every row has m); track_of [batch] or NULL (row = variant);
 * vx [batch][mmax]: the output of mcq_vel_profile_device*; closed: one int per launch, as the field of mcq_vel_forms -- closed rows have m elements, unclosed
 * rows m - 1; drag_coeff / m_veh / v_max [batch]; ggv [batch][n_ggv][3] or NULL; ax_max_machines [batch][n_machines][2] or NULL; curvlim.
 *   traj_out [batch][mmax][MCQ_TRAJ_COLS] (or NULL): s = running sum of el_lengths in numpy.cumsum's order, from 0 (the script's s_points);
 *     ax_i = (v_(i+1)^2 - v_i^2) / (2 l_i), closed rows with v_m := v_0, unclosed rows with a written 0 in row m - 1 (eq_length_output=True).
 *   t_out [batch][mmax + 1] (or NULL): t_0 = 0, t_(i+1) = t_i + 2 l_i / (v_i + v_(i+1)) -- the stable form of tph.calc_t_profile, summed in the order
 *     of the velocity kernel, so t_out[m] (closed) / t_out[m - 1] (unclosed) is BITWISE the lap_time_out of mcq_vel_profile_device* on the same arrays.
 *   length_out [batch]: s after the last element.
 *   limits_out [batch][MCQ_TRAJ_NLIM]: max |kappa|, max ay, max ax_wo_drag, min ax_wo_drag, max a_tot, max vx over the m stations, with
 *     ay = vx^2 / |1 / kappa| (0 where kappa is 0), ax_wo_drag = ax + vx^2 drag_coeff / m_veh, a_tot = sqrt(ax_wo_drag^2 + ay^2).
 *   flags_out [batch]: MCQ_CHK_* bits, each tested as check_traj tests: KAPPA: max |kappa| > curvlim (no margin); AY: > max ggv[:, 2] + margin;
 *     AX_POS: > max ggv[:, 1] + margin; AX_NEG: < min(-ggv[:, 1]) - margin; A_TOT: > max ggv[:, 1:] + margin; MACHINES: ax_wo_drag > max
 *     ax_max_machines[:, 1] + margin; V_MAX: vx > v_max + margin; margin = MCQ_CHECK_ACC_MARGIN.  ggv == NULL leaves the four ggv bits 0,
 *     ax_max_machines == NULL the machine bit.
 * NaN rule (as for the profile): a row length outside [2, mmax] or a vx row holding a NaN gives NaN rows, NaN times, NaN length and limits and
 * flags -1.  Rows m .. mmax-1 of traj_out and the entries of t_out behind the last time are NaN: no output keeps stale memory.
 * Asynchronous on the handle's stream. */
#define MCQ_TRAJ_COLS 7
#define MCQ_TRAJ_NLIM 6
#define MCQ_CHECK_ACC_MARGIN 0.1
#define MCQ_CHK_KAPPA 1
#define MCQ_CHK_AY 2
#define MCQ_CHK_AX_POS 4
#define MCQ_CHK_AX_NEG 8
#define MCQ_CHK_A_TOT 16
#define MCQ_CHK_MACHINES 32
#define MCQ_CHK_V_MAX 64
int mcq_trajectory_device(mcq_handle* h, int batch, int m, int mmax, const int* m_of_track, const int* track_of, const double* raceline,
                          const double* psi, const double* kappa, const double* el_lengths, const double* vx, int closed,
                          const double* drag_coeff, const double* m_veh, const double* v_max, const double* ggv, int n_ggv,
                          const double* ax_max_machines, int n_machines, double curvlim, double* traj_out, double* t_out,
                          double* length_out, double* limits_out, int* flags_out);

/* mcq_bound_dists_device: check_traj's first block -- the minimum distance of the vehicle's four corners to the two track boundaries, per station
 * and per track.  All pointers DEVICE pointers.  reftrack [tracks][nmax][4], normvec [tracks][nmax][2], n_list [tracks] or NULL (all nmax);
 * raceline [tracks][mmax][2], psi [tracks][mmax], m_list [tracks] or NULL (all mmax); length_veh / width_veh, or per track length_veh_list /
 * width_veh_list [tracks] (either may be NULL, then the scalar applies).
 *   boundaries  bound_r = p + n w_r, bound_l = p - n w_l (bound_out [tracks][2][nmax][2], optional: what check_traj returns; right first);
 *   re-sampling interp_track's rule for each: closed polyline, element lengths sqrt(dx^2 + dy^2), running sum in numpy.cumsum's order,
 *               ceil(total / stepsize_bound) + 1 samples of numpy.linspace(0, total), numpy.interp in each coordinate, last sample dropped
 *               (nb_out [tracks][2]: samples kept per boundary);
 *   corners     (+-width / 2, +-length / 2) rotated by psi (0 = north, the length along y) and added to the station;
 *   outputs     min_dists_out [tracks][mmax]: per station the minimum over 4 corners x every sample of both boundaries (entries m .. mmax-1 NaN);
 *               min_dist_out [tracks]: its minimum over the stations (check_traj warns below MCQ_CHECK_DIST_WARN).
 * mode: MCQ_BOUNDS_ALL (0) is what calc_min_bound_dists documents.  MCQ_BOUNDS_FIRST_ROW (1) measures against the FIRST sample of each boundary
 * only -- what the reference's call computes, because it passes interp_track(...)[0], one row, as the boundary [REF helper_funcs_glob/src/check_traj.py:57-60]: a quirk
 * reproduced on request, not fixed and not the default (nb_out still reports the samples per boundary).
 * status_out [tracks]: MCQ_BAD_INPUT for n < 3 (or > nmax), m < 1 (or > mmax), non-finite input, a boundary element of length 0 (numpy.interp has
 * no answer there) or more samples than the handle's scratch holds per boundary: min(MCQ_BOUND_NB_MAX, $MCQ_BOUND_BYTES / (32 tracks)) with
 * $MCQ_BOUND_BYTES 1 GiB by default (nb_out then reports the samples needed); such a track's distances are NaN.  The scratch grows on demand.
 * The minimum is taken over squared distances and the root once per station: results are bit-identical whatever the tiling, grid or launch order.
 * Asynchronous on the handle's stream. */
#define MCQ_BOUNDS_ALL 0
#define MCQ_BOUNDS_FIRST_ROW 1
#define MCQ_CHECK_DIST_WARN 1.0
#define MCQ_BOUND_NB_MAX 65536
int mcq_bound_dists_device(mcq_handle* h, int tracks, int nmax, const int* n_list, const double* reftrack, const double* normvec, int mmax,
                           const int* m_list, const double* raceline, const double* psi, double length_veh, double width_veh,
                           const double* length_veh_list, const double* width_veh_list, double stepsize_bound, int mode,
                           double* min_dists_out, double* min_dist_out, int* nb_out, double* bound_out, int* status_out);

/* ---- tph.spline_approximation behind FITPACK's fit [REF helper_funcs_glob/src/prep_track.py:39-45]: from the smoothing B-spline of the centre line
 * (scipy.interpolate.splprep's tck: the one step of prep_track that stays on the host) and the raw rows to the prepared rows.  All pointers
 * DEVICE pointers; asynchronous on the handle's stream.  Per track:
 *   closing     track_cl = the n rows and row 0 again; element lengths sqrt(dx^2 + dy^2), running sum in numpy.cumsum's order: total;
 *               first guesses t_guess_i = cum_i / total, i = 0 .. n.
 *   evaluation  splev(t, tck) with ext = 0: the interval l with knots[l] <= t < knots[l + 1] clamped to [k, nk - k - 2], t itself neither
 *               clamped nor wrapped (a parameter below 0 or above 1 is evaluated on the first / last polynomial piece; the search goes there),
 *               FITPACK's recursion for the k + 1 B-splines.
 *   length      4 ceil(total) samples at numpy.linspace(0, 1), the sum of the chords (a fixed order: 256 strided partial sums, then a tree);
 *               no_points_reg_cl = ceil(len_smoothed / stepsize_reg) + 1; m = no_points_reg_cl - 1 rows at numpy.linspace(0, 1,
 *               no_points_reg_cl), the last one dropped.
 *   search      per row i of track_cl: scipy.optimize.fmin(|s(t) - p_i|, x0 = t_guess_i) with its defaults, restated for one variable with
 *               scipy's roundings (second vertex 1.05 x0, or 0.00025 for x0 == 0; at most 200 calls): closest_t_i; dists_i = |s(closest_t_i) - p_i|.
 *   widths      side_i = sign((p_(i+1) - p_i) x (s(closest_t_i) - p_i)), side_n = side_0; w_r + side dist and w_l - side dist, carried to the
 *               rows by numpy.interp's rule over closest_t (plain bisection: the last i with closest_t_i <= x; slope * (x - xp_i) + fp_i; the
 *               first / last value outside the range).  Where closest_t descends numpy's own answer depends on its search heuristic; the
 *               entry's is the bisection's, and nonmono_out counts the i with closest_t_(i+1) <= closest_t_i.  Not an error (upstream does
 *               not check either).
 * status_out: MCQ_BAD_INPUT -- that track's reftrack_out / closest_t_out / dists_out / dev_out NaN, nonmono_out 0 -- for n < 3 or n > nmax, a
 *   non-finite row, knot or coefficient, nk < 2 k + 2 or nk > nkmax, descending knots, total == 0 (or beyond 2^22 m), m < 3 and m > mmax (m_out
 *   then reports the m needed, as the raceline entries do; otherwise m_out of a refused track is 0).  The other tracks are not affected.
 * MCQ_E_ARG: k outside 1 .. 5, nmax < 3, nkmax < 2 k + 2, mmax < 3, stepsize_reg <= 0, NULL where an array is required, more than
 *   MCQ_SPL_MAX_TRACKS tracks in one launch (the tracks are one axis of the search kernel's grid) or nmax above MCQ_SPL_MAX_N. */
#define MCQ_SPL_MAX_TRACKS 65535
#define MCQ_SPL_MAX_N 16777216
int mcq_spline_approx_device(mcq_handle* h, int tracks,
        int nmax, const int* n_list, const double* track,      /* [tracks][nmax][4] raw rows [x, y, w_r, w_l], NOT closed; n_list NULL: all nmax */
        int k, int nkmax, const int* nk_list,                  /* degree 1..5; knots per track (NULL: all nkmax) */
        const double* knots, const double* coef,               /* [tracks][nkmax], [tracks][2][nkmax] (nk - k - 1 valid per coordinate: splprep's tck) */
        double stepsize_reg, int mmax,
        double* reftrack_out,                                  /* [tracks][mmax][4]; rows m_out .. mmax-1 NaN */
        int* m_out,                                            /* rows written = no_points_reg_cl - 1 (the count needed when it exceeds mmax) */
        double* closest_t_out, double* dists_out,              /* [tracks][nmax + 1] each, optional (NULL) */
        double* dev_out,                                       /* [tracks][2] = mean, max of dists_closest (the debug line's two numbers), optional */
        int* nonmono_out,                                      /* [tracks]: count of i with closest_t[i+1] <= closest_t[i], optional */
        int* status_out);

/* ---- FITPACK's periodic smoothing fit, the step in front of mcq_spline_approx_device [REF helper_funcs_glob/src/prep_track.py:39-45]: what
 * scipy.interpolate.splprep([x, y], k = k_reg, s = s_reg, per = 1) computes inside tph.spline_approximation (FITPACK's clocur / fpclos) with
 * interp_track's linear re-sampling at stepsize_prep in front of it.  nk_out / knots_out / coef_out have the layout mcq_spline_approx_device
 * reads (nk_list / knots / coef), so raw rows become prepared rows without a host round trip.  All pointers DEVICE pointers; asynchronous on
 * the handle's stream; the scratch is the handle's and grows on demand.  Per track:
 *   re-sampling interp_track's rule (see mcq_bound_dists_device): closed polyline, element lengths, running sum in numpy.cumsum's order,
 *               ceil(total / stepsize_prep) + 1 samples of numpy.linspace(0, total), numpy.interp per coordinate, the last sample dropped; then
 *               sample 0 is appended again: mi closed points.  stepsize_prep <= 0: the raw rows themselves are closed and fitted (mi = n + 1).
 *   parameter   u_0 = 0, u_i = u_(i-1) + sqrt(dx^2 + dy^2), each divided by u_(mi-1), u_(mi-1) = 1 (scipy's u, bit for bit).
 *   fit         fpclos with unit weights, iopt = 0, tol = 0.001, maxit = 20, nest = nkmax on the mi - 1 distinct points: s = 0 the
 *               interpolating periodic spline (ier -1); otherwise knots are added at data parameters by fpknot's rule, starting from the
 *               constant (ier -2 if that is within s) and u[(mi + 1) / 2 - 1], until the least-squares spline's fp is at most s; then the
 *               smoothing spline with |fp - s| < 0.001 s by fprati's rational search for p (ier 0; 1: nkmax knots do not suffice, the
 *               least-squares spline of that stage is returned; 2 / 3: the search failed / took more than 20 rounds, the last spline is
 *               returned, as scipy returns it with a warning).  The interior knots are bitwise elements of u.  The triangularisation is
 *               by Givens rotations as FITPACK's (no normal equations), on one layout for both stages; the observations of a knot interval
 *               are reduced sixteen at a time to k + 1 rows before they enter it; fp is the sum of the squared residuals in the points' order.  Coefficients and fp agree with scipy's to roundings, not bitwise.
 *   outputs     nk_out = n; knots_out[0 .. n-1]; coef_out[d][0 .. n-k-2] with the last k equal to the first k (scipy's tck); entries behind
 *               are NaN; fp_out, ier_out FITPACK's values; mi_out (optional) the closed sample count, or the count needed when it exceeds
 *               mimax; pts_out (optional) [tracks][mimax][2] the closed points that were fitted, NaN behind mi.
 * status_out [tracks]: MCQ_BAD_INPUT -- nk_out 0, ier_out 10, every other output of the track NaN, the other tracks unaffected -- for n < 3 or
 *   n > nmax, a non-finite row, mi <= k, mi > mimax, a zero-length element (u is not strictly increasing), total == 0.
 * MCQ_E_ARG: k outside 1 .. 5, s < 0 or not finite, nkmax < 2 k + 2, nmax < 3, mimax < 2, NULL where an array is required, more than
 *   MCQ_SPL_MAX_TRACKS tracks in one launch.  No output keeps stale memory. */
int mcq_spline_fit_device(mcq_handle* h, int tracks,
        int nmax, const int* n_list, const double* track,   /* [tracks][nmax][4] raw rows, NOT closed; n_list NULL: all nmax */
        double stepsize_prep, int mimax,                    /* re-sampling step; samples a track may take (closed count) */
        int k, double s, int nkmax,                         /* degree 1..5, smoothing factor >= 0, nkmax = FITPACK's nest */
        int* nk_out, double* knots_out, double* coef_out,   /* [tracks], [tracks][nkmax], [tracks][2][nkmax] */
        double* fp_out, int* ier_out, int* mi_out,          /* [tracks] each; fp_out / mi_out optional */
        double* pts_out,                                    /* [tracks][mimax][2], optional */
        int* status_out);

/* prep_track's tail [REF helper_funcs_glob/src/prep_track.py:89-98]: where w_r + w_l < min_width both widths of reftrack_io [batch][nmax][4] grow by
 * half the deficit; changed_out [batch] = 1 if any row of the track changed (upstream's warning), else 0.  n_list [batch] or NULL (all nmax).
 * A separate entry because prep_track runs the normals-crossing check on the un-inflated widths.  DEVICE pointers; asynchronous. */
int mcq_min_width_device(mcq_handle* h, int batch, int nmax, const int* n_list, double* reftrack_io, double min_width, int* changed_out);

/* ---- the export tables [REF main_globaltraj.py:502-552, helper_funcs_glob/src/export_traj_ltpl.py:35-63]: the local planner's rows and the
 * total that closes the race table, the last stage of the post-QP flow.  All pointers DEVICE pointers; asynchronous on the handle's stream; rings
 * only (the reference's export always closes its table; a chain has no definition upstream).
 * Per track of n waypoints (n_list [tracks] or NULL: all nmax): the raceline points P_i = p_i + alpha_i n_i, the closed cubic spline through them
 *   with unit scalings, spline_lengths_i from 15 points / 14 chords per segment (tph.calc_spline_lengths: what tph.create_raceline returns as
 *   spline_lengths_opt), s_ref_0 = 0 and s_ref_(i+1) their running sum in numpy.cumsum's order, spline_total = s_ref_n.  These are the bits
 *   mcq_raceline_device forms internally for the same inputs, and they do not depend on which other tracks are in the launch.
 *   NOTE: upstream closes the race table with numpy.sum(spline_lengths) (pairwise summation); this entry has the running sum's last value.  The
 *   two differ in the last bits.
 * Per variant b (track_of [batch] or NULL: row = variant; m_of_track [tracks] stations of the track's trajectories or NULL: all mmax), on
 *   traj [batch][mmax][MCQ_TRAJ_COLS], the traj_out of mcq_trajectory_device:
 *   lookup  idx_i = numpy.argmin(|traj[b][0..m-1][0] - s_ref_i|), i = 0 .. n-1, first minimum; only the m stations are searched and the table is
 *           not wrapped (upstream's behaviour: the last waypoints may be nearer to the lap's end than to any station).  On the non-decreasing s
 *           column this is: lo = count of j with s_j < s_ref_i; of the candidates lo - 1 and lo the one that exists, or the nearer one (the lower
 *           at equal distance); then downwards while the station below is at the same distance.
 *   rows    ltpl_out [batch][nmax + 1][MCQ_LTPL_COLS]: row i <= n-1 = [x_ref, y_ref, w_r, w_l, n_x, n_y, alpha, s_ref_i, psi, kappa, vx, ax] -- the
 *           first seven bit-for-bit copies of the inputs, the last four bit-for-bit copies of traj[b][idx_i][3..6]; row n = row 0 with column 7
 *           = spline_total (upstream's traj_ltpl_cl; the FILE upstream writes holds the first n rows only); rows n+1 .. nmax NaN.
 *           idx_out [batch][nmax] (optional): idx_i, entries n .. nmax-1 are -1.
 *   spline_lengths_out [tracks][nmax] (optional; NaN behind n), s_ref_out [tracks][nmax + 1] (optional; s_ref_0 .. s_ref_n, NaN behind),
 *   spline_total_out [tracks].
 * status_out [batch]: MCQ_OK, or MCQ_BAD_INPUT for n < 3 or n > nmax, m < 2 or m > mmax, a track_of entry outside the tracks, a non-finite reftrack /
 *   normvec / alpha entry among the n (or a raceline whose length is not finite), a NaN among the m entries of the s column (the trajectory entry's
 *   NaN rule arrives here as such) or an s column that descends somewhere.  That variant's whole table is NaN and its idx -1; the other variants are
 *   not affected.  A refused TRACK has NaN spline_lengths_out / s_ref_out / spline_total_out.  No output keeps stale memory.
 * MCQ_E_ARG: nmax < 3, mmax < 2, batch or tracks <= 0, NULL where an array is required; MCQ_E_TOO_LARGE: batch x ceil((nmax + 1) / 1024) beyond 2^31 - 1
 *   (the second launch's grid).  Indices and copies: identical whatever the grid or order. */
#define MCQ_LTPL_COLS 12
int mcq_export_device(mcq_handle* h, int tracks, int nmax, const int* n_list, const double* reftrack, const double* normvec,
                      const double* alpha, int batch, int mmax, const int* m_of_track, const int* track_of, const double* traj,
                      double* ltpl_out, int* idx_out, double* spline_lengths_out, double* s_ref_out, double* spline_total_out,
                      int* status_out);

/* ---- friction maps [REF opt_mintime_traj/src/friction_map_interface.py, extract_friction_coeffs.py, approx_friction_map.py]: what produces the
 * `mu` of mcq_vel_opts / mcq_vel_forms, and the reference's grids of friction along the normals with their lines.
 * A map is one object, resident on the handle's device: cells points (any point set -- no lattice is assumed) with a friction value each.
 * mcq_fmap_create builds the index on the host (deterministic, O(cells)) and uploads it once: a uniform grid of bins of side bin_side over the
 *   cells' bounding box in CSR form (bin_start [bins_x * bins_y + 1], the cells' coordinates and original indices sorted by bin, mue in original
 *   order).  bin_side <= 0: automatic, sqrt(box area / cells); more than 2^22 bins: the side is doubled until they fit.  A degenerate box (all
 *   cells on one line or at one point) has one bin along that axis.  xy_host [cells][2], mue_host [cells]: HOST memory, read before the call
 *   returns.  MCQ_E_ARG: cells < 1, a cell coordinate that is not finite, NULL.  A NaN in mue is allowed and handed through by the lookups.
 * mcq_fmap_destroy waits for the handle's stream first; NULL is a success.  mcq_fmap_info: any pointer may be NULL.
 *
 * mcq_fmap_query_device: the nearest cell of each of count points.  DEVICE pointers; asynchronous on the handle's stream.
 *   The lookup is EXACT: for any finite query, wherever it lies, idx is a cell of minimum computed squared distance dx * dx + dy * dy (double,
 *   every operation rounded on its own).  TIE RULE (the engine's own; scipy's cKDTree documents none): among cells at exactly equal computed
 *   squared distance, the lowest original index -- duplicated cells included.  A query far outside the box is slow (the whole grid may be
 *   scanned) and correct.
 *   mue_out [count] = mue[idx], bits unchanged (a NaN there is handed through); idx_out [count] (optional); dist_out [count] (optional) = the
 *   square root of the minimum.  A query that is not finite: idx -1, mue NaN, dist NaN.  count == 0: success without a launch.
 *
 * mcq_friction_grid_device: extract_friction_coeffs and approx_friction_map(var_friction = "linear") for a batch of tracks in one launch.
 *   reftrack [tracks][nmax][4], normvec [tracks][nmax][2], n_list [tracks] or NULL (all nmax); width_list [tracks] or NULL (width_opt for all).
 *   A track of n waypoints has n + 1 rows: row n is row 0 again, as the reference closes it.  Per row, with w_r, w_l the row's widths:
 *   cnt_out [tracks][nmax + 1] = num_right + num_left + 1, num_x = floor((w_x - 0.5 * width - 0.5) / dn): Python's operations, bit for bit its
 *     decisions ((5.0 - 1.7 - 0.5) / 0.1 is 27.999999999999996 and floors to 27);
 *   n_out [tracks][nmax + 1][jmax] = numpy.linspace(-dn * num_right, dn * num_left, cnt): j * step + start with the product and the sum rounded
 *     separately, the last entry the stop value itself -- numpy's bits;
 *   mue_out [tracks][4][nmax + 1][jmax]: the wheels fl, fr, rl, rr at (p +- wheelbase * tang) - (n_j +- 0.5 * width) * normvec with
 *     tang = (-n_y, n_x), the reference's four expressions rounded as numpy rounds them, looked up as mcq_fmap_query_device does;
 *     idx_out (optional), same shape: the cells;
 *   w_mue_out [tracks][4][nmax + 1][2] (optional): slope, then intercept of the least-squares line through (n_j, mue_j), numpy.polyfit(n, mue, 1)'s
 *     order, from centred sums taken in one fixed order: bit-identical whatever the grid, the launch's company or the order of the tracks.
 *   Entries beyond a row's count, rows beyond n and every output of a refused track are NaN (idx -1, cnt 0).
 *   DEVIATIONS from the reference, both stated: a row whose count is <= 0 has cnt_out equal to that count and NaN outputs, and the track stays
 *     MCQ_OK (numpy.linspace raises for a negative number, and the reference fails in polyfit for an empty row); a row of exactly one position
 *     delivers its mue and a NaN line (numpy returns a minimum-norm answer with a RankWarning).
 *   status_out [tracks]: MCQ_OK, or MCQ_BAD_INPUT for n < 1 or n > nmax, a row (or a width or wheelbase) that is not finite -- cnt_out 0 -- or
 *     a count above jmax -- cnt_out then reports the counts the track needs, as the raceline entries report m.  Other tracks are not affected.
 *   MCQ_E_ARG: dn <= 0 or not finite, jmax < 1, nmax < 1, tracks <= 0, NULL where an array is required; MCQ_E_TOO_LARGE: tracks x
 *     ceil((nmax + 1) / 4) beyond 2^31 - 1 (the launch's grid).  The entry needs no temporaries. */
typedef struct mcq_fmap mcq_fmap;
int mcq_fmap_create(mcq_handle* h, int cells, const double* xy_host, const double* mue_host, double bin_side, mcq_fmap** fmap_out);
int mcq_fmap_destroy(mcq_handle* h, mcq_fmap* fmap);
int mcq_fmap_info(const mcq_fmap* fmap, int* cells, int* bins_x, int* bins_y, double* bin_side, long long* device_bytes);
int mcq_fmap_query_device(mcq_handle* h, const mcq_fmap* fmap, int count, const double* xy, double* mue_out, int* idx_out, double* dist_out);
int mcq_friction_grid_device(mcq_handle* h, const mcq_fmap* fmap, int tracks, int nmax, const int* n_list, const double* reftrack,
                             const double* normvec, double width_opt, const double* width_list, double wheelbase_front, double wheelbase_rear,
                             double dn, int jmax, double* n_out, int* cnt_out, double* mue_out, int* idx_out, double* w_mue_out,
                             int* status_out);

/* mcq_friction_gauss_device: approx_friction_map(var_friction = "gauss") [REF opt_mintime_traj/src/approx_friction_map.py:102-127, GaussianFeatures]
 *   on what mcq_friction_grid_device left on the device -- n_out, cnt_out, mue_out, status_out with the same tracks, nmax, jmax; nothing is looked
 *   up again.  DEVICE pointers; asynchronous on the handle's stream.  Per row of cnt positions and per wheel, N = 2 n_gauss + 1 Gaussian bumps and an
 *   intercept, as sklearn 1.7's dense LinearRegression(fit_intercept = True) behind the reference's features computes them:
 *   centres  numpy.linspace(n[0], n[cnt - 1], N): k * step + start in two roundings, the last entry the stop value itself;
 *   width    2.0 * (c[1] - c[0]);   features  exp(-0.5 * ((n_j - c_k) / width)^2);
 *   centring the features' column means and the mean of the wheel's friction are subtracted;
 *   solve    the minimum-norm least-squares solution of the centred cnt x N system: every singular value <= rcond * sigma_max counts as zero;
 *            rcond <= 0: sklearn's own max(cnt, N) * DBL_EPSILON.  The singular values come from a one-sided Jacobi (Hestenes) decomposition of the
 *            centred matrix itself -- no Gram matrix -- with one fixed pair order and fixed summation orders: a row's bits do not depend on the
 *            launch's company, the order of the tracks or the grid.  The four wheels share the decomposition.
 *   intercept mean(mue) - mean(features) . weights.
 *   w_gauss_out [tracks][4][nmax + 1][N + 1]: the N weights, then the intercept (the reference's column order);
 *   center_dist_out [tracks][nmax + 1] = (n[cnt - 1] - n[0]) / (2 * n_gauss), the reference's bits;
 *   rank_out [tracks][nmax + 1] (optional): singular values above the cut; sweeps_out (optional), same shape: Jacobi sweeps taken.
 *   Where the weights are not unique to working precision (a singular value within rounding of the cut) the answer is one of the two ranks';
 *   where they are, they agree with sklearn's to the conditioning of the problem (sigma_min / sigma_max is about 6e-7 at n_gauss = 5).
 *   EDGES: cnt == 1: NaN weights, center_dist 0, rank 0 (the reference's width is 0, its features are NaN and sklearn raises);
 *     cnt <= 0, rows beyond n, every row of a track the grid call refused: NaN weights, NaN center_dist, rank 0;
 *     a NaN among one wheel's friction values: that wheel's weights are NaN, the other three are not affected;
 *     a row that has not settled after 40 sweeps: NaN weights, rank -1 (none is known);
 *     outputs are always overwritten.
 *   MCQ_E_ARG: n_gauss < 1 or > 15 (the reference divides by 2 * n_gauss and indexes centers_[1]), rcond NaN, jmax < 1, nmax < 1, tracks <= 0,
 *     NULL where an array is required; MCQ_E_TOO_LARGE: a single row -- N * (jmax + N + 6) + 384 doubles of LDS -- beyond 64 KB, or more
 *     workgroups than one launch holds.  Rows per workgroup (a wave each, at most 4) are chosen from jmax and N so that a workgroup stays within
 *     64 KB.  The entry needs no temporaries.
 *
 * mcq_friction_model_device: a fitted model at lateral positions q [tracks][nmax + 1][qmax] (qcnt [tracks][nmax + 1] positions per row, or
 *   NULL: all qmax) -> mue_out [tracks][4][nmax + 1][qmax].  weights [tracks][4][nmax + 1][P]:
 *   MCQ_FRIC_LINEAR  P = 2, slope then intercept (w_mue_out): slope * q + intercept in two roundings; center_dist, n, cnt are not read;
 *   MCQ_FRIC_GAUSS   P = N + 1 (w_gauss_out): sum over k in rising order of feature_k * w_k, then + intercept, with the centres of
 *     MCQ_FRIC_CENTRES_FIT      n[0] + k * center_dist in linspace's form (the last centre is n[cnt - 1] itself; n = n_out, cnt = cnt_out,
 *                               jmax their stride), width 2 * (c[1] - c[0]): what the fitted pipeline's predict evaluates;
 *     MCQ_FRIC_CENTRES_MINTIME  numpy.linspace(-n_gauss, n_gauss, N) * center_dist, sigma = 2 * center_dist, exp(-(q - c_k)^2 / (2 sigma^2)):
 *                               what the reference's only consumer evaluates [REF opt_mintime_traj/src/opt_mintime.py:733-747]; n, cnt not read.
 *     The two forms agree only where a row's positions are symmetric about 0 (n[0] = -n[cnt - 1]): the consumer places the bumps around 0,
 *     the fit around the middle of the row.
 *   A NaN weight gives NaN (so does a row without a fit); entries beyond qcnt are NaN.  Outputs are always overwritten.
 *   MCQ_E_ARG: an unknown model or centre form, n_gauss outside 1 .. 15 for the Gaussian model, qmax < 1, nmax < 1, tracks <= 0, jmax < 1 with
 *     MCQ_FRIC_CENTRES_FIT, NULL where an array is required; MCQ_E_TOO_LARGE: more workgroups than one launch holds. */
#define MCQ_FRIC_LINEAR 0
#define MCQ_FRIC_GAUSS 1
#define MCQ_FRIC_CENTRES_FIT 0
#define MCQ_FRIC_CENTRES_MINTIME 1
int mcq_friction_gauss_device(mcq_handle* h, int tracks, int nmax, int jmax, const double* n_out, const int* cnt_out, const double* mue_out,
                              const int* status, int n_gauss, double rcond, double* w_gauss_out, double* center_dist_out, int* rank_out,
                              int* sweeps_out);
int mcq_friction_model_device(mcq_handle* h, int tracks, int nmax, int qmax, const double* q, const int* qcnt, int model, const double* weights,
                              int n_gauss, int centres, const double* center_dist, const double* n_out, const int* cnt_out, int jmax,
                              double* mue_out);

/* ---- friction map generation [REF main_gen_frictionmap.py, frictionmap/src/reftrack_functions.py]: the producer of the maps the entries above
 * consume -- the cells of a square grid that lie on a track or within 1.1 cell widths of it.  DEVICE pointers, launches on the handle's stream.
 *
 * mcq_points_in_path_device: matplotlib's Path(verts).contains_points(xy, radius = r) for a batch of closed polygons and one set of points.
 *   verts [paths][vmax][2], v_list [paths] or NULL (all vmax), radius [paths], xy [count][2] -> inside_out [paths][count], one byte (0 / 1) each.
 *   With r != 0 matplotlib does not test the polygon: it tests agg's CONTOUR of it, offset by r / 2, on the side the polygon's ORIENTATION and
 *   the sign of r select.  Restated here operation by operation (fp64, no fused multiply-add), so that the verdicts are matplotlib's exactly:
 *   vertices  one within 1e-14 of the previous KEPT one is dropped, then trailing ones within 1e-14 of the first; prev / next are cyclic;
 *   join      per kept vertex v1 between v0 and v2, w = r / 2: the segments' offsets (dx, dy) = w * (delta y, delta x) / length; with
 *             cp = (v2.x - v1.x)(v1.y - v0.y) - (v2.y - v1.y)(v1.x - v0.x), an INNER join where |cp| > 1e-14 and cp has w's sign: a miter reverted
 *             beyond max(min(len1, len2) / |w|, 1.01) half widths; otherwise an OUTER join: a miter cut beyond 4 half widths.  The miter point is
 *             the intersection of the two offset lines (given up where |den| < 1e-30); a join contributes one point or two;
 *   crossing  per edge (x0, y0) -> (x1, y1) of that polygon, the closing one included: toggle where (y0 >= ty) != (y1 >= ty) and
 *             ((y1 - ty)(x0 - x1) >= (x1 - tx)(y0 - y1)) == (y1 >= ty).  radius 0: the path itself, no vertex dropped.
 *   A path of fewer than 3 vertices, or fewer than 2 kept ones: False everywhere (matplotlib's answer).  A point that is not finite: False.
 *   contour_out [paths][2 * vmax][2] and contour_count_out [paths] (both optional, both or neither): the polygon the crossing test ran on;
 *   rows beyond the count are not written.  count == 0 (xy and inside_out may be NULL): only the contours.
 *   status_out [paths]: 0, MCQ_FGEN_NONFINITE (a vertex or radius that is not finite: False everywhere, count 0 -- matplotlib would split the path
 *   at a NaN; here it is refused) or MCQ_FGEN_FEW (v_list outside 0 .. vmax).
 *   MCQ_E_ARG: paths <= 0, vmax < 1, count < 0, NULL where an array is required; MCQ_E_TOO_LARGE: more than 65535 paths (they lie along the launch's second axis).
 *   Asynchronous.  Temporaries: the handle's scratch, 7 doubles per vertex.
 *
 * mcq_friction_gen_device: the reference's script for a batch of tracks, reftrack [tracks][nmax][4] = x, y, w_right, w_left; n_list [tracks] or
 *   NULL (all nmax).  Per track:
 *   closed    where the last waypoint lies within 10 m of the first; the differences of numpy.gradient on the line (closed: cyclic; open: one-sided
 *             at the ends), the normal (gy, -gx) / sqrt(gy^2 + gx^2), right = p + normal * w_right, left = p - normal * w_left:
 *             bound_r_out, bound_l_out [tracks][nmax][2] (optional), the reference's calc_trackboundaries bit for bit;
 *   grid      d = ceil(max w_right + max w_left + 5), x0 = floor(min x - d), x1 = ceil(max x + d), y likewise; the axes are numpy.arange(x0, x1 + 0.1,
 *             cellwidth)'s own values: ceil((x1 + 0.1 - x0) / cellwidth) entries, entry i = x0 + i * ((x0 + cellwidth) - x0) (entry 1 the sum
 *             itself); points x-major, y inner.  grid_out [tracks][6] = x0, x1, y0, y1, nx, ny as doubles;
 *   cells     closed: contains(outside boundary, +-1.1 cellwidth) and not contains(inside boundary, -+1.1 cellwidth), the signs as the reference
 *             picks them from inside_right [tracks] (nonzero: the right boundary is the inner one; NULL: all right); open: the one polygon
 *             (left, right reversed) at radius -1.1 cellwidth.  `contains` is mcq_points_in_path_device's.  count_out [tracks] = cells found;
 *             cells_out [tracks][cmax][2] (optional) = their coordinates in the order of coordinates[bool_OnTrack]; rows beyond the count are not
 *             written.  cells_out NULL: counts only (cmax is not read).  count > cmax: the first cmax cells, the true count, MCQ_FGEN_OVERFLOW.
 *             count_out NULL (then cells_out must be NULL too): boundaries, grids and status only -- one launch, no wait, no grid point tested.
 *   status_out [tracks], bits: MCQ_FGEN_NONFINITE (a waypoint, width or boundary point that is not finite -- a waypoint whose neighbours coincide
 *   has a zero gradient and gives one; matplotlib would split the path at a NaN, here the track is REFUSED with count 0), MCQ_FGEN_FEW (n < 3 or
 *   n > nmax), MCQ_FGEN_OVERFLOW, MCQ_FGEN_GRID (more than 2^31 - 1 grid points).  A refused track has count 0, nx = ny = 0 (MCQ_FGEN_GRID keeps
 *   its range and counts), its boundary rows NaN (a zero gradient: as computed), and does not affect the others; a track's bytes do not depend on
 *   the launch's company, its position in the batch or nmax / cmax.  Boundary rows beyond n are not written.
 *   MCQ_E_ARG: cellwidth <= 0 or not finite, nmax < 3, tracks <= 0, cmax < 0 (with cells_out), cells_out without count_out, NULL where an
 *   array is required; MCQ_E_TOO_LARGE: more than 32767 tracks (they lie along the launches' second axis) -- the only case: a track's
 *   item blocks are bounded by MCQ_FGEN_GRID.
 *   With count_out the entry WAITS ONCE, for the boundaries' launch, and reads 2 ints per track back: the grids' sizes decide the launches and temporaries that
 *   follow (the handle's scratch: 34 doubles per waypoint and about 0.26 bytes per grid point of the largest track, times tracks); those launches are
 *   asynchronous. */
#define MCQ_FGEN_NONFINITE 1
#define MCQ_FGEN_FEW 2
#define MCQ_FGEN_OVERFLOW 4
#define MCQ_FGEN_GRID 8
int mcq_points_in_path_device(mcq_handle* h, int paths, int vmax, const int* v_list, const double* verts, const double* radius, int count,
                              const double* xy, unsigned char* inside_out, int* status_out, double* contour_out, int* contour_count_out);
int mcq_friction_gen_device(mcq_handle* h, int tracks, int nmax, const int* n_list, const double* reftrack, double cellwidth,
                            const int* inside_right, int cmax, double* bound_r_out, double* bound_l_out, double* grid_out, int* count_out,
                            double* cells_out, int* status_out);

/* ---- the minimum-time optimal-control problem: evaluate, differentiate, certify [REF opt_mintime_traj/src/opt_mintime.py:143-861] ----
 * The reference's NLP -- double-track model, nx = 5 states [v, beta, omega_z, n, xi] scaled by [50, 0.5, 1, 5, 1], nu = 4 controls [delta, f_drive,
 * f_brake, gamma_y] scaled by [0.5, 7500, 20000, 5000], Gauss-Legendre collocation of degree 3 over N intervals of a closed track -- as FUNCTIONS of
 * a decision vector w: the constraint vector g, the objective J, the reference's f_sol outputs, the Jacobian of g, the gradients of J and of the
 * energy sum, the KKT residual of a primal-dual point, the Hessian of the Lagrangian and its products with vectors; the Newton step built from
 * them follows below.  No NLP loop, no powertrain states (pwr_behavior: MCQ_E_ARG), and not tph's nonreg_sampling / calc_head_curv_num: curvature and station steps
 * are inputs.
 *
 * Layouts (csrc/mcq_mintime.inc; mcq_mintime_layout states them as numbers):
 *   w  [nw = 5 + 24 N]: X_0 | per interval k: U_k (4), Xc_k,0 Xc_k,1 Xc_k,2 (5 each), X_k+1 (5)  ->  X_k at 24 k, U_k at 24 k + 5, Xc_k,j at 24 k + 9 + 5 j.
 *   g  [ng = N (27 + 2 safe) + 4 (N - 1) + 5 + energy], per interval k in the reference's order: 15 collocation rows h_k f(Xc_k,j, U_k, kappa_j) - xp_j,
 *      5 continuity rows, 1 power row, 4 Kamm rows (fl, fr, rl, rr), 1 roll-moment row, 1 pedal row, 4 actuator rows where k > 0, 2 safe-trajectory
 *      rows where enabled; interval k starts at k (27 + 2 safe) + 4 max(k - 1, 0).  After the last interval: 5 periodicity rows X_0 - X_N, then the
 *      energy row (sum of v_k f_drive_k dt_k) / 3.6e6 where enabled.
 *   Curvature at collocation point j of interval k: kappa_cl[k] + tau_j (kappa_cl[k + 1] - kappa_cl[k]) -- CasADi's linear interpolant is NOT pinned bit
 *      for bit.  The reference's quirks are kept: f_y with the constant mue under every friction model; path rows at X_k+1 with U_k and friction row
 *      k + 1; actuator rows (U_k - U_k-1) / (h[k - 1] sigma), sigma = (1 - kappa_cl[k] n_k+1) / v_k+1; energy with the interval's START state; the pedal
 *      row's lower bound -20000 / (7500 * 20000); the cyclic regularisation sum of (p_k - p_k+1)^2 with the last term wrapped to the first.
 *   Jacobian blocks [batch][nmax][33][33], row-major: block k holds the 33 row slots of interval k in the order above (the 4 actuator and 2 safe slots
 *      zero where absent) against the 33 column slots [X_k (5), U_k (4), Xc_k,0..2 (15), X_k+1 (5), U_k-1 (4)]: slots 0 .. 28 are w[24 k .. 24 k + 28].  The
 *      periodicity rows (+1 at X_0, -1 at X_N) are constant and not stored; the energy row is the dense grad_energy.
 *   Hessian blocks [batch][nmax][33][33], row-major, symmetric bit for bit: H(w, sigma, lam_g) = sigma hess J + sum_i lam_g[i] hess g_i (CasADi's
 *      hess_lag; the certificate's signs) is the sum over the intervals of S_k^T (hess phi_k) S_k, block k = hess phi_k over the SAME 33 column slots,
 *        phi_k = sum over the rows r of interval k that exist of lam_g[row0(k) + r] g_k,r
 *              + sigma (dt_k + penalty_delta (d_k-1 - d_k)^2 + penalty_F (F_k-1 - F_k)^2) + lam_g[row_energy] ec_k / 3.6e6 (with limit_energy only),
 *      d = 0.5 U[0], F = U[1] 7500 / 10000 + U[2] 20000 / 10000, k - 1 cyclic.  AT k = 0 SLOTS 29 .. 32 STAND FOR U_N-1: they carry the
 *      regularisation's wrapped term alone (interval 0 has no actuator rows) -- the one place where the slots differ in meaning from the Jacobian's;
 *      at N = 2 each block then holds one of the two equal terms, as J does.  Continuity and periodicity rows are linear and contribute nothing.
 *      The overlaps (X_k+1 / the next block's X_k, U_k / the next block's U_k-1 slots) are the consumer's to add, as the certificate reads a column
 *      from up to two Jacobian blocks.  The reference's quirks stay: the constant mue in f_y, the path rows at X_k+1 with U_k and friction row k + 1,
 *      sigma of the actuator rows with kappa_cl[k], the energy with the START state (its cross terms between X_k[0], U_k[1] and Xc_k,j); the safe
 *      rows take the second derivative of the branch of max / min taken.
 *   Sums (J, lap time, energy) are taken in ONE order that depends on N alone: thread t of 256 adds intervals t, t + 256, .. in rising order, then a
 *      binary tree over the 256 partial sums -- a problem's bits do not depend on the launch's company, the batch order or the buffers' width.
 *
 * mcq_mintime_pars: the entries of veh_params, vehicle_params_mintime, tire_params_mintime and optim_opts the model reads, ONE record per problem
 *   (a DEVICE array [batch]), so that a sweep over masses or friction levels is one launch.  mcq_mintime_opts: friction -1 (the constant mue),
 *   MCQ_FRIC_LINEAR or MCQ_FRIC_GAUSS (n_gauss 1 .. 15) for the Kamm rows; safe_traj, limit_energy: the optional rows; pwr_behavior must be 0.
 * mcq_mintime_data: the DEVICE arrays of a launch, stated once for the device entries.  n_list [batch] (NULL: all nmax) intervals per problem,
 *   h [batch][nmax], kappa_cl / w_tr_right_cl / w_tr_left_cl [batch][nmax + 1] (the closed arrays: entry N repeats entry 0), w_mue [batch][4][nmax + 1][P]
 *   (P = 2: slope, intercept; P = 2 n_gauss + 2) and center_dist [batch][nmax + 1] exactly as mcq_friction_grid_device / mcq_friction_gauss_device
 *   emit them for tracks of nmax waypoints, w [batch][5 + 24 nmax].
 *
 * mcq_mintime_layout: host, pure.  N >= 2 (the reference's difference matrix degenerates at N = 1).  Also the collocation constants tau, C, D, B
 *   as the kernels use them (computed once on the host; numpy.poly1d's construction to rounding).
 * mcq_mintime_bounds_device: w0 (the flat guess v = 20 m/s), lbw, ubw [batch][5 + 24 nmax], lbg, ubg [batch][ng of nmax] as the reference builds them; the
 *   n bounds from the widths and width_opt.  Entries past a problem's own nw / ng: NaN.
 * mcq_mintime_eval_device: g [batch][ng of nmax], J, lap_time, energy [batch] (energy in kWh, the energy row's value, computed with or without the row),
 *   x_opt [batch][nmax + 1][5], u_opt [batch][nmax][4], tf_opt [batch][nmax][12] (x, y, z of fl, fr, rl, rr at X_k+1), dt_opt, ax_opt, ay_opt, ec_opt
 *   [batch][nmax] (ec in Ws), status [batch].  Any output but g, J and status may be NULL.
 * mcq_mintime_jac_device: blocks, grad_J [batch][5 + 24 nmax], grad_energy (the same; may be NULL).  One lane per (evaluation point, direction): 36 lanes
 *   per interval, a one-tangent dual number each.
 * mcq_mintime_kkt_device: r = grad_J + J_g^T lam_g + lam_x [batch][5 + 24 nmax] under CasADi's sign convention L = f + lam_g . g + lam_x . w, from the blocks
 *   and gradients of mcq_mintime_jac_device and g of mcq_mintime_eval_device; kkt_out [batch][3]: max |r|; the largest violation of lbw <= w <= ubw and
 *   lbg <= g <= ubg (0 where none); the largest |lam * distance to the bound it belongs to| over FINITE bounds -- a positive multiplier belongs to the
 *   upper bound, a negative one to the lower.  grad_energy is read with limit_energy only.
 * mcq_mintime_hess_device: the Hessian blocks from lam_g [batch][ng of nmax] and sigma [batch] (NULL: 1).  A workgroup per interval, one lane per
 *   (evaluation point, unordered pair of its 9 directions): 180 hyper-dual evaluations; every entry has one writer.  Block k is NaN entirely when an
 *   input of interval k is not finite -- its 33 slots of w, h[k] (and h[k - 1] where k > 0), kappa_cl[k], kappa_cl[k + 1], the multiplier of one of
 *   its existing rows, sigma, the energy row's multiplier where enabled -- and no other block is affected.  Multipliers of periodicity rows, of
 *   absent rows and of a disabled energy row are not read.
 * mcq_mintime_hessvec_device: y = H v for nvec vectors per problem, v and y [batch][nvec][5 + 24 nmax], from the blocks.  A lane per entry of w in ONE
 *   order: the products of the block that holds entry 24 k + s at slot s, slots rising, then those of the other block that holds it (block k - 1
 *   for a state of X_k, block k + 1 -- block 0 after the last -- for a control); X_N lies in block N - 1 alone.  Reads n_list alone of the launch's
 *   arrays (h, kappa_cl, w may be NULL).  Entries past a problem's own nw: NaN.  nvec <= 0: MCQ_E_ARG.
 * Edges: outputs are always overwritten.  A NaN or inf in a problem's w or inputs gives NaN in the rows and outputs computed from it and in that problem's
 *   sums and maxima (status MCQ_BAD_INPUT on the evaluation), and has no effect on another problem.  Rows, blocks and entries past a problem's own
 *   N are NaN.  A problem whose n_list entry is below 2 or above nmax: status MCQ_BAD_INPUT, every output of that problem NaN.
 * MCQ_E_ARG: N < 2 (layout), nmax < 2, batch <= 0, an unknown friction model, n_gauss outside 1 .. 15 with the Gaussian model, friction weights or
 *   center_dist missing for the model, pwr_behavior != 0, NULL where an array is required; MCQ_E_TOO_LARGE: 5 + 24 nmax or the launch's blocks beyond
 *   2^31 - 1, more than 65535 problems (they lie along the launches' second axis).  DEVICE pointers; asynchronous on the handle's stream. */
#define MCQ_MT_NX 5
#define MCQ_MT_NU 4
#define MCQ_MT_BLOCK 33
#define MCQ_MT_NPARS 40
typedef struct mcq_mintime_pars {
    double mass, dragcoeff, g, v_max;                                                              /* veh_params */
    double wheelbase_front, wheelbase_rear, track_width_front, track_width_rear, cog_z, I_z;       /* vehicle_params_mintime */
    double liftcoeff_front, liftcoeff_rear, k_brake_front, k_drive_front, k_roll, t_delta, t_drive, t_brake;
    double power_max, f_drive_max, f_brake_max, delta_max;
    double c_roll, f_z0, B_front, C_front, eps_front, E_front, B_rear, C_rear, eps_rear, E_rear;   /* tire_params_mintime */
    double width_opt, mue, penalty_F, penalty_delta, energy_limit, ax_pos_safe, ax_neg_safe, ay_safe;   /* optim_opts */
} mcq_mintime_pars;
typedef struct mcq_mintime_opts {
    int friction, n_gauss, safe_traj, limit_energy, pwr_behavior;
} mcq_mintime_opts;
typedef struct mcq_mintime_dims {
    int nw, ng;
    int off_x, off_u, off_xc, stride_w;            /* X_k at off_x + k stride_w, U_k at off_u + k stride_w, Xc_k,j at off_xc + k stride_w + 5 j */
    int rows_first, rows_next;                     /* rows of interval 0, of every later interval: interval k >= 1 starts at rows_first + (k - 1) rows_next */
    int row_colloc, row_cont, row_power, row_kamm, row_roll, row_pedal, row_act, row_safe;   /* within an interval; row_safe for k >= 1 (4 less at k = 0), -1 where absent */
    int row_periodic, row_energy;                  /* in g; row_energy -1 where absent */
    double tau[4], C[4][4], D[4], B[4];
} mcq_mintime_dims;
typedef struct mcq_mintime_data {
    int batch, nmax;
    const int* n_list;
    const double* h;
    const double* kappa_cl;
    const double* w_tr_right_cl;
    const double* w_tr_left_cl;
    const mcq_mintime_pars* pars;
    const double* w_mue;
    const double* center_dist;
    const double* w;
} mcq_mintime_data;
int mcq_mintime_layout(int N, const mcq_mintime_opts* opts, mcq_mintime_dims* dims_out);
int mcq_mintime_bounds_device(mcq_handle* h, const mcq_mintime_data* data, const mcq_mintime_opts* opts, double* w0_out, double* lbw_out,
                              double* ubw_out, double* lbg_out, double* ubg_out);
int mcq_mintime_eval_device(mcq_handle* h, const mcq_mintime_data* data, const mcq_mintime_opts* opts, double* g_out, double* J_out,
                            double* lap_time_out, double* energy_out, double* x_opt_out, double* u_opt_out, double* tf_opt_out, double* dt_opt_out,
                            double* ax_opt_out, double* ay_opt_out, double* ec_opt_out, int* status_out);
int mcq_mintime_jac_device(mcq_handle* h, const mcq_mintime_data* data, const mcq_mintime_opts* opts, double* blocks_out, double* grad_J_out,
                           double* grad_energy_out);
int mcq_mintime_kkt_device(mcq_handle* h, const mcq_mintime_data* data, const mcq_mintime_opts* opts, const double* g, const double* blocks,
                           const double* grad_J, const double* grad_energy, const double* lam_g, const double* lam_x, const double* lbw,
                           const double* ubw, const double* lbg, const double* ubg, double* r_out, double* kkt_out);
int mcq_mintime_hess_device(mcq_handle* h, const mcq_mintime_data* data, const mcq_mintime_opts* opts, const double* lam_g, const double* sigma,
                            double* hblocks_out);
int mcq_mintime_hessvec_device(mcq_handle* h, const mcq_mintime_data* data, const mcq_mintime_opts* opts, const double* hblocks, const double* v,
                               int nvec, double* y_out);

/* ---- the minimum-time problem: the regularised primal-dual Newton step from the resident blocks (csrc/mcq_mtstep.inc) ----
 * One linear-algebra entry over the layouts above, what an interior-point or SQP iteration needs per iteration: the solution of
 *     K [x_w; x_lam] = rhs,    K = [ H + diag(dw)   J^T ; J   -diag(dg) ]
 * and K's inertia.  H is the sum of the Hessian blocks (overlaps added, block 0's slots 29 .. 32 on U_N-1; the blocks are read as SYMMETRIC, as
 * mcq_mintime_hess_device emits them), J the Jacobian blocks' existing row slots, the constant periodicity rows (+1 at X_0, -1 at X_N) and, with
 * limit_energy, the dense row grad_energy -- the matrix mintime.kkt_matrix assembles.  dw [batch][5 + 24 nmax] and dg [batch][ng of nmax] are the
 * caller's diagonals (barrier and slack terms plus regularisation); any finite value of either sign is taken, the inertia says what came of it.
 * Signs are the certificate's (L = f + lam_g . g).  It is not an NLP loop: no step length, no barrier update, no inertia correction.
 *   hblocks, blocks [batch][nmax][33][33]; grad_energy [batch][5 + 24 nmax], read with limit_energy only (NULL otherwise); rhs and sol_out
 *   [batch][nvec][(5 + 24 nmax) + (ng of nmax)]: the w part at 0, the multiplier part at 5 + 24 nmax.  Of `data` only batch, nmax and n_list are read.
 * Method: a multifrontal LDL^T WITHOUT pivoting in one static order, a front per interval: front k eliminates U_k-1, X_k, Xc_k, the path rows of
 *   interval k - 1 and the collocation and continuity rows of interval k -- no row before the variables it reads -- and passes a Schur complement of
 *   37 on; the lap closes through a border of X_0, U_N-1, the periodicity rows and the energy row, eliminated last.  refine >= 0 steps of
 *   iterative refinement follow, each the float64 residual of K from the blocks and the factor's correction.  res_out [batch][nvec]: the max-norm
 *   of the final residual as computed.  inertia_out [batch][3]: positive, negative and zero pivots.
 * status_out [batch]: MCQ_OK where every pivot is finite and non-zero; MCQ_SINGULAR where one is not -- that problem's solution and residual NaN,
 *   its inertia counted up to that pivot, which is the one zero; MCQ_BAD_INPUT for an n_list entry outside 2 .. nmax or a non-finite entry of an
 *   input inside the problem's own extent (its N blocks, nw, ng entries) -- solution and residual NaN, inertia -1.  No other problem is affected.
 *   Outputs are always overwritten; entries past a problem's own nw / ng are NaN; inputs past them are not read.  A problem's bits depend on
 *   its own N and data alone -- not on the launch's company, the batch order, nmax, nvec or the buffers' width.
 * mcq_mintime_step_bytes (host, pure): the workspace per problem -- per interval the front's 94 x 57 panel of the factor, once the last 37 x 37,
 *   and one residual vector per right-hand side; the handle keeps batch times that between calls (mcq_mintime_step_workspace: what it holds now).
 * MCQ_E_ARG: nvec <= 0, refine < 0, NULL where an array is required, and the option refusals above; MCQ_E_TOO_LARGE: as the entries above, or
 *   nvec times the vector's length beyond 2^31 - 1.  DEVICE pointers; asynchronous on the handle's stream. */
int mcq_mintime_step_bytes(int nmax, const mcq_mintime_opts* opts, int nvec, size_t* bytes_per_problem);
long long mcq_mintime_step_workspace(mcq_handle* h);
int mcq_mintime_step_device(mcq_handle* h, const mcq_mintime_data* data, const mcq_mintime_opts* opts, const double* hblocks, const double* blocks,
                            const double* grad_energy, const double* dw, const double* dg, const double* rhs, int nvec, int refine,
                            double* sol_out, double* res_out, int* inertia_out, int* status_out);

/* Host-buffer entry for a UNIFORM batch (every track n waypoints): reftrack [batch][n][4], normvec [batch][n][2] or NULL,
 * scaling [batch][n] or NULL in host memory, results to host memory.  One asynchronous copy per array straight from / to the
 * caller's buffers -- no packing pass; buffers from mcq_host_alloc (pinned) are copied at PCIe speed, pageable ones go through
 * the runtime's staging.  This is the wall SURVEY.md section 8d defines the metric on ("inputs resident in host pinned memory
 * -> alpha resident in host memory"); bench.py reports it next to the device-resident rate.  Blocking.  Round 6: a batch of 512 or more
 * (minimum-curvature objective, default algorithm) goes in two SLICES, one per compute stream of the handle -- the second slice's upload and the
 * first slice's download overlap the kernels (11.8 ms where the one launch took 13.0 for 1024 x N = 2000; four slices: 11.5, but then a heavy-tailed
 * batch waits for its slowest problems slice by slice);
 * results bitwise those of the one launch; mcq_last_timing is not valid after such a call.  mcq_solve_batch does the same behind its packing
 * threads.  Knobs (environment): MCQ_HOST_ONE_LAUNCH=1, MCQ_HOST_SLICES (2 .. 8), MCQ_HOST_SLICE_MIN. */
int mcq_solve_host(mcq_handle* h, int batch, int n, const double* reftrack, const double* normvec, const double* scaling,
                   double kappa_bound, double w_veh, const mcq_opts* opts, double* alpha_out, double* curv_err_out,
                   int* status_out, mcq_info* info_out);

/* A STREAM of uniform batches from / to host memory with the PCIe hidden behind the kernels (SURVEY.md section 8d defines the
 * metric "inputs resident in host pinned memory -> alpha resident in host memory"): step k's kernels run while step k+1's rows are
 * uploaded and step k-1's results are downloaded, on two copy streams and two sets of device staging buffers -- and, since round 5, on TWO
 * COMPUTE STREAMS with a workspace each (a second 1.8 MB per problem while the entry is in use): consecutive steps are independent, so the
 * kernels of step k+1 start on the compute units step k's launch has already left instead of waiting for its slowest problems.
 * curv_err_out / status_out may be pageable (they pass through pinned staging of the handle and are filled when the call returns); alpha_out and
 * the inputs should be pinned (mcq_host_alloc).  Debugging knobs (environment): MCQ_PIPE_ONE_STREAM=1 keeps every step on the handle's first
 * compute stream (round 4's behaviour, for A/B measurements), MCQ_PIPE_TRACE=1 prints when the host enqueued each step.  Arrays of `steps`
 * host pointers (pinned memory from mcq_host_alloc for full PCIe speed): reftrack[k] [batch][n][4], normvec[k] [batch][n][2] (array or
 * entries may be NULL: derived on the device), scaling[k] [batch][n] (may be NULL), alpha_out[k] [batch][n], curv_err_out[k] [batch],
 * status_out[k] [batch].  Results of step k are bitwise those of mcq_solve_host on the same buffers.  Blocking; returns when
 * every step's results are in host memory. */
int mcq_solve_host_pipelined(mcq_handle* h, int steps, int batch, int n, const double* const* reftrack, const double* const* normvec,
                             const double* const* scaling, double kappa_bound, double w_veh, const mcq_opts* opts,
                             double* const* alpha_out, double* const* curv_err_out, int* const* status_out);

/* The same for batches already RESIDENT in device memory (round 5): arrays of `steps` DEVICE pointers, layouts as for mcq_solve_device; normvec / scaling
 * arrays or entries may be NULL.  The launches of consecutive steps alternate between the handle's two compute streams (a workspace each), so a
 * step's slowest problems finish while the next step's workgroups already fill the compute units the others have left: 113 k solves/s where
 * launch-by-launch calls of mcq_solve_device give 98 k (1024 rings of 2000 waypoints).  The steps must be independent of each other (distinct
 * output buffers; an input may repeat).  Asynchronous: ordered behind what the handle's stream holds when it is called; mcq_sync (or any later
 * call on the handle) waits for every step.  Results of step k are bitwise those of mcq_solve_device on the same buffers. */
int mcq_solve_device_stream(mcq_handle* h, int steps, int batch, int n, const double* const* reftrack, const double* const* normvec,
                            const double* const* scaling, double kappa_bound, double w_veh, const mcq_opts* opts, double* const* alpha_out,
                            double* const* curv_err_out, int* const* status_out);

/* ---- tph.iqp_handler [REF main_globaltraj.py:273-284] as ONE call: the whole iterated re-linearisation of a batch of tracks.
 *
 * Every round is one batched QP pass (mcq_solve_device_ragged; passes 2+ warm-started from the working set the glue carried
 * over) followed, on the device, by the termination test of iqp_handler (round >= iters_min and curv_error_max <=
 * curv_error_allowed), the damping of the early rounds (alpha * round / iters_min) and the glue of mcq_relinearise_device for
 * the tracks that go on.  The host enqueues the first iters_min rounds without looking and then reads ONE int per round (how
 * many tracks are still iterating).  A track whose QP fails keeps that status and stops; the others are not affected.
 * Those first rounds are ONE launch in which every workgroup takes its track through the rounds on its own (a track's passes
 * depend on its own previous pass only: launched round by round, every round would wait for the batch's slowest track);
 * results bitwise those of one launch per round, which is what runs with `stats->timed`, with a round callback, or with
 * $MCQ_IQP_FUSED=0.
 *
 * mcq_iqp_device: everything resident.  reftrack_a / normvec_a [batch][nmax][*] hold the tracks on entry (n_io [batch] their
 * waypoint counts), reftrack_b / normvec_b are the second set of the double buffer; scaling [batch][nmax] (first pass) or NULL.
 * On return: alpha_out [batch][nmax] = alpha of the last pass AS THE QP RETURNED IT, never damped: the damping of the early rounds
 * belongs to the step into the next ring, and no step follows the last pass.  So reftrack + alpha_out * normvectors of the returned
 * state is that pass's own raceline -- also for a track that max_rounds cut off before round iters_min (status MCQ_ITER_CAP,
 * rounds_out = max_rounds, ring, normals and undamped alpha of pass max_rounds; upstream has no round cap and cannot end there).
 * n_io = waypoint counts of the last re-linearisation, buf_out [batch] = 0 / 1: which
 * set holds a track's final reftrack / normvectors, curv_err_out / status_out / rounds_out [batch]; curv_trace_out
 * [batch][MCQ_IQP_TRACE] (optional) = curv_error_max of every round of a track (what iqp_handler prints with print_debug;
 * rounds beyond MCQ_IQP_TRACE are not recorded: rounds_out tells when the trace is truncated).  A track with n_io == 0 on entry is
 * not a track: it never runs (status MCQ_BAD_INPUT from its first, empty pass, rounds_out 1).  stats (optional, host): see mcq_iqp_stats.  Blocking (the loop needs the
 * live count).  A call of either entry that fails in the HIP runtime returns MCQ_E_DEVICE with nothing of it left in flight, and
 * mcq_last_error names the HIP call that failed ("<call> failed: <hip error> (<file>:<line>)"), whatever the thread reported before. */
#define MCQ_IQP_TRACE 16
typedef struct {
    int rounds;             /* rounds run (the slowest track) */
    int qp_solves;          /* QP passes summed over the tracks */
    float solver_ms[16];    /* per round: the QP pass's launch sequence (HIP events; rounds beyond 16 are not recorded; only
                             * filled when `timed` is set on entry: costs one event synchronisation per round) */
    int fallbacks[16];      /* per round: warm starts abandoned for the cold path (needs info read-back: only when `timed`) */
    int timed;              /* in: 1 => fill solver_ms / fallbacks */
} mcq_iqp_stats;
int mcq_iqp_device(mcq_handle* h, int batch, int nmax, int* n_io, double* reftrack_a, double* normvec_a, double* reftrack_b,
                   double* normvec_b, const double* scaling, double kappa_bound, double w_veh, double stepsize_interp,
                   int iters_min, double curv_error_allowed, int max_rounds, const mcq_opts* opts, double* alpha_out,
                   int* buf_out, double* curv_err_out, int* status_out, int* rounds_out, double* curv_trace_out,
                   mcq_iqp_stats* stats);
/* The same from / to host buffers -- what iqp_handler binds.  problems [batch] as for mcq_solve_batch (normvec required; batches
 * above 8 MB are packed into the pinned staging by $MCQ_PACK_THREADS host threads -- default 8 -- in chunks whose uploads overlap
 * the packing of the next; mcq_solve_batch packs the same way);
 * outputs padded to nmax_out waypoints per track (caller's capacity for the re-sampled rings; MCQ_E_TOO_LARGE names nothing
 * partial: a track whose ring outgrows it gets status MCQ_BAD_INPUT): alpha_out [batch][nmax_out], reftrack_out
 * [batch][nmax_out][4], normvec_out [batch][nmax_out][2], n_out / status_out / rounds_out [batch], curv_err_out [batch],
 * curv_trace_out [batch][MCQ_IQP_TRACE] or NULL. */
int mcq_iqp_batch(mcq_handle* h, const mcq_problem* probs, int batch, double stepsize_interp, int iters_min,
                  double curv_error_allowed, int max_rounds, const mcq_opts* opts, int nmax_out, double* alpha_out,
                  double* reftrack_out, double* normvec_out, int* n_out, double* curv_err_out, int* status_out,
                  int* rounds_out, double* curv_trace_out, mcq_iqp_stats* stats);

/* Optional per-round callback of mcq_iqp_device / mcq_iqp_batch (what tph.iqp_handler prints per iteration with print_debug
 * [REF main_globaltraj.py:270,280]): called on the host after the QP pass of every round, before its termination test, with the
 * curvature errors of the pass and the tracks that ran it (live[k] != 0).  Costs one small device-to-host copy and a synchronisation per
 * round while set; cb == NULL removes it. */
typedef void (*mcq_iqp_round_cb)(void* user, int round, int batch, const double* curv_err, const int* live);
int mcq_iqp_set_round_callback(mcq_handle* h, mcq_iqp_round_cb cb, void* user);

/* The one thing the engine reads from the dense spline matrix the reference passes [REF main_globaltraj.py:267 `A=a_interp`;
 * helper_funcs_glob/src/prep_track.py:48-51]: the n spline scalings s_i encoded in the [4n][4n] row-major matrix of tph.calc_splines' closed-spline
 * system (s_i = -A[4i+2][4i+5], s_(n-1) = A[4n-2][1]) -> s_out [n].  check != 0 verifies that A IS that matrix -- the 12 n structural entries at
 * their places and values, the four that mirror the scalings, and not one non-zero anywhere else -- in ONE pass over the matrix on a host thread per 16 MB
 * (32 at most; $MCQ_PACK_THREADS overrides) (512 MB at n = 2000: the numpy restatement of the same check in trajectory_planning_helpers/calc_splines.py took 100-200 ms of
 * a call whose kernel takes 3; round 6).  No GPU involved, no handle.  Returns 0, or MCQ_E_ARG when A does not have the structure (the message
 * names the first offending entry). */
int mcq_les_scalings(const double* A, int n, double* s_out, int check);
/* The same for the [4(n-1)][4(n-1)] matrix of tph.calc_splines' OPEN system through n waypoints: s_out[i] = -A[4i+2][4i+5] for i <= n-3,
 * s_out[n-2] = s_out[n-1] = 1.  check != 0 verifies the 12 n - 15 structural entries: the closed template for splines 0..n-3, the last spline's
 * rows [1 0 0 0] and [1 1 1 1], the heading rows A[-2][1] = 1 and A[-1][-4:] = [0 1 2 3], and nothing else. */
int mcq_les_scalings_open(const double* A, int n, double* s_out, int check);

/* Pinned (page-locked) host memory for callers that want their buffers copied at PCIe speed (mcq_solve_host, mcq_solve_batch,
 * mcq_copy_*). */
int mcq_host_alloc(mcq_handle* h, size_t bytes, void** out);
int mcq_host_free(mcq_handle* h, void* ptr);

/* Device memory plumbing on the handle's device and stream, for callers that keep data resident between calls (the
 * Python IQP driver) without loading a second HIP runtime into the process: allocate (zero-filled) / free / blocking
 * copies.  A reference-side binding would use these exactly where a CUDA/HIP-aware caller uses its own allocator. */
int mcq_device_alloc(mcq_handle* h, size_t bytes, void** out);
int mcq_device_free(mcq_handle* h, void* ptr);
int mcq_copy_to_device(mcq_handle* h, void* dst, const void* src, size_t bytes);
int mcq_copy_to_host(mcq_handle* h, void* dst, const void* src, size_t bytes);
int mcq_sync(mcq_handle* h);
void* mcq_stream(mcq_handle* h);

/* Timing of the last mcq_solve_device / mcq_solve_batch call, measured with HIP events on the handle's stream(s):
 * ms[2] the solver kernel (since round 4 the whole QP pass: assembly, solve, post-check -- and, round 5, the Goldfarb-Idnani path of the
 * problems that need it), ms[4] the whole launch sequence; ms[0] the assembly kernel of the shortest-path objective (else ~0);
 * ms[1], ms[3] are 0 (the kernels they timed until round 3 no longer exist; the slots stay for ABI compatibility).
 * After a SLICED mcq_solve_device, ms[2] and ms[4] run from the start of the first slice to the later of the two slices' ends, through events on
 * both compute streams (neither waits for the other): with earlier calls still in flight that includes the time a slice spent queued behind
 * them -- a launch's own duration only for a call enqueued on an idle handle. */
int mcq_last_timing(mcq_handle* h, float ms[5]);

/* A SPAN of launches timed on the device: mcq_timing_begin orders the handle's compute stream behind everything enqueued so far (pending slices of
 * mcq_solve_device included) and records an event on it; mcq_timing_end records an end event on that stream -- and one on the second compute stream
 * where slices of mcq_solve_device are pending there --, waits, and returns the milliseconds from the begin event to the LATER end and the number
 * of solver launches the handle enqueued in between (mcq_solve_device* / the QP passes of the IQP entries; not the second stream of
 * mcq_solve_host_pipelined).  A sliced call -- mcq_solve_device, and likewise mcq_solve_host / mcq_solve_batch / mcq_solve_batch_ends, which were
 * not counted at all before -- counts as ONE launch, per call (mcq_last_timing still refuses after a sliced HOST call: no pair of events spans
 * its slices).  With calls enqueued back to back -- no host
 * synchronisation inside the span -- ms / launches is the average device time per step, launch gaps included: what bench.py's
 * `roofline.kernel_ms` is (round 5; until then it synchronised after every step to read mcq_last_timing, and a slow host showed up in `value`).
 * With slices of consecutive calls overlapping, that is no longer the duration of any single kernel. */
int mcq_timing_begin(mcq_handle* h);
int mcq_timing_end(mcq_handle* h, float* ms_out, int* launches_out);

/* Bytes of device workspace the handle currently holds (for DESIGN.md / bench reporting). */
long long mcq_workspace_bytes(mcq_handle* h);

/* 1 if the last host-buffer batch of problem records (mcq_solve_batch, mcq_iqp_batch) was uploaded WITHOUT the packing pass (round 6): a
 * uniform batch -- every track n waypoints -- whose reftrack / normvec / scaling rows lie back to back in page-locked memory (mcq_host_alloc) goes
 * to the device straight from there, one strided copy per array; anything else (ragged, pageable, scattered) is packed into the handle's pinned
 * staging first (several host threads, chunk by chunk).  $MCQ_PACK_ALWAYS=1 forces the packing pass.  Same results either way. */
int mcq_last_upload_was_direct(mcq_handle* h);

/* ---- the one collective of a multi-GPU job (north_star: "a single RCCL all-gather over xGMI to collect the alpha
 *      vectors").  One process per GPU, one handle per process; independent QPs are block-partitioned over the ranks and every rank
 *      solves its shard with the entries above -- no collective inside a solve.  The gather is the engine's own: ncclAllGather of RCCL
 *      (loaded with dlopen on first use: $MCQ_RCCL_LIB, else $ROCM_PATH/lib/librccl.so.1, else /opt/rocm/lib/librccl.so.1, else
 *      librccl.so.1 -- a process that never gathers never loads it).  ORDERING, stated once: a gather runs on a COMM STREAM of the handle,
 *      ordered behind everything enqueued on the handle's compute stream at the time of the call (an event) -- so after the solve that
 *      filled `send` -- and concurrent with whatever is enqueued on the compute stream afterwards (the next solve).  Work on the compute
 *      stream is NOT ordered behind a gather; a caller waits with mcq_comm_wait or mcq_sync before it reads `recv` or overwrites `send`.
 *      (The blocking helpers mcq_copy_to_host and mcq_device_free do wait for the gathers enqueued before them, since round 5.)
 *      No torch, no second HIP runtime in the process.
 *      Reference side: nothing to replace -- the reference is a single-process script; a caller that shards its sweeps
 *      [REF main_globaltraj.py:441-505, the lap-time matrix loops] would call these three.
 *   mcq_comm_unique_id   rank 0 creates the 128-byte id and ships it to the other ranks by whatever means the launcher offers
 *                        (bench.py: one broadcast over the gloo rendezvous of torch.distributed.run; a file; MPI ...)
 *   mcq_comm_init        collective over all ranks: ncclCommInitRank on the handle's device
 *   mcq_comm_allgather   recv [world][count] <- send [count] of every rank, device pointers, dtype MCQ_DT_*.  Asynchronous: ordered behind
 *                        everything enqueued on the handle's stream so far (the solve that filled `send`), but on a stream of its own,
 *                        so the handle's stream goes on with the NEXT solve while the gather runs (keep two send buffers and alternate).
 *                        `send` must not be overwritten and `recv` not read before mcq_comm_wait / mcq_sync.  world == 1: the same call
 *                        path (RCCL is initialised and used).
 *   mcq_comm_wait        blocks the host until the gather enqueued `lag` gathers ago has finished (0: the latest, 1: the one before:
 *                        what a caller alternating two send buffers waits for before it reuses one); ms_out (optional): its duration
 *                        on the device.  mcq_sync waits for all of them.
 *   mcq_comm_destroy     also done by mcq_destroy */
#define MCQ_COMM_ID_BYTES 128
enum { MCQ_DT_F64 = 0, MCQ_DT_F32 = 1, MCQ_DT_I32 = 2 };
int mcq_comm_unique_id(unsigned char id_out[MCQ_COMM_ID_BYTES]);
int mcq_comm_init(mcq_handle* h, int rank, int world, const unsigned char id[MCQ_COMM_ID_BYTES]);
int mcq_comm_allgather(mcq_handle* h, const void* send, void* recv, size_t count, int dtype);
int mcq_comm_wait(mcq_handle* h, int lag, float* ms_out);
int mcq_comm_world(mcq_handle* h, int* rank_out, int* world_out);      /* MCQ_E_ARG if no communicator was initialised */
int mcq_comm_destroy(mcq_handle* h);

#ifdef __cplusplus
}
#endif
#endif /* MCQ_H */
