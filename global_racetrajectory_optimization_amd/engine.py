"""
ctypes host binding of libmcq.so (C ABI in include/mcq.h) -- the MI355X minimum-curvature QP engine.

This is plumbing, not a fallback layer: the only implementation behind these calls is the hand-written HIP library
built by csrc/build.sh for gfx950.  If it is missing or cannot be loaded the import of the engine fails loudly;
there is no CPU path in the product (the CPU oracle lives in /oracle and is test infrastructure only).

Mirrors the reference-side interface for the hot path:
    solve_batch(problems)          -> what tph.opt_min_curv.opt_min_curv binds  [REF main_globaltraj.py:264-271]
    Engine.solve_device(...)       -> device-resident batch entry (bench, IQP driver, multi-GPU shards)
"""
import ctypes
import math
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(_HERE, "csrc", "libmcq.so")

STATUS_OK, STATUS_INFEASIBLE, STATUS_NOT_PD, STATUS_ITER_CAP, STATUS_BAD_INPUT, STATUS_KAPPA_INFEASIBLE, \
    STATUS_KAPPA_ACTIVE, STATUS_RING_OVERFLOW, STATUS_KAPPA_NO_SLOT, STATUS_SINGULAR = range(10)

_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int)


class McqProblem(ctypes.Structure):
    _fields_ = [("n", ctypes.c_int), ("reftrack", _dp), ("normvec", _dp), ("scaling", _dp),
                ("kappa_bound", ctypes.c_double), ("w_veh", ctypes.c_double)]


class McqEnds(ctypes.Structure):
    """mcq_ends: per-problem ring / open-chain record of mcq_solve_batch_ends (include/mcq.h)."""
    _fields_ = [("closed", ctypes.c_int), ("fix_s", ctypes.c_int), ("fix_e", ctypes.c_int), ("psi_s", ctypes.c_double),
                ("psi_e", ctypes.c_double)]


FIX_HALF_WIDTH = 0.05       # MCQ_FIX_HALF_WIDTH
CHAIN_MAXN = 2048           # MCQ_CHAIN_MAXN


# the same record as a numpy structured type (field offsets taken from the ctypes layout): a batch's records are filled column by
# column -- one ctypes attribute store per field and track, as the per-track loop did it, costs 12 ms for 1024 tracks
_PROBLEM_DTYPE = np.dtype({"names": ["n", "reftrack", "normvec", "scaling", "kappa_bound", "w_veh"],
                           "formats": ["<i4", "<u8", "<u8", "<u8", "<f8", "<f8"],
                           "offsets": [getattr(McqProblem, f).offset for f in ("n", "reftrack", "normvec", "scaling", "kappa_bound", "w_veh")],
                           "itemsize": ctypes.sizeof(McqProblem)})


def _addr(a):
    return 0 if a is None else a.__array_interface__["data"][0]


def _addrs(arrays):
    """Addresses of a batch's per-track arrays: a list of arrays (None = NULL), or ONE stacked C-contiguous array [B, ...] (row k is
    track k: base + k * stride, no per-track Python work), or None (all NULL)."""
    if arrays is None:
        return 0
    if isinstance(arrays, np.ndarray):
        return arrays.__array_interface__["data"][0] + np.arange(arrays.shape[0], dtype=np.uint64) * np.uint64(arrays.strides[0])
    return [_addr(a) for a in arrays]


def problem_records(refs, nvs, scs, kappa_bound, w_veh):
    """mcq_problem records of a batch: refs / nvs / scs are lists of C-contiguous float64 arrays (entries of nvs / scs may be None =
    NULL) or stacked arrays [B, n, 4] / [B, n, 2] / [B, n] (see _addrs), kappa_bound / w_veh scalars or per-track sequences.  Returns
    (records, pointer for the C ABI); the caller keeps the arrays alive."""
    rec = np.zeros(len(refs), dtype=_PROBLEM_DTYPE)
    rec["n"] = refs.shape[1] if isinstance(refs, np.ndarray) else [r.shape[0] for r in refs]
    rec["reftrack"] = _addrs(refs)
    rec["normvec"] = _addrs(nvs)
    rec["scaling"] = _addrs(scs)
    rec["kappa_bound"] = kappa_bound
    rec["w_veh"] = w_veh
    return rec, ctypes.cast(rec.ctypes.data, ctypes.POINTER(McqProblem))


OBJ_MIN_CURV, OBJ_SHORTEST_PATH = 0, 1      # mcq_opts.objective (include/mcq.h)
ALG_DEFAULT, ALG_GI = 0, 1                  # mcq_opts.algorithm


class McqOpts(ctypes.Structure):
    _fields_ = [("algorithm", ctypes.c_int), ("max_ipm_iter", ctypes.c_int), ("max_as_iter", ctypes.c_int),
                ("refine_steps", ctypes.c_int), ("check_kappa", ctypes.c_int), ("objective", ctypes.c_int),
                ("warm_start", ctypes.c_int)]


class McqVelOpts(ctypes.Structure):
    _fields_ = [("dyn_model_exp", ctypes.c_double), ("filt_window", ctypes.c_int), ("reserved_", ctypes.c_int), ("mu", ctypes.c_void_p)]


class McqVelForms(ctypes.Structure):
    _fields_ = [("dyn_model_exp", ctypes.c_double), ("filt_window", ctypes.c_int), ("closed", ctypes.c_int), ("mu", ctypes.c_void_p),
                ("loc_gg", ctypes.c_void_p), ("v_start", ctypes.c_void_p), ("v_end", ctypes.c_void_p)]


class McqInfo(ctypes.Structure):
    _fields_ = [("ipm_iters", ctypes.c_int), ("as_iters", ctypes.c_int), ("n_active_box", ctypes.c_int),
                ("n_active_kappa", ctypes.c_int), ("kappa_max", ctypes.c_double), ("kkt_res", ctypes.c_double),
                ("ticks", ctypes.c_longlong * 8), ("refine_rounds", ctypes.c_int), ("second_attempt", ctypes.c_int),
                ("f32_factorisations", ctypes.c_int), ("gi_iters", ctypes.c_int)]


class McqIqpStats(ctypes.Structure):
    _fields_ = [("rounds", ctypes.c_int), ("qp_solves", ctypes.c_int), ("solver_ms", ctypes.c_float * 16),
                ("fallbacks", ctypes.c_int * 16), ("timed", ctypes.c_int)]


IQP_TRACE = 16      # MCQ_IQP_TRACE

# include/mcq.h: the columns of a trajectory row, the limit quantities, check_traj's verdict bits and margins, the boundary modes
TRAJ_COLS = 7
TRAJ_NLIM = 6
LIMIT_NAMES = ("kappa_max", "ay_max", "ax_wo_drag_max", "ax_wo_drag_min", "a_tot_max", "vx_max")
CHECK_ACC_MARGIN = 0.1
CHECK_DIST_WARN = 1.0
CHK_KAPPA, CHK_AY, CHK_AX_POS, CHK_AX_NEG, CHK_A_TOT, CHK_MACHINES, CHK_V_MAX = 1, 2, 4, 8, 16, 32, 64
BOUNDS_ALL, BOUNDS_FIRST_ROW = 0, 1
LTPL_COLS = 12      # MCQ_LTPL_COLS: x_ref, y_ref, w_r, w_l, n_x, n_y, alpha, s_ref, psi, kappa, vx, ax
FRIC_LINEAR, FRIC_GAUSS = 0, 1                      # MCQ_FRIC_*: the model mcq_friction_model_device evaluates
FRIC_CENTRES_FIT, FRIC_CENTRES_MINTIME = 0, 1       # MCQ_FRIC_CENTRES_*: where the Gaussian model's bumps sit
FGEN_NONFINITE, FGEN_FEW, FGEN_OVERFLOW, FGEN_GRID = 1, 2, 4, 8     # MCQ_FGEN_*: the status bits of the friction-map generation

# ---- the minimum-time NLP (include/mcq.h "the minimum-time optimal-control problem") ----
MINTIME_PARS = ("mass", "dragcoeff", "g", "v_max",
                "wheelbase_front", "wheelbase_rear", "track_width_front", "track_width_rear", "cog_z", "I_z", "liftcoeff_front", "liftcoeff_rear",
                "k_brake_front", "k_drive_front", "k_roll", "t_delta", "t_drive", "t_brake", "power_max", "f_drive_max", "f_brake_max", "delta_max",
                "c_roll", "f_z0", "B_front", "C_front", "eps_front", "E_front", "B_rear", "C_rear", "eps_rear", "E_rear",
                "width_opt", "mue", "penalty_F", "penalty_delta", "energy_limit", "ax_pos_safe", "ax_neg_safe", "ay_safe")      # mcq_mintime_pars, in order
MT_BLOCK = 33           # MCQ_MT_BLOCK: row and column slots of a Jacobian block
MT_FRICTION = {None: -1, "linear": FRIC_LINEAR, "gauss": FRIC_GAUSS}


class McqMintimeOpts(ctypes.Structure):
    _fields_ = [("friction", ctypes.c_int), ("n_gauss", ctypes.c_int), ("safe_traj", ctypes.c_int), ("limit_energy", ctypes.c_int),
                ("pwr_behavior", ctypes.c_int)]


class McqMintimeDims(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int) for k in ("nw", "ng", "off_x", "off_u", "off_xc", "stride_w", "rows_first", "rows_next", "row_colloc", "row_cont",
                                            "row_power", "row_kamm", "row_roll", "row_pedal", "row_act", "row_safe", "row_periodic", "row_energy")] + \
               [("tau", ctypes.c_double * 4), ("C", ctypes.c_double * 16), ("D", ctypes.c_double * 4), ("B", ctypes.c_double * 4)]


class McqMintimeData(ctypes.Structure):
    _fields_ = [("batch", ctypes.c_int), ("nmax", ctypes.c_int)] + \
               [(k, ctypes.c_void_p) for k in ("n_list", "h", "kappa_cl", "w_tr_right_cl", "w_tr_left_cl", "pars", "w_mue", "center_dist", "w")]


IQP_ROUND_CB = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int))

# The C ABI of include/mcq.h, name -> (restype, argtypes), in the order the entries were added: what load_library declares, and
# EXPORTED_SYMBOLS.  ctypes checks none of it against the library (tests/helper_checks.py counts the header's parameters).
_vp, _ci, _cd, _sz, _P = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_size_t, ctypes.POINTER
_po = _P(McqOpts)
_SOLVE_DEVICE = [_vp, _ci, _ci, _vp, _vp, _vp, _cd, _cd, _po, _vp, _vp, _vp, _vp]
_SOLVE_ROWS = [_vp, _ci, _ci, _ci, _vp, _vp, _cd, _cd, _po, _vp, _vp, _vp, _vp]
_SOLVE_STREAM = [_vp, _ci, _ci, _ci, _vp, _vp, _vp, _cd, _cd, _po, _vp, _vp, _vp]
_ABI = {
    "mcq_create": (_ci, [_ci, _P(_vp)]),
    "mcq_destroy": (None, [_vp]),
    "mcq_last_error": (ctypes.c_char_p, []),
    "mcq_default_opts": (None, [_po]),
    "mcq_solve_batch": (_ci, [_vp, _P(McqProblem), _ci, _po, _dp, _dp, _ip, _P(McqInfo)]),
    "mcq_solve_host": (_ci, _SOLVE_DEVICE),
    "mcq_iqp_device": (_ci, [_vp, _ci, _ci, _vp, _vp, _vp, _vp, _vp, _vp, _cd, _cd, _cd, _ci, _cd, _ci, _po, _vp, _vp, _vp, _vp, _vp, _vp,
                             _P(McqIqpStats)]),
    "mcq_iqp_batch": (_ci, [_vp, _P(McqProblem), _ci, _cd, _ci, _cd, _ci, _po, _ci, _dp, _dp, _dp, _ip, _dp, _ip, _ip, _dp, _P(McqIqpStats)]),
    "mcq_iqp_set_round_callback": (_ci, [_vp, IQP_ROUND_CB, _vp]),
    "mcq_host_alloc": (_ci, [_vp, _sz, _P(_vp)]),
    "mcq_host_free": (_ci, [_vp, _vp]),
    "mcq_solve_device": (_ci, _SOLVE_DEVICE),
    "mcq_solve_device_f32": (_ci, _SOLVE_DEVICE),
    "mcq_solve_device_f32_rows": (_ci, _SOLVE_ROWS),
    "mcq_solve_batch_f32": (_ci, _SOLVE_ROWS),
    "mcq_solve_host_pipelined": (_ci, _SOLVE_STREAM),
    "mcq_solve_device_stream": (_ci, _SOLVE_STREAM),
    "mcq_solve_device_ragged": (_ci, [_vp, _ci, _ci, _vp, _vp, _vp, _vp, _cd, _cd, _po, _vp, _vp, _vp, _vp]),
    "mcq_solve_device_ragged_params": (_ci, [_vp, _ci, _ci, _vp, _vp, _vp, _vp, _cd, _cd, _vp, _vp, _po, _vp, _vp, _vp, _vp]),
    "mcq_prep_device": (_ci, [_vp, _ci, _ci, _vp, _vp, _vp, _vp, _vp]),
    "mcq_relinearise_device": (_ci, [_vp, _ci, _ci, _vp, _vp, _vp, _vp, _vp, _cd, _cd, _vp, _vp, _vp, _vp]),
    "mcq_vel_profile_device": (_ci, [_vp, _ci, _ci, _ci, _vp, _vp, _vp, _vp, _ci, _vp, _ci, _vp, _vp, _vp, _cd, _vp, _vp]),
    "mcq_vel_profile_device_ragged": (_ci, [_vp, _ci, _ci, _vp, _vp, _vp, _vp, _vp, _ci, _vp, _ci, _vp, _vp, _vp, _cd, _vp, _vp]),
    "mcq_vel_profile_device_opts": (_ci, [_vp, _ci, _ci, _ci, _vp, _vp, _vp, _vp, _vp, _ci, _vp, _ci, _vp, _vp, _vp, _P(McqVelOpts), _vp, _vp]),
    "mcq_vel_profile_device_forms": (_ci, [_vp, _ci, _ci, _ci, _vp, _vp, _vp, _vp, _vp, _ci, _vp, _ci, _vp, _vp, _vp, _P(McqVelForms), _vp, _vp]),
    "mcq_raceline_device": (_ci, [_vp, _ci, _ci, _vp, _vp, _vp, _vp, _cd, _ci, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mcq_normals_crossing_device": (_ci, [_vp, _ci, _ci, _vp, _vp, _vp, _ci, _vp]),
    "mcq_device_alloc": (_ci, [_vp, _sz, _P(_vp)]),
    "mcq_device_free": (_ci, [_vp, _vp]),
    "mcq_copy_to_device": (_ci, [_vp, _vp, _vp, _sz]),
    "mcq_copy_to_host": (_ci, [_vp, _vp, _vp, _sz]),
    "mcq_sync": (_ci, [_vp]),
    "mcq_stream": (_vp, [_vp]),
    "mcq_last_timing": (_ci, [_vp, _P(ctypes.c_float * 5)]),
    "mcq_timing_begin": (_ci, [_vp]),
    "mcq_timing_end": (_ci, [_vp, _P(ctypes.c_float), _ip]),
    "mcq_workspace_bytes": (ctypes.c_longlong, [_vp]),
    "mcq_comm_unique_id": (_ci, [ctypes.c_char_p]),
    "mcq_comm_init": (_ci, [_vp, _ci, _ci, ctypes.c_char_p]),
    "mcq_comm_allgather": (_ci, [_vp, _vp, _vp, _sz, _ci]),
    "mcq_comm_wait": (_ci, [_vp, _ci, _P(ctypes.c_float)]),
    "mcq_comm_world": (_ci, [_vp, _ip, _ip]),
    "mcq_comm_destroy": (_ci, [_vp]),
    "mcq_les_scalings": (_ci, [_vp, _ci, _vp, _ci]),
    "mcq_last_upload_was_direct": (_ci, [_vp]),
    "mcq_solve_batch_ends": (_ci, [_vp, _P(McqProblem), _P(McqEnds), _ci, _po, _dp, _dp, _ip, _P(McqInfo)]),
    "mcq_les_scalings_open": (_ci, [_vp, _ci, _vp, _ci]),
    "mcq_raceline_device_ends": (_ci, [_vp, _ci, _ci, _vp, _vp, _vp, _vp, _vp, _vp, _cd, _ci, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mcq_trajectory_device": (_ci, [_vp, _ci, _ci, _ci, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _ci, _vp, _vp, _vp, _vp, _ci, _vp, _ci, _cd, _vp, _vp, _vp,
                                    _vp, _vp]),
    "mcq_bound_dists_device": (_ci, [_vp, _ci, _ci, _vp, _vp, _vp, _ci, _vp, _vp, _vp, _cd, _cd, _vp, _vp, _cd, _ci, _vp, _vp, _vp, _vp, _vp]),
    "mcq_spline_approx_device": (_ci, [_vp, _ci, _ci, _vp, _vp, _ci, _ci, _vp, _vp, _vp, _cd, _ci, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mcq_spline_fit_device": (_ci, [_vp, _ci, _ci, _vp, _vp, _cd, _ci, _ci, _cd, _ci, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mcq_min_width_device": (_ci, [_vp, _ci, _ci, _vp, _vp, _cd, _vp]),
    "mcq_export_device": (_ci, [_vp, _ci, _ci, _vp, _vp, _vp, _vp, _ci, _ci, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mcq_fmap_create": (_ci, [_vp, _ci, _vp, _vp, _cd, _P(_vp)]),
    "mcq_fmap_destroy": (_ci, [_vp, _vp]),
    "mcq_fmap_info": (_ci, [_vp, _ip, _ip, _ip, _dp, _P(ctypes.c_longlong)]),
    "mcq_fmap_query_device": (_ci, [_vp, _vp, _ci, _vp, _vp, _vp, _vp]),
    "mcq_friction_grid_device": (_ci, [_vp, _vp, _ci, _ci, _vp, _vp, _vp, _cd, _vp, _cd, _cd, _cd, _ci, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mcq_friction_gauss_device": (_ci, [_vp, _ci, _ci, _ci, _vp, _vp, _vp, _vp, _ci, _cd, _vp, _vp, _vp, _vp]),
    "mcq_friction_model_device": (_ci, [_vp, _ci, _ci, _ci, _vp, _vp, _ci, _vp, _ci, _ci, _vp, _vp, _vp, _ci, _vp]),
    "mcq_points_in_path_device": (_ci, [_vp, _ci, _ci, _vp, _vp, _vp, _ci, _vp, _vp, _vp, _vp, _vp]),
    "mcq_friction_gen_device": (_ci, [_vp, _ci, _ci, _vp, _vp, _cd, _vp, _ci, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mcq_f32_rows_device": (_ci, [_vp, _ci, _ci, _ci, _vp, _vp, _vp]),
    "mcq_f32_widen_device": (_ci, [_vp, _sz, _vp, _vp]),
    "mcq_f32_narrow_device": (_ci, [_vp, _sz, _vp, _vp]),
    "mcq_mintime_layout": (_ci, [_ci, _P(McqMintimeOpts), _P(McqMintimeDims)]),
    "mcq_mintime_bounds_device": (_ci, [_vp, _P(McqMintimeData), _P(McqMintimeOpts), _vp, _vp, _vp, _vp, _vp]),
    "mcq_mintime_eval_device": (_ci, [_vp, _P(McqMintimeData), _P(McqMintimeOpts), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mcq_mintime_jac_device": (_ci, [_vp, _P(McqMintimeData), _P(McqMintimeOpts), _vp, _vp, _vp]),
    "mcq_mintime_kkt_device": (_ci, [_vp, _P(McqMintimeData), _P(McqMintimeOpts), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mcq_mintime_hess_device": (_ci, [_vp, _P(McqMintimeData), _P(McqMintimeOpts), _vp, _vp, _vp]),
    "mcq_mintime_hessvec_device": (_ci, [_vp, _P(McqMintimeData), _P(McqMintimeOpts), _vp, _vp, _ci, _vp]),
    "mcq_mintime_step_bytes": (_ci, [_ci, _P(McqMintimeOpts), _ci, _P(_sz)]),
    "mcq_mintime_step_workspace": (ctypes.c_longlong, [_vp]),
    "mcq_mintime_step_device": (_ci, [_vp, _P(McqMintimeData), _P(McqMintimeOpts), _vp, _vp, _vp, _vp, _vp, _vp, _ci, _ci, _vp, _vp, _vp, _vp]),
}
EXPORTED_SYMBOLS = tuple(_ABI)


class EngineError(RuntimeError):
    pass


def load_library(path=None):
    """Load libmcq.so and declare the C ABI.  Raises EngineError if the HIP library is absent -- never falls back."""
    path = path or os.environ.get("MCQ_LIB") or DEFAULT_LIB
    if not os.path.exists(path):
        raise EngineError("MI355X engine library not found at %s -- build it with "
                          "global_racetrajectory_optimization_amd/csrc/build.sh (hipcc, gfx950)" % path)
    lib = ctypes.CDLL(path)
    for name, (restype, argtypes) in _ABI.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    return lib


def _as_dp(a):
    return a.ctypes.data_as(_dp)


F32_ABSOLUTE, F32_INCREMENTS = 0, 1      # MCQ_F32_* (include/mcq.h): layout of the coordinate columns of float rows


def rows_to_increments(reftrack):
    """fp64 rows [..., n, 4] = [x, y, w_r, w_l] -> (float32 rows [..., n, 4] = [x_{i+1} - x_i, y_{i+1} - y_i, w_r, w_l] around the
    ring, float64 origin [..., 2] = the first waypoint): the MCQ_F32_INCREMENTS layout of the fp32 entries.  The differences are
    taken in fp64 and rounded once."""
    ref = np.asarray(reftrack, dtype=np.float64)
    out = np.empty(ref.shape, dtype=np.float32)
    out[..., :2] = np.roll(ref[..., :2], -1, axis=-2) - ref[..., :2]
    out[..., 2:] = ref[..., 2:]
    return out, np.ascontiguousarray(ref[..., 0, :2])


def increments_to_rows(rows32, origin=None):
    """What the device rebuilds from MCQ_F32_INCREMENTS rows (mcq_widen_rows_kernel), in numpy: fp64 running sum from the origin with
    the closure defect of the float increments spread evenly over the ring.  For tests and for callers that want the reference
    line the engine saw.  Equal to the device's rows up to rounding, not bit for bit: the cumsum rounds once per waypoint where the
    kernel's slices round ceil(n / 64) times, so x, y stand within (2 n + 12) 2^-53 (max|origin| + 2 max_col sum |increment|) of the exact
    rebuild (tests/f32_ref.py: host_guard; the device meets the same bound with 3 ceil(n / 64) + 12).  The device's own rows:
    Engine.f32_rows_device."""
    r = np.asarray(rows32, dtype=np.float64)
    n = r.shape[-2]
    d = r[..., :2] - r[..., :2].mean(axis=-2, keepdims=True)
    xy = np.concatenate((np.zeros(r.shape[:-2] + (1, 2)), np.cumsum(d, axis=-2)[..., :-1, :]), axis=-2)
    if origin is not None:
        xy = xy + np.asarray(origin, dtype=np.float64)[..., None, :]
    return np.concatenate((xy, r[..., 2:]), axis=-1)


def _pad_rows(rows, cols, nmin=0, strict=True):
    """A ragged list of [n_k, c] arrays as (ns int32 [B], padded float64 [B, max(nmax, nmin), cols]), zeros behind each n_k.  strict: a row
    with fewer than `cols` columns is numpy's ValueError; strict=False zero-fills its missing columns."""
    rows = [np.asarray(r, dtype=np.float64)[:, :cols] for r in rows]
    ns = np.array([r.shape[0] for r in rows], dtype=np.int32)
    out = np.zeros((len(rows), max(int(ns.max()), nmin), cols))
    for k, r in enumerate(rows):
        out[k, :ns[k], :cols if strict else r.shape[1]] = r
    return ns, out


def _pad_like(rows, ns, tail=(), nmin=0):
    """A second list (normals: tail (2,); alphas: ()) behind the lengths of a packed one, [B, max(nmax, nmin)] + tail: row k must fill ns[k] rows."""
    out = np.zeros((len(rows), max(int(ns.max()), nmin)) + tail)
    for k, r in enumerate(rows):
        out[k, :ns[k]] = r
    return out


def _pad_last(rows, width, lead=()):
    """A ragged list of float64 arrays lead + [n_k] as [B] + lead + [width], zeros behind each n_k <= width."""
    out = np.zeros((len(rows),) + lead + (width,))
    for k, r in enumerate(rows):
        out[k, ..., :r.shape[-1]] = r
    return out


def _closed_length(xy):
    """The length of the closed polygon through the rows of xy [n, 2]."""
    return float(np.sum(np.hypot(*np.diff(np.vstack((xy, xy[:1])), axis=0).T)))


def _per_variant(bsz, *values):
    """Scalars or [bsz] sequences as contiguous float64 arrays [bsz] each."""
    return [np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float64), (bsz,))) for a in values]


INFO_FIELDS = tuple(f[0] for f in McqInfo._fields_)


def _info_dicts(infos, fields=INFO_FIELDS):
    """A sequence of McqInfo records as dicts of the named fields."""
    return [{f: list(getattr(i, f)) if f == "ticks" else getattr(i, f) for f in fields} for i in infos]


def export_result(tab, idx, lens, s_ref, total, status, ns, ms, tr, tj):
    """Engine.export_batch's host piece: the padded outputs of mcq_export_device cut to lists (ns [tracks], ms [tracks], tr [batch] = track_of,
    tj = the padded trajectories), and the closed race tables."""
    tracks = len(ns)
    in_range = lambda t: 0 <= t < tracks        # noqa: E731
    n_of = [min(max(int(ns[t]), 0), tab.shape[1] - 1) if in_range(t) else 0 for t in tr]
    m_of = [min(max(int(ms[t]), 0), tj.shape[1]) if in_range(t) else 0 for t in tr]
    race_cl = []
    for v, t in enumerate(tr):
        rows = tj[v, :m_of[v]]
        last = rows[:1].copy() if m_of[v] else np.full((1, tj.shape[2]), np.nan)
        last[0, 0] = total[t] if (in_range(t) and status[v] == 0) else np.nan
        race_cl.append(np.vstack((rows, last)))
    return dict(ltpl=[tab[v, :n_of[v] + 1].copy() for v in range(len(tr))], idx=[idx[v, :n_of[v]].copy() for v in range(len(tr))],
                spline_lengths=[lens[t, :max(min(int(ns[t]), lens.shape[1]), 0)].copy() for t in range(tracks)],
                s_ref=[s_ref[t, :max(min(int(ns[t]), lens.shape[1]), 0) + 1].copy() for t in range(tracks)],
                spline_total=total, status=status, race_cl=race_cl)


class _Scope:
    """The device allocations of one call (Engine.scope): freed on exit, in allocation order, with or without an exception in flight."""

    def __init__(self, eng):
        self.eng, self.ptrs, self.extent = eng, [], {}      # extent: pointer -> (shape, dtype) of what out / up / adopt put behind it

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        while self.ptrs:
            self.eng.free(self.ptrs.pop(0))

    def new(self, nbytes):
        self.ptrs.append(self.eng.alloc(nbytes))
        return self.ptrs[-1]

    def out(self, shape, dtype=np.float64, floor=0):
        """Pointer to a zero-filled array of that shape (an int: [shape]) and dtype, at least `floor` bytes; get(pointer) fetches it."""
        ptr = self.new(max(int(np.prod(shape)) * np.dtype(dtype).itemsize, floor))
        self.extent[ptr] = (shape, dtype)
        return ptr

    def get(self, ptr):
        """The array behind a pointer of out, up or adopt(ptr, shape), as the device holds it now."""
        return self.eng.download(ptr, *self.extent[ptr])

    def up(self, a):
        """Pointer to a device copy of the array (made contiguous); None for None."""
        if a is None:
            return None
        a = np.ascontiguousarray(a)
        self.eng.upload(self.new(a.nbytes), a)
        self.extent[self.ptrs[-1]] = (a.shape, a.dtype)
        return self.ptrs[-1]

    def adopt(self, ptr, shape=None, dtype=np.float64):
        """A pointer another scope released: this one frees it.  shape: what get(ptr) fetches."""
        self.ptrs.append(ptr)
        if shape is not None:
            self.extent[ptr] = (shape, dtype)
        return ptr

    def release(self, ptr):
        """The pointer leaves the scope: the caller frees it."""
        self.ptrs.remove(ptr)
        self.extent.pop(ptr, None)
        return ptr


class FrictionMap:
    """A friction map resident on an engine's device (mcq_fmap_create): Engine.friction_map makes it, close() or the context manager frees it, and
    the engine's close() frees whatever is still open.  info: cells, bins_x, bins_y, bin_side, device_bytes."""

    def __init__(self, eng, ptr, mue):
        self.eng, self.ptr = eng, ptr
        self.mue = mue          # the host's copy, in the cells' order
        c, bx, by, side, nbytes = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_double(), ctypes.c_longlong()
        eng._check(eng.lib.mcq_fmap_info(ptr, ctypes.byref(c), ctypes.byref(bx), ctypes.byref(by), ctypes.byref(side), ctypes.byref(nbytes)),
                   "mcq_fmap_info")
        self.info = dict(cells=c.value, bins_x=bx.value, bins_y=by.value, bin_side=side.value, device_bytes=nbytes.value)

    def close(self):
        if self.ptr and getattr(self.eng, "h", None):
            self.eng._check(self.eng.lib.mcq_fmap_destroy(self.eng.h, self.ptr), "mcq_fmap_destroy")
        if self in getattr(self.eng, "_fmaps", []):
            self.eng._fmaps.remove(self)
        self.ptr = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _live(self):
        if not self.ptr:
            raise EngineError("the friction map has been closed")
        return self.ptr


class Engine:
    """One handle == one GPU + one HIP stream + its device workspace.  One host thread at a time."""

    def __init__(self, device_id=0, lib_path=None):
        self.lib = load_library(lib_path)
        h = ctypes.c_void_p()
        rc = self.lib.mcq_create(int(device_id), ctypes.byref(h))
        if rc != 0:
            raise EngineError("mcq_create(%d) failed: %s" % (device_id, self.lib.mcq_last_error().decode()))
        self.h = h
        self.device_id = int(device_id)
        self.lib_path = lib_path

    def last_upload_was_direct(self):
        """True if the last solve_batch / iqp_batch went to the device without the packing pass (uniform batch, rows back to back in host_array memory)."""
        return bool(self.lib.mcq_last_upload_was_direct(self.h))

    def close(self):
        if getattr(self, "h", None):
            for fm in list(getattr(self, "_fmaps", [])):
                fm.close()
            for p in getattr(self, "_pinned", []):
                self.lib.mcq_host_free(self.h, p)
            self._pinned = []
            self.lib.mcq_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _opts(self, algorithm=ALG_DEFAULT, max_ipm_iter=0, max_as_iter=0, refine_steps=-1, check_kappa=1, objective=OBJ_MIN_CURV,
              warm_start=0):
        """mcq_opts.  algorithm=ALG_GI: every problem through the engine's Goldfarb-Idnani path (quadprog's algorithm; a reference mode).
        $MCQ_ALGORITHM=gi selects it for callers that cannot pass options -- the drop-in package under the untouched main_globaltraj.py."""
        if int(algorithm) == ALG_DEFAULT and os.environ.get("MCQ_ALGORITHM", "").lower() in ("gi", "goldfarb-idnani", "quadprog"):
            algorithm = ALG_GI
        return McqOpts(int(algorithm), int(max_ipm_iter), int(max_as_iter), int(refine_steps), int(check_kappa),
                       int(objective), int(warm_start))

    def _check(self, rc, what):
        if rc != 0:
            raise EngineError("%s failed (%d): %s" % (what, rc, self.lib.mcq_last_error().decode()))

    # ------------------------------------------------------------------------------------------------------------------
    def solve_batch(self, problems, ends=None, **opt_kw):
        """problems: list of dicts {reftrack [n,4], normvec [n,2], scaling [n] or None, kappa_bound, w_veh}.

        ends: None (every problem a ring: mcq_solve_batch), or one entry per problem -- None (a ring) or a dict {closed (default False),
        psi_s, psi_e, fix_s, fix_e} -- through mcq_solve_batch_ends.  A chain's scaling holds its n - 2 inner joints' s_i in entries
        0..n-3 (the rest is not read; les_scalings(A, closed=False) gives the [n] vector).
        Returns (alphas: list of [n] arrays, curv_err [B], status [B] int32, info: list of dicts).
        """
        bsz = len(problems)
        keep = []
        total = 0
        for k, p in enumerate(problems):
            ref = np.ascontiguousarray(p["reftrack"], dtype=np.float64)
            nv = None if p.get("normvec") is None else np.ascontiguousarray(p["normvec"], dtype=np.float64)
            n = ref.shape[0]
            if ref.ndim != 2 or ref.shape[1] != 4 or (nv is not None and nv.shape != (n, 2)):
                raise ValueError("reftrack must be [n,4] and normvec [n,2]")
            sc = p.get("scaling")
            if sc is not None:
                sc = np.ascontiguousarray(sc, dtype=np.float64)
                if sc.shape != (n,):
                    raise ValueError("scaling must be [n]")
            keep.append((ref, nv, sc))
            total += n
        rec, arr = problem_records([q[0] for q in keep], [q[1] for q in keep], [q[2] for q in keep],
                                   [float(p["kappa_bound"]) for p in problems], [float(p["w_veh"]) for p in problems])
        alpha = np.zeros(total)
        curv = np.zeros(bsz)
        status = np.zeros(bsz, dtype=np.int32)
        info = (McqInfo * bsz)()
        opts = self._opts(**opt_kw)
        if ends is None:
            rc = self.lib.mcq_solve_batch(self.h, arr, bsz, ctypes.byref(opts), _as_dp(alpha), _as_dp(curv),
                                          status.ctypes.data_as(_ip), info)
            self._check(rc, "mcq_solve_batch")
        else:
            if len(ends) != bsz:
                raise ValueError("ends must have one entry per problem")
            er = (McqEnds * bsz)()
            for k, e in enumerate(ends):
                if e is None or e.get("closed", False):
                    er[k].closed = 1
                    continue
                er[k].closed = 0
                er[k].fix_s = 1 if e.get("fix_s", False) else 0
                er[k].fix_e = 1 if e.get("fix_e", False) else 0
                er[k].psi_s = float(e["psi_s"])
                er[k].psi_e = float(e["psi_e"])
            rc = self.lib.mcq_solve_batch_ends(self.h, arr, er, bsz, ctypes.byref(opts), _as_dp(alpha), _as_dp(curv),
                                               status.ctypes.data_as(_ip), info)
            self._check(rc, "mcq_solve_batch_ends")
        out, off = [], 0
        for ref, _, _ in keep:
            out.append(alpha[off:off + ref.shape[0]].copy())
            off += ref.shape[0]
        return out, curv, status, _info_dicts(info)

    # ------------------------------------------------------------------------------------------------------------------
    def solve_device(self, batch, n, d_reftrack, d_normvec, d_scaling, kappa_bound, w_veh, d_alpha, d_curv, d_status,
                     d_info=None, **opt_kw):
        """Device-resident batch (raw device pointers as ints, e.g. torch.Tensor.data_ptr()).  Asynchronous."""
        opts = self._opts(**opt_kw)
        rc = self.lib.mcq_solve_device(self.h, int(batch), int(n), d_reftrack, d_normvec, d_scaling or None,
                                       float(kappa_bound), float(w_veh), ctypes.byref(opts), d_alpha, d_curv, d_status,
                                       d_info or None)
        self._check(rc, "mcq_solve_device")

    def solve_device_f32(self, batch, n, d_reftrack, d_normvec, d_scaling, kappa_bound, w_veh, d_alpha, d_curv, d_status,
                         d_info=None, **opt_kw):
        """As solve_device with float32 tracks and float32 alpha in HBM (mcq_solve_device_f32: fp32 at the boundary, fp64
        arithmetic inside; d_curv stays float64).  d_normvec / d_scaling may be None."""
        opts = self._opts(**opt_kw)
        rc = self.lib.mcq_solve_device_f32(self.h, int(batch), int(n), d_reftrack, d_normvec or None, d_scaling or None,
                                           float(kappa_bound), float(w_veh), ctypes.byref(opts), d_alpha, d_curv, d_status,
                                           d_info or None)
        self._check(rc, "mcq_solve_device_f32")

    def solve_host(self, reftrack, normvec, scaling, kappa_bound, w_veh, alpha_out=None, **opt_kw):
        """Uniform batch from / to host arrays in one call (mcq_solve_host): reftrack [B, n, 4], normvec [B, n, 2] or None,
        scaling [B, n] or None -- float64, C-contiguous, ideally views of pinned memory (host_array).  Returns (alpha [B, n],
        curv_err [B], status [B], info as a structured array of McqInfo)."""
        ref = np.ascontiguousarray(reftrack, dtype=np.float64)
        bsz, n = ref.shape[0], ref.shape[1]
        nv = None if normvec is None else np.ascontiguousarray(normvec, dtype=np.float64)
        sc = None if scaling is None else np.ascontiguousarray(scaling, dtype=np.float64)
        if alpha_out is None:
            alpha = np.empty((bsz, n))
        else:
            alpha = alpha_out
            if not isinstance(alpha, np.ndarray) or alpha.dtype != np.float64 or alpha.shape != (bsz, n) or not alpha.flags["C_CONTIGUOUS"] \
                    or not alpha.flags["WRITEABLE"]:
                raise ValueError("alpha_out must be a writeable C-contiguous float64 array of shape %r" % ((bsz, n),))
        curv = np.empty(bsz)
        status = np.empty(bsz, dtype=np.int32)
        info = (McqInfo * bsz)()
        opts = self._opts(**opt_kw)
        rc = self.lib.mcq_solve_host(self.h, bsz, n, ref.ctypes.data, nv.ctypes.data if nv is not None else None,
                                     sc.ctypes.data if sc is not None else None, float(kappa_bound), float(w_veh),
                                     ctypes.byref(opts), alpha.ctypes.data, curv.ctypes.data, status.ctypes.data,
                                     ctypes.addressof(info))
        self._check(rc, "mcq_solve_host")
        return alpha, curv, status, info

    def solve_device_stream(self, batch, n, d_reftracks, d_normvecs, d_scalings, kappa_bound, w_veh, d_alphas, d_curvs, d_statuses, **opt_kw):
        """A stream of resident uniform batches on the engine's two compute streams (mcq_solve_device_stream): lists of raw device pointers, one
        entry per step (d_normvecs / d_scalings: None, or lists whose entries may be None).  Asynchronous: sync() waits for every step."""
        steps = len(d_reftracks)

        def arr(seq):
            if seq is None:
                return None
            a = (ctypes.c_void_p * steps)()
            for k, p in enumerate(seq):
                a[k] = p
            return a
        opts = self._opts(**opt_kw)
        rc = self.lib.mcq_solve_device_stream(self.h, steps, int(batch), int(n), arr(d_reftracks), arr(d_normvecs), arr(d_scalings),
                                              float(kappa_bound), float(w_veh), ctypes.byref(opts), arr(d_alphas), arr(d_curvs), arr(d_statuses))
        self._check(rc, "mcq_solve_device_stream")

    def host_array(self, shape, dtype=np.float64):
        """numpy array backed by pinned (page-locked) host memory of the engine (mcq_host_alloc).  LIFETIME: the memory belongs to
        the engine -- it is released by host_free(array) or by close() / garbage collection of the engine, after which the array
        (and every view of it) must not be touched.  Keep the engine alive as long as the arrays are in use."""
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = ctypes.c_void_p()
        self._check(self.lib.mcq_host_alloc(self.h, max(nbytes, 1), ctypes.byref(p)), "mcq_host_alloc")
        self._pinned = getattr(self, "_pinned", [])
        self._pinned.append(p.value)
        buf = (ctypes.c_char * max(nbytes, 1)).from_address(p.value)
        return np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)

    def host_free(self, arr):
        """Release a host_array before the engine goes away (the array must not be used afterwards)."""
        addr = int(arr.ctypes.data)
        pinned = getattr(self, "_pinned", [])
        if addr not in pinned:
            raise ValueError("host_free: not the start of an array from host_array of this engine")
        pinned.remove(addr)
        self._check(self.lib.mcq_host_free(self.h, addr), "mcq_host_free")

    def solve_host_pipelined(self, reftracks, normvecs, scalings, kappa_bound, w_veh, alpha_outs, **opt_kw):
        """A stream of uniform host batches with the PCIe hidden behind the kernels (mcq_solve_host_pipelined): reftracks / normvecs /
        scalings / alpha_outs are lists (one entry per step) of C-contiguous float64 arrays [B, n, 4] / [B, n, 2] or None / [B, n] or
        None / [B, n] -- ideally host_array (pinned) memory; entries may repeat.  Returns (curv_err [steps, B], status [steps, B])."""
        steps = len(reftracks)
        bsz, n = reftracks[0].shape[0], reftracks[0].shape[1]

        keep = []

        def ptrs(seq, shape, allow_none, output=False):
            arr = (ctypes.c_void_p * steps)()
            for k, a in enumerate(seq):
                if a is None:
                    if not allow_none:
                        raise ValueError("missing buffer for step %d" % k)
                    arr[k] = None
                    continue
                if output:
                    if not isinstance(a, np.ndarray) or a.dtype != np.float64 or a.shape != shape or not a.flags["C_CONTIGUOUS"] \
                            or not a.flags["WRITEABLE"]:
                        raise ValueError("step %d: expected a writeable C-contiguous float64 array of shape %r" % (k, shape))
                else:
                    a = np.ascontiguousarray(a, dtype=np.float64)       # a no-op for the pinned arrays this entry is meant for
                    if a.shape != shape:
                        raise ValueError("step %d: expected shape %r" % (k, shape))
                    keep.append(a)
                arr[k] = a.ctypes.data
            return arr
        p_ref = ptrs(reftracks, (bsz, n, 4), False)
        p_nv = ptrs(normvecs, (bsz, n, 2), True) if normvecs is not None else None
        p_sc = ptrs(scalings, (bsz, n), True) if scalings is not None else None
        p_al = ptrs(alpha_outs, (bsz, n), False, output=True)
        curv = np.zeros((steps, bsz))
        status = np.zeros((steps, bsz), dtype=np.int32)
        p_cu = (ctypes.c_void_p * steps)(*[curv[k].ctypes.data for k in range(steps)])
        p_st = (ctypes.c_void_p * steps)(*[status[k].ctypes.data for k in range(steps)])
        opts = self._opts(**opt_kw)
        rc = self.lib.mcq_solve_host_pipelined(self.h, steps, bsz, n, p_ref, p_nv, p_sc, float(kappa_bound), float(w_veh),
                                               ctypes.byref(opts), p_al, p_cu, p_st)
        self._check(rc, "mcq_solve_host_pipelined")
        return curv, status

    def solve_device_f32_rows(self, batch, n, layout, d_rows, d_origin, kappa_bound, w_veh, d_alpha, d_curv, d_status, d_info=None,
                              **opt_kw):
        """Device-resident float rows in either layout (F32_ABSOLUTE / F32_INCREMENTS; mcq_solve_device_f32_rows): d_rows
        [batch, n, 4] float32, d_origin [batch, 2] float64 or None, d_alpha [batch, n] float32.  Asynchronous."""
        opts = self._opts(**opt_kw)
        rc = self.lib.mcq_solve_device_f32_rows(self.h, int(batch), int(n), int(layout), d_rows, d_origin or None, float(kappa_bound),
                                                float(w_veh), ctypes.byref(opts), d_alpha, d_curv, d_status, d_info or None)
        self._check(rc, "mcq_solve_device_f32_rows")

    def f32_rows_device(self, batch, n, layout, d_rows, d_origin, d_reftrack_out):
        """The fp64 rows [batch, n, 4] solve_device_f32_rows solves, without the solve (mcq_f32_rows_device: the same launch): d_rows
        [batch, n, 4] float32 in `layout`, d_origin [batch, 2] float64 or None.  Input and output must not overlap.  Asynchronous."""
        rc = self.lib.mcq_f32_rows_device(self.h, int(batch), int(n), int(layout), d_rows, d_origin or None, d_reftrack_out)
        self._check(rc, "mcq_f32_rows_device")

    def f32_widen_device(self, count, d_src, d_dst):
        """d_dst[i] = float64(d_src[i]) for count float32 values on the device (mcq_f32_widen_device; exact).  Asynchronous."""
        self._check(self.lib.mcq_f32_widen_device(self.h, int(count), d_src, d_dst), "mcq_f32_widen_device")

    def f32_narrow_device(self, count, d_src, d_dst):
        """d_dst[i] = float32(d_src[i]) for count float64 values on the device, rounded to nearest even as alpha is on the way out of the
        fp32 entries (mcq_f32_narrow_device).  Asynchronous."""
        self._check(self.lib.mcq_f32_narrow_device(self.h, int(count), d_src, d_dst), "mcq_f32_narrow_device")

    def solve_batch_f32(self, rows32, origin, kappa_bound, w_veh, layout=F32_INCREMENTS, **opt_kw):
        """Host-buffer fp32 entry (mcq_solve_batch_f32): rows32 [B, n, 4] float32 in `layout`, origin [B, 2] float64 or None.
        Returns (alpha float32 [B, n], curv_err [B], status [B], info as a ctypes array of McqInfo)."""
        rows = np.ascontiguousarray(rows32, dtype=np.float32)
        bsz, n = rows.shape[0], rows.shape[1]
        org = None if origin is None else np.ascontiguousarray(origin, dtype=np.float64)
        if rows.ndim != 3 or rows.shape[2] != 4 or (org is not None and org.shape != (bsz, 2)):
            raise ValueError("rows32 must be [B, n, 4] and origin [B, 2]")
        alpha = np.zeros((bsz, n), dtype=np.float32)
        curv = np.zeros(bsz)
        status = np.zeros(bsz, dtype=np.int32)
        info = (McqInfo * bsz)()
        opts = self._opts(**opt_kw)
        rc = self.lib.mcq_solve_batch_f32(self.h, bsz, n, int(layout), rows.ctypes.data, org.ctypes.data if org is not None else None,
                                          float(kappa_bound), float(w_veh), ctypes.byref(opts), alpha.ctypes.data, curv.ctypes.data,
                                          status.ctypes.data, ctypes.addressof(info))
        self._check(rc, "mcq_solve_batch_f32")
        return alpha, curv, status, info

    def iqp_batch(self, tracks, kappa_bound, w_veh, stepsize_interp, iters_min=3, curv_error_allowed=0.01, max_rounds=50,
                  nmax=None, timed=False, out=None, **opt_kw):
        """tph.iqp_handler for a batch of tracks as ONE engine call (mcq_iqp_batch): tracks = list of dicts {reftrack [N,4],
        normvectors [N,2], scaling [N] or None}.  Returns a dict: alpha / reftrack / normvectors (lists of the final arrays),
        n, curv_err, status, rounds (arrays [B]), curv_trace [B, IQP_TRACE], stats (rounds, qp_solves, and with timed=True
        solver_ms / fallbacks per round).
        out (optional): dict with preallocated 'alpha' [B, nmax], 'reftrack' [B, nmax, 4], 'normvectors' [B, nmax, 2] float64 arrays
        (e.g. from host_array: page-locked) that receive the end states -- a caller that runs batch after batch keeps them; the
        returned per-track arrays are views into them.  Without it fresh arrays are allocated AND touched here: a device-to-host
        copy into never-touched pageable memory runs at a tenth of the PCIe rate (page faults inside the copy)."""
        stacked = isinstance(tracks, dict)
        if stacked:
            # a uniform batch as ONE dict of stacked arrays {reftrack [B,N,4], normvectors [B,N,2], scaling [B,N] or None}: no per-track
            # Python work at all (building 1024 records track by track costs 4-12 ms of a 40 ms call)
            refs = np.ascontiguousarray(tracks["reftrack"], dtype=np.float64)
            nvs = np.ascontiguousarray(tracks["normvectors"], dtype=np.float64)
            scs = None if tracks.get("scaling") is None else np.ascontiguousarray(tracks["scaling"], dtype=np.float64)
            if refs.ndim != 3 or refs.shape[2] != 4 or nvs.shape != refs.shape[:2] + (2,) or (scs is not None and scs.shape != refs.shape[:2]):
                raise ValueError("stacked tracks: reftrack must be [B,n,4], normvectors [B,n,2], scaling [B,n]")
            bsz = refs.shape[0]
        else:
            bsz = len(tracks)
            refs = [np.ascontiguousarray(t["reftrack"], dtype=np.float64) for t in tracks]
            nvs = [np.ascontiguousarray(t["normvectors"], dtype=np.float64) for t in tracks]
            scs = [None if t.get("scaling") is None else np.ascontiguousarray(t["scaling"], dtype=np.float64) for t in tracks]
        if nmax is None:
            # capacity for the re-sampled rings: the raceline is never much longer than the polygon through the reference
            # points; 30 % + 16 points of headroom (a ring that outgrows it is reported per track, not truncated)
            if stacked or len({r.shape for r in refs}) == 1:           # uniform batch: one vectorised pass over all tracks
                xy = refs[:, :, :2] if stacked else np.stack([r[:, :2] for r in refs])
                seg = xy - np.roll(xy, -1, axis=1)
                lengths = np.sqrt(np.einsum("bnk,bnk->bn", seg, seg)).sum(axis=1)
            else:
                lengths = np.array([_closed_length(r[:, :2]) for r in refs])
            finite = lengths[np.isfinite(lengths)]          # (a track with non-finite rows is reported by the engine: status 4)
            longest = float(finite.max()) if finite.size else 0.0
            nmax = max(refs.shape[1] if stacked else max(r.shape[0] for r in refs), int(np.ceil(1.3 * longest / stepsize_interp)) + 16)
        for k in range(0 if stacked else bsz):
            n = refs[k].shape[0]
            if refs[k].ndim != 2 or refs[k].shape[1] != 4 or nvs[k].shape != (n, 2) or (scs[k] is not None and scs[k].shape != (n,)):
                raise ValueError("reftrack must be [n,4], normvectors [n,2], scaling [n]")
        rec, arr = problem_records(refs, nvs, scs, float(kappa_bound), float(w_veh))
        def _out(key, shape):
            if out is not None and key in out:
                a = out[key]
                if a.dtype != np.float64 or not a.flags["C_CONTIGUOUS"] or a.shape != shape:
                    raise ValueError("out[%r] must be a C-contiguous float64 array of shape %r" % (key, shape))
                return a
            a = np.empty(shape)
            a.fill(0.0)              # touch the pages before the driver copies into them
            return a
        alpha = _out("alpha", (bsz, nmax))
        ref_o = _out("reftrack", (bsz, nmax, 4))
        nv_o = _out("normvectors", (bsz, nmax, 2))
        n_o = np.zeros(bsz, dtype=np.int32)
        curv = np.zeros(bsz)
        status = np.zeros(bsz, dtype=np.int32)
        rounds = np.zeros(bsz, dtype=np.int32)
        trace = np.zeros((bsz, IQP_TRACE))
        st = McqIqpStats()
        st.timed = 1 if timed else 0
        opts = self._opts(**opt_kw)
        rc = self.lib.mcq_iqp_batch(self.h, arr, bsz, float(stepsize_interp), int(iters_min), float(curv_error_allowed),
                                    int(max_rounds), ctypes.byref(opts), int(nmax), _as_dp(alpha), _as_dp(ref_o), _as_dp(nv_o),
                                    n_o.ctypes.data_as(_ip), _as_dp(curv), status.ctypes.data_as(_ip),
                                    rounds.ctypes.data_as(_ip), _as_dp(trace), ctypes.byref(st))
        self._check(rc, "mcq_iqp_batch")
        return dict(alpha=[alpha[k, :n_o[k]] for k in range(bsz)], reftrack=[ref_o[k, :n_o[k]] for k in range(bsz)],
                    normvectors=[nv_o[k, :n_o[k]] for k in range(bsz)], n=n_o, curv_err=curv, status=status, rounds=rounds,
                    curv_trace=trace, stats=self._iqp_stats(st, nmax, timed))

    @staticmethod
    def _iqp_stats(st, nmax, timed):
        stats = dict(rounds=int(st.rounds), qp_solves=int(st.qp_solves), nmax=int(nmax))
        if timed:
            stats["solver_ms"] = [float(st.solver_ms[k]) for k in range(min(st.rounds, 16))]
            stats["fallbacks"] = [int(st.fallbacks[k]) for k in range(min(st.rounds, 16))]
        return stats

    def iqp_device(self, batch, nmax, d_n, d_ref_a, d_nv_a, d_ref_b, d_nv_b, d_scaling, kappa_bound, w_veh, stepsize_interp, iters_min,
                   curv_error_allowed, max_rounds, d_alpha, d_buf, d_curv, d_status, d_rounds, d_trace=None, timed=False, **opt_kw):
        """tph.iqp_handler for a RESIDENT batch (mcq_iqp_device in include/mcq.h): the tracks in set a, [batch][nmax][*], d_n [batch] their
        waypoint counts on entry and those of the end states on return; d_buf says which set holds a track's end state.  Blocking.  Returns
        the stats of iqp_batch."""
        st = McqIqpStats()
        st.timed = 1 if timed else 0
        opts = self._opts(**opt_kw)
        rc = self.lib.mcq_iqp_device(self.h, int(batch), int(nmax), d_n, d_ref_a, d_nv_a, d_ref_b, d_nv_b, d_scaling or None, float(kappa_bound),
                                     float(w_veh), float(stepsize_interp), int(iters_min), float(curv_error_allowed), int(max_rounds),
                                     ctypes.byref(opts), d_alpha, d_buf, d_curv, d_status, d_rounds, d_trace or None, ctypes.byref(st))
        self._check(rc, "mcq_iqp_device")
        return self._iqp_stats(st, nmax, timed)

    def solve_uniform_f32(self, reftrack, normvec, scaling, kappa_bound, w_veh, **opt_kw):
        """Host convenience around solve_device_f32 for a uniform-n batch: reftrack [B,n,4] (cast to float32), normvec
        [B,n,2] or None (derived on the device), scaling [B,n] or None.  Returns (alpha float32 [B,n], curv_err [B],
        status [B], info [B])."""
        ref = np.ascontiguousarray(reftrack, dtype=np.float32)
        bsz, n = ref.shape[0], ref.shape[1]
        nv = None if normvec is None else np.ascontiguousarray(normvec, dtype=np.float32)
        sc = None if scaling is None else np.ascontiguousarray(scaling, dtype=np.float32)
        with self.scope() as dev:
            d_ref, d_nv, d_sc = dev.up(ref), dev.up(nv), dev.up(sc)
            d_alpha, d_curv, d_status = dev.out((bsz, n), np.float32), dev.out(bsz), dev.out(bsz, np.int32)
            d_info = dev.out((bsz, ctypes.sizeof(McqInfo)), np.uint8)
            self.solve_device_f32(bsz, n, d_ref, d_nv, d_sc, kappa_bound, w_veh, d_alpha, d_curv, d_status, d_info, **opt_kw)
            self.sync()
            alpha, curv, status, raw = dev.get(d_alpha), dev.get(d_curv), dev.get(d_status), dev.get(d_info)
        return alpha, curv, status, _info_dicts((McqInfo * bsz).from_buffer_copy(raw.tobytes()), INFO_FIELDS[:6])

    def solve_device_ragged(self, batch, nmax, d_n, d_reftrack, d_normvec, d_scaling, kappa_bound, w_veh, d_alpha,
                            d_curv, d_status, d_info=None, **opt_kw):
        """Device-resident batch with per-problem waypoint counts d_n [batch] (int32, device); arrays strided by nmax."""
        opts = self._opts(**opt_kw)
        rc = self.lib.mcq_solve_device_ragged(self.h, int(batch), int(nmax), d_n, d_reftrack, d_normvec,
                                              d_scaling or None, float(kappa_bound), float(w_veh), ctypes.byref(opts),
                                              d_alpha, d_curv, d_status, d_info or None)
        self._check(rc, "mcq_solve_device_ragged")

    def solve_device_ragged_params(self, batch, nmax, d_n, d_reftrack, d_normvec, d_scaling, kappa_bound, w_veh, d_kappa_list,
                                   d_w_veh_list, d_alpha, d_curv, d_status, d_info=None, **opt_kw):
        """solve_device_ragged with per-problem kappa_bound / w_veh (device arrays [batch] or None)."""
        opts = self._opts(**opt_kw)
        rc = self.lib.mcq_solve_device_ragged_params(self.h, int(batch), int(nmax), d_n, d_reftrack, d_normvec or None,
                                                     d_scaling or None, float(kappa_bound), float(w_veh), d_kappa_list or None,
                                                     d_w_veh_list or None, ctypes.byref(opts), d_alpha, d_curv, d_status,
                                                     d_info or None)
        self._check(rc, "mcq_solve_device_ragged_params")

    def prep_batch(self, reftracks):
        """Unit normals and spline scalings of the closed distance-scaled splines through a list of reference lines
        ([n,>=2] arrays), computed on the device (mcq_prep_device).  Returns (list of [n,2], list of [n])."""
        ns, ref = _pad_rows(reftracks, 4, strict=False)
        bsz, nmax = ref.shape[:2]
        with self.scope() as dev:
            d_ref, d_n = dev.up(ref), dev.up(ns)
            d_nv, d_sc, d_st = dev.out((bsz, nmax, 2)), dev.out((bsz, nmax)), dev.out(bsz, np.int32)
            self._check(self.lib.mcq_prep_device(self.h, bsz, nmax, d_n, d_ref, d_nv, d_sc, d_st), "mcq_prep_device")
            st, nv, sc = dev.get(d_st), dev.get(d_nv), dev.get(d_sc)
        if np.any(st != 0):
            raise EngineError("mcq_prep_device: bad input in problem(s) %s" % np.nonzero(st)[0].tolist())
        return [nv[k, :ns[k]].copy() for k in range(bsz)], [sc[k, :ns[k]].copy() for k in range(bsz)]

    def vel_profile_batch(self, kappa, el_lengths, ggv, ax_max_machines, drag_coeff, m_veh, v_max, dyn_model_exp=1.0,
                          track_of=None, n_of_track=None, mu=None, filt_window=None, closed=True, loc_gg=None, v_start=None, v_end=None,
                          timed=False):
        """Velocity profiles and lap times of a batch of variants on the device: tph.calc_vel_profile in all the forms of its signature
        (mcq_vel_profile_device; with mu -- friction coefficient per waypoint, [tracks, n] -- or filt_window -- tph.conv_filt's odd
        moving-average width over the finished profile -- mcq_vel_profile_device_opts; unclosed rows or local limits:
        mcq_vel_profile_device_forms).

        kappa, el_lengths: [tracks, n]; ggv: [batch, g, 3]; ax_max_machines: [batch, m, 2]; drag_coeff, m_veh, v_max: [batch];
        track_of: [batch] ints (row of kappa / el per variant) or None when tracks == batch; n_of_track: [tracks] valid entries
        per row (ragged tracks, mcq_vel_profile_device_ragged) or None (all rows full).
        closed=False: unclosed rows -- a row of n curvatures has n - 1 element lengths (el_lengths keeps the shape of kappa, entry n - 1 of a
        row is not read); v_start (scalar or [batch]) is required, v_end (scalar or [batch], NaN entries: none for that variant) optional;
        the returned time is that of the n - 1 elements (+inf for a profile that stands at both ends of an element).
        loc_gg: [tracks, n, 2] = (ax_max, ay_max) per waypoint in place of the diagram: ggv=None, no mu.
        Returns (vx [batch, n], lap_time [batch]); timed=True: a third entry, the milliseconds the launch took on the device (a span of
        mcq_timing_begin / mcq_timing_end around the entry alone: no copies; after a call of the same size, no allocation either)."""
        kappa = np.ascontiguousarray(kappa, dtype=np.float64)
        el = np.ascontiguousarray(el_lengths, dtype=np.float64)
        axm = np.ascontiguousarray(ax_max_machines, dtype=np.float64)
        # the argument errors of tph.calc_vel_profile, in its words
        if (ggv is not None or mu is not None) and loc_gg is not None:
            raise RuntimeError("Either ggv and optionally mu OR loc_gg must be supplied, not both (or all) of them!")
        if ggv is None and loc_gg is None:
            raise RuntimeError("Either ggv or loc_gg must be supplied!")
        if loc_gg is not None:
            if v_max is None:
                raise RuntimeError("v_max must be supplied if loc_gg is used!")
            loc_gg = np.ascontiguousarray(loc_gg, dtype=np.float64)
            if loc_gg.shape != kappa.shape + (2,):
                raise RuntimeError("loc_gg must have the shape [no_points, 2]!")
        if not closed and v_start is None:
            raise RuntimeError("v_start must be provided for the unclosed case!")
        if ggv is not None:
            ggv = np.ascontiguousarray(ggv, dtype=np.float64)
        bsz, n = (ggv if ggv is not None else axm).shape[0], kappa.shape[1]
        scal = _per_variant(bsz, drag_coeff, m_veh, v_max)
        # what tph.calc_vel_profile raises on (the kernel itself flags such a variant with lap_time = NaN)
        if ggv is not None and np.any(ggv[:, -1, 0] < scal[2]):
            raise RuntimeError("ggv has to cover the entire velocity range of the car (i.e. >= v_max)!")
        if np.any(axm[:, -1, 0] < scal[2]):
            raise RuntimeError("ax_max_machines has to cover the entire velocity range of the car (i.e. >= v_max)!")
        if filt_window is not None and int(filt_window) % 2 == 0:
            raise RuntimeError("Window width of moving average filter must be odd!")
        if filt_window is not None and int(filt_window) > 1:
            # a window wider than the ring: the kernel flags the variant with lap_time = NaN (tph.conv_filt wraps the ring more than once
            # and returns something of another length) -- refused here instead of handed back as NaNs
            n_min = int(np.min(n_of_track)) if n_of_track is not None else n
            if int(filt_window) > n_min:
                raise ValueError("vel_profile_batch: filt_window %d is wider than the shortest profile (%d points)" % (int(filt_window), n_min))
        if mu is not None:
            mu = np.ascontiguousarray(mu, dtype=np.float64)
            if mu.shape != kappa.shape:
                raise RuntimeError("kappa and mu must have the same length!")
        tr = None if track_of is None else np.ascontiguousarray(track_of, dtype=np.int32)
        nt = None if n_of_track is None else np.ascontiguousarray(n_of_track, dtype=np.int32)
        with self.scope() as dev:
            up = dev.up
            d_k, d_e, d_a = up(kappa), up(el), up(axm)
            d_g, n_g = up(ggv), ggv.shape[1] if ggv is not None else 0
            d_s = [up(a) for a in scal]
            d_t, d_vx, d_lt = up(tr), dev.out((bsz, n)), dev.out(bsz)
            d_n, d_mu, d_lg = up(nt), up(mu), up(loc_gg)
            d_vs = d_ve = None
            if not closed:
                d_vs = up(_per_variant(bsz, v_start)[0])
                if v_end is not None:
                    d_ve = up(_per_variant(bsz, v_end)[0])
            if timed:
                self.timing_begin()
            if not closed or loc_gg is not None:
                vf = McqVelForms(float(dyn_model_exp), int(filt_window or 0), 1 if closed else 0, d_mu, d_lg, d_vs, d_ve)
                rc = self.lib.mcq_vel_profile_device_forms(self.h, bsz, n, n, d_n, d_t, d_k, d_e, d_g, n_g,
                                                           d_a, axm.shape[1], d_s[0], d_s[1], d_s[2], ctypes.byref(vf), d_vx, d_lt)
            elif mu is not None or filt_window is not None:
                vo = McqVelOpts(float(dyn_model_exp), int(filt_window or 0), 0, d_mu)
                rc = self.lib.mcq_vel_profile_device_opts(self.h, bsz, n, n, d_n, d_t, d_k, d_e, d_g,
                                                          ggv.shape[1], d_a, axm.shape[1], d_s[0], d_s[1], d_s[2], ctypes.byref(vo),
                                                          d_vx, d_lt)
            elif nt is not None:
                rc = self.lib.mcq_vel_profile_device_ragged(self.h, bsz, n, d_n, d_t, d_k, d_e, d_g, ggv.shape[1], d_a,
                                                            axm.shape[1], d_s[0], d_s[1], d_s[2], float(dyn_model_exp),
                                                            d_vx, d_lt)
            else:
                rc = self.lib.mcq_vel_profile_device(self.h, bsz, n, n, d_t, d_k, d_e, d_g, ggv.shape[1], d_a, axm.shape[1],
                                                     d_s[0], d_s[1], d_s[2], float(dyn_model_exp), d_vx, d_lt)
            self._check(rc, "mcq_vel_profile_device")
            ms = self.timing_end()[0] if timed else None
            res = (dev.get(d_vx), dev.get(d_lt))
            return res + (ms,) if timed else res

    def normals_crossing_batch(self, reftracks, normvecs, horizon=10):
        """tph.check_normals_crossing of a list of tracks on the device [REF helper_funcs_glob/src/prep_track.py:57-59].
        Returns an int32 array: 1 crossing, 0 none, -1 where tph would raise (horizon >= n)."""
        ns, ref = _pad_rows(reftracks, 4)
        nv = _pad_like(normvecs, ns, (2,))
        bsz, nmax = ref.shape[:2]
        with self.scope() as dev:
            d_ref, d_nv, d_n, d_out = dev.up(ref), dev.up(nv), dev.up(ns), dev.out(bsz, np.int32)
            rc = self.lib.mcq_normals_crossing_device(self.h, bsz, nmax, d_n, d_ref, d_nv, int(horizon), d_out)
            self._check(rc, "mcq_normals_crossing_device")
            return dev.get(d_out)

    def spline_approx_device(self, tracks, nmax, d_n, d_track, k, nkmax, d_nk, d_knots, d_coef, stepsize_reg, mmax, d_ref, d_m, d_ct, d_dist,
                             d_dev, d_nonmono, d_status):
        """mcq_spline_approx_device (include/mcq.h) on device pointers; d_n / d_nk / d_ct / d_dist / d_dev / d_nonmono may be None.  Asynchronous."""
        rc = self.lib.mcq_spline_approx_device(self.h, int(tracks), int(nmax), d_n or None, d_track or None, int(k), int(nkmax), d_nk or None,
                                               d_knots or None, d_coef or None, float(stepsize_reg), int(mmax), d_ref or None, d_m or None,
                                               d_ct or None, d_dist or None, d_dev or None, d_nonmono or None, d_status or None)
        self._check(rc, "mcq_spline_approx_device")

    def min_width_device(self, batch, nmax, d_n, d_ref, min_width, d_changed):
        """mcq_min_width_device (include/mcq.h) on device pointers, in place.  Asynchronous."""
        self._check(self.lib.mcq_min_width_device(self.h, int(batch), int(nmax), d_n or None, d_ref or None, float(min_width), d_changed or None),
                    "mcq_min_width_device")

    @staticmethod
    def pack_tcks(tcks):
        """[(t, c, k)] of scipy.interpolate.splprep -> (k, nk [B] int32, knots [B, nkmax], coef [B, 2, nkmax]); one degree per launch."""
        ks = {int(tck[2]) for tck in tcks}
        if len(ks) != 1:
            raise ValueError("spline_approx_batch: the splines of one launch must share their degree")
        nk = np.array([np.asarray(tck[0]).shape[0] for tck in tcks], dtype=np.int32)
        nkmax = int(nk.max())
        knots = np.zeros((len(tcks), nkmax))
        coef = np.zeros((len(tcks), 2, nkmax))
        for b, (t, c, _) in enumerate(tcks):
            knots[b, :nk[b]] = np.asarray(t, dtype=np.float64)
            for q in range(2):
                cq = np.asarray(c[q], dtype=np.float64)[:nkmax]
                coef[b, q, :cq.shape[0]] = cq
        return ks.pop(), nk, knots, coef

    def spline_approx_batch(self, tracks, tcks, stepsize_reg, mmax=None, keep=None, resident=None):
        """tph.spline_approximation behind FITPACK's fit for a list of raw tracks ([n_k, 4] rows [x, y, w_r, w_l], not closed) and their
        smoothing splines (tcks: the (t, c, k) tuples scipy.interpolate.splprep returns; one degree per launch), on the device
        (mcq_spline_approx_device).  mmax: rows the output holds per track (default: enough for every track of the launch).
        Returns a dict: reftrack -- list of (m_k, 4) arrays (None where status != 0) --, m [B], closest_t / dists [B, nmax + 1] (NaN behind n_k),
        dev [B, 2] = mean and maximum deviation, nonmono [B], status [B].
        keep: a list that receives (d_ref, d_n, mmax) -- the rows stay on the device, padded to mmax, and the caller frees both (prep_track_batch).
        resident: (k, nkmax, d_nk, d_knots, d_coef) as Engine.spline_fit_batch(keep=...) leaves them on the device, instead of tcks (then None)."""
        ns, trk = _pad_rows(tracks, 4, nmin=3)
        bsz, nmax = trk.shape[:2]
        if resident is None:
            k, nk, knots, coef = self.pack_tcks(tcks)
            nkmax = knots.shape[1]
        else:
            k, nkmax = int(resident[0]), int(resident[1])
        if mmax is None:      # a smoothed line is shorter than its raw one: room for one twice as long (a track that needs more reports its m)
            finite = [e for e in (_closed_length(trk[b, :ns[b], :2]) for b in range(bsz)) if np.isfinite(e)]
            mmax = max(int(2.0 * max(finite + [0.0]) / float(stepsize_reg)) + 8, 8)
        with self.scope() as dev:
            up, out, get = dev.up, dev.out, dev.get
            d_trk, d_n = up(trk), up(ns)
            d_nk, d_kn, d_cf = (up(nk), up(knots), up(coef)) if resident is None else resident[2:5]
            d_m, d_ct, d_ds, d_dev, d_nm, d_st = out(bsz, np.int32), out((bsz, nmax + 1)), out((bsz, nmax + 1)), out((bsz, 2)), out(bsz, np.int32), out(bsz, np.int32)
            d_ref = out((bsz, mmax, 4))
            self.spline_approx_device(bsz, nmax, d_n, d_trk, k, nkmax, d_nk, d_kn, d_cf, stepsize_reg, mmax, d_ref, d_m, d_ct, d_ds,
                                      d_dev, d_nm, d_st)
            m, st, ref = get(d_m), get(d_st), get(d_ref)
            res = dict(reftrack=[ref[b, :m[b]].copy() if st[b] == 0 else None for b in range(bsz)], m=m, status=st,
                       closest_t=get(d_ct), dists=get(d_ds), dev=get(d_dev), nonmono=get(d_nm))
            if keep is not None:
                keep.extend((dev.release(d_ref), dev.release(d_m), mmax))
            return res

    def spline_fit_device(self, tracks, nmax, d_n, d_track, stepsize_prep, mimax, k, s, nkmax, d_nk, d_knots, d_coef, d_fp, d_ier, d_mi, d_pts,
                          d_status):
        """mcq_spline_fit_device (include/mcq.h) on device pointers; d_n / d_fp / d_mi / d_pts may be None.  Asynchronous."""
        rc = self.lib.mcq_spline_fit_device(self.h, int(tracks), int(nmax), d_n or None, d_track or None, float(stepsize_prep), int(mimax), int(k),
                                            float(s), int(nkmax), d_nk or None, d_knots or None, d_coef or None, d_fp or None, d_ier or None,
                                            d_mi or None, d_pts or None, d_status or None)
        self._check(rc, "mcq_spline_fit_device")

    def spline_fit_batch(self, tracks, k=3, s=10, stepsize_prep=1.0, nest=None, keep=None, mimax=None, points=False):
        """FITPACK's periodic smoothing fit -- scipy.interpolate.splprep(..., k=k, s=s, per=1) behind interp_track's re-sampling at stepsize_prep,
        as tph.spline_approximation runs them -- for a list of raw tracks ([n_k, >= 2] rows, not closed) on the device (mcq_spline_fit_device).
        stepsize_prep <= 0: the raw rows are closed and fitted as they are.  nest: FITPACK's knot budget (default: scipy's, mi + 2 k of the
        longest track).  Returns a dict: tcks -- scipy-shaped (t, [cx, cy], k), None where status != 0 --, nk, fp, ier, mi, status [B] (and pts,
        the closed points that were fitted, with points=True).
        keep: a list that receives (k, nkmax, d_nk, d_knots, d_coef) -- the splines stay on the device in mcq_spline_approx_device's layout and
        the caller frees the three pointers (prep_track_batch)."""
        ns, trk = _pad_rows([np.asarray(t, dtype=np.float64)[:, :2] for t in tracks], 2, nmin=3)
        trk = np.concatenate((trk, np.zeros_like(trk)), axis=2)
        bsz, nmax = trk.shape[:2]
        if mimax is None:
            if stepsize_prep > 0.0:
                finite = [e for e in (_closed_length(trk[b, :ns[b], :2]) for b in range(bsz)) if np.isfinite(e)]
                mimax = max(int(np.ceil(max(finite + [0.0]) / float(stepsize_prep))) + 3, 4)
            else:
                mimax = nmax + 1
        nkmax = int(nest) if nest is not None else mimax + 2 * int(k)
        with self.scope() as dev:
            up, out, get = dev.up, dev.out, dev.get
            d_trk, d_n = up(trk), up(ns)
            d_nk, d_kn, d_cf = out(bsz, np.int32), out((bsz, nkmax)), out((bsz, 2, nkmax))
            d_fp, d_ier, d_mi, d_st = out(bsz), out(bsz, np.int32), out(bsz, np.int32), out(bsz, np.int32)
            d_pts = out((bsz, mimax, 2)) if points else None
            self.spline_fit_device(bsz, nmax, d_n, d_trk, stepsize_prep, mimax, k, s, nkmax, d_nk, d_kn, d_cf, d_fp, d_ier, d_mi, d_pts, d_st)
            nk, st, kn, cf = get(d_nk), get(d_st), get(d_kn), get(d_cf)
            res = dict(tcks=[(kn[b, :nk[b]].copy(), [cf[b, 0, :nk[b] - k - 1].copy(), cf[b, 1, :nk[b] - k - 1].copy()], int(k)) if st[b] == 0 else None
                             for b in range(bsz)],
                       nk=nk, fp=get(d_fp), ier=get(d_ier), mi=get(d_mi), status=st, knots=kn, coef=cf)
            if points:
                pts = get(d_pts)
                res["pts"] = [pts[b, :res["mi"][b]].copy() if st[b] == 0 else None for b in range(bsz)]
            if keep is not None:
                keep.extend((int(k), nkmax, dev.release(d_nk), dev.release(d_kn), dev.release(d_cf)))
            return res

    def min_width_batch(self, reftracks, min_width):
        """prep_track's tail for a list of prepared tracks (mcq_min_width_device): rows narrower than min_width grow by half the deficit on both
        sides.  Returns (list of [n, 4] arrays, changed [B] int32: 1 where upstream would print its warning)."""
        ns, ref = _pad_rows(reftracks, 4)
        bsz, nmax = ref.shape[:2]
        with self.scope() as dev:
            d_ref, d_n, d_ch = dev.up(ref), dev.up(ns), dev.out(bsz, np.int32)
            self.min_width_device(bsz, nmax, d_n, d_ref, min_width, d_ch)
            out = dev.get(d_ref)
            return [out[b, :ns[b]].copy() for b in range(bsz)], dev.get(d_ch)

    def prep_track_batch(self, tracks, k_reg=3, s_reg=10, stepsize_prep=1.0, stepsize_reg=3.0, min_width=None, tcks=None, horizon=10, fit="host"):
        """prep_track [REF helper_funcs_glob/src/prep_track.py] for a list of raw tracks ([n_k, 4] rows, not closed).  On the host, per track:
        the linear re-sampling at stepsize_prep and FITPACK's periodic smoothing fit (scipy.interpolate.splprep) -- or the caller's tcks, one
        (t, c, k) per track.  Then on the device, the rows staying there: mcq_spline_approx_device, mcq_prep_device (normals and scalings of
        the prepared rows), mcq_normals_crossing_device (on the un-inflated widths, as upstream) and, with min_width, mcq_min_width_device.
        Returns a dict: reftrack -- list of (m_k, 4) arrays (None where status != 0) --, normvec (m_k, 2), scaling (m_k), crossing [B] (1 / 0,
        -1 where tph raises), inflated [B] (all 0 without min_width), status [B], m [B], dev [B, 2], nonmono [B], tcks (the splines used: the
        caller's, or the ones fitted here): reftrack / normvec / scaling are what solve_batch takes.
        fit="device": the re-sampling and the fit run on the device as well (mcq_spline_fit_device) and the launches are chained -- the spline
        stays on the device between the fit and mcq_spline_approx_device; tcks are its download, None for a track whose fit was refused, which
        is refused as a whole (status MCQ_BAD_INPUT) while the others go on; fit_ier [B] holds FITPACK's ier."""
        if fit not in ("host", "device"):
            raise ValueError("prep_track_batch: fit must be 'host' or 'device'")
        resident, fitted = None, None
        if tcks is None and fit == "device":
            resident = []
            fitted = self.spline_fit_batch(tracks, k=k_reg, s=s_reg, stepsize_prep=stepsize_prep, keep=resident)
            tcks = fitted["tcks"]
        elif tcks is None:
            from scipy import interpolate
            from .trajectory_planning_helpers import interp_track as _it
            tcks = []
            for trk in tracks:
                ti = _it.interp_track(track=np.asarray(trk, dtype=np.float64), stepsize=stepsize_prep)
                cl = np.vstack((ti, ti[0]))
                tcks.append(interpolate.splprep([cl[:, 0], cl[:, 1]], k=k_reg, s=s_reg, per=1)[0])
        bsz = len(tracks)
        keep = []
        if resident is None:
            out = self.spline_approx_batch(tracks, tcks, stepsize_reg, keep=keep)
        else:       # (a refused fit left nk = 0 and NaN knots: mcq_spline_approx_device refuses that track by itself)
            try:
                out = self.spline_approx_batch(tracks, None, stepsize_reg, keep=keep, resident=resident)
            finally:
                for ptr in resident[2:5]:
                    self.free(ptr)
        with self.scope() as dev:
            mmax = keep[2]
            d_ref, d_m = dev.adopt(keep[0], (bsz, mmax, 4)), dev.adopt(keep[1])
            if np.any(out["status"] != 0):      # a refused track has no rows: the kernels behind must not take its m_out (the rows it would need) for a length
                self.upload(d_m, np.where(out["status"] == 0, out["m"], 0).astype(np.int32))
            d_nv, d_sc, d_st, d_cr, d_ch = dev.out((bsz, mmax, 2)), dev.out((bsz, mmax)), dev.out(bsz, np.int32), dev.out(bsz, np.int32), dev.out(bsz, np.int32)
            self._check(self.lib.mcq_prep_device(self.h, bsz, mmax, d_m, d_ref, d_nv, d_sc, d_st), "mcq_prep_device")
            self._check(self.lib.mcq_normals_crossing_device(self.h, bsz, mmax, d_m, d_ref, d_nv, int(horizon), d_cr), "mcq_normals_crossing_device")
            if min_width is not None:
                self.min_width_device(bsz, mmax, d_m, d_ref, min_width, d_ch)
            ref, nv, sc = dev.get(d_ref), dev.get(d_nv), dev.get(d_sc)
            st = np.where(out["status"] != 0, out["status"], dev.get(d_st))
            m = out["m"]
            good = [st[b] == 0 for b in range(bsz)]
            return dict(reftrack=[ref[b, :m[b]].copy() if good[b] else None for b in range(bsz)],
                        normvec=[nv[b, :m[b]].copy() if good[b] else None for b in range(bsz)],
                        scaling=[sc[b, :m[b]].copy() if good[b] else None for b in range(bsz)],
                        crossing=dev.get(d_cr), inflated=dev.get(d_ch) if min_width is not None else np.zeros(bsz, dtype=np.int32), status=st, m=m,
                        dev=out["dev"], nonmono=out["nonmono"], tcks=tcks, **({} if fitted is None else dict(fit_ier=fitted["ier"], fit_fp=fitted["fp"])))

    def raceline_device_ends(self, batch, nmax, d_n, d_ref, d_nv, d_alpha, d_closed, d_psi, stepsize, mmax, d_xy, d_psi_out, d_kappa,
                             d_el, d_m, d_status):
        """mcq_raceline_device_ends (include/mcq.h) on device pointers; d_closed None: every row a chain.  Asynchronous."""
        rc = self.lib.mcq_raceline_device_ends(self.h, int(batch), int(nmax), d_n, d_ref, d_nv, d_alpha, d_closed or None, d_psi or None,
                                               float(stepsize), int(mmax), d_xy, d_psi_out, d_kappa, d_el, d_m, d_status)
        self._check(rc, "mcq_raceline_device_ends")

    def raceline_batch(self, reftracks, normvecs, alphas, stepsize, mmax=None, ends=None):
        """tph.create_raceline + tph.calc_head_curv_an of a list of tracks on the device (mcq_raceline_device)
        [REF main_globaltraj.py:371-387].  reftracks [n_k, >=2], normvecs [n_k, 2], alphas [n_k].  Returns a dict of padded
        arrays: xy [B, mmax, 2], psi / kappa / el_lengths [B, mmax], m [B] (valid entries per row), status [B].

        ends: None (every track a ring), or what solve_batch takes -- one entry per track, None or {closed: True} for a ring, else a dict
        with psi_s, psi_e (fix_s / fix_e are ignored): that track is an open chain (mcq_raceline_device_ends: the open unit-scaling spline
        with the solver's heading rows, every station kept, the last one being the last raceline point); el_lengths[:m - 1] are its
        elements and el_lengths[m - 1] is 0."""
        ns, ref = _pad_rows(reftracks, 4, strict=False)
        nv, al = _pad_like(normvecs, ns, (2,)), _pad_like(alphas, ns)
        bsz, nmax = ref.shape[:2]
        if mmax is None:      # polygon length + the widest shift bounds the raceline length from above generously
            per = [float(_closed_length(r[:, :2]) + 8.0 * np.sum(np.abs(a))) for r, a in zip(reftracks, alphas)]
            mmax = int(max(per) / float(stepsize) * 1.25) + 16
        with self.scope() as dev:
            up, out, get = dev.up, dev.out, dev.get
            d_ref, d_nv, d_al, d_n = up(ref), up(nv), up(al), up(ns)
            d_xy, d_psi, d_k, d_el = out((bsz, mmax, 2)), out((bsz, mmax)), out((bsz, mmax)), out((bsz, mmax))
            d_m, d_st = out(bsz, np.int32), out(bsz, np.int32)
            if ends is None:
                rc = self.lib.mcq_raceline_device(self.h, bsz, nmax, d_n, d_ref, d_nv, d_al, float(stepsize), int(mmax), d_xy,
                                                  d_psi, d_k, d_el, d_m, d_st)
                self._check(rc, "mcq_raceline_device")
            else:
                if len(ends) != bsz:
                    raise ValueError("ends must have one entry per track")
                closed = np.array([1 if e is None or e.get("closed", False) else 0 for e in ends], dtype=np.int32)
                heads = np.zeros((bsz, 2))
                for k, e in enumerate(ends):
                    if not closed[k]:
                        heads[k] = (float(e["psi_s"]), float(e["psi_e"]))
                self.raceline_device_ends(bsz, nmax, d_n, d_ref, d_nv, d_al, up(closed), up(heads), stepsize, mmax, d_xy, d_psi, d_k,
                                          d_el, d_m, d_st)
            return dict(xy=get(d_xy), psi=get(d_psi), kappa=get(d_k), el_lengths=get(d_el), m=get(d_m), status=get(d_st))

    def trajectory_device(self, batch, m, mmax, d_m_of_track, d_track_of, d_xy, d_psi, d_kappa, d_el, d_vx, closed, d_drag, d_mass, d_vmax,
                          d_ggv, n_ggv, d_axm, n_machines, curvlim, d_traj, d_t, d_length, d_limits, d_flags):
        """mcq_trajectory_device (include/mcq.h) on device pointers; d_m_of_track / d_track_of / d_ggv / d_axm / d_traj / d_t may be None.
        Asynchronous."""
        rc = self.lib.mcq_trajectory_device(self.h, int(batch), int(m), int(mmax), d_m_of_track or None, d_track_of or None, d_xy, d_psi,
                                            d_kappa, d_el, d_vx, 1 if closed else 0, d_drag, d_mass, d_vmax, d_ggv or None, int(n_ggv),
                                            d_axm or None, int(n_machines), float(curvlim), d_traj or None, d_t or None, d_length,
                                            d_limits, d_flags)
        self._check(rc, "mcq_trajectory_device")

    def bound_dists_device(self, tracks, nmax, d_n, d_ref, d_nv, mmax, d_m, d_xy, d_psi, length_veh, width_veh, d_length_list, d_width_list,
                           stepsize_bound, mode, d_min_dists, d_min_dist, d_nb, d_bound, d_status):
        """mcq_bound_dists_device (include/mcq.h) on device pointers; d_n / d_m / the two lists / d_bound may be None.  Asynchronous."""
        rc = self.lib.mcq_bound_dists_device(self.h, int(tracks), int(nmax), d_n or None, d_ref, d_nv, int(mmax), d_m or None, d_xy, d_psi,
                                             float(length_veh), float(width_veh), d_length_list or None, d_width_list or None,
                                             float(stepsize_bound), int(mode), d_min_dists, d_min_dist, d_nb, d_bound or None, d_status)
        self._check(rc, "mcq_bound_dists_device")

    def trajectory_batch(self, race, vx, ggv, ax_max_machines, drag_coeff, m_veh, v_max, curvlim, track_of=None, closed=True):
        """The finished trajectories of a batch of variants and check_traj's limit tests on them (mcq_trajectory_device)
        [REF main_globaltraj.py:412-421, 502-534].  race: raceline_batch's dict (xy, psi, kappa, el_lengths, m); vx [batch, mmax]: the profiles of
        vel_profile_batch on race['kappa'] / race['el_lengths']; ggv [batch, g, 3] or None; ax_max_machines [batch, k, 2] or None; drag_coeff,
        m_veh, v_max: scalars or [batch]; curvlim: scalar; track_of [batch] (row of race per variant) or None when rows == batch.
        Returns a dict: traj [batch, mmax, 7] = [s, x, y, psi, kappa, vx, ax] (rows behind a variant's m are NaN), t [batch, mmax + 1]
        (t[m] for closed rows / t[m - 1] for unclosed ones is vel_profile_batch's lap time, bit for bit), length [batch], limits [batch, 6]
        (LIMIT_NAMES), flags [batch] (CHK_* bits, -1 for a variant whose row length or profile is unusable)."""
        xy = np.ascontiguousarray(race["xy"], dtype=np.float64)
        rows, mmax = xy.shape[0], xy.shape[1]
        arrs = [np.ascontiguousarray(race[k], dtype=np.float64) for k in ("psi", "kappa", "el_lengths")]
        for a in arrs:
            if a.shape != (rows, mmax):
                raise ValueError("trajectory_batch: race's arrays do not have one shape")
        ms = np.ascontiguousarray(race["m"], dtype=np.int32)
        vx = np.ascontiguousarray(vx, dtype=np.float64)
        if vx.ndim != 2 or vx.shape[1] != mmax:
            raise ValueError("trajectory_batch: vx must be [batch, %d]" % mmax)
        bsz = vx.shape[0]
        if track_of is None and rows != bsz:
            raise ValueError("trajectory_batch: %d rows for %d variants and no track_of" % (rows, bsz))
        scal = _per_variant(bsz, drag_coeff, m_veh, v_max)
        ggv = None if ggv is None else np.ascontiguousarray(ggv, dtype=np.float64)
        axm = None if ax_max_machines is None else np.ascontiguousarray(ax_max_machines, dtype=np.float64)
        if (ggv is not None and ggv.shape[0] != bsz) or (axm is not None and axm.shape[0] != bsz):
            raise ValueError("trajectory_batch: ggv / ax_max_machines need one table per variant")
        tr = None if track_of is None else np.ascontiguousarray(track_of, dtype=np.int32)
        with self.scope() as dev:
            up, out, get = dev.up, dev.out, dev.get
            d_xy, d_psi, d_k, d_el = up(xy), up(arrs[0]), up(arrs[1]), up(arrs[2])
            d_m, d_vx = up(ms), up(vx)
            d_s = [up(a) for a in scal]
            d_g, d_a, d_t = up(ggv), up(axm), up(tr)
            d_traj, d_time = out((bsz, mmax, TRAJ_COLS)), out((bsz, mmax + 1))
            d_len, d_lim, d_fl = out(bsz), out((bsz, TRAJ_NLIM)), out(bsz, np.int32)
            self.trajectory_device(bsz, 0, mmax, d_m, d_t, d_xy, d_psi, d_k, d_el, d_vx, closed, d_s[0], d_s[1], d_s[2], d_g,
                                   ggv.shape[1] if ggv is not None else 0, d_a, axm.shape[1] if axm is not None else 0, curvlim, d_traj,
                                   d_time, d_len, d_lim, d_fl)
            return dict(traj=get(d_traj), t=get(d_time), length=get(d_len), limits=get(d_lim), flags=get(d_fl))

    def bound_dists_batch(self, reftracks, normvecs, race, length_veh, width_veh, stepsize_bound=1.0, first_row_only=False):
        """check_traj's first block for a list of tracks (mcq_bound_dists_device) [REF helper_funcs_glob/src/check_traj.py:47-70]: the distance
        of the vehicle's four corners to the two boundaries re-sampled at stepsize_bound, per station of race (raceline_batch's dict: xy, psi,
        m; one row per track).  length_veh / width_veh: scalars or one value per track.  first_row_only=True measures against the first sample
        of each boundary only, which is what the reference's call computes (include/mcq.h: MCQ_BOUNDS_FIRST_ROW).
        Returns a dict: min_dists [tracks, mmax] (NaN behind a track's m), min_dist [tracks], nb [tracks, 2] (samples per boundary, right
        first), bound_r / bound_l [tracks, nmax, 2] (the raw boundaries check_traj returns; NaN behind a track's n), status [tracks]."""
        ns, ref = _pad_rows(reftracks, 4, nmin=3)
        nv = _pad_like(normvecs, ns, (2,), nmin=3)
        bsz, nmax = ref.shape[:2]
        xy = np.ascontiguousarray(race["xy"], dtype=np.float64)
        psi = np.ascontiguousarray(race["psi"], dtype=np.float64)
        ms = np.ascontiguousarray(race["m"], dtype=np.int32)
        if xy.shape[0] != bsz or psi.shape != xy.shape[:2] or ms.shape != (bsz,):
            raise ValueError("bound_dists_batch: race must hold one row per track")
        mmax = xy.shape[1]
        lens, wids = np.asarray(length_veh, dtype=np.float64), np.asarray(width_veh, dtype=np.float64)
        with self.scope() as dev:
            up, out, get = dev.up, dev.out, dev.get
            d_ref, d_nv, d_n, d_xy, d_psi, d_m = up(ref), up(nv), up(ns), up(xy), up(psi), up(ms)
            d_ll = up(np.broadcast_to(lens, (bsz,))) if lens.ndim else None
            d_wl = up(np.broadcast_to(wids, (bsz,))) if wids.ndim else None
            d_md, d_mn, d_nb, d_bd, d_st = out((bsz, mmax)), out(bsz), out((bsz, 2), np.int32), out((bsz, 2, nmax, 2)), out(bsz, np.int32)
            self.bound_dists_device(bsz, nmax, d_n, d_ref, d_nv, mmax, d_m, d_xy, d_psi, 0.0 if lens.ndim else float(lens),
                                    0.0 if wids.ndim else float(wids), d_ll, d_wl, stepsize_bound,
                                    BOUNDS_FIRST_ROW if first_row_only else BOUNDS_ALL, d_md, d_mn, d_nb, d_bd, d_st)
            bound = get(d_bd)
            return dict(min_dists=get(d_md), min_dist=get(d_mn), nb=get(d_nb), bound_r=bound[:, 0].copy(), bound_l=bound[:, 1].copy(), status=get(d_st))

    def export_device(self, tracks, nmax, d_n, d_ref, d_nv, d_alpha, batch, mmax, d_m_of_track, d_track_of, d_traj, d_ltpl, d_idx, d_lengths,
                      d_s_ref, d_total, d_status):
        """mcq_export_device (include/mcq.h) on device pointers; d_n / d_m_of_track / d_track_of / d_idx / d_lengths / d_s_ref may be None.
        Asynchronous."""
        rc = self.lib.mcq_export_device(self.h, int(tracks), int(nmax), d_n or None, d_ref, d_nv, d_alpha, int(batch), int(mmax),
                                        d_m_of_track or None, d_track_of or None, d_traj, d_ltpl, d_idx or None, d_lengths or None,
                                        d_s_ref or None, d_total, d_status)
        self._check(rc, "mcq_export_device")

    def export_batch(self, reftracks, normvecs, alphas, traj, track_of=None):
        """The EXPORT block for a batch of variants (mcq_export_device) [REF main_globaltraj.py:502-552, helper_funcs_glob/src/
        export_traj_ltpl.py:35-63]: the local planner's table and the closed race table.  reftracks [n_k, 4], normvecs [n_k, 2], alphas [n_k]: one
        entry per track; traj: trajectory_batch's dict (traj [batch, mmax, 7]; m [tracks] -- when absent, the rows that are not NaN are counted) or
        the padded array itself; track_of [batch] (track per variant) or None when tracks == batch.
        Returns a dict of lists / arrays: ltpl (per variant an (n + 1, 12) array: upstream's traj_ltpl_cl; export.write_traj_ltpl writes its first
        n rows, as upstream does), idx (per variant [n]), spline_lengths (per track [n]), s_ref (per track [n + 1]), spline_total [tracks],
        status [batch], race_cl (per variant (m + 1, 7): the trajectory's rows, then row 0 again with s = spline_total).
        NOTE: upstream closes the race table with numpy.sum(spline_lengths); spline_total is the running sum's last value (numpy.cumsum's order),
        so the two differ in the last bits.  A refused variant (status MCQ_BAD_INPUT) has NaN tables and idx -1."""
        ns, ref = _pad_rows(reftracks, 4, nmin=3)
        nv, al = _pad_like(normvecs, ns, (2,), nmin=3), _pad_like(alphas, ns, nmin=3)
        tracks, nmax = ref.shape[:2]
        ms = None
        if isinstance(traj, dict):
            ms = traj.get("m")
            traj = traj["traj"]
        tj = np.ascontiguousarray(traj, dtype=np.float64)
        if tj.ndim != 3 or tj.shape[2] != TRAJ_COLS:
            raise ValueError("export_batch: traj must be [batch, mmax, %d]" % TRAJ_COLS)
        bsz, mmax = tj.shape[:2]
        if track_of is None and tracks != bsz:
            raise ValueError("export_batch: %d tracks for %d variants and no track_of" % (tracks, bsz))
        tr = np.arange(bsz, dtype=np.int32) if track_of is None else np.ascontiguousarray(track_of, dtype=np.int32)
        if tr.shape != (bsz,):
            raise ValueError("export_batch: track_of must be [batch]")
        if ms is None:      # rows behind a variant's m are NaN (trajectory_batch): the stations of a track are those of its first variant
            ms = np.zeros(tracks, dtype=np.int32)
            for v in range(bsz - 1, -1, -1):
                if 0 <= tr[v] < tracks:
                    ms[tr[v]] = int(np.sum(~np.isnan(tj[v, :, 1])))
        ms = np.ascontiguousarray(ms, dtype=np.int32)
        if ms.shape != (tracks,):
            raise ValueError("export_batch: m must hold one count per track")
        with self.scope() as dev:
            up, out = dev.up, dev.out
            d_ref, d_nv, d_al, d_n = up(ref), up(nv), up(al), up(ns)
            d_m, d_t, d_tj = up(ms), up(tr), up(tj)
            d_tab, d_idx = out((bsz, nmax + 1, LTPL_COLS)), out((bsz, nmax), np.int32)
            d_len, d_s, d_tot, d_st = out((tracks, nmax)), out((tracks, nmax + 1)), out(tracks), out(bsz, np.int32)
            self.export_device(tracks, nmax, d_n, d_ref, d_nv, d_al, bsz, mmax, d_m, d_t, d_tj, d_tab, d_idx, d_len, d_s, d_tot, d_st)
            res = [dev.get(d) for d in (d_tab, d_idx, d_len, d_s, d_tot, d_st)]
        return export_result(*res, ns, ms, tr, tj)

    # ---- friction maps (include/mcq.h "friction maps"; the reference's names on top of these: friction.py) ----------------------------------
    def friction_map(self, cells, mue, bin_side=None):
        """A FrictionMap of cells [c, 2] with mue [c] (NaN: a cell without data), resident on the device (mcq_fmap_create).  bin_side None: automatic."""
        xy = np.ascontiguousarray(cells, dtype=np.float64)
        mu = np.ascontiguousarray(mue, dtype=np.float64).reshape(-1)
        if xy.ndim != 2 or xy.shape[1] != 2 or mu.shape[0] != xy.shape[0]:
            raise ValueError("friction_map: cells must be [c, 2] and mue [c]")
        p = ctypes.c_void_p()
        rc = self.lib.mcq_fmap_create(self.h, xy.shape[0], xy.ctypes.data, mu.ctypes.data, float(bin_side) if bin_side else 0.0, ctypes.byref(p))
        self._check(rc, "mcq_fmap_create")
        fm = FrictionMap(self, p.value, mu.copy())
        if not hasattr(self, "_fmaps"):
            self._fmaps = []
        self._fmaps.append(fm)
        return fm

    def friction_query_device(self, fmap, count, d_xy, d_mue, d_idx=None, d_dist=None):
        """mcq_fmap_query_device on device pointers: d_xy [count][2] -> d_mue [count] (d_idx, d_dist optional).  Asynchronous.  On raceline_batch's
        resident xy [batch][mmax][2] with count = batch * mmax, d_mue IS the mu [batch][mmax] of mcq_vel_profile_device_opts: padding rows that
        are NaN going in are NaN coming out (the raceline entry itself leaves the rows behind m unwritten, and the profile entries do not read
        them)."""
        rc = self.lib.mcq_fmap_query_device(self.h, fmap._live(), int(count), d_xy, d_mue, d_idx or None, d_dist or None)
        self._check(rc, "mcq_fmap_query_device")

    def friction_query_batch(self, fmap, points, want_idx=False, want_dist=False):
        """The friction under points [..., 2]: mue [...] of the nearest cell each (lowest index among exact ties), or a tuple (mue, idx, dist) with
        the entries asked for.  A point that is not finite: NaN, -1, NaN."""
        pts = np.ascontiguousarray(points, dtype=np.float64)
        if pts.ndim < 1 or pts.shape[-1] != 2:
            raise ValueError("friction_query_batch: points must be [..., 2]")
        shape, count = pts.shape[:-1], int(pts.size // 2)
        fmap._live()
        if count == 0:
            res = (np.empty(shape), np.empty(shape, dtype=np.int32), np.empty(shape))
        else:
            with self.scope() as dev:
                d_xy, d_mu = dev.up(pts), dev.out(shape)
                d_i, d_d = dev.out(shape, np.int32) if want_idx else None, dev.out(shape) if want_dist else None
                self.friction_query_device(fmap, count, d_xy, d_mu, d_i, d_d)
                res = (dev.get(d_mu), dev.get(d_i) if want_idx else None, dev.get(d_d) if want_dist else None)
        out = (res[0],) + ((res[1],) if want_idx else ()) + ((res[2],) if want_dist else ())
        return out if len(out) > 1 else out[0]

    def friction_grid_device(self, fmap, tracks, nmax, d_n, d_ref, d_nv, width_opt, d_width, wheelbase_front, wheelbase_rear, dn, jmax, d_n_out,
                             d_cnt, d_mue, d_idx, d_w, d_status):
        """mcq_friction_grid_device (include/mcq.h) on device pointers; d_n / d_width / d_idx / d_w may be None.  Asynchronous."""
        rc = self.lib.mcq_friction_grid_device(self.h, fmap._live(), int(tracks), int(nmax), d_n or None, d_ref, d_nv, float(width_opt),
                                               d_width or None, float(wheelbase_front), float(wheelbase_rear), float(dn), int(jmax), d_n_out,
                                               d_cnt, d_mue, d_idx or None, d_w or None, d_status)
        self._check(rc, "mcq_friction_grid_device")

    @staticmethod
    def friction_jmax(reftracks, widths, dn):
        """The largest count of lateral positions over the finite rows of a list of tracks: Python's own floors, as the kernel takes them."""
        jmax = 1
        for r, w in zip(reftracks, widths):
            for wr, wl in np.asarray(r, dtype=np.float64)[:, 2:4].tolist():
                q = ((wr - 0.5 * w - 0.5) / dn, (wl - 0.5 * w - 0.5) / dn)
                if all(math.isfinite(v) and abs(v) < 1e9 for v in q):
                    jmax = max(jmax, math.floor(q[0]) + math.floor(q[1]) + 1)
        return jmax

    def friction_grid_batch(self, fmap, reftracks, normvecs, width_opt, wheelbase_front, wheelbase_rear, dn, fit=True, jmax=None, want_idx=False,
                            n_gauss=5, rcond=None):
        """extract_friction_coeffs and the linear approx_friction_map of a list of (ragged) tracks in one launch (mcq_friction_grid_device).
        reftracks [n_k, 4], normvecs [n_k, 2]; width_opt: a scalar or one value per track; jmax None: from the widths, on the host.
        Returns a dict of padded arrays: n [tracks, nmax + 1, jmax], cnt [tracks, nmax + 1], mue [tracks, 4, nmax + 1, jmax] (fl, fr, rl, rr),
        w_mue [tracks, 4, nmax + 1, 2] (slope, intercept; fit=False: None), idx (want_idx), status [tracks], rows [tracks] = n_k + 1.
        fit="gauss": the Gaussian-basis fit on the resident grids instead of the lines (mcq_friction_gauss_device; n_gauss bumps on each side,
        rcond None: sklearn's cut-off) -- w_mue is None and the dict also holds w_gauss [tracks, 4, nmax + 1, 2 n_gauss + 2] (weights, then the
        intercept), center_dist [tracks, nmax + 1], rank and sweeps [tracks, nmax + 1].  n_gauss and rcond are read only with fit="gauss";
        there an n_gauss outside 1 .. 15 or a jmax whose row does not fit into 64 KB of LDS is a ValueError before anything is launched."""
        gauss = isinstance(fit, str)
        if gauss and fit != "gauss":
            raise ValueError("friction_grid_batch: fit must be True, False or 'gauss'")
        fit = bool(fit) and not gauss
        ns, ref = _pad_rows(reftracks, 4)
        nv = _pad_like(normvecs, ns, (2,))
        tracks, nmax = ref.shape[:2]
        wl = None if np.ndim(width_opt) == 0 else np.ascontiguousarray(width_opt, dtype=np.float64)
        if wl is not None and wl.shape != (tracks,):
            raise ValueError("friction_grid_batch: width_opt must be a scalar or hold one width per track")
        w0 = float(width_opt) if wl is None else 0.0
        if jmax is None:
            jmax = self.friction_jmax(reftracks, [w0] * tracks if wl is None else wl.tolist(), float(dn))
        jmax, rows = int(jmax), nmax + 1
        if gauss:       # what mcq_friction_gauss_device would refuse, before the grid is launched for nothing
            n_gauss = int(n_gauss)
            if not 1 <= n_gauss <= 15:
                raise ValueError("friction_grid_batch: n_gauss must be 1 .. 15, got %d" % n_gauss)
            if jmax >= 1 and 8 * ((2 * n_gauss + 1) * (jmax + 2 * n_gauss + 7) + 384) > 65536:
                raise ValueError("friction_grid_batch: a row of jmax %d at n_gauss %d does not fit into 64 KB of LDS" % (jmax, n_gauss))
        with self.scope() as dev:
            up, out, get = dev.up, dev.out, dev.get
            d_ref, d_nv, d_n, d_wl = up(ref), up(nv), up(ns), up(wl)
            d_no, d_cnt, d_mu = out((tracks, rows, jmax)), out((tracks, rows), np.int32), out((tracks, 4, rows, jmax))
            d_ix = out((tracks, 4, rows, jmax), np.int32) if want_idx else None
            d_w = out((tracks, 4, rows, 2)) if fit else None
            d_st = out(tracks, np.int32)
            self.friction_grid_device(fmap, tracks, nmax, d_n, d_ref, d_nv, w0, d_wl, wheelbase_front, wheelbase_rear, dn, jmax, d_no, d_cnt,
                                      d_mu, d_ix, d_w, d_st)
            res = dict(n=get(d_no), cnt=get(d_cnt), mue=get(d_mu), w_mue=get(d_w) if fit else None, idx=get(d_ix) if want_idx else None,
                       status=get(d_st), rows=ns + 1)
            if gauss:       # (n_gauss >= 1: the weights' rows are not empty)
                d_wg, d_cd = out((tracks, 4, rows, 2 * n_gauss + 2)), out((tracks, rows))
                d_rk, d_sw = out((tracks, rows), np.int32), out((tracks, rows), np.int32)
                self.friction_gauss_device(tracks, nmax, jmax, d_no, d_cnt, d_mu, d_st, n_gauss, rcond, d_wg, d_cd, d_rk, d_sw)
                res.update(w_gauss=get(d_wg), center_dist=get(d_cd), rank=get(d_rk), sweeps=get(d_sw))
            return res

    def friction_gauss_device(self, tracks, nmax, jmax, d_n, d_cnt, d_mue, d_status, n_gauss, rcond, d_w_gauss, d_center_dist, d_rank=None,
                              d_sweeps=None):
        """mcq_friction_gauss_device (include/mcq.h) on the device pointers mcq_friction_grid_device filled; rcond None: sklearn's cut-off;
        d_rank / d_sweeps may be None.  Asynchronous."""
        rc = self.lib.mcq_friction_gauss_device(self.h, int(tracks), int(nmax), int(jmax), d_n, d_cnt, d_mue, d_status, int(n_gauss),
                                                0.0 if rcond is None else float(rcond), d_w_gauss, d_center_dist, d_rank or None, d_sweeps or None)
        self._check(rc, "mcq_friction_gauss_device")

    def friction_model_device(self, tracks, nmax, qmax, d_q, d_qcnt, model, d_w, d_mue_out, n_gauss=0, centres=FRIC_CENTRES_FIT, d_center_dist=None,
                              d_n=None, d_cnt=None, jmax=0):
        """mcq_friction_model_device (include/mcq.h) on device pointers: model FRIC_LINEAR (d_w [tracks][4][nmax + 1][2]) or FRIC_GAUSS (d_w
        [tracks][4][nmax + 1][2 n_gauss + 2], d_center_dist; with FRIC_CENTRES_FIT also the grid's d_n, d_cnt, jmax).  Asynchronous."""
        rc = self.lib.mcq_friction_model_device(self.h, int(tracks), int(nmax), int(qmax), d_q, d_qcnt or None, int(model), d_w, int(n_gauss),
                                                int(centres), d_center_dist or None, d_n or None, d_cnt or None, int(jmax), d_mue_out)
        self._check(rc, "mcq_friction_model_device")

    def friction_model_batch(self, q, weights, model=None, center_dist=None, n=None, cnt=None, qcnt=None, centres=FRIC_CENTRES_FIT):
        """A fitted model at lateral positions: q [tracks, rows, qmax] (qcnt [tracks, rows] positions per row, None: all) with weights
        [tracks, 4, rows, P] -> mue [tracks, 4, rows, qmax].  model None: FRIC_LINEAR for P == 2, else FRIC_GAUSS with n_gauss = (P - 2) / 2 and
        center_dist [tracks, rows]; FRIC_CENTRES_FIT also takes the grid's n [tracks, rows, jmax] and cnt [tracks, rows]."""
        q = np.ascontiguousarray(q, dtype=np.float64)
        w = np.ascontiguousarray(weights, dtype=np.float64)
        if q.ndim != 3 or w.ndim != 4 or w.shape[:3] != (q.shape[0], 4, q.shape[1]) or q.shape[1] < 2:
            raise ValueError("friction_model_batch: q must be [tracks, rows, qmax] (rows >= 2) and weights [tracks, 4, rows, P]")
        tracks, rows, qmax = q.shape
        P = w.shape[3]
        model = (FRIC_LINEAR if P == 2 else FRIC_GAUSS) if model is None else int(model)
        n_gauss, jmax = 0, 0
        if model == FRIC_GAUSS:
            if P < 4 or P % 2 or center_dist is None:
                raise ValueError("friction_model_batch: the Gaussian model takes weights [.., 2 n_gauss + 2] and center_dist")
            n_gauss = (P - 2) // 2
            center_dist = np.ascontiguousarray(center_dist, dtype=np.float64)
            if center_dist.shape != (tracks, rows):
                raise ValueError("friction_model_batch: center_dist must be [tracks, rows]")
            if centres == FRIC_CENTRES_FIT:
                if n is None or cnt is None:
                    raise ValueError("friction_model_batch: FRIC_CENTRES_FIT takes the grid's n and cnt")
                n, cnt = np.ascontiguousarray(n, dtype=np.float64), np.ascontiguousarray(cnt, dtype=np.int32)
                if n.ndim != 3 or n.shape[:2] != (tracks, rows) or cnt.shape != (tracks, rows):
                    raise ValueError("friction_model_batch: n must be [tracks, rows, jmax] and cnt [tracks, rows]")
                jmax = n.shape[2]
            else:
                n = cnt = None
        elif P != 2:
            raise ValueError("friction_model_batch: the linear model takes weights [.., 2]")
        else:
            center_dist = n = cnt = None
        if qcnt is not None:
            qcnt = np.ascontiguousarray(qcnt, dtype=np.int32)
            if qcnt.shape != (tracks, rows):
                raise ValueError("friction_model_batch: qcnt must be [tracks, rows]")
        with self.scope() as dev:
            d_out = dev.out((tracks, 4, rows, qmax))
            self.friction_model_device(tracks, rows - 1, qmax, dev.up(q), dev.up(qcnt), model, dev.up(w), d_out, n_gauss, centres,
                                       dev.up(center_dist), dev.up(n), dev.up(cnt), jmax)
            return dev.get(d_out)

    # ---- the minimum-time NLP as functions of w (include/mcq.h; the reference's names and files on top of these: mintime.py) -----------------
    @staticmethod
    def mintime_opts(friction=None, n_gauss=0, safe_traj=False, limit_energy=False, pwr_behavior=False):
        """mcq_mintime_opts from the reference's words: friction None / "linear" / "gauss" (optim_opts var_friction) or an MCQ_FRIC_* number.
        pwr_behavior: NotImplementedError -- the 11-state powertrain model is not built."""
        if pwr_behavior:
            raise NotImplementedError("mintime: pwr_behavior (the powertrain's six thermal and charge states) is not implemented")
        if friction in MT_FRICTION:
            friction = MT_FRICTION[friction]
        elif isinstance(friction, str):
            raise ValueError("mintime: var_friction must be None, 'linear' or 'gauss', got %r" % (friction,))
        return McqMintimeOpts(int(friction), int(n_gauss), int(bool(safe_traj)), int(bool(limit_energy)), 0)

    def mintime_layout(self, N, **opt_kw):
        """mcq_mintime_layout: nw, ng, the offsets in w and g, and the collocation constants tau [4], C [4, 4], D [4], B [4] as a dict."""
        o, d = self.mintime_opts(**opt_kw), McqMintimeDims()
        self._check(self.lib.mcq_mintime_layout(int(N), ctypes.byref(o), ctypes.byref(d)), "mcq_mintime_layout")
        res = {k: getattr(d, k) for k, t in McqMintimeDims._fields_ if t is ctypes.c_int}
        res.update(tau=np.array(d.tau), C=np.array(d.C).reshape(4, 4), D=np.array(d.D), B=np.array(d.B))
        return res

    @staticmethod
    def mintime_sizes(nmax, opts):
        """(5 + 24 nmax, ng of nmax): the widths of the w-shaped and g-shaped buffers of a launch."""
        from . import mintime
        return 5 + 24 * int(nmax), mintime.g_rows(nmax, opts.safe_traj, opts.limit_energy)[1]

    @staticmethod
    def mintime_data(batch, nmax, d_n, d_h, d_kappa, d_w_right, d_w_left, d_pars, d_w=None, d_w_mue=None, d_center_dist=None):
        """mcq_mintime_data from device pointers (None where an entry does not read the array)."""
        return McqMintimeData(int(batch), int(nmax), d_n or None, d_h or None, d_kappa or None, d_w_right, d_w_left, d_pars, d_w_mue or None,
                              d_center_dist or None, d_w or None)

    def mintime_bounds_device(self, data, opts, d_w0, d_lbw, d_ubw, d_lbg, d_ubg):
        """mcq_mintime_bounds_device on device pointers.  Asynchronous."""
        self._check(self.lib.mcq_mintime_bounds_device(self.h, ctypes.byref(data), ctypes.byref(opts), d_w0, d_lbw, d_ubw, d_lbg, d_ubg),
                    "mcq_mintime_bounds_device")

    def mintime_eval_device(self, data, opts, d_g, d_J, d_status, d_lap=None, d_energy=None, d_x=None, d_u=None, d_tf=None, d_dt=None, d_ax=None,
                            d_ay=None, d_ec=None):
        """mcq_mintime_eval_device on device pointers; every output but d_g, d_J, d_status may be None.  Asynchronous."""
        self._check(self.lib.mcq_mintime_eval_device(self.h, ctypes.byref(data), ctypes.byref(opts), d_g, d_J, d_lap or None, d_energy or None,
                                                     d_x or None, d_u or None, d_tf or None, d_dt or None, d_ax or None, d_ay or None, d_ec or None,
                                                     d_status), "mcq_mintime_eval_device")

    def mintime_jac_device(self, data, opts, d_blocks, d_grad_J, d_grad_energy=None):
        """mcq_mintime_jac_device on device pointers: d_blocks [batch][nmax][33][33], d_grad_J and d_grad_energy [batch][5 + 24 nmax].  Asynchronous."""
        self._check(self.lib.mcq_mintime_jac_device(self.h, ctypes.byref(data), ctypes.byref(opts), d_blocks, d_grad_J, d_grad_energy or None),
                    "mcq_mintime_jac_device")

    def mintime_kkt_device(self, data, opts, d_g, d_blocks, d_grad_J, d_grad_energy, d_lam_g, d_lam_x, d_lbw, d_ubw, d_lbg, d_ubg, d_r, d_kkt):
        """mcq_mintime_kkt_device on device pointers: what the three entries above left on the device, and the multipliers.  Asynchronous."""
        self._check(self.lib.mcq_mintime_kkt_device(self.h, ctypes.byref(data), ctypes.byref(opts), d_g, d_blocks, d_grad_J, d_grad_energy or None,
                                                    d_lam_g, d_lam_x, d_lbw, d_ubw, d_lbg, d_ubg, d_r, d_kkt), "mcq_mintime_kkt_device")

    def _mintime_up(self, dev, problems, opts, nmax, need_w, resident=None):
        """The padded device arrays of a list of problems -- dicts of h [N], kappa_cl / w_tr_right_cl / w_tr_left_cl [N + 1], pars (a dict of
        MINTIME_PARS or their 40 values), w [5 + 24 N], and with a friction model w_mue [4, N + 1, P] (and center_dist [N + 1]).  resident:
        (d_w_mue, d_center_dist) device pointers in the friction entries' layout for these problems at this nmax, instead of the host arrays."""
        if not problems:
            raise ValueError("mintime: no problems")
        Ns = np.array([np.asarray(q["h"]).shape[0] for q in problems], dtype=np.int32)
        nmax = int(Ns.max()) if nmax is None else int(nmax)
        if Ns.min() < 2 or Ns.max() > nmax:
            raise ValueError("mintime: every problem needs 2 <= N <= nmax intervals (N = %s, nmax = %d)" % (Ns.tolist(), nmax))
        batch, nwmax = len(problems), 5 + 24 * nmax
        P = 0 if opts.friction < 0 else (2 if opts.friction == FRIC_LINEAR else 2 * opts.n_gauss + 2)
        h, w = np.zeros((batch, nmax)), np.zeros((batch, nwmax))
        closed = np.zeros((3, batch, nmax + 1))
        pars = np.zeros((batch, len(MINTIME_PARS)))
        wm, cd = np.zeros((batch, 4, nmax + 1, max(P, 1))), np.zeros((batch, nmax + 1))
        for b, q in enumerate(problems):
            N = int(Ns[b])
            h[b, :N] = np.asarray(q["h"], dtype=np.float64)
            for a, key in enumerate(("kappa_cl", "w_tr_right_cl", "w_tr_left_cl")):
                v = np.asarray(q[key], dtype=np.float64)
                if v.shape != (N + 1,):
                    raise ValueError("mintime: %s must hold N + 1 = %d values" % (key, N + 1))
                closed[a, b, :N + 1] = v
            pars[b] = [q["pars"][k] for k in MINTIME_PARS] if isinstance(q["pars"], dict) else np.asarray(q["pars"], dtype=np.float64)
            if need_w:
                v = np.asarray(q["w"], dtype=np.float64)
                if v.shape != (5 + 24 * N,):
                    raise ValueError("mintime: w must hold 5 + 24 N = %d values" % (5 + 24 * N))
                w[b, :5 + 24 * N] = v
            if P and resident is None:
                v = np.asarray(q["w_mue"], dtype=np.float64)
                if v.shape != (4, N + 1, P):
                    raise ValueError("mintime: w_mue must be [4, N + 1, %d]" % P)
                wm[b, :, :N + 1] = v
                if opts.friction == FRIC_GAUSS:
                    cd[b, :N + 1] = np.asarray(q["center_dist"], dtype=np.float64)
        d_wm, d_cd = resident if resident is not None else ((dev.up(wm), dev.up(cd)) if P else (None, None))
        data = self.mintime_data(batch, nmax, dev.up(Ns), dev.up(h), dev.up(closed[0]), dev.up(closed[1]), dev.up(closed[2]), dev.up(pars),
                                 dev.up(w) if need_w else None, d_wm, d_cd)
        return data, Ns, nmax

    def mintime_bounds_batch(self, problems, nmax=None, **opt_kw):
        """w0, lbw, ubw [batch, 5 + 24 nmax], lbg, ubg [batch, ng of nmax] as the reference builds them (NaN past a problem's own sizes)."""
        opts = self.mintime_opts(**opt_kw)
        with self.scope() as dev:
            data, Ns, nmax = self._mintime_up(dev, problems, opts, nmax, False)
            nw, ng = self.mintime_sizes(nmax, opts)
            d = [dev.out((len(Ns), nw)) for _ in range(3)] + [dev.out((len(Ns), ng)) for _ in range(2)]
            self.mintime_bounds_device(data, opts, *d)
            return dict(zip(("w0", "lbw", "ubw", "lbg", "ubg"), [dev.get(q) for q in d]), N=Ns)

    def mintime_eval_batch(self, problems, nmax=None, resident=None, **opt_kw):
        """g, J, the lap time, the energy and the reference's f_sol outputs of a list of problems in one launch (mcq_mintime_eval_device): a dict of
        padded arrays g [batch, ng of nmax], J, lap_time, energy, status [batch], x_opt [batch, nmax + 1, 5], u_opt [batch, nmax, 4], tf_opt
        [batch, nmax, 12], dt_opt, ax_opt, ay_opt, ec_opt [batch, nmax], N [batch].  resident: see _mintime_up."""
        opts = self.mintime_opts(**opt_kw)
        with self.scope() as dev:
            data, Ns, nmax = self._mintime_up(dev, problems, opts, nmax, True, resident)
            B, (nw, ng) = len(Ns), self.mintime_sizes(nmax, opts)
            shapes = dict(g=(B, ng), J=(B,), lap_time=(B,), energy=(B,), x_opt=(B, nmax + 1, 5), u_opt=(B, nmax, 4), tf_opt=(B, nmax, 12),
                          dt_opt=(B, nmax), ax_opt=(B, nmax), ay_opt=(B, nmax), ec_opt=(B, nmax))
            d = {k: dev.out(v) for k, v in shapes.items()}
            d_st = dev.out(B, np.int32)
            self.mintime_eval_device(data, opts, d["g"], d["J"], d_st, d["lap_time"], d["energy"], d["x_opt"], d["u_opt"], d["tf_opt"], d["dt_opt"],
                                     d["ax_opt"], d["ay_opt"], d["ec_opt"])
            res = {k: dev.get(v) for k, v in d.items()}
            res.update(status=dev.get(d_st), N=Ns)
            return res

    def mintime_jac_batch(self, problems, nmax=None, **opt_kw):
        """The Jacobian of g in interval blocks [batch, nmax, 33, 33], grad_J and grad_energy [batch, 5 + 24 nmax] (mcq_mintime_jac_device)."""
        opts = self.mintime_opts(**opt_kw)
        with self.scope() as dev:
            data, Ns, nmax = self._mintime_up(dev, problems, opts, nmax, True)
            B, (nw, ng) = len(Ns), self.mintime_sizes(nmax, opts)
            shapes = dict(blocks=(B, nmax, MT_BLOCK, MT_BLOCK), grad_J=(B, nw), grad_energy=(B, nw))
            d = {k: dev.out(v) for k, v in shapes.items()}
            self.mintime_jac_device(data, opts, d["blocks"], d["grad_J"], d["grad_energy"])
            res = {k: dev.get(v) for k, v in d.items()}
            res.update(N=Ns)
            return res

    def mintime_kkt_batch(self, problems, lam_g, lam_x, nmax=None, **opt_kw):
        """The certificate of primal-dual points: bounds, evaluation, Jacobian and mcq_mintime_kkt_device chained on the device.  lam_g [ng_k] and
        lam_x [nw_k] per problem.  Returns r [batch, 5 + 24 nmax] and kkt [batch, 3] (max |r|, the largest bound violation, the largest
        complementarity product), with g, J, lap_time, status of the evaluation."""
        opts = self.mintime_opts(**opt_kw)
        with self.scope() as dev:
            data, Ns, nmax = self._mintime_up(dev, problems, opts, nmax, True)
            B, (nw, ng) = len(Ns), self.mintime_sizes(nmax, opts)
            bad = "mintime_kkt_batch: lam_x must hold nw values and lam_g ng values of its problem"
            vx = [np.asarray(lam_x[b], dtype=np.float64) for b in range(B)]
            if any(q.shape != (5 + 24 * int(n),) for q, n in zip(vx, Ns)):
                raise ValueError(bad)
            lg, lx = self._mintime_lam(Ns, lam_g, None, ng, bad)[0], _pad_last(vx, nw)
            bw = [dev.out((B, nw)) for _ in range(3)]
            bg = [dev.out((B, ng)) for _ in range(2)]
            d_g, d_J, d_lap, d_st = dev.out((B, ng)), dev.out(B), dev.out(B), dev.out(B, np.int32)
            d_blk, d_gJ, d_gE = dev.out((B, nmax, MT_BLOCK, MT_BLOCK)), dev.out((B, nw)), dev.out((B, nw))
            d_r, d_k = dev.out((B, nw)), dev.out((B, 3))
            self.mintime_bounds_device(data, opts, bw[0], bw[1], bw[2], bg[0], bg[1])
            self.mintime_eval_device(data, opts, d_g, d_J, d_st, d_lap)
            self.mintime_jac_device(data, opts, d_blk, d_gJ, d_gE)
            self.mintime_kkt_device(data, opts, d_g, d_blk, d_gJ, d_gE, dev.up(lg), dev.up(lx), bw[1], bw[2], bg[0], bg[1], d_r, d_k)
            return dict(r=dev.get(d_r), kkt=dev.get(d_k), g=dev.get(d_g), J=dev.get(d_J), lap_time=dev.get(d_lap), status=dev.get(d_st), N=Ns)

    def mintime_hess_device(self, data, opts, d_lam_g, d_sigma, d_hblocks):
        """mcq_mintime_hess_device on device pointers: d_lam_g [batch][ng of nmax], d_sigma [batch] or None (1), d_hblocks [batch][nmax][33][33].
        Asynchronous."""
        self._check(self.lib.mcq_mintime_hess_device(self.h, ctypes.byref(data), ctypes.byref(opts), d_lam_g, d_sigma or None, d_hblocks),
                    "mcq_mintime_hess_device")

    def mintime_hessvec_device(self, data, opts, d_hblocks, d_v, nvec, d_y):
        """mcq_mintime_hessvec_device on device pointers: d_v and d_y [batch][nvec][5 + 24 nmax].  Asynchronous."""
        self._check(self.lib.mcq_mintime_hessvec_device(self.h, ctypes.byref(data), ctypes.byref(opts), d_hblocks, d_v, int(nvec), d_y),
                    "mcq_mintime_hessvec_device")

    @staticmethod
    def _mintime_lam(Ns, lam_g, sigma, ng, bad="mintime: lam_g must hold the ng values of its problem"):
        """lam_g (one vector per problem, at most ng values) and sigma (None, or one number per problem) as padded arrays [batch, ng], [batch]"""
        B = len(Ns)
        vg = [np.asarray(lam_g[b], dtype=np.float64) for b in range(B)]
        if any(q.ndim != 1 or q.shape[0] > ng for q in vg):
            raise ValueError(bad)
        sg = None if sigma is None else np.ascontiguousarray(np.broadcast_to(np.asarray(sigma, dtype=np.float64), (B,)))
        return _pad_last(vg, ng), sg

    def mintime_hess_batch(self, problems, lam_g, sigma=None, nmax=None, **opt_kw):
        """The Hessian of the Lagrangian sigma J + lam_g . g in interval blocks hblocks [batch, nmax, 33, 33] (mcq_mintime_hess_device; the slots and the
        k = 0 rule: include/mcq.h; mintime.hessian_coo assembles them).  lam_g [ng_k] per problem, sigma None (1) or one number per problem."""
        opts = self.mintime_opts(**opt_kw)
        with self.scope() as dev:
            data, Ns, nmax = self._mintime_up(dev, problems, opts, nmax, True)
            B, (nw, ng) = len(Ns), self.mintime_sizes(nmax, opts)
            lg, sg = self._mintime_lam(Ns, lam_g, sigma, ng)
            d_h = dev.out((B, nmax, MT_BLOCK, MT_BLOCK))
            self.mintime_hess_device(data, opts, dev.up(lg), None if sg is None else dev.up(sg), d_h)
            return dict(hblocks=dev.get(d_h), N=Ns)

    def mintime_hessvec_batch(self, problems, lam_g, v, sigma=None, nmax=None, **opt_kw):
        """y = H v for the vectors v [nvec, nw_k] of every problem (the same nvec for all): the Hessian blocks and mcq_mintime_hessvec_device chained on
        the device.  Returns y [batch, nvec, 5 + 24 nmax] (NaN past a problem's own nw) and hblocks."""
        opts = self.mintime_opts(**opt_kw)
        with self.scope() as dev:
            data, Ns, nmax = self._mintime_up(dev, problems, opts, nmax, True)
            B, (nw, ng) = len(Ns), self.mintime_sizes(nmax, opts)
            lg, sg = self._mintime_lam(Ns, lam_g, sigma, ng)
            vs = [np.atleast_2d(np.asarray(q, dtype=np.float64)) for q in v]
            nvec = vs[0].shape[0] if vs else 0
            if len(vs) != B or any(q.shape != (nvec, 5 + 24 * int(n)) for q, n in zip(vs, Ns)):
                raise ValueError("mintime_hessvec_batch: v must hold [nvec, nw] values per problem, the same nvec for all")
            vv = _pad_last(vs, nw, (max(nvec, 1),))
            d_h, d_y = dev.out((B, nmax, MT_BLOCK, MT_BLOCK)), dev.out((B, max(nvec, 1), nw))
            self.mintime_hess_device(data, opts, dev.up(lg), None if sg is None else dev.up(sg), d_h)
            self.mintime_hessvec_device(data, opts, d_h, dev.up(vv), nvec, d_y)
            return dict(y=dev.get(d_y), hblocks=dev.get(d_h), N=Ns)

    # ---- the regularised primal-dual Newton step from the resident blocks (include/mcq.h; mintime.kkt_matrix assembles the same matrix) ----
    def mintime_step_bytes(self, nmax, nvec=1, **opt_kw):
        """mcq_mintime_step_bytes: the workspace of mcq_mintime_step_device per problem, in bytes."""
        out = ctypes.c_size_t(0)
        self._check(self.lib.mcq_mintime_step_bytes(int(nmax), ctypes.byref(self.mintime_opts(**opt_kw)), int(nvec), ctypes.byref(out)),
                    "mcq_mintime_step_bytes")
        return int(out.value)

    def mintime_step_workspace(self):
        """The bytes the handle holds for mcq_mintime_step_device now (it grows, never shrinks)."""
        return int(self.lib.mcq_mintime_step_workspace(self.h))

    def mintime_step_device(self, data, opts, d_hblocks, d_blocks, d_grad_energy, d_dw, d_dg, d_rhs, nvec, refine, d_sol, d_res, d_inertia, d_status):
        """mcq_mintime_step_device on device pointers: d_hblocks, d_blocks [batch][nmax][33][33], d_grad_energy [batch][5 + 24 nmax] or None (read
        with limit_energy only), d_dw [batch][5 + 24 nmax], d_dg [batch][ng of nmax], d_rhs and d_sol [batch][nvec][nw + ng of nmax], d_res
        [batch][nvec], d_inertia [batch][3] and d_status [batch] int32.  Asynchronous."""
        self._check(self.lib.mcq_mintime_step_device(self.h, ctypes.byref(data), ctypes.byref(opts), d_hblocks, d_blocks, d_grad_energy or None, d_dw,
                                                     d_dg, d_rhs, int(nvec), int(refine), d_sol, d_res, d_inertia, d_status),
                    "mcq_mintime_step_device")

    @staticmethod
    def _mintime_step_pad(Ns, ngs, nw, ng, dw, dg, rhs):
        """the diagonals and right-hand sides of every problem (dw [nw_k], dg [ng_k], rhs [nvec, nw_k + ng_k]: w part, then multiplier part) as
        padded arrays [batch, nw], [batch, ng], [batch, nvec, nw + ng] with the multiplier part at nw"""
        B = len(Ns)
        rs = [np.atleast_2d(np.asarray(q, dtype=np.float64)) for q in rhs]
        nvec = rs[0].shape[0] if rs else 0
        if len(rs) != B or len(dw) != B or len(dg) != B:
            raise ValueError("mintime_step_batch: dw, dg and rhs must hold one entry per problem")
        nws = [5 + 24 * int(n) for n in Ns]
        a, c = [np.asarray(q, dtype=np.float64) for q in dw], [np.asarray(q, dtype=np.float64) for q in dg]
        if any(a[b].shape != (nws[b],) or c[b].shape != (ngs[b],) or rs[b].shape != (nvec, nws[b] + ngs[b]) for b in range(B)):
            raise ValueError("mintime_step_batch: dw must hold nw, dg ng and rhs [nvec, nw + ng] values of its problem, the same nvec for all")
        lead = (max(nvec, 1),)
        pr = np.concatenate((_pad_last([r[:, :n] for r, n in zip(rs, nws)], nw, lead), _pad_last([r[:, n:] for r, n in zip(rs, nws)], ng, lead)), axis=2)
        return _pad_last(a, nw), _pad_last(c, ng), pr, nvec

    def mintime_step_batch(self, problems, lam_g, dw, dg, rhs, sigma=None, refine=2, nmax=None, **opt_kw):
        """The Newton step of every problem at its w and lam_g: Jacobian -> Hessian -> mcq_mintime_step_device chained on resident blocks.  dw [nw_k],
        dg [ng_k] and rhs [nvec, nw_k + ng_k] per problem (the same nvec for all).  Returns sol [batch, nvec, nw + ng of nmax] (the multiplier part
        at nw_max; mintime.step_of splits it), res [batch, nvec], inertia [batch, 3], status [batch], and the blocks, hblocks and grad_energy used."""
        opts = self.mintime_opts(**opt_kw)
        with self.scope() as dev:
            data, Ns, nmax = self._mintime_up(dev, problems, opts, nmax, True)
            B, (nw, ng) = len(Ns), self.mintime_sizes(nmax, opts)
            ngs = np.array([self.mintime_sizes(int(n), opts)[1] for n in Ns])
            lg, sg = self._mintime_lam(Ns, lam_g, sigma, ng)
            pw, pg, pr, nvec = self._mintime_step_pad(Ns, ngs, nw, ng, dw, dg, rhs)
            d_blk, d_gJ, d_gE, d_h = dev.out((B, nmax, MT_BLOCK, MT_BLOCK)), dev.out((B, nw)), dev.out((B, nw)), dev.out((B, nmax, MT_BLOCK, MT_BLOCK))
            d_sol, d_res = dev.out((B, max(nvec, 1), nw + ng)), dev.out((B, max(nvec, 1)))
            d_in, d_st = dev.out((B, 3), np.int32), dev.out(B, np.int32)
            self.mintime_jac_device(data, opts, d_blk, d_gJ, d_gE)
            self.mintime_hess_device(data, opts, dev.up(lg), None if sg is None else dev.up(sg), d_h)
            self.mintime_step_device(data, opts, d_h, d_blk, d_gE, dev.up(pw), dev.up(pg), dev.up(pr), nvec, refine, d_sol, d_res, d_in, d_st)
            return dict(sol=dev.get(d_sol), res=dev.get(d_res), inertia=dev.get(d_in), status=dev.get(d_st), blocks=dev.get(d_blk),
                        hblocks=dev.get(d_h), grad_energy=dev.get(d_gE), N=Ns, ng=ngs, nw_max=nw)

    # ---- friction map generation (include/mcq.h "friction map generation"; the reference's names on top of these: friction.py) -------------
    def contains_points_device(self, paths, vmax, d_v, d_verts, d_radius, count, d_xy, d_inside, d_status, d_contour=None, d_contour_count=None):
        """mcq_points_in_path_device on device pointers: d_verts [paths][vmax][2], d_v [paths] or None, d_radius [paths], d_xy [count][2] ->
        d_inside [paths][count] bytes, d_status [paths]; d_contour [paths][2 vmax][2] and d_contour_count [paths]: both or neither.  Asynchronous."""
        rc = self.lib.mcq_points_in_path_device(self.h, int(paths), int(vmax), d_v or None, d_verts, d_radius, int(count), d_xy or None,
                                                d_inside or None, d_status, d_contour or None, d_contour_count or None)
        self._check(rc, "mcq_points_in_path_device")

    def contains_points_batch(self, paths, points, radius=0.0, want_contours=False):
        """matplotlib's Path(v).contains_points(points, radius=r) for a list of polygons [v_k, 2] and one point set [count, 2], on the device:
        inside bool [paths, count] and status int32 [paths] (FGEN_* bits) -- with want_contours also the list of polygons [c_k, 2] the crossing
        test ran on (agg's contour at radius / 2; the path itself for radius 0).  radius: a scalar or one per path."""
        verts = [np.asarray(v, dtype=np.float64).reshape(-1, 2) for v in paths]
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 2)
        if not verts:
            raise ValueError("contains_points_batch: no paths")
        k, count = len(verts), pts.shape[0]
        vs = np.array([v.shape[0] for v in verts], dtype=np.int32)
        vmax = max(int(vs.max()), 1)
        pad = np.zeros((k, vmax, 2))
        for i, v in enumerate(verts):
            pad[i, :vs[i]] = v
        rad = _per_variant(k, radius)[0]
        with self.scope() as dev:
            d_in, d_st = dev.out((k, count), np.uint8, floor=1), dev.out(k, np.int32)
            d_c, d_cc = (dev.out((k, 2 * vmax, 2)), dev.out(k, np.int32)) if want_contours else (None, None)
            self.contains_points_device(k, vmax, dev.up(vs), dev.up(pad), dev.up(rad), count, dev.up(pts) if count else None, d_in if count else None,
                                        d_st, d_c, d_cc)
            inside = dev.get(d_in).astype(bool) if count else np.zeros((k, 0), dtype=bool)
            status = dev.get(d_st)
            if not want_contours:
                return inside, status
            cc, c = dev.get(d_cc), dev.get(d_c)
        return inside, status, [c[i, :cc[i]].copy() for i in range(k)]

    def friction_gen_device(self, tracks, nmax, d_n, d_ref, cellwidth, d_inside_right, cmax, d_bound_r, d_bound_l, d_grid, d_count, d_cells, d_status):
        """mcq_friction_gen_device (include/mcq.h) on device pointers; d_n / d_inside_right / d_bound_r / d_bound_l / d_cells may be None (d_cells
        None: counts only; d_count None as well: boundaries, grids and status only, one asynchronous launch).  With d_count it waits once for the
        boundaries' launch; the launches after it are asynchronous."""
        rc = self.lib.mcq_friction_gen_device(self.h, int(tracks), int(nmax), d_n or None, d_ref, float(cellwidth), d_inside_right or None, int(cmax),
                                              d_bound_r or None, d_bound_l or None, d_grid, d_count or None, d_cells or None, d_status)
        self._check(rc, "mcq_friction_gen_device")

    def track_boundaries_batch(self, reftracks):
        """The reference's calc_trackboundaries for a list of (ragged) tracks [n_k, 4]: (bound_right, bound_left: lists of [n_k, 2], status
        [tracks]) from mcq_friction_gen_device's boundaries-only form (count_out NULL): one launch, no grid point tested.  A waypoint whose
        neighbours coincide has NaN rows there and FGEN_NONFINITE; a track with a non-finite waypoint or width, or with FGEN_FEW, has all rows NaN."""
        ns, ref = _pad_rows(reftracks, 4, nmin=3)
        tracks, nmax = ref.shape[:2]
        with self.scope() as dev:
            d_br, d_bl, d_grid, d_st = dev.out((tracks, nmax, 2)), dev.out((tracks, nmax, 2)), dev.out((tracks, 6)), dev.out(tracks, np.int32)
            self.friction_gen_device(tracks, nmax, dev.up(ns), dev.up(ref), 1.0, None, 0, d_br, d_bl, d_grid, None, None, d_st)
            br, bl = dev.get(d_br), dev.get(d_bl)
            status = dev.get(d_st) & ~FGEN_GRID      # (the grid of the 1 m cell asked for is not the caller's)
        return [br[t, :ns[t]].copy() for t in range(tracks)], [bl[t, :ns[t]].copy() for t in range(tracks)], status

    def friction_gen_batch(self, reftracks, cellwidth_m, inside_trackbound="right", cmax=None):
        """The reference's main_gen_frictionmap for a list of (ragged) tracks [n_k, 4] = x, y, w_right, w_left: a counting call, then the cells
        into buffers of the largest count (cmax given: one call, a track with more cells is cut and carries FGEN_OVERFLOW).  inside_trackbound:
        "right" / "left", or one of them per track.  Returns a dict: cells (a list of [count_k, 2] in the reference's order), counts [tracks],
        grids [tracks, 6] = x0, x1, y0, y1, nx, ny, bound_right / bound_left (lists of [n_k, 2]), status [tracks] (FGEN_* bits; a refused track
        has no cells)."""
        sides = [inside_trackbound] * len(reftracks) if isinstance(inside_trackbound, str) else list(inside_trackbound)
        if len(sides) != len(reftracks) or any(s not in ("right", "left") for s in sides):
            raise ValueError("friction_gen_batch: inside_trackbound must be 'right' or 'left', or one of them per track")
        ns, ref = _pad_rows(reftracks, 4, nmin=3)
        tracks, nmax = ref.shape[:2]
        with self.scope() as dev:
            d_ref, d_n, d_side = dev.up(ref), dev.up(ns), dev.up(np.array([s == "right" for s in sides], dtype=np.int32))
            d_br, d_bl, d_grid = dev.out((tracks, nmax, 2)), dev.out((tracks, nmax, 2)), dev.out((tracks, 6))
            d_cnt, d_st = dev.out(tracks, np.int32), dev.out(tracks, np.int32)
            if cmax is None:
                self.friction_gen_device(tracks, nmax, d_n, d_ref, cellwidth_m, d_side, 0, None, None, d_grid, d_cnt, None, d_st)
                cmax = int(dev.get(d_cnt).max())
            cmax = int(cmax)
            d_cells = dev.out((tracks, max(cmax, 1), 2))
            self.friction_gen_device(tracks, nmax, d_n, d_ref, cellwidth_m, d_side, cmax, d_br, d_bl, d_grid, d_cnt, d_cells, d_st)
            counts, status, cells = dev.get(d_cnt), dev.get(d_st), dev.get(d_cells)
            br, bl, grids = dev.get(d_br), dev.get(d_bl), dev.get(d_grid)
        return dict(cells=[cells[t, :min(int(counts[t]), cmax)].copy() for t in range(tracks)], counts=counts, grids=grids,
                    bound_right=[br[t, :ns[t]].copy() for t in range(tracks)], bound_left=[bl[t, :ns[t]].copy() for t in range(tracks)], status=status)

    def relinearise_device(self, batch, nmax, d_n_in, d_ref_in, d_nv_in, d_alpha, d_live, alpha_scale, stepsize,
                           d_ref_out, d_nv_out, d_n_out, d_status):
        """IQP glue between two passes, on the device (mcq_relinearise_device in include/mcq.h).  Asynchronous."""
        rc = self.lib.mcq_relinearise_device(self.h, int(batch), int(nmax), d_n_in, d_ref_in, d_nv_in, d_alpha,
                                             d_live or None, float(alpha_scale), float(stepsize), d_ref_out, d_nv_out,
                                             d_n_out, d_status)
        self._check(rc, "mcq_relinearise_device")

    def set_iqp_round_callback(self, fn):
        """fn(round, curv_err [batch] ndarray, live [batch] ndarray) after every QP pass of mcq_iqp_batch / mcq_iqp_device, or None to remove
        it (the per-iteration print_debug lines of tph.iqp_handler, as they happen)."""
        if fn is None:
            self._iqp_cb = None
            self._check(self.lib.mcq_iqp_set_round_callback(self.h, ctypes.cast(None, IQP_ROUND_CB), None), "mcq_iqp_set_round_callback")
            return

        def tramp(_user, rnd, batch, curv, live):
            fn(int(rnd), np.ctypeslib.as_array(curv, shape=(batch,)).copy(), np.ctypeslib.as_array(live, shape=(batch,)).copy())
        self._iqp_cb = IQP_ROUND_CB(tramp)          # kept alive while registered
        self._check(self.lib.mcq_iqp_set_round_callback(self.h, self._iqp_cb, None), "mcq_iqp_set_round_callback")

    # ---- device memory plumbing (mcq_device_alloc & co): numpy in, numpy out, raw device pointers as ints ----------------
    def scope(self):
        """Context manager owning device allocations: up(array or None) / out(shape, dtype) / new(nbytes) give pointers it frees on exit, get(ptr)
        fetches what up or out put there, release(ptr) takes one out."""
        return _Scope(self)

    def alloc(self, nbytes):
        p = ctypes.c_void_p()
        self._check(self.lib.mcq_device_alloc(self.h, int(nbytes), ctypes.byref(p)), "mcq_device_alloc")
        return p.value

    def free(self, ptr):
        self._check(self.lib.mcq_device_free(self.h, ptr), "mcq_device_free")

    def upload(self, ptr, arr, offset_bytes=0):
        arr = np.ascontiguousarray(arr)
        self._check(self.lib.mcq_copy_to_device(self.h, int(ptr) + int(offset_bytes), arr.ctypes.data, arr.nbytes), "mcq_copy_to_device")

    def download(self, ptr, shape, dtype, offset_bytes=0):
        out = np.empty(shape, dtype=dtype)
        if out.nbytes >= (1 << 20):
            out.fill(0)          # touched pages: a copy into never-touched pageable memory faults page by page inside the driver (10x slower)
        self._check(self.lib.mcq_copy_to_host(self.h, out.ctypes.data, int(ptr) + int(offset_bytes), out.nbytes), "mcq_copy_to_host")
        return out

    def sync(self):
        self._check(self.lib.mcq_sync(self.h), "mcq_sync")

    def stream(self):
        return self.lib.mcq_stream(self.h)

    def last_timing_ms(self):
        ms = (ctypes.c_float * 5)()
        self._check(self.lib.mcq_last_timing(self.h, ctypes.byref(ms)), "mcq_last_timing")
        return dict(solve=ms[2], total=ms[4], assemble_sp=ms[0])      # (ms[1], ms[3]: kernels that no longer exist -- include/mcq.h)

    def timing_begin(self):
        """Opens a span of launches timed on the device (mcq_timing_begin)."""
        self._check(self.lib.mcq_timing_begin(self.h), "mcq_timing_begin")

    def timing_end(self):
        """Closes the span: (milliseconds on the device between begin and end, solver launches enqueued in between).  Blocks until the span's last launch is done."""
        ms, cnt = ctypes.c_float(), ctypes.c_int()
        self._check(self.lib.mcq_timing_end(self.h, ctypes.byref(ms), ctypes.byref(cnt)), "mcq_timing_end")
        return float(ms.value), int(cnt.value)

    def workspace_bytes(self):
        return int(self.lib.mcq_workspace_bytes(self.h))

    # ---- the one collective of a multi-GPU job: RCCL's all-gather through the C ABI, on the engine's own stream (include/mcq.h) -----
    COMM_ID_BYTES = 128
    DT_F64, DT_F32, DT_I32 = 0, 1, 2

    def comm_unique_id(self):
        """128 opaque bytes: created by rank 0, shipped to every rank by the launcher's rendezvous."""
        buf = ctypes.create_string_buffer(self.COMM_ID_BYTES)
        rc = self.lib.mcq_comm_unique_id(buf)
        if rc != 0:
            raise EngineError("mcq_comm_unique_id failed: %s" % self.lib.mcq_last_error().decode())
        return buf.raw

    def comm_init(self, rank, world, unique_id):
        if len(unique_id) != self.COMM_ID_BYTES:
            raise ValueError("comm_init: the unique id has %d bytes, not %d" % (len(unique_id), self.COMM_ID_BYTES))
        self._check(self.lib.mcq_comm_init(self.h, int(rank), int(world), bytes(unique_id)), "mcq_comm_init")

    def comm_allgather(self, d_send, d_recv, count, dtype=0):
        """recv [world][count] <- send [count] of every rank (device pointers); asynchronous on the engine's stream."""
        self._check(self.lib.mcq_comm_allgather(self.h, d_send, d_recv, int(count), int(dtype)), "mcq_comm_allgather")

    def comm_wait(self, lag=0):
        """Blocks until the gather enqueued `lag` gathers ago is done; returns its device time in ms (0.0 if there was none)."""
        ms = ctypes.c_float(0.0)
        self._check(self.lib.mcq_comm_wait(self.h, int(lag), ctypes.byref(ms)), "mcq_comm_wait")
        return float(ms.value)

    def comm_world(self):
        r, w = ctypes.c_int(), ctypes.c_int()
        self._check(self.lib.mcq_comm_world(self.h, ctypes.byref(r), ctypes.byref(w)), "mcq_comm_world")
        return r.value, w.value

    def comm_destroy(self):
        self._check(self.lib.mcq_comm_destroy(self.h), "mcq_comm_destroy")


_LIB_FOR_HOST_HELPERS = None


def les_scalings(A, check=True, closed=True):
    """The N spline scalings out of the dense [4N, 4N] matrix the reference passes as `A` (mcq_les_scalings: one threaded pass over the matrix in
    C, no GPU, no handle) -- the structural check of trajectory_planning_helpers.calc_splines.scalings_from_les_matrix, which stays as its
    numpy statement (and takes any array this entry cannot: other dtypes, non-contiguous views).  Raises RuntimeError with upstream-style
    wording when `A` is not calc_splines' closed-spline system.

    closed=False: `A` is the [4(N-1), 4(N-1)] matrix of calc_splines' OPEN system through N waypoints (mcq_les_scalings_open); returns [N]
    scalings, the inner joints' in entries 0..N-3 and ones in the last two (what solve_batch reads for a chain)."""
    global _LIB_FOR_HOST_HELPERS
    if not (isinstance(A, np.ndarray) and A.dtype == np.float64 and A.ndim == 2 and A.shape[0] == A.shape[1] and A.shape[0] % 4 == 0
            and A.shape[0] >= (12 if closed else 8) and A.flags["C_CONTIGUOUS"]):
        from .trajectory_planning_helpers import calc_splines as _cs
        return (_cs.scalings_from_les_matrix if closed else _cs.scalings_from_open_les_matrix)(A, check=check)
    if _LIB_FOR_HOST_HELPERS is None:
        _LIB_FOR_HOST_HELPERS = _DEFAULT_ENGINE.lib if _DEFAULT_ENGINE is not None else load_library()
    lib = _LIB_FOR_HOST_HELPERS
    n = A.shape[0] // 4 + (0 if closed else 1)
    s = np.empty(n)
    if (lib.mcq_les_scalings if closed else lib.mcq_les_scalings_open)(A.ctypes.data, n, s.ctypes.data, 1 if check else 0) != 0:
        words = ("closed", "N spline scalings it encodes and cannot use an arbitrary matrix") if closed else ("open", "spline scalings it encodes")
        raise RuntimeError("Spline equation system matrix A does not have the structure of calc_splines' %s-spline system (the MI355X engine derives "
                           "everything from the %s): " % words + lib.mcq_last_error().decode())
    return s


_DEFAULT_ENGINE = None


def default_engine():
    """Process-wide engine on the device given by LOCAL_RANK (one process per GPU) or device 0."""
    global _DEFAULT_ENGINE
    if _DEFAULT_ENGINE is None:
        _DEFAULT_ENGINE = Engine(int(os.environ.get("MCQ_DEVICE", os.environ.get("LOCAL_RANK", "0"))))
    return _DEFAULT_ENGINE
