"""TEST-ONLY: runs the reference's opt_mintime.py UNMODIFIED, by file path from a reference tree, on top of oracle/casadi_trace.py, and keeps what
it built: the NLP's f, x, g as expression graphs, the bounds its nlpsol call received, its f_sol Function, the keyword arguments of its export call
and what it returned.  Around the one run sys.modules holds the stand-in as `casadi`, a `trajectory_planning_helpers` made of the package's own
calc_splines and calc_spline_lengths plus two functions that return INJECTED arrays (calc_head_curv_num: the curvature; nonreg_sampling: the kept
rows and indices -- input data of the NLP, not what is under test), and an `opt_mintime_traj` with two members (approx_friction_map returns the
injected weights in the reference's shapes, export_mintime_solution captures its keyword arguments); afterwards sys.modules is as it was.

The `pars` handed to the reference is its nested dictionary, built here from a flat set of the 40 parameters (nested_pars).  In a longdouble run
the 40 parameters and center_dist are longdouble scalars, so the constants the reference folds before they meet a symbol carry no float64
rounding; what it stores in float64 arrays of its own (the collocation matrices C, D, B; h = diff(s_opt)) stays float64 -- see
tests/test_mintime_trace_ref.py for how the comparison accounts for it."""
import importlib
import importlib.util
import os
import sys
import types

import numpy as np

from . import casadi_trace as ct

LD = np.longdouble
REFERENCE = os.environ.get("MCQ_REFERENCE_DIR", "/root/reference")
VEH = ("mass", "dragcoeff", "g", "v_max")
VEHICLE = ("wheelbase_front", "wheelbase_rear", "track_width_front", "track_width_rear", "cog_z", "I_z", "liftcoeff_front", "liftcoeff_rear",
           "k_brake_front", "k_drive_front", "k_roll", "t_delta", "t_drive", "t_brake", "power_max", "f_drive_max", "f_brake_max", "delta_max")
TIRE = ("c_roll", "f_z0", "B_front", "C_front", "eps_front", "E_front", "B_rear", "C_rear", "eps_rear", "E_rear")
OPTIM = ("width_opt", "mue", "penalty_F", "penalty_delta", "energy_limit", "ax_pos_safe", "ax_neg_safe", "ay_safe")
FSOL = ("x_opt", "u_opt", "tf_opt", "dt_opt", "ax_opt", "ay_opt", "ec_opt")


def source_path(ref_dir=None):
    return os.path.join(ref_dir or REFERENCE, "opt_mintime_traj", "src", "opt_mintime.py")


def available(ref_dir=None):
    return os.path.isfile(source_path(ref_dir))


def nested_pars(flat, opts, stepsize, nonreg=False, cast=float):
    """The reference's `pars` from the flat 40 parameters and the option keywords (friction, n_gauss, safe_traj, limit_energy).  wheelbase is the
    sum the reference's main script forms [REF main_globaltraj.py:188]."""
    p = {k: cast(flat[k]) for k in VEH + VEHICLE + TIRE + OPTIM}
    vehicle = {k: p[k] for k in VEHICLE}
    vehicle["wheelbase"] = p["wheelbase_front"] + p["wheelbase_rear"]
    optim = {k: p[k] for k in OPTIM}
    optim.update(var_friction=opts.get("friction"), n_gauss=int(opts.get("n_gauss", 0)), dn=0.25, safe_traj=bool(opts.get("safe_traj")),
                 limit_energy=bool(opts.get("limit_energy")), warm_start=False, step_non_reg=3 if nonreg else 0, eps_kappa=1e-3)
    return dict(veh_params={k: p[k] for k in VEH}, vehicle_params_mintime=vehicle, tire_params_mintime={k: p[k] for k in TIRE}, optim_opts=optim,
                stepsize_opts=dict(stepsize_reg=float(stepsize)),
                curv_calc_opts=dict(d_preview_curv=2.0, d_review_curv=2.0, d_preview_head=1.0, d_review_head=1.0),
                pwr_params_mintime=dict(pwr_behavior=False))


class Trace:
    """What one run built.  point(values) binds the NLP's leaves; nlp / outputs evaluate in any scalar type (casadi_trace.Ops)."""

    def __init__(self, solver, functions, export, returned, dtype):
        self.solver, self.functions, self.export, self.returned, self.dtype = solver, functions, export, returned, dtype
        self.nw, self.ng = len(solver.x), len(solver.g)

    def nlp(self, ops, w):
        """(J, [g_i]) at the scalars w [nw] of ops' type: one pass over the graph of both"""
        binding = {id(leaf): x for leaf, x in zip(self.solver.x.items, w)}
        vals = ct.evaluate([self.solver.f] + self.solver.g.items, binding, ops)
        return vals[0], vals[1:]

    def outputs(self, ops, w):
        """{name: [scalars]} of the reference's f_sol at w"""
        res = self.functions["f_sol"].eval([ct.Vec(w)], ops, lambda a: a)
        return {k: v for k, (v, _) in zip(FSOL, res)}

    def numbers(self, w):
        """g, J and the f_sol outputs as arrays of the run's dtype, with the lap time and the energy as the running sums the reference's own
        post-processing forms (cumsum: from the first interval on)"""
        t, ops = self.dtype, ct.number_ops(self.dtype)
        pt = [t(x) for x in w]
        J, g = self.nlp(ops, pt)
        out = {k: np.array(v, dtype=t) for k, v in self.outputs(ops, pt).items()}
        N = out["dt_opt"].shape[0]
        out.update(g=np.array(g, dtype=t), J=t(J), lap_time=np.cumsum(out["dt_opt"])[-1], energy=np.cumsum(out["ec_opt"])[-1] / t(3600000.0),
                   x_opt=out["x_opt"].reshape(N + 1, 5), u_opt=out["u_opt"].reshape(N, 4), tf_opt=out["tf_opt"].reshape(N, 12))
        return out

    def bounds(self):
        c = self.solver.call
        return tuple(np.asarray(c[k]) for k in ("x0", "lbx", "ubx", "lbg", "ubg"))


def _load(path):
    spec = importlib.util.spec_from_file_location("_reference_opt_mintime", path)
    mod = importlib.util.module_from_spec(spec)
    keep = sys.dont_write_bytecode
    sys.dont_write_bytecode = True           # the reference tree is read, never written
    try:
        spec.loader.exec_module(mod)
    finally:
        sys.dont_write_bytecode = keep
    return mod


def run(setup, dtype=np.float64, ref_dir=None, scale=None):
    """One run of the reference's opt_mintime.  setup: flat (the 40 parameters), opts, stepsize, reftrack [n, 4] (the track handed in), kappa [N],
    w [5 + 24 N], lam_x, lam_g, with a friction model w_mue [4, N + 1, P] (and center_dist [N + 1]), and for non-regular sampling sampled [N, 4]
    and discr_points [N].  scale: {parameter: factor} applied to the flat parameters of this run alone.  Returns a Trace."""
    path = source_path(ref_dir)
    if not os.path.isfile(path):
        raise FileNotFoundError(path)
    flat = dict(setup["flat"])
    for k, f in (scale or {}).items():
        flat[k] = flat[k] * f
    nonreg = setup.get("sampled") is not None
    pars = nested_pars(flat, setup["opts"], setup["stepsize"], nonreg, (lambda v: LD(v)) if dtype is LD else float)
    reftrack = np.array(setup["reftrack"], dtype=np.float64)
    kappa = np.array(setup["kappa"], dtype=np.float64)
    captured = {}

    def calc_head_curv_num(path, el_lengths, is_closed, **kw):
        assert is_closed and np.asarray(path).shape[0] == kappa.shape[0]
        return np.zeros(kappa.shape[0]), kappa.copy()

    def nonreg_sampling(track, eps_kappa, step_non_reg):
        assert np.array_equal(track, reftrack)
        return np.array(setup["sampled"], dtype=np.float64), np.array(setup["discr_points"])

    def approx_friction_map(reftrack, normvectors, tpamap_path, tpadata_path, pars, dn, n_gauss, print_debug, plot_debug):
        wm = np.asarray(setup["w_mue"], dtype=np.float64).astype(dtype)
        cd = setup.get("center_dist")
        cd = np.zeros((wm.shape[1], 1)) if cd is None else np.asarray(cd, dtype=np.float64).astype(dtype)[:, None]
        return wm[0], wm[1], wm[2], wm[3], cd

    def export_mintime_solution(**kw):
        captured.update(kw)

    pkg = importlib.import_module("global_racetrajectory_optimization_amd.trajectory_planning_helpers")
    tph = types.ModuleType("trajectory_planning_helpers")
    tph.calc_splines, tph.calc_spline_lengths = pkg.calc_splines, pkg.calc_spline_lengths
    tph.calc_head_curv_num = types.SimpleNamespace(calc_head_curv_num=calc_head_curv_num)
    tph.nonreg_sampling = types.SimpleNamespace(nonreg_sampling=nonreg_sampling)
    omt = types.ModuleType("opt_mintime_traj")
    omt.src = types.SimpleNamespace(approx_friction_map=types.SimpleNamespace(approx_friction_map=approx_friction_map),
                                    export_mintime_solution=types.SimpleNamespace(export_mintime_solution=export_mintime_solution))
    seeded = {"casadi": ct, "trajectory_planning_helpers": tph, "opt_mintime_traj": omt}
    saved = {k: sys.modules.get(k) for k in seeded}
    ct.configure(dtype, setup["w"], setup["lam_x"], setup["lam_g"])
    try:
        sys.modules.update(seeded)
        mod = _load(path)
        n = reftrack.shape[0]
        returned = mod.opt_mintime(reftrack=reftrack, coeffs_x=np.zeros((n, 4)), coeffs_y=np.zeros((n, 4)), normvectors=np.zeros((n, 2)), pars=pars,
                                   tpamap_path="", tpadata_path="", export_path="", print_debug=False, plot_debug=False)
        solver, functions = ct.record()
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return Trace(solver, functions, captured, returned, dtype)
