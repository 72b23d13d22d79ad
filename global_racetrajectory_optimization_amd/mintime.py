"""The reference's names, arrays and files around the engine's minimum-time entries (Engine.mintime_*_batch; include/mcq.h "the minimum-time
optimal-control problem") [REF opt_mintime_traj/src/opt_mintime.py, export_mintime_solution.py].  The engine evaluates, differentiates and
certifies a decision vector w; it does not solve.  Names, headers and number formats are the boundary to the reference, as in export.py."""
import os

import numpy as np

from . import engine

EXPORT_FILES = ("states.csv", "controls.csv", "tire_forces.csv", "accelerations.csv", "w0.csv", "lam_x0.csv", "lam_g0.csv")
_VEH = ("mass", "dragcoeff", "g", "v_max")
_OPT = ("width_opt", "mue", "penalty_F", "penalty_delta", "energy_limit", "ax_pos_safe", "ax_neg_safe", "ay_safe")


def pars_from_ini(pars):
    """The reference's parsed `pars` dictionary -> (the parameter block as a dict of engine.MINTIME_PARS, the option keywords of the mintime_*
    methods).  A limit the file leaves null is NaN (it is read only with its option on); pwr_behavior true: NotImplementedError."""
    if pars.get("pwr_params_mintime", {}).get("pwr_behavior"):
        raise NotImplementedError("mintime: pwr_behavior (the powertrain's six thermal and charge states) is not implemented")
    oo = pars["optim_opts"]
    block = {k: pars["veh_params"][k] for k in _VEH}
    block.update({k: pars["vehicle_params_mintime"][k] for k in engine.MINTIME_PARS[4:22]})
    block.update({k: pars["tire_params_mintime"][k] for k in engine.MINTIME_PARS[22:32]})
    block.update({k: oo.get(k) for k in _OPT})
    block = {k: float("nan") if v is None else float(v) for k, v in block.items()}
    opts = dict(friction=oo.get("var_friction"), n_gauss=int(oo.get("n_gauss", 0)) if oo.get("var_friction") == "gauss" else 0,
                safe_traj=bool(oo.get("safe_traj")), limit_energy=bool(oo.get("limit_energy")))
    return block, opts


def problem_from_track(reftrack, kappa, stepsize, discr_points=None, no_points_orig=None, s_opt=None):
    """The reference's closing of the arrays (:99-117) for the track the NLP runs on.  Regular sampling (discr_points None): reftrack [N, 4] and
    kappa [N], stations k * stepsize.  Non-regular sampling: reftrack and kappa are the SAMPLED track (N rows, curvature recomputed on it, as the
    reference does behind tph.nonreg_sampling), discr_points [N] the indices the sampling kept and no_points_orig the point count of the track
    BEFORE sampling, which closes the lap: stations discr_points * stepsize, the last one no_points_orig * stepsize.  s_opt: N + 1 stations given
    outright, for a caller whose points are not equidistant (stepsize is not read).  Returns h [N], s_opt [N + 1] and kappa_cl, w_tr_right_cl,
    w_tr_left_cl [N + 1] with entry 0 repeated at the end."""
    reftrack, kappa = np.asarray(reftrack, dtype=np.float64), np.asarray(kappa, dtype=np.float64)
    n = reftrack.shape[0]
    if kappa.shape != (n,):
        raise ValueError("problem_from_track: kappa must hold one curvature per row of reftrack")
    if s_opt is None:
        if discr_points is None:
            discr, last = np.arange(n), n if no_points_orig is None else int(no_points_orig)
        else:
            discr = np.asarray(discr_points)
            if no_points_orig is None:
                raise ValueError("problem_from_track: discr_points needs no_points_orig, the point count before the sampling")
            last = int(no_points_orig)
        if discr.shape != (n,) or (n and last <= int(discr[-1])):
            raise ValueError("problem_from_track: discr_points must hold one index per row of the sampled reftrack, all below no_points_orig")
        s_opt = np.append(discr, last) * stepsize
    s_opt = np.asarray(s_opt, dtype=np.float64)
    if s_opt.shape != (n + 1,):
        raise ValueError("problem_from_track: s_opt must hold N + 1 stations")
    return dict(h=np.diff(s_opt), s_opt=s_opt, kappa_cl=np.append(kappa, kappa[0]), w_tr_right_cl=np.append(reftrack[:, 2], reftrack[0, 2]),
                w_tr_left_cl=np.append(reftrack[:, 3], reftrack[0, 3]))


def extract_solution(out, b=0):
    """Problem b of Engine.mintime_eval_batch's result in the reference's final arrays (:951-973): N + 1 rows of tire forces and accelerations whose
    row 0 is the LAST interval's (the lap closes), t_opt and the cumulative energy in Wh starting at 0, atot_opt, and the reference's return pair
    (alpha_opt = -n at the first N nodes, v_opt there)."""
    N = int(out["N"][b])
    x_opt, u_opt = out["x_opt"][b, :N + 1], out["u_opt"][b, :N]
    last_first = np.arange(-1, N) % N                   # N - 1, 0, 1, .., N - 1
    tf_opt = out["tf_opt"][b, :N][last_first]
    ax_opt, ay_opt = out["ax_opt"][b, :N][last_first], out["ay_opt"][b, :N][last_first]
    t_opt, ec_opt_cum = np.zeros(N + 1), np.zeros(N + 1)
    t_opt[1:] = np.cumsum(out["dt_opt"][b, :N])
    ec_opt_cum[1:] = np.cumsum(out["ec_opt"][b, :N])
    return dict(x_opt=x_opt, u_opt=u_opt, tf_opt=tf_opt, t_opt=t_opt, ax_opt=ax_opt, ay_opt=ay_opt, atot_opt=np.sqrt(ax_opt ** 2 + ay_opt ** 2),
                ec_opt_cum=ec_opt_cum / 3600.0, alpha_opt=-x_opt[:N, 3], v_opt=x_opt[:N, 0])


def export_mintime_solution(file_path, pars, s, t, x, u, tf, ax, ay, atot, w0, lam_x0, lam_g0, pwr=None):
    """The reference's seven files, byte for byte: states.csv, controls.csv, tire_forces.csv, accelerations.csv, w0.csv, lam_x0.csv, lam_g0.csv."""
    if pars["pwr_params_mintime"]["pwr_behavior"] or pwr is not None:
        raise NotImplementedError("mintime: pwr_behavior (the powertrain's six thermal and charge states) is not implemented")
    tables = (("states.csv", np.column_stack((s, t, x)), "%.1f; %.3f; %.2f; %.5f; %.5f; %.5f; %.5f",
               "s_m; t_s; v_mps; beta_rad; omega_z_radps; n_m; xi_rad"),
              ("controls.csv", np.column_stack((s[:-1], t[:-1], u)), "%.1f; %.3f; %.5f; %.1f; %.1f; %.1f",
               "s_m; t_s; delta_rad; f_drive_N; f_brake_N; gamma_y_N"),
              ("tire_forces.csv", np.column_stack((s, t, tf)), "%.1f; %.3f" + "; %.1f" * 12,
               "s_m; t_s; f_x_fl_N; f_y_fl_N; f_z_fl_N; f_x_fr_N; f_y_fr_N; f_z_fr_N;f_x_rl_N; f_y_rl_N; f_z_rl_N; f_x_rr_N;f_y_rr_N; f_z_rr_N;"),
              ("accelerations.csv", np.column_stack((s, t, ax, ay, atot)), "%.1f; %.3f; %.3f; %.3f; %.3f", "s_m; t_s; ax_mps2; ay_mps2; atot_mps2"))
    for name, table, fmt, header in tables:
        np.savetxt(os.path.join(file_path, name), table, fmt=fmt, header=header)
    for name, vec in (("w0.csv", w0), ("lam_x0.csv", lam_x0), ("lam_g0.csv", lam_g0)):
        np.savetxt(os.path.join(file_path, name), vec, delimiter=";")


def g_rows(N, safe_traj=False, limit_energy=False):
    """The rows of g of a problem of N intervals as (row0, ng, slots): row0 [N + 1] the first row of every interval and, at N, of the periodicity
    rows; slots[k] the row slots of block k that exist, in the order of their rows -- 0 .. 26, the actuator rows 27 .. 30 from interval 1 on, the
    pair 31, 32 with safe_traj alone."""
    safe, k = int(bool(safe_traj)), np.arange(int(N) + 1)
    row0 = k * (27 + 2 * safe) + 4 * np.maximum(k - 1, 0)
    slots = [list(range(27)) + (list(range(27, 31)) if j > 0 else []) + ([31, 32] if safe else []) for j in range(int(N))]
    return row0, int(row0[-1]) + 5 + int(bool(limit_energy)), slots


def jacobian_coo(blocks, N, safe_traj=False, grad_energy=None):
    """The interval blocks [>= N, 33, 33] of one problem -> the Jacobian of g as a scipy.sparse COO matrix [ng, nw] in the reference's row and column
    numbering: the blocks' present row slots, the constant periodicity rows (+1 at X_0, -1 at X_N), and with grad_energy [>= nw] the energy row."""
    import scipy.sparse as sp
    blocks = np.asarray(blocks)[:N]
    nw = 5 + 24 * N
    row0, ng, slots = g_rows(N, safe_traj, grad_energy is not None)
    per = int(row0[N])
    rows, cols, vals = [], [], []
    for k in range(N):
        colmap = np.concatenate((24 * k + np.arange(29), 24 * (k - 1) + 5 + np.arange(4)))
        ncol = 33 if k > 0 else 29
        sub = blocks[k][slots[k]][:, :ncol]
        r, c = np.nonzero(sub)
        rows.append(row0[k] + r)
        cols.append(colmap[c])
        vals.append(sub[r, c])
    rows += [per + np.arange(5), per + np.arange(5)]
    cols += [np.arange(5), 24 * N + np.arange(5)]
    vals += [np.ones(5), -np.ones(5)]
    if grad_energy is not None:
        ge = np.asarray(grad_energy)[:nw]
        c = np.flatnonzero(ge)
        rows.append(np.full(c.shape, per + 5))
        cols.append(c)
        vals.append(ge[c])
    return sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(ng, nw))


def hessian_slots(N, k):
    """the entries of w behind the 33 slots of Hessian block k: slots 0 .. 28 are w[24 k ..], slots 29 .. 32 are U_k-1 -- at k = 0 U_N-1"""
    return np.concatenate((24 * k + np.arange(29), 24 * ((k - 1) % N) + 5 + np.arange(4)))


def hessian_coo(hblocks, N, triangle="full"):
    """The Hessian blocks [>= N, 33, 33] of one problem (Engine.mintime_hess_batch) -> the Hessian of the Lagrangian as a scipy.sparse COO matrix
    [nw, nw] in the reference's numbering of w.  The overlaps of neighbouring blocks are added (COO duplicates sum on conversion), slots 29 .. 32 of
    block 0 go to U_N-1.  triangle "full", or "lower" (CasADi's hess_lag output is a triangle; rows >= columns here)."""
    import scipy.sparse as sp
    if triangle not in ("full", "lower"):
        raise ValueError("hessian_coo: triangle must be 'full' or 'lower'")
    hblocks = np.asarray(hblocks)[:N]
    nw = 5 + 24 * N
    rows, cols, vals = [], [], []
    for k in range(N):
        idx = hessian_slots(N, k)
        r, c = np.nonzero(hblocks[k])
        if triangle == "lower":
            keep = idx[r] >= idx[c]
            r, c = r[keep], c[keep]
        rows.append(idx[r])
        cols.append(idx[c])
        vals.append(hblocks[k][r, c])
    A = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(nw, nw))
    A.sum_duplicates()
    return A


def lagrangian_hessian(out, b=0, triangle="full"):
    """The Hessian of problem b of Engine.mintime_hess_batch's (or mintime_hessvec_batch's) result as a sparse matrix (hessian_coo)."""
    return hessian_coo(out["hblocks"][b], int(out["N"][b]), triangle)


def kkt_matrix(hblocks, blocks, N, dw, dg, safe_traj=False, grad_energy=None):
    """The regularised primal-dual matrix of one problem as a scipy.sparse CSC matrix [nw + ng, nw + ng] in the (w, lam_g) numbering that
    Engine.mintime_step_batch solves with: [[H + diag(dw), J^T], [J, -diag(dg)]], H from hessian_coo, J from jacobian_coo (with grad_energy [>= nw]
    the energy row is its last row), dw [>= nw] and dg [>= ng] the caller's diagonals."""
    import scipy.sparse as sp
    H = hessian_coo(hblocks, N)
    J = jacobian_coo(blocks, N, safe_traj, grad_energy)
    ng, nw = J.shape
    dw, dg = np.asarray(dw, dtype=np.float64)[:nw], np.asarray(dg, dtype=np.float64)[:ng]
    if dw.shape != (nw,) or dg.shape != (ng,):
        raise ValueError("kkt_matrix: dw must hold nw = %d entries and dg ng = %d" % (nw, ng))
    return sp.bmat([[H + sp.diags(dw), J.T], [J, -sp.diags(dg)]], format="csc")


def step_of(out, b=0, t=0):
    """Right-hand side t of problem b of Engine.mintime_step_batch's result as (x_w [nw], x_lam [ng]): the solution without its NaN tails."""
    N = int(out["N"][b])
    nw, ng = 5 + 24 * N, int(out["ng"][b])
    sol = out["sol"][b, t]
    off = int(out["nw_max"])
    return sol[:nw].copy(), sol[off:off + ng].copy()


def certificate(out, b=0):
    """The KKT maxima of problem b of Engine.mintime_kkt_batch's result as a dictionary."""
    k = out["kkt"][b]
    return dict(stationarity=float(k[0]), violation=float(k[1]), complementarity=float(k[2]), status=int(out["status"][b]))
