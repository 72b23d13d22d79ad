"""A plain restatement of what the reference runs on a finished raceline -- calc_ax_profile, the time profile (the project's stable form,
oracle/vel_ref.lap_time_stable), the trajectory rows, and check_traj with its two helpers interp_track and calc_min_bound_dists
[REF main_globaltraj.py:412-421, 502-534; helper_funcs_glob/src/check_traj.py, interp_track.py, calc_min_bound_dists.py] -- parametrised by
dtype: numpy.longdouble is THE reference of tests/traj_check_checks.py, numpy.float64 is for spreads and for the comparison with the arrays
recorded from the reference's own functions (tests/test_traj_check_ref.py).  No device code, no engine.

numpy.interp and numpy.linspace work in float64 only, so both are written out: linspace(0, total, N)[j] = j * (total / (N - 1)); interp =
slope * (x - xp[k]) + fp[k] with slope = (fp[k+1] - fp[k]) / (xp[k+1] - xp[k]) on the last k with xp[k] <= x."""
import math

import numpy as np

LD = np.longdouble
ACC_MARGIN = 0.1            # MCQ_CHECK_ACC_MARGIN
CHK = dict(kappa=1, ay=2, ax_pos=4, ax_neg=8, a_tot=16, machines=32, v_max=64)
LIMITS = ("kappa", "ay", "ax_pos", "ax_neg", "a_tot", "vx")


def boundaries(reftrack, normvec, dtype):
    """(bound_r, bound_l) [n, 2]."""
    r, nv = np.asarray(reftrack).astype(dtype), np.asarray(normvec).astype(dtype)
    return r[:, :2] + nv * r[:, 2:3], r[:, :2] - nv * r[:, 3:4]


def interp_track(points, stepsize, dtype, info=None):
    """interp_track on the two coordinate columns of a closed polyline: [nb, 2], the closing sample dropped.  info (dict) receives `ratio` =
    total / stepsize (how far the sample count is from flipping) and `el_min`."""
    p = np.asarray(points).astype(dtype)
    cl = np.vstack((p, p[:1]))
    el = np.sqrt(np.sum(np.power(np.diff(cl, axis=0), 2), axis=1))
    cum = np.concatenate((np.zeros(1, dtype=dtype), np.cumsum(el)))
    total = cum[-1]
    ratio = total / dtype(stepsize)
    num = int(math.ceil(ratio)) + 1
    if info is not None:
        info["ratio"], info["el_min"] = ratio, float(np.min(el))
    x = np.arange(num - 1).astype(dtype) * (total / dtype(num - 1))
    k = np.clip(np.searchsorted(cum, x, side="right") - 1, 0, p.shape[0] - 1)
    slope = (cl[k + 1] - cl[k]) / (cum[k + 1] - cum[k])[:, None]
    return slope * (x - cum[k])[:, None] + cl[k]


def corners(xy, psi, length_veh, width_veh, dtype):
    """[m, 4, 2]: front left, front right, rear left, rear right of the vehicle at every station (heading 0 = north, the length along y)."""
    xy, psi = np.asarray(xy).astype(dtype), np.asarray(psi).astype(dtype)
    hw, hl = dtype(width_veh) / 2, dtype(length_veh) / 2
    c, s = np.cos(psi), np.sin(psi)
    out = np.zeros((xy.shape[0], 4, 2), dtype=dtype)
    for q, (ox, oy) in enumerate(((-hw, hl), (hw, hl), (-hw, -hl), (hw, -hl))):
        out[:, q, 0] = xy[:, 0] + (c * ox - s * oy)
        out[:, q, 1] = xy[:, 1] + (s * ox + c * oy)
    return out


def min_bound_dists(xy, psi, bound1, bound2, length_veh, width_veh, dtype):
    """calc_min_bound_dists: per station the smallest distance of a corner to a point of either boundary."""
    b = np.vstack((bound1, bound2)).astype(dtype)
    cr = corners(xy, psi, length_veh, width_veh, dtype)
    out = np.zeros(cr.shape[0], dtype=dtype)
    for i in range(cr.shape[0]):
        d = np.sqrt(np.power(b[None, :, 0] - cr[i, :, 0, None], 2) + np.power(b[None, :, 1] - cr[i, :, 1, None], 2))
        out[i] = np.min(d)
    return out


def bound_dists(reftrack, normvec, xy, psi, length_veh, width_veh, stepsize_bound=1.0, first_row_only=False, dtype=LD):
    """check_traj's first block.  first_row_only: against the first sample of each boundary, which is what the reference's own call computes."""
    br, bl = boundaries(reftrack, normvec, dtype)
    ir, il = {}, {}
    sr, sl = interp_track(br, stepsize_bound, dtype, ir), interp_track(bl, stepsize_bound, dtype, il)
    nb = (sr.shape[0], sl.shape[0])
    if first_row_only:
        sr, sl = sr[:1], sl[:1]
    md = min_bound_dists(xy, psi, sr, sl, length_veh, width_veh, dtype)
    return dict(min_dists=md, min_dist=np.min(md), nb=nb, bound_r=br, bound_l=bl, samples_r=sr, samples_l=sl,
                ratios=(ir["ratio"], il["ratio"]), el_min=min(ir["el_min"], il["el_min"]))


def trajectory(xy, psi, kappa, el_lengths, vx, closed, dtype):
    """Rows [s, x, y, psi, kappa, vx, ax] of m stations, the times t [ne + 1] (stable form: t_(i+1) = t_i + 2 l_i / (v_i + v_(i+1))) and the
    length.  closed: m elements, v_m := v_0; unclosed: m - 1 elements and a 0 in the last row's ax (eq_length_output=True)."""
    vx = np.asarray(vx).astype(dtype)
    m = vx.shape[0]
    ne = m if closed else m - 1
    el = np.asarray(el_lengths).astype(dtype)[:ne]
    v_cl = np.append(vx, vx[0]) if closed else vx
    ax = np.zeros(m, dtype=dtype)
    ax[:ne] = (np.power(v_cl[1:], 2) - np.power(v_cl[:-1], 2)) / (2 * el)
    cum = np.cumsum(el)
    s = np.concatenate((np.zeros(1, dtype=dtype), cum))[:m]
    t = np.concatenate((np.zeros(1, dtype=dtype), np.cumsum(2 * el / (v_cl[:-1] + v_cl[1:]))))
    rows = np.column_stack((s, np.asarray(xy).astype(dtype), np.asarray(psi).astype(dtype), np.asarray(kappa).astype(dtype), vx, ax))
    return dict(traj=rows, t=t, length=cum[-1])


def limits(traj, drag_coeff, m_veh, dtype):
    """The six quantities check_traj tests: max |kappa|, max ay, max / min ax_wo_drag, max a_tot, max vx."""
    kap, vx, ax = traj[:, 4], traj[:, 5], traj[:, 6]
    radii = np.abs(np.divide(dtype(1), kap, out=np.full(kap.shape[0], np.inf, dtype=dtype), where=kap != 0))
    ay = np.power(vx, 2) / radii
    ax_wo = ax - (-np.power(vx, 2) * dtype(drag_coeff) / dtype(m_veh))
    a_tot = np.sqrt(np.power(ax_wo, 2) + np.power(ay, 2))
    return np.array([np.max(np.abs(kap)), np.max(ay), np.max(ax_wo), np.min(ax_wo), np.max(a_tot), np.max(vx)], dtype=dtype)


def verdicts(lim, ggv, ax_max_machines, v_max, curvlim, dtype):
    """(flags, gaps): check_traj's seven tests on the limit quantities, and for each test made the distance of the quantity from its threshold
    relative to the threshold's size (how far the decision is from flipping)."""
    flags, gaps = 0, {}

    def test(name, value, thr, below=False):
        nonlocal flags
        thr = dtype(thr)
        if (value < thr) if below else (value > thr):
            flags |= CHK[name]
        gaps[name] = float(abs(value - thr) / max(abs(thr), dtype(1e-300)))
    test("kappa", lim[0], curvlim)
    if ggv is not None:
        g = np.asarray(ggv).astype(dtype)
        mg = dtype(ACC_MARGIN)
        test("ay", lim[1], np.max(g[:, 2]) + mg)
        test("ax_pos", lim[2], np.max(g[:, 1]) + mg)
        test("ax_neg", lim[3], np.min(-g[:, 1]) - mg, below=True)
        test("a_tot", lim[4], np.max(g[:, 1:]) + mg)
    if ax_max_machines is not None:
        test("machines", lim[2], np.max(np.asarray(ax_max_machines).astype(dtype)[:, 1]) + dtype(ACC_MARGIN))
    test("v_max", lim[5], dtype(v_max) + dtype(ACC_MARGIN))
    return flags, gaps
