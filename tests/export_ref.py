"""A plain restatement of the reference's EXPORT block [REF main_globaltraj.py:502-552, helper_funcs_glob/src/export_traj_ltpl.py:35-63]: what
mcq_export_device is tested against.  The raceline's spline and its lengths come from tests/glue_ref.py in the dtype asked for (numpy.longdouble is
THE reference); the lookup is literally numpy.abs(col - s).argmin().  Per waypoint the lookup also returns its MARGIN: with c1 / c2 the stations
either side of s (c1 the last below s, c2 the first not below), | |s_c1 - s| - |s_c2 - s| |, infinite where only one of them exists: how far s
may move before the index changes."""
import numpy as np

import glue_ref

LD = np.longdouble
LTPL_COLS = 12


def front(ref, nv, alpha, dtype=LD):
    """dict(lengths [n], s_ref [n + 1], total) of one ring in `dtype`: spline_lengths_opt, its running sum from 0, the sum's last value."""
    fr = glue_ref.front(ref, nv, alpha, dtype)
    s_ref = np.concatenate((np.zeros(1, dtype=dtype), fr["cum"]))
    return dict(lengths=fr["lengths"], s_ref=s_ref, total=s_ref[-1])


def front_variants(ref, nv, alpha):
    """float64 restatements of front() in other evaluation and summation orders (what the spread of s_ref / spline_total is taken over):
    the plain float64 run; the segments' points in power form (a + b t + c t^2 + d t^3) with the running sum taken from the far end
    (total - reversed running sum); the c-coefficients by the closed-form convolution with the inverse of circ(1, 4, 1) and pairwise partial sums."""
    f64 = np.float64
    out = [front(ref, nv, alpha, f64)]
    fr = glue_ref.front(ref, nv, alpha, f64)
    a, b, c, d = fr["coef"]

    def lengths_power(a, b, c, d):
        t = (np.arange(15, dtype=f64) / 14.0)[None, :, None]
        pts = a[:, None, :] + b[:, None, :] * t + c[:, None, :] * t * t + d[:, None, :] * t * t * t
        ch = np.diff(pts, axis=1)
        return np.sum(np.hypot(ch[..., 0], ch[..., 1]), axis=1)
    L = lengths_power(a, b, c, d)
    tot = np.sum(L)
    rev = np.cumsum(L[::-1])[::-1]                        # sum of L[i:]
    s_ref = np.concatenate((tot - rev, [tot]))
    s_ref[0] = 0.0
    out.append(dict(lengths=L, s_ref=s_ref, total=tot))
    # c by convolution with the periodic inverse of circ(1, 4, 1): c_i = sc (sum_(k>=0) lam^k rhs_(i+k) + sum_(j>=1) lam^j rhs_(i-j)), sc = A / (1 - lam^n),
    # lam = sqrt(3) - 2, A = 1 / (4 + 2 lam); both sums over one turn of the ring, cut where lam^k is below 1e-40
    P = np.asarray(a, dtype=f64)
    n = P.shape[0]
    rhs = 3.0 * ((np.roll(P, -1, axis=0) - P) - (P - np.roll(P, 1, axis=0)))
    lam = np.sqrt(3.0) - 2.0
    sc = 1.0 / (4.0 + 2.0 * lam) / (1.0 - lam ** n)
    cc = np.zeros_like(P)
    for k in range(min(n, 72) - 1, -1, -1):              # smallest terms first
        cc += (sc * lam ** k) * np.roll(rhs, -k, axis=0)
    for k in range(min(n, 72), 0, -1):
        cc += (sc * lam ** k) * np.roll(rhs, k, axis=0)
    cn = np.roll(cc, -1, axis=0)
    D = np.roll(P, -1, axis=0) - P
    bb = D - (2.0 * cc + cn) / 3.0
    dd = (cn - cc) / 3.0
    L2 = lengths_power(P, bb, cc, dd)
    half = n // 2
    c1, c2 = np.cumsum(L2[:half]), np.cumsum(L2[half:])
    s2 = np.concatenate(([0.0], c1, (c1[-1] if half else 0.0) + c2))
    out.append(dict(lengths=L2, s_ref=s2, total=s2[-1]))
    return out


def lookup(col, s_ref):
    """(idx [n], margin [n], c1 [n], c2 [n]) of the queries s_ref [n] on the stations col [m]; c1 / c2 are -1 where they do not exist."""
    col = np.asarray(col)
    m = col.shape[0]
    idx = np.array([int(np.abs(col - s).argmin()) for s in s_ref], dtype=np.int64)
    lo = np.searchsorted(col.astype(s_ref.dtype), s_ref, side="left")
    c1 = lo - 1
    c2 = np.where(lo < m, lo, -1)
    both = (c1 >= 0) & (c2 >= 0)
    d1 = np.abs(col[np.maximum(c1, 0)] - s_ref)
    d2 = np.abs(col[np.maximum(c2, 0)] - s_ref)
    margin = np.where(both, np.abs(d1 - d2), np.inf).astype(np.float64)
    return idx, margin, c1, c2


def table(ref, nv, alpha, traj, dtype=LD):
    """The EXPORT block for one variant: traj (m, 7).  dict(ltpl (n + 1, 12) float64 = traj_ltpl_cl, idx, margin, c1, c2, lengths, s_ref, total,
    race_cl (m + 1, 7) with upstream's numpy.sum of the lengths in its last s)."""
    ref, nv, alpha, traj = (np.asarray(a, dtype=np.float64) for a in (ref, nv, alpha, traj))
    fr = front(ref, nv, alpha, dtype)
    idx, margin, c1, c2 = lookup(traj[:, 0], fr["s_ref"][:-1])
    ltpl = np.column_stack((ref[:, :4], nv, alpha, fr["s_ref"][:-1].astype(np.float64), traj[idx, 3], traj[idx, 4], traj[idx, 5], traj[idx, 6]))
    ltpl_cl = np.vstack((ltpl, ltpl[0]))
    ltpl_cl[-1, 7] = np.float64(fr["total"])
    race_cl = np.vstack((traj, traj[0]))
    race_cl[-1, 0] = np.float64(np.sum(fr["lengths"]))
    return dict(ltpl=ltpl_cl, idx=idx, margin=margin, c1=c1, c2=c2, lengths=fr["lengths"], s_ref=fr["s_ref"], total=fr["total"], race_cl=race_cl)


def rule(col, s):
    """The entry's lookup rule (include/mcq.h), for the hand-made tables: bisection, the nearer candidate, then downwards over equal distances."""
    m = len(col)
    lo = int(np.searchsorted(col, s, side="left"))
    c1, c2 = lo - 1, lo
    if c1 < 0:
        idx = c2
    elif c2 >= m:
        idx = c1
    else:
        idx = c1 if abs(col[c1] - s) <= abs(col[c2] - s) else c2
    while idx > 0 and abs(col[idx - 1] - s) == abs(col[idx] - s):
        idx -= 1
    return idx
