"""One plain reference for the device kernels AROUND the QP (csrc/mcq_kernels.hip: mcq_relinearise_kernel, mcq_raceline_kernel, the derive branch
of assemble_problem behind mcq_prep_device, mcq_normals_crossing_kernel, the fp32 boundary kernels), written from the maths of DESIGN.md /
include/mcq.h: numpy, O(n), no structure shared with the kernels (no closed-form inverse, no truncated convolution, no chunked sums).

Every function takes a `dtype` and runs the same statements in np.float64 and np.longdouble (80-bit on x86: eps 1.1e-19); the longdouble run is
the reference, the float64 run measures how far the maths itself is determined in the engine's number format (tests/glue_guard.py).

The closed cubic spline.  Segment i runs from P_i to P_(i+1) with t in [0, 1]:  a + b t + c t^2 + d t^3.  tph.calc_splines' joint conditions
b_i + 2 c_i + 3 d_i = s_i b_(i+1),  2 c_i + 6 d_i = 2 s_i^2 c_(i+1)  with s_i = l_i / l_(i+1) say: the curve is C2 in the parameter u = l_i t.
So with M_i = 2 c_i / l_i^2 (second derivative in u at joint i) the textbook periodic system holds,
    l_(i-1) M_(i-1) + 2 (l_(i-1) + l_i) M_i + l_i M_(i+1) = 6 ((P_(i+1) - P_i) / l_i - (P_i - P_(i-1)) / l_(i-1)),
and c_i = M_i l_i^2 / 2,  d_i = (M_(i+1) - M_i) l_i^2 / 6,  b_i = (P_(i+1) - P_i) - c_i - d_i.  Unit scalings (the glue, the raceline): l = 1;
distance scalings (prep): l_i = |P_(i+1) - P_i|.  Cyclic tridiagonal: Thomas + Sherman-Morrison, a dense elimination below n = 8.

Values at a station are compared, never segment indices: the curve is C2, so a station on a joint is no edge for this reference."""
import math

import numpy as np

LD = np.longdouble


def pi_of(dtype):
    return dtype(4) * np.arctan(dtype(1))


def _gauss(A, B):
    """Dense solve with partial pivoting in A's dtype (numpy.linalg has no longdouble); B [n, k]."""
    A = A.copy()
    B = B.copy()
    n = A.shape[0]
    for k in range(n):
        p = k + int(np.argmax(np.abs(A[k:, k])))
        if p != k:
            A[[k, p]] = A[[p, k]]
            B[[k, p]] = B[[p, k]]
        for r in range(k + 1, n):
            f = A[r, k] / A[k, k]
            A[r, k:] -= f * A[k, k:]
            B[r] -= f * B[k]
    X = np.zeros_like(B)
    for k in range(n - 1, -1, -1):
        X[k] = (B[k] - A[k, k + 1:] @ X[k + 1:]) / A[k, k]
    return X


def _thomas(sub, diag, sup, B):
    """Tridiagonal solve: sub[i] x[i-1] + diag[i] x[i] + sup[i] x[i+1] = B[i] (sub[0], sup[-1] unused); B [n, k]."""
    n = diag.shape[0]
    cp = np.zeros_like(diag)
    Bp = np.zeros_like(B)
    cp[0] = sup[0] / diag[0]
    Bp[0] = B[0] / diag[0]
    for i in range(1, n):
        den = diag[i] - sub[i] * cp[i - 1]
        cp[i] = sup[i] / den
        Bp[i] = (B[i] - sub[i] * Bp[i - 1]) / den
    X = np.zeros_like(B)
    X[n - 1] = Bp[n - 1]
    for i in range(n - 2, -1, -1):
        X[i] = Bp[i] - cp[i] * X[i + 1]
    return X


def cyclic_tridiag_solve(sub, diag, sup, B):
    """sub[i] x[i-1] + diag[i] x[i] + sup[i] x[i+1] = B[i], indices modulo n."""
    n = diag.shape[0]
    dt = diag.dtype.type
    if n < 8:
        A = np.zeros((n, n), dtype=dt)
        for i in range(n):
            A[i, i] += diag[i]
            A[i, (i - 1) % n] += sub[i]
            A[i, (i + 1) % n] += sup[i]
        return _gauss(A, B)
    # A = T + u v',  u = (g, 0, .., 0, sub[0])... with the two corners moved into a rank-one term (Sherman-Morrison)
    g = -diag[0]
    d2 = diag.copy()
    d2[0] -= g
    d2[n - 1] -= sup[n - 1] * sub[0] / g
    u = np.zeros((n, 1), dtype=dt)
    u[0, 0] = g
    u[n - 1, 0] = sup[n - 1]
    Y = _thomas(sub, d2, sup, np.concatenate((B, u), axis=1))
    y, z = Y[:, :-1], Y[:, -1]
    vy = y[0] + (sub[0] / g) * y[n - 1]
    vz = z[0] + (sub[0] / g) * z[n - 1]
    return y - np.outer(z, vy / (dt(1) + vz))


def closed_spline(P, dtype, dist_scaling=False):
    """Coefficients (a, b, c, d), each [n, 2], of the closed cubic spline through the ring P [n, 2], and the scalings s_i = l_i / l_(i+1)."""
    P = np.asarray(P, dtype=dtype)
    n = P.shape[0]
    D = np.roll(P, -1, axis=0) - P
    l = np.sqrt(D[:, 0] ** 2 + D[:, 1] ** 2) if dist_scaling else np.ones(n, dtype=dtype)
    lm = np.roll(l, 1)
    rhs = dtype(6) * (D / l[:, None] - np.roll(D, 1, axis=0) / lm[:, None])
    M = cyclic_tridiag_solve(lm, dtype(2) * (lm + l), l, rhs)
    l2 = (l * l)[:, None]
    c = M * l2 / dtype(2)
    d = (np.roll(M, -1, axis=0) - M) * l2 / dtype(6)
    b = D - c - d
    return (P, b, c, d), l / np.roll(l, -1)


def normals_of(coef):
    """Unit normals pointing right: the tangent at the joint rotated clockwise, (b_y, -b_x) / |b|."""
    b = coef[1]
    nrm = np.sqrt(b[:, 0] ** 2 + b[:, 1] ** 2)
    return np.stack((b[:, 1] / nrm, -b[:, 0] / nrm), axis=1)


def spline_lengths(coef, dtype):
    """15 points per segment, the sum of the 14 chords (tph.calc_spline_lengths)."""
    a, b, c, d = coef
    t = (np.arange(15, dtype=dtype) / dtype(14))[None, :, None]
    pts = a[:, None, :] + t * (b[:, None, :] + t * (c[:, None, :] + t * d[:, None, :]))
    ch = np.diff(pts, axis=1)
    return np.sum(np.sqrt(ch[..., 0] ** 2 + ch[..., 1] ** 2), axis=1)


def running_sum(x):
    return np.cumsum(x)                 # sequential in x's dtype


def point_count(total, stepsize, dtype):
    """(no_interp_points - 1, total / stepsize): tph.interp_splines keeps ceil(total / stepsize) + 1 points less the closing one."""
    r = dtype(total) / dtype(stepsize)
    return int(math.ceil(r)), r


def _eval(coef, cum, lengths, q, dtype):
    n = lengths.shape[0]
    s = np.minimum(np.searchsorted(cum, q, side="right"), n - 1)
    start = np.where(s > 0, cum[np.maximum(s - 1, 0)], dtype(0))
    t = (q - start) / lengths[s]
    a, b, c, d = (k[s] for k in coef)
    tt = t[:, None]
    xy = a + tt * (b + tt * (c + tt * d))
    d1 = b + tt * (dtype(2) * c + dtype(3) * tt * d)
    d2 = dtype(2) * c + dtype(6) * tt * d
    return s, t, xy, d1, d2


def front(ref, nv, alpha, dtype, alpha_scale=1.0):
    """What does not depend on the stepsize: the closed unit-scaling spline through ref + alpha_scale alpha nv, its lengths, their running
    sum, and the widths shifted by -/+ alpha_scale alpha."""
    ref = np.asarray(ref, dtype=dtype)
    a = dtype(alpha_scale) * np.asarray(alpha, dtype=dtype)
    P = ref[:, :2] + a[:, None] * np.asarray(nv, dtype=dtype)
    coef, _ = closed_spline(P, dtype)
    L = spline_lengths(coef, dtype)
    cum = running_sum(L)
    return dict(coef=coef, lengths=L, cum=cum, total=cum[-1], wr=ref[:, 2] - a, wl=ref[:, 3] + a, dtype=dtype)


def stations(fr, stepsize):
    """mcq_raceline_device's outputs (tph.create_raceline + calc_head_curv_an) for one stepsize, from front()'s result.  Returns a dict:
    m (points kept), ratio (total / stepsize), total, xy [m, 2], psi, kappa, el_lengths [m], seg / t (segment and parameter per station)."""
    dtype, total = fr["dtype"], fr["total"]
    m, ratio = point_count(total, stepsize, dtype)
    out = dict(m=m, ratio=ratio, total=total)
    if m < 1:
        return out
    q = np.arange(m, dtype=dtype) * total / dtype(m)
    s, t, xy, d1, d2 = _eval(fr["coef"], fr["cum"], fr["lengths"], q, dtype)
    pi = pi_of(dtype)
    psi = np.arctan2(d1[:, 1], d1[:, 0]) - pi / dtype(2)
    psi = np.where(psi >= pi, psi - dtype(2) * pi, np.where(psi < -pi, psi + dtype(2) * pi, psi))
    v2 = d1[:, 0] ** 2 + d1[:, 1] ** 2
    kappa = (d1[:, 0] * d2[:, 1] - d1[:, 1] * d2[:, 0]) / (v2 * np.sqrt(v2))
    el = np.append(np.diff(q), total - q[-1])
    out.update(xy=xy, psi=psi, kappa=kappa, el_lengths=el, seg=s, t=t)
    return out


def raceline(ref, nv, alpha, stepsize, dtype, alpha_scale=1.0):
    return stations(front(ref, nv, alpha, dtype, alpha_scale), stepsize)


def resample(fr, stepsize):
    """mcq_relinearise_device's outputs for one stepsize, from front()'s result: m, rows [m, 4] = (x, y, w_right, w_left) of the re-sampled
    ring -- the widths carried over linearly between the ends of a station's segment -- and the unit normals [m, 2] of the closed
    unit-scaling spline through the new ring."""
    r = stations(fr, stepsize)
    if r["m"] < 3:
        return dict(m=r["m"], ratio=r["ratio"])
    s, t = r["seg"], r["t"]
    sp = (s + 1) % fr["lengths"].shape[0]
    wr = fr["wr"][s] + (fr["wr"][sp] - fr["wr"][s]) * t
    wl = fr["wl"][s] + (fr["wl"][sp] - fr["wl"][s]) * t
    coef, _ = closed_spline(r["xy"], fr["dtype"])
    return dict(m=r["m"], ratio=r["ratio"], rows=np.column_stack((r["xy"], wr, wl)), normals=normals_of(coef))


def relinearise(ref, nv, alpha, alpha_scale, stepsize, dtype):
    return resample(front(ref, nv, alpha, dtype, alpha_scale), stepsize)


def prep(xy, dtype):
    """mcq_prep_device: unit normals and scalings s_i = l_i / l_(i+1) of the closed distance-scaled spline through the reference line."""
    coef, s = closed_spline(np.asarray(xy, dtype=dtype)[:, :2], dtype, dist_scaling=True)
    return normals_of(coef), s


# ---- the fp32 boundary (include/mcq.h: MCQ_F32_ABSOLUTE / MCQ_F32_INCREMENTS) ----------------------------------------------------------
def rows_absolute(rows32, origin, dtype):
    r = np.asarray(rows32).astype(dtype)
    if origin is not None:
        r[..., :2] += np.asarray(origin, dtype=dtype)[..., None, :]
    return r


def rows_increments(rows32, origin, dtype):
    """x, y rebuilt as a running sum of the increments from the origin, the closure defect (sum of the increments) spread evenly:
    x_i = o + sum_(k < i) inc_k - i * defect / n."""
    r = np.asarray(rows32).astype(dtype)
    n = r.shape[-2]
    inc = r[..., :2]
    defect = np.sum(inc, axis=-2, keepdims=True) / dtype(n)
    cs = np.cumsum(inc, axis=-2)
    xy = np.concatenate((np.zeros_like(cs[..., :1, :]), cs[..., :-1, :]), axis=-2) - np.arange(n, dtype=dtype)[:, None] * defect
    if origin is not None:
        xy = xy + np.asarray(origin, dtype=dtype)[..., None, :]
    return np.concatenate((xy, r[..., 2:]), axis=-1)


# ---- tph.check_normals_crossing -----------------------------------------------------------------------------------------------------------
COLLINEAR = 1e-8            # numpy.isclose(cross, 0.0): |cross| <= atol


def normals_crossing(track, nv, horizon, dtype, wrap=True):
    """(verdict, margin).  verdict 1 / 0, or -1 where tph raises (horizon >= n).  margin: over every pair (i, i + d), d = 1 .. horizon, the
    smallest distance of a quantity from the threshold that decides about it -- |cross| from 1e-8; for a pair that is not skipped, the
    distance of the deciding parameter from its bound (a hit: the nearest bound of the four; no hit: the largest violation).
    wrap=False leaves out the pairs that reach across the end of the arrays (what a search without the wrap would see)."""
    track = np.asarray(track, dtype=dtype)
    nv = np.asarray(nv, dtype=dtype)
    n = track.shape[0]
    if n < 2 or horizon >= n:
        return -1, np.inf
    verdict, margin = 0, np.inf
    for d in range(1, horizon + 1):
        j = (np.arange(n) + d) % n
        a, b = nv, nv[j]
        cross = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
        margin = min(margin, float(np.min(np.abs(np.abs(cross) - dtype(COLLINEAR)))))
        keep = np.abs(cross) > dtype(COLLINEAR)
        if not wrap:
            keep &= np.arange(n) + d < n
        if not np.any(keep):
            continue
        r = track[j, :2] - track[:, :2]
        det = np.where(keep, -cross, dtype(1))
        l0 = (-r[:, 0] * b[:, 1] + r[:, 1] * b[:, 0]) / det
        l1 = (a[:, 0] * r[:, 1] - a[:, 1] * r[:, 0]) / det
        slack = np.stack((l0 + track[:, 3], track[:, 2] - l0, l1 + track[j, 3], track[j, 2] - l1))       # all >= 0: a hit
        worst = np.min(slack, axis=0)
        if np.any(keep & (worst >= 0)):
            verdict = 1
        margin = min(margin, float(np.min(np.abs(worst[keep]))))
    return verdict, margin
