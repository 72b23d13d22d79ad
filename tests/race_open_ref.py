"""A plain reference for the chain form of the raceline kernel (csrc/mcq_kernels.hip: race_chain_body behind mcq_raceline_device_ends), written from
the formulas of include/mcq.h: numpy, O(n), no structure shared with the kernel (a Thomas sweep -- a dense elimination below n = 8 -- where the
kernel convolves a mirrored ring with a closed-form inverse; numpy.cumsum where it sums in chunks).

Every function takes a `dtype` and runs the same statements in np.float64 and np.longdouble; the longdouble run is THE reference, the float64 run
measures how far the maths itself is determined in the engine's number format (tests/race_open_guard.py).

The open cubic spline with unit scalings through P_0 .. P_(n-1), n >= 2, D_i = P_(i+1) - P_i, segment i: a + b t + c t^2 + d t^3 on [0, 1]:
    2 c_0 + c_1                 = 3 (D_0 - h_s)
    c_(m-1) + 4 c_m + c_(m+1)   = 3 (D_m - D_(m-1))        1 <= m <= n-2
    c_(n-2) + 2 c_(n-1)         = 3 (h_e - D_(n-2))
    a_i = P_i,   b_i = D_i - (2 c_i + c_(i+1)) / 3,   d_i = (c_(i+1) - c_i) / 3,   i <= n-2
with the heading rows' UNIT vectors h = HEADING_SCALE (cos(psi + pi/2), sin(psi + pi/2)) (MCQ_HEADING_SCALE = 1: the solver's rows).
c_(n-1) belongs to no segment: it is half the second derivative at the last point."""
import math

import numpy as np

import glue_ref

LD = np.longdouble
HEADING_SCALE = 1.0         # MCQ_HEADING_SCALE


def heading_vector(psi, dtype):
    a = dtype(psi) + glue_ref.pi_of(dtype) / dtype(2)
    return dtype(HEADING_SCALE) * np.array([np.cos(a), np.sin(a)], dtype=dtype)


def open_spline(P, psi_s, psi_e, dtype):
    """Coefficients (a, b, c, d), each [n - 1, 2], of the open unit-scaling spline through P [n, 2] with the end headings, and c_all [n, 2]."""
    P = np.asarray(P, dtype=dtype)
    n = P.shape[0]
    D = P[1:] - P[:-1]
    rhs = np.zeros((n, 2), dtype=dtype)
    rhs[0] = dtype(3) * (D[0] - heading_vector(psi_s, dtype))
    rhs[1:n - 1] = dtype(3) * (D[1:] - D[:-1])
    rhs[n - 1] = dtype(3) * (heading_vector(psi_e, dtype) - D[n - 2])
    diag = np.full(n, 4, dtype=dtype)
    diag[0] = diag[n - 1] = dtype(2)
    one = np.ones(n, dtype=dtype)
    if n < 8:
        A = np.diag(diag) + np.diag(one[:n - 1], 1) + np.diag(one[:n - 1], -1)
        c = glue_ref._gauss(A.astype(dtype), rhs)
    else:
        c = glue_ref._thomas(one, diag, one, rhs)
    b = D - (dtype(2) * c[:-1] + c[1:]) / dtype(3)
    d = (c[1:] - c[:-1]) / dtype(3)
    return (P[:-1], b, c[:-1], d), c


def front(ref, nv, alpha, psi_s, psi_e, dtype):
    """What does not depend on the stepsize: raceline points, spline, the n - 1 lengths, their running sum."""
    ref = np.asarray(ref, dtype=dtype)
    P = ref[:, :2] + np.asarray(alpha, dtype=dtype)[:, None] * np.asarray(nv, dtype=dtype)
    coef, c_all = open_spline(P, psi_s, psi_e, dtype)
    L = glue_ref.spline_lengths(coef, dtype)
    cum = glue_ref.running_sum(L)
    return dict(coef=coef, c_all=c_all, lengths=L, cum=cum, total=cum[-1], P=P, dtype=dtype)


def point_count(total, stepsize, dtype):
    """(m, total / stepsize): tph.interp_splines' ceil(total / stepsize) + 1 points, all kept."""
    r = dtype(total) / dtype(stepsize)
    return int(math.ceil(r)) + 1, r


def stations(fr, stepsize):
    """mcq_raceline_device_ends' outputs of one chain row for one stepsize: m, ratio, total, xy [m, 2], psi / kappa / el_lengths [m] (the last
    element length is the 0 the kernel writes), last (the last raceline point P_(n-1))."""
    dtype, total = fr["dtype"], fr["total"]
    m, ratio = point_count(total, stepsize, dtype)
    q = np.arange(m - 1, dtype=dtype) * (total / dtype(m - 1))
    _, _, xy, d1, d2 = glue_ref._eval(fr["coef"], fr["cum"], fr["lengths"], q, dtype)
    a, b, c, d = (k[-1] for k in fr["coef"])                     # station m - 1: t = 1 on the last segment
    xy = np.vstack((xy, a + b + c + d))
    d1 = np.vstack((d1, b + dtype(2) * c + dtype(3) * d))
    d2 = np.vstack((d2, dtype(2) * c + dtype(6) * d))
    pi = glue_ref.pi_of(dtype)
    psi = np.arctan2(d1[:, 1], d1[:, 0]) - pi / dtype(2)
    psi = np.where(psi >= pi, psi - dtype(2) * pi, np.where(psi < -pi, psi + dtype(2) * pi, psi))
    v2 = d1[:, 0] ** 2 + d1[:, 1] ** 2
    kappa = (d1[:, 0] * d2[:, 1] - d1[:, 1] * d2[:, 0]) / (v2 * np.sqrt(v2))
    el = np.concatenate((np.diff(q), [total - q[-1]], [dtype(0)]))
    return dict(m=m, ratio=ratio, total=total, xy=xy, psi=psi, kappa=kappa, el_lengths=el, last=fr["P"][-1])


def raceline(ref, nv, alpha, psi_s, psi_e, stepsize, dtype):
    return stations(front(ref, nv, alpha, psi_s, psi_e, dtype), stepsize)
