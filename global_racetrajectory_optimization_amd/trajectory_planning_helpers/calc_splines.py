"""
Host-side shim of tph.calc_splines.calc_splines -- boundary [REF helper_funcs_glob/src/prep_track.py:48-51],
[REF main_globaltraj.py:568-569].  Closed tracks (the reference's mincurv flow) and open paths with given end headings
(psi_s, psi_e: DESIGN.md "Open chains").

Instead of the dense 4N x 4N solve of the upstream formulation, the closed cubic-spline conditions are reduced to the
cyclic tridiagonal system in the quadratic coefficients c_i (derivation in DESIGN.md section 3):

    c_i + (2 s_i^2 + 2 s_i) c_{i+1} + s_i s_{i+1}^2 c_{i+2} = 3 (s_i D_{i+1} - D_i),     D_i = p_{i+1} - p_i
    d_i = (s_i^2 c_{i+1} - c_i) / 3,   b_i = D_i - (2 c_i + s_i^2 c_{i+1}) / 3,   a_i = p_i

The dense matrix M is still returned because the reference hands it on to opt_min_curv
[REF main_globaltraj.py:267]; our opt_min_curv only reads the N scalings s_i back out of it.
"""
import numpy as np
from scipy.linalg import solve_banded


def _solve_cyclic_tridiag(sub, diag, sup, rhs):
    """Rows m: sub[m] x[m-1] + diag[m] x[m] + sup[m] x[m+1] = rhs[m] (indices cyclic); rhs [N, k]."""
    n = diag.size
    if n < 3:
        raise ValueError("need at least 3 spline segments")
    ab = np.zeros((3, n))
    ab[0, 1:] = sup[:-1]
    ab[1, :] = diag
    ab[2, :-1] = sub[1:]
    # Woodbury for the two corner entries T[0, n-1] = sub[0], T[n-1, 0] = sup[n-1]
    U = np.zeros((n, 2))
    U[0, 0] = 1.0
    U[n - 1, 1] = 1.0
    V = np.zeros((2, n))
    V[0, n - 1] = sub[0]
    V[1, 0] = sup[n - 1]
    y = solve_banded((1, 1), ab, np.column_stack((rhs, U)))
    yr, yu = y[:, :rhs.shape[1]], y[:, rhs.shape[1]:]
    corr = np.linalg.solve(np.eye(2) + V @ yu, V @ yr)
    return yr - yu @ corr


def spline_scalings(path_cl, el_lengths=None, use_dist_scaling=True):
    n = path_cl.shape[0] - 1
    if not use_dist_scaling:
        return np.ones(n)
    if el_lengths is None:
        el = np.sqrt(np.sum(np.diff(path_cl, axis=0) ** 2, axis=1))
    else:
        el = np.array(el_lengths, dtype=np.float64)
    return el / np.roll(el, -1)


def closed_spline_coeffs(points, scaling):
    """points [N, k] (unclosed), scaling [N] -> a, b, c, d each [N, k]."""
    n = points.shape[0]
    s = scaling
    s_next = np.roll(s, -1)
    delta = np.roll(points, -1, axis=0) - points
    rhs = 3.0 * (s[:, None] * np.roll(delta, -1, axis=0) - delta)
    # equation i couples c_i, c_{i+1}, c_{i+2}; index rows by the centre unknown m = i + 1
    sub = np.roll(np.ones(n), 1)
    diag = np.roll(2.0 * s ** 2 + 2.0 * s, 1)
    sup = np.roll(s * s_next ** 2, 1)
    c = _solve_cyclic_tridiag(sub, diag, sup, np.roll(rhs, 1, axis=0))
    c_next = np.roll(c, -1, axis=0)
    d = (s[:, None] ** 2 * c_next - c) / 3.0
    b = delta - (2.0 * c + s[:, None] ** 2 * c_next) / 3.0
    return points.copy(), b, c, d


def build_les_matrix(n, scaling):
    """The dense 4N x 4N matrix of the upstream formulation -- returned for interface parity."""
    M = np.zeros((4 * n, 4 * n))
    i = np.arange(n)
    j = 4 * i
    M[j, j] = 1.0
    for k in range(4):
        M[j + 1, j + k] = 1.0
    inner = i[:-1]
    ji = 4 * inner
    M[ji + 2, ji + 1], M[ji + 2, ji + 2], M[ji + 2, ji + 3] = 1.0, 2.0, 3.0
    M[ji + 2, ji + 5] = -scaling[:-1]
    M[ji + 3, ji + 2], M[ji + 3, ji + 3] = 2.0, 6.0
    M[ji + 3, ji + 6] = -2.0 * scaling[:-1] ** 2
    M[-2, 1] = scaling[-1]
    M[-2, -3:] = (-1.0, -2.0, -3.0)
    M[-1, 2] = 2.0 * scaling[-1] ** 2
    M[-1, -2:] = (-2.0, -6.0)
    return M


def scalings_from_les_matrix(A, check=True):
    """Recover s_i from the matrix calc_splines returned: the inverse of build_les_matrix.

    The engine never sees `A`: everything opt_min_curv needs from it is the N scalings.  That is only valid if `A` IS the
    matrix of the closed-spline system (what the reference passes on from calc_splines [REF main_globaltraj.py:267,
    prep_track.py:48-51]); `check` verifies it in O(N) + one counting pass -- the structural entries of every 4-row block, the four entries
    that must mirror the scalings (-s, -2 s^2), positivity, and the number of non-zeros (12 N: nothing outside the
    pattern) -- and raises RuntimeError otherwise: a silently wrong alpha is the alternative (there is no dense CPU path in
    the product to fall back to).
    """
    A = np.asarray(A)
    n = A.shape[0] // 4
    i = np.arange(n - 1)
    s = np.empty(n)
    s[:-1] = -A[4 * i + 2, 4 * i + 5]
    s[-1] = A[4 * n - 2, 1]
    if check:
        j = 4 * np.arange(n)
        ji = 4 * i
        ok = bool(np.all(np.isfinite(s)) and np.all(s > 0.0))
        ok = ok and bool(np.all(A[j, j] == 1.0) and np.all(A[j + 1, j] == 1.0) and np.all(A[j + 1, j + 1] == 1.0)
                         and np.all(A[j + 1, j + 2] == 1.0) and np.all(A[j + 1, j + 3] == 1.0))
        ok = ok and bool(np.all(A[ji + 2, ji + 1] == 1.0) and np.all(A[ji + 2, ji + 2] == 2.0) and np.all(A[ji + 2, ji + 3] == 3.0)
                         and np.all(A[ji + 3, ji + 2] == 2.0) and np.all(A[ji + 3, ji + 3] == 6.0))
        ok = ok and bool(np.all(A[-2, -3:] == (-1.0, -2.0, -3.0)) and np.all(A[-1, -2:] == (-2.0, -6.0)))
        if ok:
            s2 = 2.0 * s * s
            ok = bool(np.allclose(-A[ji + 3, ji + 6], s2[:-1], rtol=1e-12, atol=0.0) and np.isclose(A[-1, 2], s2[-1], rtol=1e-12, atol=0.0))
        if ok:
            # the 12 N entries checked above are all there is: one pass over A, no temporaries (~60 ms at N = 2000, where
            # upstream spends 13 s inverting the same matrix)
            ok = int(np.count_nonzero(A)) == 12 * n
        if not ok:
            raise RuntimeError("Spline equation system matrix A does not have the structure of calc_splines' closed-spline "
                               "system (the MI355X engine derives everything from the N spline scalings it encodes and "
                               "cannot use an arbitrary matrix)")
    return s


# ----------------------------------------------------------------------------------------------------------------------
# open paths: N points, N - 1 splines, headings psi_s / psi_e at the ends (tph convention: rad, 0 = north)
# ----------------------------------------------------------------------------------------------------------------------
# tph.calc_splines multiplies its heading rows by el_lengths[0] / el_lengths[-1] (1.0 when el_lengths is None), while tph.opt_min_curv's own
# heading rows use the unit vectors (include/mcq.h MCQ_HEADING_SCALE).  Reproduced, not fixed: the two disagree upstream too.

def open_spline_coeffs(points, scaling, h_s, h_e):
    """points [N, k], scaling [N - 2] (inner joints), h_s / h_e [k] heading vectors as the heading rows carry them -> a, b, c, d [N - 1, k].

    Unknowns c_0 .. c_(N-1) (x'' = 2 c; c_(N-1) is half the second derivative at t = 1 of the last spline), s_(N-2) := 1:
        2 c_0 + s_0^2 c_1 = 3 (D_0 - h_s)
        c_(m-1) + (2 s_(m-1)^2 + 2 s_(m-1)) c_m + s_(m-1) s_m^2 c_(m+1) = 3 (s_(m-1) D_m - D_(m-1))     1 <= m <= N-2
        c_(N-2) + 2 c_(N-1) = 3 (h_e - D_(N-2))
    """
    n = points.shape[0]
    s = np.append(np.asarray(scaling, dtype=np.float64), 1.0)          # s_0 .. s_(N-2)
    delta = np.diff(points, axis=0)                                    # D_0 .. D_(N-2)
    diag = np.empty(n)
    sup = np.zeros(n)
    sub = np.ones(n)
    diag[0], diag[-1] = 2.0, 2.0
    diag[1:-1] = 2.0 * s[:-1] ** 2 + 2.0 * s[:-1]
    sup[0] = s[0] ** 2
    sup[1:-1] = s[:-1] * s[1:] ** 2
    rhs = np.empty((n, points.shape[1]))
    rhs[0] = 3.0 * (delta[0] - h_s)
    rhs[1:-1] = 3.0 * (s[:-1, None] * delta[1:] - delta[:-1])
    rhs[-1] = 3.0 * (h_e - delta[-1])
    ab = np.zeros((3, n))
    ab[0, 1:] = sup[:-1]
    ab[1, :] = diag
    ab[2, :-1] = sub[1:]
    c = solve_banded((1, 1), ab, rhs)
    cn = c[1:]
    cc = c[:-1]
    d = (s[:, None] ** 2 * cn - cc) / 3.0
    b = delta - (2.0 * cc + s[:, None] ** 2 * cn) / 3.0
    return points[:-1].copy(), b, cc, d


def build_open_les_matrix(n, scaling):
    """The dense [4(N-1), 4(N-1)] matrix of tph's open system through N points (12 N - 15 non-zeros)."""
    ns = n - 1
    M = np.zeros((4 * ns, 4 * ns))
    i = np.arange(ns)
    j = 4 * i
    M[j, j] = 1.0
    for k in range(4):
        M[j + 1, j + k] = 1.0
    ji = 4 * i[:-1]
    M[ji + 2, ji + 1], M[ji + 2, ji + 2], M[ji + 2, ji + 3] = 1.0, 2.0, 3.0
    M[ji + 2, ji + 5] = -np.asarray(scaling)
    M[ji + 3, ji + 2], M[ji + 3, ji + 3] = 2.0, 6.0
    M[ji + 3, ji + 6] = -2.0 * np.asarray(scaling) ** 2
    M[-2, 1] = 1.0
    M[-1, -4:] = (0.0, 1.0, 2.0, 3.0)
    return M


def scalings_from_open_les_matrix(A, check=True):
    """[N] scalings out of the open matrix (N - 2 inner joints, then two ones), with the structural check of mcq_les_scalings_open."""
    A = np.asarray(A)
    ns = A.shape[0] // 4
    n = ns + 1
    i = np.arange(ns - 1)
    s = np.ones(n)
    s[:-2] = -A[4 * i + 2, 4 * i + 5]
    if check:
        ok = A.ndim == 2 and A.shape[0] == A.shape[1] == 4 * ns and ns >= 2
        ok = ok and bool(np.all(np.isfinite(s)) and np.all(s > 0.0))
        if ok:
            ok = bool(np.array_equal(A, build_open_les_matrix(n, s[:-2])) or
                      (np.count_nonzero(A) == 12 * n - 15 and np.allclose(A, build_open_les_matrix(n, s[:-2]), rtol=1e-12, atol=0.0)))
        if not ok:
            raise RuntimeError("Spline equation system matrix A does not have the structure of calc_splines' open-spline system (the "
                               "MI355X engine derives everything from the spline scalings it encodes and cannot use an arbitrary matrix)")
    return s


def calc_splines(path: np.ndarray, el_lengths: np.ndarray = None, psi_s: float = None, psi_e: float = None,
                 use_dist_scaling: bool = True) -> tuple:
    path = np.asarray(path, dtype=np.float64)
    closed = bool(np.all(np.isclose(path[0], path[-1]))) and psi_s is None
    if not closed and (psi_s is None or psi_e is None):
        raise RuntimeError("Headings must be provided for unclosed spline calculation!")
    if el_lengths is not None and path.shape[0] != el_lengths.size + 1:
        raise RuntimeError("el_lengths input must be one element smaller than path input!")
    if not closed:
        n = path.shape[0]
        if use_dist_scaling:
            el = np.sqrt(np.sum(np.diff(path, axis=0) ** 2, axis=1)) if el_lengths is None else np.array(el_lengths, dtype=np.float64)
            scaling = el[:-1] / el[1:]
        else:
            scaling = np.ones(n - 2)
        l_s = 1.0 if el_lengths is None else float(el_lengths[0])
        l_e = 1.0 if el_lengths is None else float(el_lengths[-1])
        h_s = np.array((np.cos(psi_s + np.pi / 2), np.sin(psi_s + np.pi / 2))) * l_s
        h_e = np.array((np.cos(psi_e + np.pi / 2), np.sin(psi_e + np.pi / 2))) * l_e
        a, b, c, d = open_spline_coeffs(path, scaling, h_s, h_e)
        coeffs_x = np.column_stack((a[:, 0], b[:, 0], c[:, 0], d[:, 0]))
        coeffs_y = np.column_stack((a[:, 1], b[:, 1], c[:, 1], d[:, 1]))
        normvec = np.stack((coeffs_y[:, 1], -coeffs_x[:, 1]), axis=1)
        normvec_normalized = normvec / np.sqrt(np.sum(normvec ** 2, axis=1))[:, None]
        return coeffs_x, coeffs_y, build_open_les_matrix(n, scaling), normvec_normalized
    n = path.shape[0] - 1
    scaling = spline_scalings(path, el_lengths, use_dist_scaling)
    a, b, c, d = closed_spline_coeffs(path[:-1], scaling)
    coeffs_x = np.column_stack((a[:, 0], b[:, 0], c[:, 0], d[:, 0]))
    coeffs_y = np.column_stack((a[:, 1], b[:, 1], c[:, 1], d[:, 1]))
    normvec = np.stack((coeffs_y[:, 1], -coeffs_x[:, 1]), axis=1)
    normvec_normalized = normvec / np.sqrt(np.sum(normvec ** 2, axis=1))[:, None]
    return coeffs_x, coeffs_y, build_les_matrix(n, scaling), normvec_normalized
