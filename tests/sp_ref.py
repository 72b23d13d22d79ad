"""A plain reference for the shortest-path QP (MCQ_OBJ_SHORTEST_PATH; include/mcq.h, mcq_assemble_sp_kernel's header):

    minimise 1/2 a'Ha + f'a,  lo <= a <= hi,      H cyclic tridiagonal:  hd_i = 4 |n_i|^2,  hu_i = H[i, i+1 mod n] = -2 n_i . n_(i+1 mod n),
    f_i = 2 n_i . (2 p_i - p_(i-1) - p_(i+1)),    lo_i = -max(w_l - w_veh / 2, 0.001),  hi_i = max(w_r - w_veh / 2, 0.001).

numpy only, the working dtype a parameter (np.longdouble is THE reference, np.float64 a second run that says how far the answer is determined);
no dense matrix, nothing of oracle/, nothing of the engine.  Box rows only and a tridiagonal H: block principal pivoting, every round O(n) --
the ring cut at the pinned rows into chains, one Thomas sweep per chain; a ring without a pinned row by Sherman-Morrison.  The QP is strictly
convex, so a point that passes the certificate at the end IS the optimum: the result does not depend on the route to it."""
from fractions import Fraction

import numpy as np

LD = np.longdouble
FREE, AT_LO, AT_HI = 0, -1, 1
CLIP = 0.001
CERT_FACTOR = 64            # free rows: |g_i| <= CERT_FACTOR eps_longdouble max|f|
REFINE_STEPS = 2
MAX_ROUNDS_FACTOR = 8       # rounds allowed: MAX_ROUNDS_FACTOR n + 200 (Murty's rule is finite; this only bounds the loop)


def bounds(reftrack, w_veh, dt=np.float64):
    """(lo, hi) by the kernel's own formula; in float64 numpy gives the kernel's bits."""
    ref = np.asarray(reftrack, dtype=dt)
    half = dt(0.5) * dt(w_veh)
    return -np.maximum(ref[:, 3] - half, dt(CLIP)), np.maximum(ref[:, 2] - half, dt(CLIP))


def assemble(reftrack, normvec, w_veh, dt=LD):
    """hd, hu, f, lo, hi in dtype dt."""
    ref, nv = np.asarray(reftrack, dtype=dt), np.asarray(normvec, dtype=dt)
    p = ref[:, :2]
    hd = dt(4) * np.sum(nv * nv, axis=1)
    hu = dt(-2) * np.sum(nv * np.roll(nv, -1, axis=0), axis=1)
    f = dt(2) * np.sum(nv * (dt(2) * p - np.roll(p, 1, axis=0) - np.roll(p, -1, axis=0)), axis=1)
    lo, hi = bounds(ref, w_veh, dt)
    return hd, hu, f, lo, hi


def gradient(hd, hu, f, x):
    """g = H x + f on the ring."""
    return hd * x + hu * np.roll(x, -1) + np.roll(hu, 1) * np.roll(x, 1) + f


def _thomas(d, o, r):
    """Solve the chain  o[k-1] x[k-1] + d[k] x[k] + o[k] x[k+1] = r[k]  (o has len(d) - 1 entries) in the dtype of its arguments."""
    m = len(d)
    u, y = [d[0]] * m, [r[0]] * m
    for k in range(1, m):
        mlt = o[k - 1] / u[k - 1]
        u[k] = d[k] - mlt * o[k - 1]
        y[k] = r[k] - mlt * y[k - 1]
    x = [y[m - 1] / u[m - 1]] * m
    for k in range(m - 2, -1, -1):
        x[k] = (y[k] - o[k] * x[k + 1]) / u[k]
    return x


def _cyclic(hd, hu, r):
    """The whole ring free: Sherman-Morrison on the corners, two Thomas sweeps."""
    n = len(hd)
    dt = hd.dtype.type
    gam = -hd[0]
    c0 = hu[n - 1]
    d = list(hd)
    d[0] = hd[0] - gam
    d[n - 1] = hd[n - 1] - c0 * c0 / gam
    o = list(hu[:n - 1])
    u = [dt(0)] * n
    u[0], u[n - 1] = gam, c0
    y, z = _thomas(d, o, list(r)), _thomas(d, o, u)
    fac = (y[0] + c0 * y[n - 1] / gam) / (dt(1) + z[0] + c0 * z[n - 1] / gam)
    return np.array([a - fac * b for a, b in zip(y, z)], dtype=hd.dtype)


def solve_state(hd, hu, f, lo, hi, state):
    """x with the pinned rows on their bounds and  (H x + f)_i = 0  on the free rows."""
    n = len(hd)
    pinned = state != FREE
    if not pinned.any():
        return _cyclic(hd, hu, -f)
    x = np.where(state == AT_LO, lo, np.where(state == AT_HI, hi, np.zeros_like(f)))
    # right-hand side of the free rows with the pinned neighbours moved over
    r = -f - np.where(np.roll(pinned, -1), hu * np.roll(x, -1), 0) - np.where(np.roll(pinned, 1), np.roll(hu, 1) * np.roll(x, 1), 0)
    p0 = int(np.argmax(pinned))                  # rotate: a pinned row first, the ring becomes a line
    idx = (np.arange(n) + p0) % n
    fr = ~pinned[idx]
    edge = np.diff(np.concatenate(([0], fr.astype(np.int8), [0])))
    for a, b in zip(np.flatnonzero(edge == 1), np.flatnonzero(edge == -1)):      # free run idx[a:b]
        rows = idx[a:b]
        x[rows] = _thomas(list(hd[rows]), list(hu[rows[:-1]]), list(r[rows]))
    return x


def offenders(x, g, lo, hi, state):
    """The state every row asks for: a free row outside its box is pinned there, a pinned row whose multiplier has the wrong sign is freed."""
    want = state.copy()
    free = state == FREE
    want[free & (x < lo)] = AT_LO
    want[free & (x > hi)] = AT_HI
    want[(state == AT_LO) & (g < 0)] = FREE
    want[(state == AT_HI) & (g > 0)] = FREE
    return want


def _exact(a):
    """The entries of a longdouble (or float64) array as exact Fractions (a 64-bit mantissa splits into two doubles without loss)."""
    a = np.asarray(a, dtype=LD)
    hi = a.astype(np.float64)
    lo = (a - hi.astype(LD)).astype(np.float64)
    return [Fraction(h) + Fraction(l) for h, l in zip(hi.tolist(), lo.tolist())]


def exact_gradient(hd, hu, f, x, x_tail=None):
    """g = H (x + x_tail) + f in exact rational arithmetic on the given (rounded) hd, hu, f; a list of Fractions."""
    n = len(hd)
    D, U, F, X = _exact(hd), _exact(hu), _exact(f), _exact(x)
    if x_tail is not None:
        X = [a + b for a, b in zip(X, _exact(x_tail))]
    return [D[i] * X[i] + U[i] * X[(i + 1) % n] + U[i - 1] * X[i - 1] + F[i] for i in range(n)]


def certificate(hd, hu, f, lo, hi, x, x_tail, state):
    """The KKT conditions of the point x + x_tail (two longdouble terms, not added up: the sum's own rounding, eps |x| / 2, moves g by more
    than the bound below wherever |H| |x| is large against max|f| -- the rings on which nothing is active).  g is evaluated exactly.
    Returns the largest free |g| relative to max|f|; raises AssertionError if a condition fails."""
    g = exact_gradient(hd, hu, f, x, x_tail)
    fmax = max(abs(v) for v in _exact(f))
    bound = Fraction(CERT_FACTOR) * Fraction(float(np.finfo(LD).eps)) * fmax
    free = state == FREE
    worst = max([abs(g[i]) for i in np.flatnonzero(free)], default=Fraction(0))
    assert worst <= bound, "free gradient %.3e max|f|, allowed %.3e" % (worst / fmax, bound / fmax)
    tail = np.zeros_like(x) if x_tail is None else x_tail
    assert np.all(x[state == AT_LO] == lo[state == AT_LO]) and np.all(x[state == AT_HI] == hi[state == AT_HI]) and not np.any(tail[~free]), \
        "a pinned row is off its bound"
    assert all(g[i] >= 0 for i in np.flatnonzero(state == AT_LO)) and all(g[i] <= 0 for i in np.flatnonzero(state == AT_HI)), \
        "a multiplier has the wrong sign"
    s = x + tail
    assert np.all(s >= lo) and np.all(s <= hi), "a row is outside its box"
    return float(worst / fmax)


def refine(hd, hu, f, x, state, steps=REFINE_STEPS):
    """x_tail such that the free rows of H (x + x_tail) + f vanish to far below eps: the exact residual, rounded, through the same sweeps."""
    tail = np.zeros_like(x)
    zero = np.zeros_like(x)
    for _ in range(steps):
        g = np.array([LD(float(v)) for v in exact_gradient(hd, hu, f, x, tail)], dtype=LD)
        tail = tail + solve_state(hd, hu, g, zero, zero, state) if (state == FREE).any() else tail
    return tail


def solve(reftrack, normvec, w_veh, dt=LD, single_from_start=False):
    """Returns a dict: alpha (dtype dt), state (int8: 0 free, -1 at lo, +1 at hi), rounds, murty (rounds under the single-pivot rule),
    margin_x (smallest distance of a free row to a bound, m), margin_g (smallest |multiplier| of a pinned row), margin = the smaller,
    cert (longdouble only: largest free |g| / max|f| of the certified point), lo, hi (dtype dt)."""
    hd, hu, f, lo, hi = assemble(reftrack, normvec, w_veh, dt)
    n = len(hd)
    if n < 3:
        raise ValueError("a ring needs three waypoints")
    state = np.zeros(n, dtype=np.int8)
    seen = set()
    single = bool(single_from_start)     # (tests: the fallback rule as a route of its own)
    rounds = murty = 0
    while True:
        rounds += 1
        if rounds > MAX_ROUNDS_FACTOR * n + 200:
            raise RuntimeError("block principal pivoting did not settle")
        x = solve_state(hd, hu, f, lo, hi, state)
        g = gradient(hd, hu, f, x)
        want = offenders(x, g, lo, hi, state)
        off = np.flatnonzero(want != state)
        if off.size == 0:
            break
        key = state.tobytes()
        single = single or key in seen          # the full exchange cycles: from here on Murty's rule, the highest-index offender alone
        seen.add(key)
        if single:
            murty += 1
            state[off[-1]] = want[off[-1]]
        else:
            state = want
    free = state == FREE
    margin_x = float(min(np.min(x[free] - lo[free]), np.min(hi[free] - x[free]))) if free.any() else float("inf")
    margin_g = float(np.min(np.abs(g[~free]))) if (~free).any() else float("inf")
    out = dict(alpha=x, state=state, rounds=rounds, murty=murty, margin_x=margin_x, margin_g=margin_g, margin=min(margin_x, margin_g),
               cert=None, lo=lo, hi=hi)
    if dt is LD:            # THE reference certifies itself; the float64 run only says how far the answer is determined
        tail = refine(hd, hu, f, x, state)
        out["cert"] = certificate(hd, hu, f, lo, hi, x, tail, state)
        out["alpha"] = x + tail
    return out
