"""A plain restatement of what mcq_spline_approx_device computes (include/mcq.h): tph.spline_approximation behind FITPACK's fit, in longdouble
and in float64.  TEST-ONLY; numpy alone (tests/test_spline_approx_ref.py pins it to scipy's splev / fmin and to the host shim).

The search is vectorised over the waypoints -- every waypoint takes its own decisions, the lanes only share the loop -- and records per
waypoint the smallest |f1 - f2| over every comparison of two function values it made (the <= 1e-4 test of the termination rule included,
as the distance of |fa - fb| to 1e-4).  The simplex points are ALWAYS formed in float64, with scipy's roundings: given the same decisions a
parameter is a rounding-exact function of x0, whatever the precision the distances were evaluated in."""
import math

import numpy as np

LD = np.longdouble
F64 = np.float64
MAXFUN = 200
XTOL = FTOL = 1e-4


def as_tck(tck, dtype):
    t, c, k = tck
    return np.asarray(t, dtype=dtype), (np.asarray(c[0], dtype=dtype), np.asarray(c[1], dtype=dtype)), int(k)


def splev(x, tck, dtype=LD):
    """splev(x, tck), ext = 0, both coordinates: interval l with t[l] <= x < t[l + 1] clamped to [k, nk - k - 2], x neither clamped nor wrapped;
    FITPACK's fpbspl recursion; the sum over c[l - k .. l] in ascending order."""
    t, (cx, cy), k = as_tck(tck, dtype)
    x = np.atleast_1d(np.asarray(x, dtype=dtype))
    nk = t.shape[0]
    l = np.clip(np.searchsorted(t, x, side="right") - 1, k, nk - k - 2)
    h = [np.ones(x.shape, dtype=dtype)]
    for j in range(1, k + 1):
        hh = list(h)
        h = [np.zeros(x.shape, dtype=dtype)] + [None] * j
        for i in range(j):
            tli, tlj = t[l + 1 + i], t[l + 1 + i - j]
            den = tli - tlj
            zero = den == 0
            f = hh[i] / np.where(zero, dtype(1), den)
            h[i] = np.where(zero, h[i], h[i] + f * (tli - x))
            h[i + 1] = np.where(zero, dtype(0), f * (x - tlj))
    sx = np.zeros(x.shape, dtype=dtype)
    sy = np.zeros(x.shape, dtype=dtype)
    for j in range(k + 1):
        sx = sx + cx[l - k + j] * h[j]
        sy = sy + cy[l - k + j] * h[j]
    return sx, sy


def hypot(a, b, dtype):
    if dtype is F64:        # the host shim's math.hypot, not numpy's
        return np.array([math.hypot(u, v) for u, v in zip(np.atleast_1d(a), np.atleast_1d(b))], dtype=F64)
    return np.hypot(a, b)


def close_track(track, dtype=LD):
    """track_cl's coordinates [n + 1, 2], the running sum [n + 1] in numpy.cumsum's order."""
    xy = np.asarray(track, dtype=dtype)[:, :2]
    cl = np.vstack((xy, xy[:1]))
    el = np.sqrt(np.sum(np.diff(cl, axis=0) ** 2, axis=1))
    return cl, np.concatenate((np.zeros(1, dtype=dtype), np.cumsum(el)))


def linspace01(num, dtype):
    """numpy.linspace(0, 1, num): i * (1 / (num - 1)), the last sample exactly 1."""
    g = np.arange(num).astype(dtype) * (dtype(1) / dtype(num - 1))
    g[-1] = dtype(1)
    return g


def length_and_count(track, tck, stepsize_reg, dtype=LD):
    """(total, len_smoothed, len_smoothed / stepsize_reg, no_points_reg_cl)."""
    _, cum = close_track(track, dtype)
    total = cum[-1]
    n_len = 4 * int(math.ceil(total))
    sx, sy = splev(linspace01(n_len, dtype), tck, dtype)
    length = np.sum(np.sqrt(np.diff(sx) ** 2 + np.diff(sy) ** 2))
    ratio = length / dtype(stepsize_reg)
    return total, length, ratio, int(math.ceil(ratio)) + 1


def search(track, tck, dtype=F64):
    """scipy.optimize.fmin(|s(t) - p_i|, x0 = t_guess_i) for every row of track_cl, restated for one variable.
    Returns dict(t [n + 1] float64, calls [n + 1], gap [n + 1]: the smallest |f1 - f2| over the comparisons made, f0: f(t_guess))."""
    cl64, cum64 = close_track(track, F64)           # the first guesses are float64 quantities of the float64 rows
    x0 = cum64 / cum64[-1]
    p = np.asarray(cl64, dtype=dtype)
    cnt = x0.shape[0]

    def f(x, idx):
        sx, sy = splev(np.asarray(x, dtype=dtype), tck, dtype)
        return hypot(sx - p[idx, 0], sy - p[idx, 1], dtype)
    everyone = np.arange(cnt)
    a = x0.copy()
    b = np.where(x0 != 0.0, (1 + 0.05) * x0, 0.00025)
    fa, fb = f(a, everyone), f(b, everyone)
    f0 = fa.copy()
    gap = np.abs(fa - fb)
    sw = fb < fa
    a, b = np.where(sw, b, a), np.where(sw, a, b)
    fa, fb = np.where(sw, fb, fa), np.where(sw, fa, fb)
    calls = np.full(cnt, 2)
    iters = np.ones(cnt, dtype=int)
    live = np.ones(cnt, dtype=bool)

    def seen(idx, u, v):
        gap[idx] = np.minimum(gap[idx], np.abs(u - v))
    while True:
        live &= (calls < MAXFUN) & (iters < MAXFUN)
        close = live & (np.abs(b - a) <= XTOL)
        ic = np.nonzero(close)[0]
        seen(ic, np.abs(fa[ic] - fb[ic]), dtype(FTOL))
        live &= ~(close & (np.abs(fa - fb) <= FTOL))
        idx = np.nonzero(live)[0]
        if idx.size == 0:
            break
        xr = 2.0 * a[idx] - b[idx]
        fxr = f(xr, idx)
        calls[idx] += 1
        seen(idx, fxr, fa[idx])
        c1 = fxr < fa[idx]
        nb, nfb = b[idx].copy(), fb[idx].copy()
        shrink = np.zeros(idx.size, dtype=bool)
        # expansion
        k1 = np.nonzero(c1)[0]
        if k1.size:
            i1 = idx[k1]
            xe = 3.0 * a[i1] - 2.0 * b[i1]
            fxe = f(xe, i1)
            calls[i1] += 1
            seen(i1, fxe, fxr[k1])
            better = fxe < fxr[k1]
            nb[k1], nfb[k1] = np.where(better, xe, xr[k1]), np.where(better, fxe, fxr[k1])
        rest = np.nonzero(~c1)[0]
        seen(idx[rest], fxr[rest], fb[idx[rest]])
        c2 = ~c1 & (fxr < fb[idx])
        k2 = np.nonzero(c2)[0]
        if k2.size:
            i2 = idx[k2]
            xc = 1.5 * a[i2] - 0.5 * b[i2]
            fxc = f(xc, i2)
            calls[i2] += 1
            seen(i2, fxc, fxr[k2])
            ok = fxc <= fxr[k2]
            nb[k2], nfb[k2] = np.where(ok, xc, nb[k2]), np.where(ok, fxc, nfb[k2])
            shrink[k2] = ~ok
        k3 = np.nonzero(~c1 & ~c2)[0]
        if k3.size:
            i3 = idx[k3]
            xcc = 0.5 * a[i3] + 0.5 * b[i3]
            fxcc = f(xcc, i3)
            calls[i3] += 1
            seen(i3, fxcc, fb[i3])
            ok = fxcc < fb[i3]
            nb[k3], nfb[k3] = np.where(ok, xcc, nb[k3]), np.where(ok, fxcc, nfb[k3])
            shrink[k3] = ~ok
        ks = np.nonzero(shrink)[0]
        if ks.size:
            i4 = idx[ks]
            nb[ks] = a[i4] + 0.5 * (b[i4] - a[i4])
            nfb[ks] = f(nb[ks], i4)
            calls[i4] += 1
        b[idx], fb[idx] = nb, nfb
        iters[idx] += 1
        seen(idx, fa[idx], fb[idx])
        sw = np.zeros(cnt, dtype=bool)
        sw[idx] = fb[idx] < fa[idx]
        a, b = np.where(sw, b, a), np.where(sw, a, b)
        fa, fb = np.where(sw, fb, fa), np.where(sw, fa, fb)
    return dict(t=np.asarray(a, dtype=F64), calls=calls, gap=np.asarray(gap, dtype=F64), f0=np.asarray(f0, dtype=F64), x0=x0)


def interp_bisect(x, xp, fp):
    """numpy.interp's rule with plain bisection (what the entry does where xp descends too): the last i with xp[i] <= x by bisection over [0, n];
    fp[0] below xp[0], fp[n] above xp[n] or at i == n; fp[i] at x == xp[i]; else slope * (x - xp[i]) + fp[i]."""
    n = xp.shape[0] - 1
    out = np.empty(x.shape, dtype=fp.dtype)
    for j, xv in enumerate(x):
        lo, hi = 0, n
        while lo < hi:
            mid = (lo + hi + 1) >> 1
            if xp[mid] <= xv:
                lo = mid
            else:
                hi = mid - 1
        if xv < xp[0]:
            out[j] = fp[0]
        elif xv > xp[n] or lo == n:
            out[j] = fp[n]
        elif xp[lo] == xv:
            out[j] = fp[lo]
        else:
            out[j] = (fp[lo + 1] - fp[lo]) / (xp[lo + 1] - xp[lo]) * (xv - xp[lo]) + fp[lo]
    return out


def finish(track, tck, stepsize_reg, closest_t, dtype=LD, npts=None):
    """Everything behind the search, from given closest parameters [n + 1]: dict(rows [m, 4], dists [n + 1], sides [n + 1], dev (mean, max),
    nonmono, m, ratio).  npts: no_points_reg_cl if it is to be imposed (a perturbed run keeps the unperturbed count)."""
    trk = np.asarray(track, dtype=dtype)
    n = trk.shape[0]
    cl, _ = close_track(trk, dtype)
    _, _, ratio, cnt = length_and_count(trk, tck, stepsize_reg, dtype)
    npts = cnt if npts is None else npts
    ct = np.asarray(closest_t, dtype=dtype)
    sx, sy = splev(ct, tck, dtype)
    dists = np.hypot(sx - cl[:, 0], sy - cl[:, 1]) if dtype is not F64 else hypot(sx - cl[:, 0], sy - cl[:, 1], F64)
    cr = (cl[1:, 0] - cl[:-1, 0]) * (sy[:-1] - cl[:-1, 1]) - (cl[1:, 1] - cl[:-1, 1]) * (sx[:-1] - cl[:-1, 0])
    sides = np.sign(cr)
    sides = np.concatenate((sides, sides[:1]))
    w_cl = np.vstack((trk[:, 2:4], trk[:1, 2:4]))
    wr, wl = w_cl[:, 0] + sides * dists, w_cl[:, 1] - sides * dists
    grid = linspace01(npts, dtype)[:-1]
    px, py = splev(grid, tck, dtype)
    rows = np.column_stack((px, py, interp_bisect(grid, ct, wr), interp_bisect(grid, ct, wl)))
    return dict(rows=rows, dists=dists, sides=sides, dev=(np.sum(dists) / dtype(n + 1), np.max(np.abs(dists))),
                nonmono=int(np.sum(ct[1:] <= ct[:-1])), m=npts - 1, ratio=ratio)


def whole(track, tck, stepsize_reg, dtype=F64):
    """The float64 (or longdouble) whole: search, then finish on its parameters -- what the host shim returns."""
    s = search(track, tck, dtype)
    return dict(finish(track, tck, stepsize_reg, s["t"], dtype), search=s)
