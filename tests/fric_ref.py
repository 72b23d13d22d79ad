"""A plain reference for the friction entries (mcq_fmap_query_device, mcq_friction_grid_device), independent of their kernels.

nearest(cells, q):  brute force in longdouble over ALL cells, the lowest index among exact ties, and each query's gap to its runner-up.
grid(...):          the rows of extract_friction_coeffs restated: counts and lateral positions in float64 with Python's and numpy's own operations
                    (the counts are math.floor's, the positions numpy.linspace's, by construction), wheel positions in float64 as the reference
                    forms them (the bits the lookup sees) and in longdouble.
line(n, mue):       the least-squares line in longdouble, closed form; line64: the same closed form in float64, summed forwards or backwards.
tests/test_fric_ref.py holds all of it to arrays recorded from the reference's own functions (tests/golden/friction)."""
import math

import numpy as np

LD = np.longdouble
WHEELS = ("fl", "fr", "rl", "rr")


def nearest(cells, q, chunk=32):
    """(idx [k], dist [k] longdouble, gap [k] longdouble: the runner-up's distance minus the minimum; inf with one cell).  Non-finite queries: -1,
    NaN.  Every cell is looked at: a float64 pass over all of them keeps those within 1e-6 m of the float64 minimum (float64's own error is about
    1e-13 m at these coordinates), longdouble decides among them.  A gap above 1e-6 m is reported from the float64 pass: only its size matters."""
    c64, q = np.asarray(cells, dtype=np.float64), np.asarray(q, dtype=np.float64).reshape(-1, 2)
    cld = c64.astype(LD)
    k = q.shape[0]
    idx, dist, gap = np.full(k, -1, dtype=np.int64), np.full(k, np.nan, dtype=LD), np.full(k, np.nan, dtype=LD)
    fin = np.nonzero(np.all(np.isfinite(q), axis=1))[0]
    for a in range(0, fin.size, chunk):
        sel = fin[a:a + chunk]
        d2 = (c64[None, :, 0] - q[sel, 0][:, None]) ** 2 + (c64[None, :, 1] - q[sel, 1][:, None]) ** 2
        thr = (np.sqrt(d2.min(axis=1)) + 1e-6) ** 2 * (1 + 1e-12)
        for r, s in enumerate(sel):
            cand = np.nonzero(d2[r] <= thr[r])[0]           # (ascending: the first minimum below is the lowest index)
            d = np.hypot(cld[cand, 0] - LD(q[s, 0]), cld[cand, 1] - LD(q[s, 1]))
            i = int(np.argmin(d))
            idx[s], dist[s] = cand[i], d[i]
            if cand.size > 1:
                gap[s] = np.delete(d, i).min() - d[i]
            elif c64.shape[0] > 1:
                gap[s] = LD(np.sqrt(np.partition(d2[r], 1)[1])) - d[i]
            else:
                gap[s] = np.inf
    return idx, dist, gap


def dists_to(cells, q, idx):
    """Longdouble distance from each query to the cell idx names."""
    c = np.asarray(cells, dtype=LD)[np.asarray(idx)]
    q = np.asarray(q, dtype=np.float64).reshape(-1, 2).astype(LD)
    return np.hypot(c[:, 0] - q[:, 0], c[:, 1] - q[:, 1])


def counts(w_right, w_left, width, dn):
    """(num_right, num_left) with Python's own operations [REF extract_friction_coeffs.py:83-84]."""
    return (math.floor((float(w_right) - 0.5 * float(width) - 0.5) / float(dn)), math.floor((float(w_left) - 0.5 * float(width) - 0.5) / float(dn)))


def positions(num_right, num_left, dn):
    """numpy.linspace's bits restated (arange * step + start, product and sum apart, last entry = stop), asserted against numpy itself."""
    cnt = num_right + num_left + 1
    if cnt <= 0:
        return np.empty(0)
    start, stop = -float(dn) * num_right, float(dn) * num_left
    delta = stop - start
    out = np.empty(cnt)
    step = delta / (cnt - 1) if cnt > 1 else delta
    for j in range(cnt):
        out[j] = float(j) * step + start
    if cnt > 1:
        out[-1] = stop
    want = np.linspace(-dn * num_right, dn * num_left, cnt)
    assert out.tobytes() == want.tobytes(), "the restatement of numpy.linspace differs from numpy (%d, %d, %r)" % (num_right, num_left, dn)
    return out


def wheel_xy(p, nvec, n_pos, width, wb_f, wb_r, dtype=np.float64):
    """[4, cnt, 2]: fl, fr, rl, rr [REF extract_friction_coeffs.py:95-98], in float64 the reference's own numpy expressions."""
    p, nvec, n_pos = np.asarray(p, dtype=dtype), np.asarray(nvec, dtype=dtype), np.asarray(n_pos, dtype=dtype)
    width, wb_f, wb_r = dtype(width), dtype(wb_f), dtype(wb_r)
    tang = np.asarray([-nvec[1], nvec[0]], dtype=dtype)
    out = np.empty((4, n_pos.shape[0], 2), dtype=dtype)
    half = dtype(0.5) * width
    for j in range(n_pos.shape[0]):
        out[0, j] = (p + wb_f * tang) - (n_pos[j] + half) * nvec
        out[1, j] = (p + wb_f * tang) - (n_pos[j] - half) * nvec
        out[2, j] = (p - wb_r * tang) - (n_pos[j] + half) * nvec
        out[3, j] = (p - wb_r * tang) - (n_pos[j] - half) * nvec
    return out


def grid(reftrack, normvec, width, wb_f, wb_r, dn):
    """Per row of the closed track: dict(cnt, n [cnt], xy [4, cnt, 2] float64).  cnt may be <= 0 (n and xy empty)."""
    ref, nv = np.asarray(reftrack, dtype=np.float64), np.asarray(normvec, dtype=np.float64)
    rows = []
    for r in list(range(ref.shape[0])) + [0]:
        nr, nl = counts(ref[r, 2], ref[r, 3], width, dn)
        n_pos = positions(nr, nl, dn)
        rows.append(dict(cnt=nr + nl + 1, n=n_pos, xy=wheel_xy(ref[r, :2], nv[r], n_pos, width, wb_f, wb_r)))
    return rows


def line(n_pos, mue):
    """(slope, intercept) of the least-squares line in longdouble, centred closed form; NaN for fewer than two positions."""
    x, y = np.asarray(n_pos, dtype=LD), np.asarray(mue, dtype=LD)
    if x.shape[0] < 2:
        return LD(np.nan), LD(np.nan)
    mx, my = x.sum() / x.shape[0], y.sum() / x.shape[0]
    slope = ((x - mx) * (y - my)).sum() / ((x - mx) ** 2).sum()
    return slope, my - slope * mx


def line64(n_pos, mue, backwards=False):
    """The same closed form in float64 with plain running sums, forwards or backwards: how far float64 determines the line."""
    x, y = [float(v) for v in n_pos], [float(v) for v in mue]
    if len(x) < 2:
        return math.nan, math.nan
    if backwards:
        x, y = x[::-1], y[::-1]
    sx = sy = 0.0
    for a, b in zip(x, y):
        sx += a
        sy += b
    mx, my = sx / len(x), sy / len(x)
    sxy = sxx = 0.0
    for a, b in zip(x, y):
        sxy += (a - mx) * (b - my)
        sxx += (a - mx) * (a - mx)
    slope = sxy / sxx
    return slope, my - slope * mx


def line_spread(n_pos, mue):
    """Largest difference between the longdouble line and line64 forwards / backwards (0 for fewer than two positions or a NaN mue)."""
    if len(n_pos) < 2 or np.any(np.isnan(np.asarray(mue, dtype=np.float64))):
        return 0.0
    s, c = line(n_pos, mue)
    return float(max(max(abs(LD(a) - s), abs(LD(b) - c)) for a, b in (line64(n_pos, mue), line64(n_pos, mue, True))))
