"""The reference of the fp32 boundary (csrc/mcq_kernels.hip, "fp32 boundary": mcq_widen_rows_kernel, mcq_widen_kernel, mcq_narrow_kernel):
numpy only, no goldens.

  rebuild_ld     what mcq_widen_rows_kernel has to write, in numpy.longdouble
  guard          how far an fp64 evaluation IN THE KERNEL'S ORDER may stand from it: derived from the roundings on the longest path to any x_i
  host_guard     the same for engine.increments_to_rows, whose cumsum rounds n times where the kernel rounds ceil(n / 64) times
  kernel_order   the kernel's summation order restated in numpy float64 (without the fma a compiler may form: the guard covers both)
  mutant_order   the same with ONE planted error: the closure defect is spread with i0 + 1 instead of i0 on every lane but lane 0.  It is
                 what the case table has to tell apart (tests/test_f32_ref.py states where it does).

Narrowing needs no restatement: numpy.ndarray.astype(numpy.float32) is IEEE round-to-nearest-even.  Widening is exact."""
import numpy as np

LD = np.longdouble
WAVE = 64
U = 2.0 ** -53          # half an ulp of 1 in float64: the bound of one rounding relative to the result


def rebuild_ld(rows32, origin, layout):
    """rows32 [..., n, 4] float32, origin [..., 2] float64 or None -> longdouble rows [..., n, 4].
    layout 1 (MCQ_F32_INCREMENTS): x_i = o + sum_{j<i} d_j - i (sum_j d_j) / n;  layout 0 (MCQ_F32_ABSOLUTE): o + x_i.  Widths copied."""
    r = np.asarray(rows32, dtype=np.float32).astype(LD)
    n = r.shape[-2]
    o = np.zeros(r.shape[:-2] + (2,), dtype=LD) if origin is None else np.asarray(origin, dtype=np.float64).astype(LD)
    out = r.copy()
    if layout == 0:
        out[..., :2] = o[..., None, :] + r[..., :2]
        return out
    assert layout == 1
    d = r[..., :2]
    cs = np.cumsum(d, axis=-2)
    before = np.concatenate((np.zeros_like(cs[..., :1, :]), cs[..., :-1, :]), axis=-2)
    out[..., :2] = o[..., None, :] + before - np.arange(n, dtype=LD)[:, None] * (cs[..., -1:, :] / LD(n))
    return out


def _scale(origin, rows32):
    """max|o| + 2 max_col sum_j |d_j| per track: no partial sum on the way to any x_i is larger (the defect's share is at most sum |d|)."""
    r = np.asarray(rows32, dtype=np.float32).astype(np.float64)
    s = np.max(np.sum(np.abs(r[..., :2]), axis=-2), axis=-1)
    o = 0.0 if origin is None else np.max(np.abs(np.asarray(origin, dtype=np.float64)), axis=-1)
    return o + 2.0 * s


def guard(n, origin, rows32):
    """(3 ceil(n / 64) + 12) 2^-53 (max|o| + 2 max_col sum_j |d_j|), per track.  The roundings on the longest path to an x_i of the kernel:
    per - 1 in the slice sum, 6 scan levels, ix - sx, the division and the product of cx i0, two additions, two per step of the write loop
    (per - 1 steps at most): 3 per + 8, covered by 3 per + 12.  Each is at most half an ulp of the largest partial sum.  Contracting
    `... - cx * i0` into an fma removes one rounding: the bound holds either way."""
    per = -(-int(n) // WAVE)
    return (3 * per + 12) * U * _scale(origin, rows32)


def host_guard(n, origin, rows32):
    """engine.increments_to_rows: one subtraction of the mean and one cumsum step per waypoint -- (2 n + 12) in the place of (3 per + 12)."""
    return (2 * int(n) + 12) * U * _scale(origin, rows32)


def _order(rows32, origin, shift):
    r = np.asarray(rows32, dtype=np.float32)
    assert r.ndim == 2 and r.shape[1] == 4
    n = r.shape[0]
    per = -(-n // WAVE)
    d = np.zeros((WAVE * per, 2))
    d[:n] = r[:, :2].astype(np.float64)
    d = d.reshape(WAVE, per, 2)
    lane = np.arange(WAVE)
    i0 = np.minimum(lane * per, n)
    i1 = np.minimum(i0 + per, n)
    s = np.zeros((WAVE, 2))
    for j in range(per):                    # (the padding adds +0.0: exact)
        s = s + d[:, j]
    inc = s.copy()
    step = 1
    while step < WAVE:                      # Hillis-Steele: every lane >= step adds the value `step` lanes below, all at once
        up = inc.copy()
        up[step:] = inc[step:] + inc[:-step]
        inc = up
        step *= 2
    c = inc[WAVE - 1] / float(n)
    o = np.zeros(2) if origin is None else np.asarray(origin, dtype=np.float64)
    k = (i0 + np.where(lane > 0, shift, 0)).astype(np.float64)
    x = (o + (inc - s)) - c * k[:, None]
    out = r.astype(np.float64)
    for j in range(per):
        live = i0 + j < i1
        out[(i0 + j)[live], :2] = x[live]
        x = x + (d[:, j] - c)
    return out


def kernel_order(rows32, origin):
    """mcq_widen_rows_kernel, layout 1, for ONE track [n, 4] in float64: slice sums, the scan over the 64 lanes, the write loop."""
    return _order(rows32, origin, 0)


def mutant_order(rows32, origin):
    return _order(rows32, origin, 1)


def dev(got, want_ld):
    """max |got - want| over x and y per track ([..., n, 4] -> [...]), taken in longdouble; NaN where the two disagree about being NaN."""
    g, w = np.asarray(got).astype(LD)[..., :2], np.asarray(want_ld)[..., :2]
    both = np.isnan(g) & np.isnan(w)
    e = np.where(both, LD(0), np.abs(g - w))
    return np.max(e, axis=(-2, -1)).astype(np.float64)
