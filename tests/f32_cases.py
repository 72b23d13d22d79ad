"""The case tables of the fp32 boundary's edges (tests/f32_checks.py, run by tests/test_emu_f32.py and tests/test_gpu_f32.py; the reference's own
test is tests/test_f32_ref.py).  Deterministic: the rings are tests/glue_cases.ring's (trefoil and peanut around the origin, the stadium centred at
(1000, -2000) m) through engine.rows_to_increments; nothing is drawn here except what this header lists.

Rebuild (mcq_f32_rows_device: no solver, any n).  One LAUNCH is the three families at one n -- three different tracks --, in one layout, with
one origin, closed or not:
  n        REBUILD_N: 3 .. 5; 63 .. 65, 127 .. 129, 191 .. 193 (below 64 every lane holds one waypoint or none; at 64 k + 1 the slice length steps
           up and whole lanes run empty: n = 65 leaves lanes 33 .. 63 empty); 2047 .. 2049; 4097
  layout   MCQ_F32_INCREMENTS and MCQ_F32_ABSOLUTE (absolute rows: the coordinates relative to the track's first waypoint, rounded to float)
  origin   none, the tracks' own first waypoints, FAR = (1.5e6, -2.5e6) m
  closed   the ring as it is (closure defect ~1e-6 m: float rounding alone), and UNCLOSED: 0.5 / n * linspace(0.5, 1.5, n) added to the x
           increments before they are rounded to float -- a defect of 0.5 m, whose distribution over the ring becomes visible.  (Absolute
           rows have no closure: that layout runs once per n and origin.)
  and one launch per n whose middle track has a NaN x increment in the middle: its x column is NaN throughout, nothing else moves.

Solves.  SOLVES: (batch, n) with batch * n = 1, 2, 1, 0, 3, 3, 2 modulo 4 -- every scalar tail of the streaming conversions --, tracks
glue_cases.f32_tracks (the families in turn) under glue's settings, at which every status is 0; NARROW: the middle of three tracks narrower than
the vehicle; NAN: a NaN increment in the middle track.

Conversions.  COUNTS, and the values of narrow_values / widen_values: the special values first, seeded finite values of every magnitude behind."""
import functools

import numpy as np

import glue_cases as gc
from global_racetrajectory_optimization_amd import engine

REBUILD_N = (3, 4, 5, 63, 64, 65, 127, 128, 129, 191, 192, 193, 2047, 2048, 2049, 4097)
FAMILIES = tuple(gc.FAMILIES)           # trefoil, peanut, stadium
ORIGINS = ("none", "own", "far")
FAR = (1.5e6, -2.5e6)
DEFECT = 0.5

SOLVES = ((1, 5), (2, 5), (3, 63), (2, 64), (3, 65), (3, 129), (2, 257))
KAPPA_BOUND, W_VEH = gc.F32_KAPPA_BOUND, gc.F32_W_VEH
NARROW_BATCH_N = (3, 63)
NAN_BATCH_N = (3, 65)

BIG = 4 * 256 * 4096 + 5                # past the 4096-workgroup cap of the conversions' grid: a second trip of the stride loop, and a tail
COUNTS = tuple(range(1, 10)) + (1023, 1024, 1025, BIG)


def _rings(n):
    return np.stack([np.array(gc.ring(f, n)[0]) for f in FAMILIES])


@functools.lru_cache(maxsize=None)
def increments(n, closed=True):
    """(float32 rows [3, n, 4] in the increment layout, float64 origins [3, 2]) of the three families at n."""
    ref = _rings(n)
    rows32, org = engine.rows_to_increments(ref)
    if not closed:
        d = np.roll(ref[..., :2], -1, axis=-2) - ref[..., :2]
        d[..., 0] += DEFECT / n * np.linspace(0.5, 1.5, n)
        rows32 = rows32.copy()
        rows32[..., :2] = d
    for a in (rows32, org):
        a.setflags(write=False)
    return rows32, org


@functools.lru_cache(maxsize=None)
def absolute(n):
    """(float32 rows [3, n, 4] = the coordinates relative to each track's first waypoint, those waypoints [3, 2])."""
    ref = _rings(n)
    org = np.ascontiguousarray(ref[:, 0, :2])
    rows32 = ref.copy()
    rows32[..., :2] -= org[:, None, :]
    rows32 = rows32.astype(np.float32)
    for a in (rows32, org):
        a.setflags(write=False)
    return rows32, org


def origin_of(which, own):
    return {"none": None, "own": own, "far": np.tile(np.array(FAR), (own.shape[0], 1))}[which]


def rebuild_launches(n):
    """(tag, layout, rows32 [3, n, 4], origin [3, 2] or None) of every launch at n."""
    out = []
    for which in ORIGINS:
        for closed in (True, False):
            rows32, own = increments(n, closed)
            out.append(("inc.%s.%s" % ("closed" if closed else "unclosed", which), engine.F32_INCREMENTS, rows32, origin_of(which, own)))
        rows32, own = absolute(n)
        out.append(("abs.%s" % which, engine.F32_ABSOLUTE, rows32, origin_of(which, own)))
    return out


def nan_rows(n, closed=True):
    rows32, own = increments(n, closed)
    rows32 = rows32.copy()
    rows32[1, n // 2, 0] = np.nan
    return rows32, own


# ---- solves ------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def solve_rows(batch, n):
    """(increment rows [batch, n, 4] float32, origins [batch, 2]) of glue_cases.f32_tracks(batch, n)."""
    rows32, org = engine.rows_to_increments(gc.f32_tracks(batch, n))
    for a in (rows32, org):
        a.setflags(write=False)
    return rows32, org


def narrow_rows():
    """NARROW_BATCH_N with the middle track 0.9 m + 0.9 m wide: narrower than W_VEH."""
    rows32, org = solve_rows(*NARROW_BATCH_N)
    rows32 = rows32.copy()
    rows32[1, :, 2:] = np.float32(0.9)
    assert 2 * 0.9 < W_VEH
    return rows32, org


def nan_solve_rows():
    rows32, org = solve_rows(*NAN_BATCH_N)
    rows32 = rows32.copy()
    rows32[1, NAN_BATCH_N[1] // 2, 0] = np.nan
    return rows32, org


# ---- conversions -------------------------------------------------------------------------------------------------------------------------------
def _f32_next(x, up):
    return np.nextafter(np.float32(x), np.float32(np.inf if up else -np.inf))


@functools.lru_cache(maxsize=None)
def narrow_specials():
    """float64 inputs of mcq_narrow_kernel at which a conversion can go wrong."""
    one = np.float32(1.0)
    up1, up2 = float(_f32_next(one, True)), float(_f32_next(_f32_next(one, True), True))       # 1 + 2^-23 (odd), 1 + 2^-22 (even)
    tie_lo, tie_hi = 0.5 * (1.0 + up1), 0.5 * (up1 + up2)           # exact ties: the first rounds DOWN to even (1), the second UP to even
    fmax = float(np.finfo(np.float32).max)
    edge = fmax + 2.0 ** 103                                        # half an ulp of FLT_MAX above it: the tie goes to 2^128 = infinity
    tiny, sub = 2.0 ** -149, 2.0 ** -126                            # the smallest float subnormal; the smallest normal
    v = [tie_lo, tie_hi, -tie_lo, -tie_hi, np.nextafter(tie_lo, 2.0), np.nextafter(tie_lo, 0.0), np.nextafter(tie_hi, 2.0), np.nextafter(tie_hi, 0.0),
         fmax, np.nextafter(edge, 0.0), edge, -np.nextafter(edge, 0.0), -edge, 1e39, -1e39,
         sub, np.nextafter(sub, 0.0), 0.75 * sub, 1.5 * tiny, 2.5 * tiny, 3.5 * tiny, tiny, -tiny,
         0.5 * tiny, np.nextafter(0.5 * tiny, 1.0), -0.5 * tiny, -np.nextafter(0.5 * tiny, 1.0), 0.25 * tiny, 5e-324, -5e-324, 1e-300,
         0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0, 4.0, 1e-3, 0.1, 1.0 / 3.0]
    a = np.array(v, dtype=np.float64)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def widen_specials():
    f = np.finfo(np.float32)
    a = np.array([f.smallest_subnormal, -f.smallest_subnormal, 3 * f.smallest_subnormal, np.nextafter(f.tiny, np.float32(0)), f.tiny, 0.0, -0.0,
                  np.inf, -np.inf, np.nan, f.max, -f.max, 1.0, -1.0, 0.1, _f32_next(1.0, True)], dtype=np.float32)
    a.setflags(write=False)
    return a


def _fill(specials, count, dtype, seed):
    rng = np.random.default_rng([seed, count])
    body = (rng.standard_normal(count) * 10.0 ** rng.uniform(-12.0, 12.0, count)).astype(dtype)
    k = specials.shape[0]
    if count >= k:
        body[:k] = specials                         # at the front, and once more at the very end: the scalar tail
        body[count - k:] = specials[::-1]
    else:
        body[:] = specials[(np.arange(count) * 7 + count) % k]
    return body


@functools.lru_cache(maxsize=None)
def narrow_values(count):
    a = _fill(narrow_specials(), count, np.float64, 32)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def widen_values(count):
    a = _fill(widen_specials(), count, np.float32, 64)
    a.setflags(write=False)
    return a
