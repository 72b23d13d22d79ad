"""The reference of the fp32 boundary's edges tests (tests/f32_ref.py) and their case table (tests/f32_cases.py) on their own: no engine, no GPU.

  - rebuild_ld against itself: its float64 evaluation stays within the guard of the longdouble one, a direct sum per waypoint agrees, the absolute
    layout is one rounding.
  - the kernel's summation order restated in numpy (f32_ref.kernel_order) and engine.increments_to_rows, each under its own derived guard, on the
    whole rebuild table.
  - what the table relies on: the planted error of f32_ref.mutant_order exceeds the guard on every unclosed launch with n > 64, and on the closed
    rings without a far origin wherever the statement below says so."""
import numpy as np
import pytest

import f32_cases as fc
import f32_ref
from global_racetrajectory_optimization_amd import engine

LD = f32_ref.LD


def inc_launches(n):
    return [launch for launch in fc.rebuild_launches(n) if launch[1] == engine.F32_INCREMENTS]


RATIO = {"kernel": 0.0, "host": 0.0, "host_in_kernel_guard": 0.0}


def test_longdouble_is_wider_than_float64():
    assert np.finfo(LD).nmant > np.finfo(np.float64).nmant, "numpy.longdouble is float64 here: the reference would be no reference"


@pytest.mark.parametrize("n", fc.REBUILD_N)
def test_reference_against_itself(n):
    for tag, layout, rows32, origin in fc.rebuild_launches(n):
        want = f32_ref.rebuild_ld(rows32, origin, layout)
        assert want.dtype == LD and want.shape == rows32.shape
        assert np.array_equal(want[..., 2:], rows32[..., 2:].astype(LD))
        o = np.zeros((3, 2)) if origin is None else origin
        if layout == engine.F32_ABSOLUTE:
            assert np.array_equal(want[..., :2], o.astype(LD)[:, None, :] + rows32[..., :2].astype(LD))
            continue
        # a direct sum per waypoint, written without cumsum
        d = rows32[..., :2].astype(LD)
        total = d.sum(axis=1)
        for i in sorted({0, 1, n // 2, n - 1}):
            direct = o.astype(LD) + d[:, :i].sum(axis=1) - LD(i) * total / LD(n)
            assert np.max(np.abs(direct - want[:, i, :2])) <= 4 * n * np.finfo(LD).eps * f32_ref._scale(origin, rows32).max()
        # the same formula evaluated in float64 (numpy's cumsum: n roundings) stays within the host's guard
        r = rows32.astype(np.float64)
        cs = np.cumsum(r[..., :2], axis=1)
        f64 = r.copy()
        f64[..., :2] = o[:, None, :] + np.concatenate((np.zeros((3, 1, 2)), cs[:, :-1]), axis=1) - np.arange(n)[:, None] * (cs[:, -1:] / n)
        assert np.all(f32_ref.dev(f64, want) <= f32_ref.host_guard(n, origin, rows32)), (n, tag)
        # closes: one more step from the last waypoint returns to the origin up to the guard
        back = want[:, -1, :2] + d[:, -1] - total / LD(n)
        assert np.all(np.max(np.abs(back - o.astype(LD)), axis=1).astype(np.float64) <= f32_ref.guard(n, origin, rows32))


def test_the_table_is_what_its_header_says():
    assert sorted((b * n) % 4 for b, n in fc.SOLVES) == [0, 1, 1, 2, 2, 3, 3] and max(n for _, n in fc.SOLVES) == 257
    assert fc.BIG // 4 > 256 * 4096 and fc.BIG % 4 == 1 and {c % 4 for c in fc.COUNTS} == {0, 1, 2, 3}
    for n in fc.REBUILD_N:
        closed, own = fc.increments(n)
        again, org = engine.rows_to_increments(np.stack([np.array(fc.gc.ring(f, n)[0]) for f in fc.FAMILIES]))
        assert np.array_equal(closed, again) and np.array_equal(own, org)
        unclosed, _ = fc.increments(n, closed=False)
        defect = unclosed[..., 0].astype(LD).sum(axis=1) - closed[..., 0].astype(LD).sum(axis=1)
        assert np.all(np.abs(defect - fc.DEFECT) <= 1e-3), (n, defect)            # (0.5 m up to the float rounding of n increments)
        assert np.all(np.abs(closed[..., :2].astype(LD).sum(axis=1)) <= 1e-4)
        assert np.array_equal(unclosed[..., 1:], closed[..., 1:])
        assert np.all(np.abs(own[2]) > 100.0) and not np.any(fc.origin_of("far", own) == own)        # the stadium sits away from the origin


def test_the_special_values_round_as_their_names_say():
    f = np.finfo(np.float32)
    with np.errstate(over="ignore", under="ignore"):
        v = fc.narrow_specials()
        r = v.astype(np.float32)
    up1 = np.nextafter(np.float32(1), np.float32(2))
    assert r[0] == 1.0 and r[1] == np.nextafter(up1, np.float32(2)) and r[4] == up1 and r[5] == 1.0          # ties to even, and next to them
    assert r[8] == f.max and r[9] == f.max and np.isposinf(r[10]) and r[11] == -f.max and np.isneginf(r[12]) and np.isposinf(r[13]) and np.isneginf(r[14])
    sub = r[(np.abs(v) < 2.0 ** -126) & (v != 0)]
    assert sub.size >= 12 and np.all(np.abs(sub) <= f.tiny) and np.any(sub == f.tiny) and np.any(sub != 0) and np.any(sub == 0)
    assert np.signbit(r[v == 0]).tolist() == [False, True] and np.signbit(r[np.abs(v) == 5e-324]).tolist() == [False, True]
    assert np.isnan(r[np.isnan(v)]).all() and np.isnan(v).sum() == 1
    for count in fc.COUNTS[:-1]:
        a, w = fc.narrow_values(count), fc.widen_values(count)
        assert a.shape == w.shape == (count,) and a.dtype == np.float64 and w.dtype == np.float32
    w = fc.widen_specials()
    assert np.any((np.abs(w) < f.tiny) & (w != 0)) and np.any(np.isnan(w)) and np.any(np.isinf(w)) and np.any(w == f.max)


@pytest.mark.parametrize("n", fc.REBUILD_N)
def test_kernel_order_and_host_restatement_under_their_guards(n):
    """f32_ref.kernel_order under guard (3 per + 12 roundings); engine.increments_to_rows under host_guard (2 n + 12 roundings: its cumsum rounds once
    per waypoint)."""
    for tag, layout, rows32, origin in inc_launches(n):
        want = f32_ref.rebuild_ld(rows32, origin, layout)
        g, hg = f32_ref.guard(n, origin, rows32), f32_ref.host_guard(n, origin, rows32)
        ko = np.stack([f32_ref.kernel_order(rows32[k], None if origin is None else origin[k]) for k in range(3)])
        d = f32_ref.dev(ko, want)
        print("n=%d %s: kernel order deviates by %s, guard %s" % (n, tag, d, g))
        assert np.all(d <= g), (n, tag, d, g)
        assert np.array_equal(ko[:, 0, :2], np.zeros((3, 2)) if origin is None else origin) and np.array_equal(ko[..., 2:], rows32[..., 2:].astype(np.float64))
        host = engine.increments_to_rows(rows32, origin)
        dh = f32_ref.dev(host, want)
        print("n=%d %s: engine.increments_to_rows deviates by %s, its guard %s" % (n, tag, dh, hg))
        assert np.all(dh <= hg), (n, tag, dh, hg)
        RATIO["kernel"] = max(RATIO["kernel"], float(np.max(d / g)))
        RATIO["host"] = max(RATIO["host"], float(np.max(dh / hg)))
        RATIO["host_in_kernel_guard"] = max(RATIO["host_in_kernel_guard"], float(np.max(dh / g)))


def test_the_table_tells_the_misplaced_defect_apart():
    """What the rebuild table relies on.  The mutant spreads the closure defect with i0 + 1 instead of i0 on every lane but lane 0 -- an error of
    defect / n per waypoint, jumping at lane boundaries, which the float alpha of a solve hides (2e-9 .. 1e-8 m against 2.4e-7 m).  It exceeds the
    guard on every track of EVERY unclosed launch, n <= 64 included (lane l holds waypoint l there); on the closed rings (defect ~1e-6 m) without an
    origin it does so on at least one of the three tracks at every n, and the far origin hides it there from n = 191 on -- which is why the far
    origin is not the only variant."""
    seen_closed = 0
    for n, (tag, layout, rows32, origin) in [(n, launch) for n in fc.REBUILD_N for launch in inc_launches(n)]:
        want = f32_ref.rebuild_ld(rows32, origin, layout)
        mu = np.stack([f32_ref.mutant_order(rows32[k], None if origin is None else origin[k]) for k in range(3)])
        d, g = f32_ref.dev(mu, want), f32_ref.guard(n, origin, rows32)
        if "unclosed" in tag:
            assert np.all(d > g), "the table cannot see the mutant at n=%d %s: %s against %s" % (n, tag, d, g)
        elif tag.endswith("none") and np.any(d > g):
            seen_closed += 1
    assert seen_closed == len(fc.REBUILD_N), seen_closed


def test_report():
    """Last: the largest ratios deviation / guard over the table (docs/NOTEBOOK.md, "fp32 boundary edges", quotes them) -- of the comparisons this
    process has run (under pytest-xdist others may have run elsewhere)."""
    print("fp32 boundary, restatements on the CPU: kernel order at most %.3f of its guard, engine.increments_to_rows at most %.3f of its own guard "
          "(%.3f of the kernel's)" % (RATIO["kernel"], RATIO["host"], RATIO["host_in_kernel_guard"]))
    assert RATIO["kernel"] <= 1.0 and RATIO["host"] <= 1.0
