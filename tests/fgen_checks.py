"""The bodies of the friction-map generation tests, shared by the SIMT interpreter's run (tests/test_emu_fgen.py) and the MI355X's
(tests/test_gpu_fgen.py): every body takes the engine under test.  Cases: tests/fgen_cases.py.  What a result is held to: matplotlib's recorded
verdicts and the reference's recorded boundaries (tests/golden/friction_gen/reference.npz, scripts/make_golden_friction_gen.py) -- EQUAL, no
tolerance -- and, for contour vertices and unrecorded tracks, the restatement tests/fgen_ref.py, which tests/test_fgen_ref.py pins to the same
recording bit for bit."""
import hashlib
import math
import os

import numpy as np
import pytest

import fgen_cases as fc
import fgen_ref as fr
from conftest import load_golden
from global_racetrajectory_optimization_amd import engine, friction

FILL = 7.25             # what outputs are pre-filled with: beyond a count nothing may be overwritten
FILL_B, FILL_I = 0x5a, 77
_CACHE = {}


def rec():
    if "z" not in _CACHE:
        _CACHE["z"] = load_golden("friction_gen/reference")
    return _CACHE["z"]


def recorded_paths():
    """(points [k, 2], verdicts bool [cases, k], tiny bool [4, radii, k])."""
    if "paths" not in _CACHE:
        z = rec()
        pts = z["paths/points"]
        _CACHE["paths"] = (pts, np.unpackbits(z["paths/verdicts"], axis=1)[:, :pts.shape[0]].astype(bool),
                           np.unpackbits(z["paths/tiny"], axis=2)[:, :, :pts.shape[0]].astype(bool))
    return _CACHE["paths"]


def recorded_cells(key_mask, reftrack, cw):
    """The cells the reference keeps: numpy.arange's grid under matplotlib's recorded mask."""
    x0, x1, y0, y1 = fr.grid_range(reftrack)
    xg, yg = np.arange(x0, x1 + 0.1, cw), np.arange(y0, y1 + 0.1, cw)
    pts = fr.grid_points(xg, yg)
    return pts[np.unpackbits(rec()[key_mask])[:pts.shape[0]].astype(bool)], xg, yg


def _bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def paths_prefilled(eng, verts, radii, pts, vmax=None, contours=True):
    """mcq_points_in_path_device on pre-filled outputs with a guard row behind each: (inside bool [k, count], status [k], contours list)."""
    verts = [np.asarray(v, dtype=np.float64).reshape(-1, 2) for v in verts]
    pts = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 2)
    k, count = len(verts), pts.shape[0]
    vs = np.array([v.shape[0] for v in verts], dtype=np.int32)
    vmax = vmax or max(int(vs.max()), 1)
    pad = np.full((k, vmax, 2), np.nan)         # (rows behind a path's count are never read: a NaN there must not refuse it)
    for i, v in enumerate(verts):
        pad[i, :vs[i]] = v
    with eng.scope() as dev:
        d_in = dev.up(np.full(k * count + 64, FILL_B, dtype=np.uint8))
        d_st = dev.up(np.full(k + 1, FILL_I, dtype=np.int32))
        d_c = dev.up(np.full((k, 2 * vmax, 2), FILL)) if contours else None
        d_cc = dev.up(np.full(k + 1, FILL_I, dtype=np.int32)) if contours else None
        eng.contains_points_device(k, vmax, dev.up(vs), dev.up(pad), dev.up(np.asarray(radii, dtype=np.float64)), count,
                                   dev.up(pts) if count else None, d_in if count else None, d_st, d_c, d_cc)
        raw, st = eng.download(d_in, (k * count + 64,), np.uint8), eng.download(d_st, (k + 1,), np.int32)
        assert (raw[k * count:] == FILL_B).all() and st[k] == FILL_I, "wrote behind its outputs"
        assert np.isin(raw[:k * count], (0, 1)).all(), "a verdict is neither 0 nor 1"
        cont = None
        if contours:
            c, cc = eng.download(d_c, (k, 2 * vmax, 2), np.float64), eng.download(d_cc, (k + 1,), np.int32)
            assert cc[k] == FILL_I and all((c[i, cc[i]:] == FILL).all() for i in range(k)), "contour rows beyond the count were written"
            cont = [c[i, :cc[i]].copy() for i in range(k)]
    return raw[:k * count].reshape(k, count).astype(bool), st[:k], cont


# ---- 1. contains_points with a radius -----------------------------------------------------------------------------------------------------------
def check_paths(eng):
    """Every (polygon, radius) of the table in ONE launch on the whole point set: matplotlib's verdicts, and the restatement's contour vertices."""
    pts, want, _ = recorded_paths()
    polys, cases = fc.polygons(), fc.path_cases()
    inside, st, cont = paths_prefilled(eng, [polys[n] for n, _ in cases], [r for _, r in cases], pts)
    assert (st == 0).all()
    for k, (n, r) in enumerate(cases):
        assert _bits(cont[k], fr.contour(polys[n], r)), "%s at radius %g: contour vertices" % (n, r)
        assert np.array_equal(inside[k], want[k]), "%s at radius %g: %d verdicts differ" % (n, r, int((inside[k] != want[k]).sum()))
    # what the table is there for
    size = {(n, r): cont[k].shape[0] for k, (n, r) in enumerate(cases)}
    assert size[("star256", 6.0)] == fc.TILE and size[("star255", 6.0)] == fc.TILE - 2 and size[("star257", 6.0)] == fc.TILE + 2
    assert size[("circle257", -2.0)] == 257 and size[("duplicates", 2.0)] < 2 * 4 + 1 and size[("two", 6.0)] == 0
    assert want[cases.index(("two", 6.0))].sum() == 0 and want[cases.index(("square_cw", 2.0))].sum() != want[cases.index(("square_ccw", 2.0))].sum()


def check_tiny_paths(eng):
    pts, _, want = recorded_paths()
    for k, v in enumerate(fc.tiny_paths()):
        inside, st, cont = paths_prefilled(eng, [v] * len(fc.RADII), fc.RADII, pts, vmax=3)
        assert (st == 0).all() and np.array_equal(inside, want[k]), "a path of %d vertices" % k
        assert all((c.shape[0] > 0) == (k == 3) for c in cont)
    assert want[:3].sum() == 0 and want[3].all(axis=1).sum() == 0 and want[3].any(axis=1).all()


PICK = (("spike", 2.0), ("star256", -6.0), ("square_cw", 0.0), ("reversal", -0.5))


def check_point_counts(eng):
    """Point counts around a wave and a workgroup, the entry and the Python surface."""
    pts, want, _ = recorded_paths()
    polys, cases = fc.polygons(), fc.path_cases()
    rows = [cases.index(c) for c in PICK]
    sel = np.flatnonzero(want[rows].any(axis=0) & ~want[rows].all(axis=0))[:257]          # points the four paths disagree on
    assert sel.shape[0] == 257
    for count in fc.COUNTS:
        inside, st, _ = paths_prefilled(eng, [polys[n] for n, _ in PICK], [r for _, r in PICK], pts[sel[:count]], contours=False)
        assert (st == 0).all() and np.array_equal(inside, want[rows][:, sel[:count]]), count
    ins, st = eng.contains_points_batch([polys[n] for n, _ in PICK], pts[sel], [r for _, r in PICK])
    assert ins.dtype == bool and np.array_equal(ins, want[rows][:, sel]) and (st == 0).all()
    ins, st, cont = eng.contains_points_batch([polys["spike"]], pts[sel[:9]], 2.0, want_contours=True)
    assert np.array_equal(ins[0], want[rows[0]][sel[:9]]) and _bits(cont[0], fr.contour(polys["spike"], 2.0))
    assert eng.contains_points_batch([polys["spike"]], np.zeros((0, 2)), 2.0)[0].shape == (1, 0)


def check_nonfinite_points(eng):
    pts, want, _ = recorded_paths()
    polys, cases = fc.polygons(), fc.path_cases()
    rows = [cases.index(c) for c in PICK]
    sel = np.flatnonzero(want[rows[0]])[:70]
    q = pts[sel].copy()
    for k, v in fc.NONFINITE.items():
        q[k] = v
    inside, st, _ = paths_prefilled(eng, [polys[n] for n, _ in PICK], [r for _, r in PICK], q, contours=False)
    good = np.array([k not in fc.NONFINITE for k in range(70)])
    assert (st == 0).all() and not inside[:, ~good].any() and np.array_equal(inside[:, good], want[rows][:, sel[good]])
    for k in fc.NONFINITE:
        alone, _, _ = paths_prefilled(eng, [polys["spike"]], [2.0], q[k:k + 1], contours=False)
        assert not alone.any(), "alone"


def check_path_refusals(eng):
    """A NaN vertex, an infinite radius, a count outside 0 .. vmax: False everywhere, their neighbours untouched; each refusal alone."""
    pts, want, _ = recorded_paths()
    polys, cases = fc.polygons(), fc.path_cases()
    sub = pts[::37]
    nan_v = polys["spike"].copy()
    nan_v[3, 0] = np.nan
    verts, radii = [polys["spike"], nan_v, polys["notch"], polys["spike"], polys["triangle"]], [2.0, 2.0, -2.0, np.inf, np.nan]
    inside, st, cont = paths_prefilled(eng, verts, radii, sub)
    assert st.tolist() == [0, fr.ST_NONFINITE, 0, fr.ST_NONFINITE, fr.ST_NONFINITE]
    assert not inside[[1, 3, 4]].any() and all(cont[k].shape[0] == 0 for k in (1, 3, 4))
    assert np.array_equal(inside[0], want[cases.index(("spike", 2.0))][::37]) and np.array_equal(inside[2], want[cases.index(("notch", -2.0))][::37])
    for k in (1, 3, 4):
        a, s, c = paths_prefilled(eng, [verts[k]], [radii[k]], sub)
        assert s[0] == fr.ST_NONFINITE and not a.any() and c[0].shape[0] == 0
    with eng.scope() as dev:        # a count the buffer cannot hold
        d_in, d_st = dev.up(np.full(sub.shape[0] * 2, FILL_B, dtype=np.uint8)), dev.new(8)
        pad = np.zeros((2, 7, 2))
        pad[0], pad[1] = polys["spike"], polys["notch"]
        for bad_v in (8, -1):
            eng.contains_points_device(2, 7, dev.up(np.array([bad_v, 7], dtype=np.int32)), dev.up(pad), dev.up(np.array([2.0, -2.0])), sub.shape[0],
                                       dev.up(sub), d_in, d_st)
            got, s = eng.download(d_in, (2, sub.shape[0]), np.uint8), eng.download(d_st, (2,), np.int32)
            assert s.tolist() == [fr.ST_FEW, 0] and not got[0].any() and np.array_equal(got[1].astype(bool), inside[2])


def check_path_layout(eng):
    """A ragged batch alone, reversed, beside others and in wider buffers: the same bytes."""
    pts, _, _ = recorded_paths()
    polys = fc.polygons()
    sub = pts[::11]
    names = [("triangle", 2.0), ("star257", 6.0), ("duplicates", -2.0), ("two", 2.0), ("circle255", -6.0), ("bowtie", 0.5), ("short_edges", 6.0)]
    verts, radii = [polys[n] for n, _ in names], [r for _, r in names]
    inside, st, cont = paths_prefilled(eng, verts, radii, sub)
    for k in range(len(names)):
        a, s, c = paths_prefilled(eng, verts[k:k + 1], radii[k:k + 1], sub)
        assert _bits(a[0], inside[k]) and s[0] == st[k] and _bits(c[0], cont[k]), "%s alone" % names[k][0]
    a, s, c = paths_prefilled(eng, verts[::-1], radii[::-1], sub)
    assert _bits(a[::-1], inside) and _bits(s[::-1], st) and all(_bits(x, y) for x, y in zip(c[::-1], cont)), "reversed"
    a, s, c = paths_prefilled(eng, [polys["notch"]] + verts + [polys["spike"]], [2.0] + radii + [-0.5], sub, vmax=300)
    assert _bits(a[1:-1], inside) and all(_bits(x, y) for x, y in zip(c[1:-1], cont)), "beside others, in wider buffers"
    a2, _, _ = paths_prefilled(eng, verts, radii, np.vstack((sub[5:], sub)), contours=False)
    assert _bits(a2[:, sub.shape[0] - 5:], inside), "points beside others"


def check_path_arguments(eng):
    with eng.scope() as dev:
        d = dev.new(4096)
        ok = dict(paths=1, vmax=3, d_v=None, d_verts=d, d_radius=d, count=1, d_xy=d, d_inside=d, d_status=d)
        for bad in (dict(paths=0), dict(vmax=0), dict(count=-1), dict(d_verts=None), dict(d_radius=None), dict(d_status=None), dict(d_xy=None),
                    dict(d_inside=None), dict(d_contour=d), dict(d_contour_count=d)):
            with pytest.raises(engine.EngineError, match=r"\(-1\)"):
                eng.contains_points_device(**dict(ok, **bad))
        with pytest.raises(engine.EngineError, match=r"\(-3\)"):
            eng.contains_points_device(**dict(ok, paths=65536))
    with pytest.raises(ValueError):
        eng.contains_points_batch([], np.zeros((1, 2)))


# ---- 2. the generation entry ------------------------------------------------------------------------------------------------------------------
def gen_prefilled(eng, tracks, cw, sides=None, cmax=None, nmax=None, cells=True, bounds=True):
    """mcq_friction_gen_device on pre-filled outputs.  cmax None: the largest count (a counting call first).  Returns a dict; nothing beyond a
    track's count, or beyond its n boundary rows, may have been written."""
    tracks = [np.asarray(t, dtype=np.float64) for t in tracks]
    ns = np.array([t.shape[0] for t in tracks], dtype=np.int32)
    k = len(tracks)
    nmax = nmax or max(int(ns.max()), 3)
    ref = np.full((k, nmax, 4), np.nan)         # (rows behind n are never read)
    for i, t in enumerate(tracks):
        ref[i, :ns[i]] = t
    with eng.scope() as dev:
        d_ref, d_n = dev.up(ref), dev.up(ns)
        d_side = dev.up(np.array([s == "right" for s in sides], dtype=np.int32)) if sides is not None else None
        d_grid, d_cnt, d_st = dev.up(np.full((k, 6), FILL)), dev.up(np.full(k + 1, FILL_I, dtype=np.int32)), dev.up(np.full(k + 1, FILL_I, dtype=np.int32))
        if cmax is None:
            eng.friction_gen_device(k, nmax, d_n, d_ref, cw, d_side, 0, None, None, d_grid, d_cnt, None, d_st)
            only = eng.download(d_cnt, (k,), np.int32)
            cmax = int(only.max())
        d_br, d_bl = (dev.up(np.full((k, nmax, 2), FILL)), dev.up(np.full((k, nmax, 2), FILL))) if bounds else (None, None)
        d_cells = dev.up(np.full((k, cmax + 1, 2), FILL)) if cells else None
        eng.friction_gen_device(k, nmax, d_n, d_ref, cw, d_side, cmax, d_br, d_bl, d_grid, d_cnt, d_cells, d_st)
        cnt, st = eng.download(d_cnt, (k + 1,), np.int32), eng.download(d_st, (k + 1,), np.int32)
        assert cnt[k] == FILL_I and st[k] == FILL_I
        out = dict(counts=cnt[:k], status=st[:k], grids=eng.download(d_grid, (k, 6), np.float64), cmax=cmax, cells=None, bound_right=None)
        if cells:
            # (the buffer is [k][cmax] for the entry; the rows of the guard's extra column are read back flat)
            flat = eng.download(d_cells, (k * (cmax + 1), 2), np.float64)
            per = flat[:k * cmax].reshape(k, cmax, 2)
            assert (flat[k * cmax:] == FILL).all(), "wrote behind cells_out"
            got = [min(int(cnt[i]), cmax) for i in range(k)]
            assert all((per[i, got[i]:] == FILL).all() for i in range(k)), "cells beyond the count were written"
            out["cells"] = [per[i, :got[i]].copy() for i in range(k)]
        if bounds:
            br, bl = eng.download(d_br, (k, nmax, 2), np.float64), eng.download(d_bl, (k, nmax, 2), np.float64)
            rows = [min(max(int(n), 0), nmax) for n in ns]
            assert all((br[i, rows[i]:] == FILL).all() and (bl[i, rows[i]:] == FILL).all() for i in range(k)), "boundary rows beyond n were written"
            out["bound_right"], out["bound_left"] = [br[i, :rows[i]].copy() for i in range(k)], [bl[i, :rows[i]].copy() for i in range(k)]
    return out


def check_small_track(eng, name):
    """n = 3, the closed / open threshold from both sides, an open arc, the cell widths 2.5, 0.3 and 0.1: the recorded masks and boundaries."""
    z = rec()
    ref, cw = z["small/%s/reftrack" % name], float(z["small/%s/cellwidth" % name])
    want, xg, yg = recorded_cells("small/%s/mask" % name, ref, cw)
    assert bool(z["small/%s/closed" % name]) == fr.check_isclosed_refline(ref[:, :2]) == friction.check_isclosed_refline(ref[:, :2])
    g = gen_prefilled(eng, [ref], cw, [fc.SMALL_INSIDE])
    assert g["status"][0] == 0 and g["counts"][0] == want.shape[0] > 0
    assert _bits(g["cells"][0], want), "%s: the cells differ from the reference's" % name
    assert _bits(g["bound_right"][0], z["small/%s/bound_right" % name]) and _bits(g["bound_left"][0], z["small/%s/bound_left" % name])
    assert g["grids"][0].tolist() == [float(v) for v in fr.grid_range(ref)] + [xg.shape[0], yg.shape[0]]
    if z["small/%s/closed" % name]:     # the other side: the offset follows the orientation, and nothing is left
        other = gen_prefilled(eng, [ref], cw, ["right"])
        assert other["counts"][0] == fr.gen_cells(ref, cw, True)[0].shape[0] and other["status"][0] == 0
    else:                               # an open track does not read the side
        assert _bits(gen_prefilled(eng, [ref], cw, ["right"])["cells"][0], want) and _bits(gen_prefilled(eng, [ref], cw, None)["cells"][0], want)


def check_whole_track(eng, track, widths=(2.0,)):
    """A reference track whole, both inside_trackbound values (one of them gives the reference's empty map)."""
    z = rec()
    ref = z[track + "/reftrack"]
    for cw in widths:
        sides = ("right", "left") if cw == 2.0 else (fc.INSIDE[track],)
        g = gen_prefilled(eng, [ref] * len(sides), cw, sides)
        for k, side in enumerate(sides):
            want, xg, yg = recorded_cells("%s/mask_%s" % (track, side) + ("" if cw == 2.0 else "_%r" % cw), ref, cw)
            assert g["status"][k] == 0 and g["counts"][k] == want.shape[0], (track, cw, side, g["counts"][k], want.shape[0])
            assert (want.shape[0] > 0) == (side == fc.INSIDE[track])
            assert _bits(g["cells"][k], want), "%s at %g, inside %s: the cells differ from the reference's" % (track, cw, side)
            assert _bits(g["bound_right"][k], z[track + "/bound_right"]) and _bits(g["bound_left"][k], z[track + "/bound_left"])
            if cw == 2.0:
                assert _bits(g["grids"][k], z[track + "/grid"])


def check_refusals(eng):
    """A NaN waypoint, an infinite width, a zero gradient and a track of two rows inside a batch: refused with count 0 and their bit, the tracks
    beside them untouched; every refusal alone; cmax = count and count - 1; counting calls."""
    z = rec()
    good_a, good_b = z["small/oval_2p5/reftrack"], z["small/open_arc/reftrack"]
    bad = fc.refused_tracks()
    alone = {k: gen_prefilled(eng, [t], 2.5, ["left"]) for k, t in (("a", good_a), ("b", good_b))}
    order = ["nan", "a", "zero_gradient", "inf_width", "b", "two_rows"]
    tracks = [bad[k][0] if k in bad else (good_a if k == "a" else good_b) for k in order]
    g = gen_prefilled(eng, tracks, 2.5, ["left"] * len(order))
    for i, k in enumerate(order):
        if k in bad:
            assert g["status"][i] == bad[k][1] == fr.status_of(bad[k][0]) and g["counts"][i] == 0 and g["cells"][i].shape[0] == 0, k
            assert g["grids"][i, 4:].tolist() == [0.0, 0.0] and np.isnan(g["grids"][i, :4]).all()
            assert np.isnan(g["bound_right"][i]).any() and np.isnan(g["bound_left"][i]).any()
            one = gen_prefilled(eng, [bad[k][0]], 2.5, ["left"])
            assert one["status"][0] == bad[k][1] and one["counts"][0] == 0 and _bits(one["bound_right"][0], g["bound_right"][i]), "%s alone" % k
        else:
            assert g["status"][i] == 0 and all(_bits(g[f][i], alone[k][f][0]) for f in ("cells", "bound_right", "bound_left", "grids")), k
    # the zero gradient is a boundary that is not finite, computed where it occurs
    zg = g["bound_right"][order.index("zero_gradient")]
    assert np.isnan(zg[12]).all() and np.isfinite(zg[:12]).all() and np.isfinite(zg[13:]).all()
    check_grid_refusal(eng, good_a, alone["a"])
    count, full = int(alone["a"]["counts"][0]), alone["a"]["cells"][0]
    fit = gen_prefilled(eng, [good_a], 2.5, ["left"], cmax=count)
    assert fit["status"][0] == 0 and _bits(fit["cells"][0], full)
    small = gen_prefilled(eng, [z["small/n3/reftrack"]], 2.5, ["left"])
    assert 0 < small["counts"][0] < count - 1
    cut = gen_prefilled(eng, [good_a, z["small/n3/reftrack"]], 2.5, ["left"] * 2, cmax=count - 1)      # (only the first outgrows the buffer)
    assert cut["status"].tolist() == [fr.ST_OVERFLOW, 0] and cut["counts"].tolist() == [count, int(small["counts"][0])]
    assert _bits(cut["cells"][0], full[:count - 1]) and _bits(cut["cells"][1], small["cells"][0])
    none = gen_prefilled(eng, [good_a], 2.5, ["left"], cmax=0)
    assert none["status"][0] == fr.ST_OVERFLOW and none["counts"][0] == count and none["cells"][0].shape[0] == 0
    only = gen_prefilled(eng, [good_a, bad["nan"][0]], 2.5, ["left"] * 2, cmax=0, cells=False, bounds=False)
    assert only["status"].tolist() == [0, fr.ST_NONFINITE] and only["counts"].tolist() == [count, 0]


def check_grid_refusal(eng, good, good_alone):
    """A grid of more than 2^31 - 1 points, alone and inside a batch (every track of a call shares the cell width, so the batch runs at the width
    that is too small for one track and small enough for its neighbours): MCQ_FGEN_GRID, count 0, no cell, the range and both counts kept in
    grid_out, the boundaries delivered; the neighbours' bytes are those of a call without it."""
    big, cw = fc.grid_refused()
    nx, ny = fr.grid_counts(big, cw)
    assert nx * ny > 2 ** 31 - 1 and nx < 2 ** 31 and ny < 2 ** 31 and fr.status_of(big, cw) == fr.ST_GRID and fr.status_of(big, 2.5) == 0
    want_grid = [float(v) for v in fr.grid_range(big)] + [float(nx), float(ny)]
    right, left = fr.calc_trackboundaries(big)
    one = gen_prefilled(eng, [big], cw, ["left"], cmax=3)
    assert one["status"][0] == fr.ST_GRID and one["counts"][0] == 0 and one["cells"][0].shape[0] == 0
    assert one["grids"][0].tolist() == want_grid and _bits(one["bound_right"][0], right) and _bits(one["bound_left"][0], left)
    only = gen_prefilled(eng, [big], cw, ["left"], cmax=0, cells=False, bounds=False)
    assert only["status"][0] == fr.ST_GRID and only["counts"][0] == 0 and only["grids"][0].tolist() == want_grid
    # beside neighbours: the three-waypoint track, whose own grid at this width is small, and a refused one
    tiny = rec()["small/n3/reftrack"]
    tiny_alone = gen_prefilled(eng, [tiny], cw, ["left"])
    assert tiny_alone["status"][0] == 0 and fr.status_of(tiny, cw) == 0
    g = gen_prefilled(eng, [tiny, big, fc.refused_tracks()["nan"][0], tiny], cw, ["left"] * 4, cmax=tiny_alone["cmax"])
    assert g["status"].tolist() == [0, fr.ST_GRID, fr.ST_NONFINITE, 0] and g["counts"].tolist() == [tiny_alone["counts"][0], 0, 0, tiny_alone["counts"][0]]
    assert g["grids"][1].tolist() == want_grid and _bits(g["bound_right"][1], right) and g["cells"][1].shape[0] == 0
    for i in (0, 3):
        assert all(_bits(g[f][i], tiny_alone[f][0]) for f in ("cells", "bound_right", "bound_left", "grids")), "a neighbour of the oversize grid"
    # the same track at a width it can hold is served
    assert good_alone["status"][0] == 0 and _bits(gen_prefilled(eng, [good, big], 2.5, ["left"] * 2)["cells"][0], good_alone["cells"][0])


def check_layout(eng):
    """A ragged batch alone, reversed, beside others, in wider buffers and with mixed sides: the same bytes per track."""
    z = rec()
    names = ["n3", "open_arc", "oval_2p5", "gap_over"]
    tracks = [z["small/%s/reftrack" % n] for n in names] + [z["rounded_rectangle/reftrack"]]
    sides = ["left", "right", "left", "left", "left"]
    g = gen_prefilled(eng, tracks, 2.5, sides)
    fields = ("cells", "bound_right", "bound_left")

    def same(a, i, b, j):
        return all(_bits(a[f][i], b[f][j]) for f in fields) and _bits(a["grids"][i], b["grids"][j]) and a["counts"][i] == b["counts"][j]
    assert (g["status"] == 0).all() and (g["counts"] > 0).all()
    for i in range(len(tracks)):
        assert same(gen_prefilled(eng, tracks[i:i + 1], 2.5, sides[i:i + 1]), 0, g, i), "track %d alone" % i
    r = gen_prefilled(eng, tracks[::-1], 2.5, sides[::-1])
    assert all(same(r, len(tracks) - 1 - i, g, i) for i in range(len(tracks))), "reversed"
    w = gen_prefilled(eng, [tracks[2]] + tracks + [fc.refused_tracks()["nan"][0]], 2.5, ["right"] + sides + ["left"], cmax=g["cmax"] + 5,
                      nmax=max(t.shape[0] for t in tracks) + 7)
    assert all(same(w, i + 1, g, i) for i in range(len(tracks))), "beside others, in wider buffers"
    assert w["counts"][0] == 0 and w["status"][0] == 0, "the oval with the wrong side inside: the reference's empty map"


def check_gen_arguments(eng):
    with eng.scope() as dev:
        d = dev.up(np.zeros(64))
        ok = dict(tracks=1, nmax=3, d_n=None, d_ref=d, cellwidth=1.0, d_inside_right=None, cmax=4, d_bound_r=None, d_bound_l=None,
                  d_grid=dev.new(64), d_count=dev.new(64), d_cells=dev.new(64), d_status=dev.new(64))
        for bad in (dict(tracks=0), dict(nmax=2), dict(cellwidth=0.0), dict(cellwidth=-1.0), dict(cellwidth=math.nan), dict(cellwidth=math.inf),
                    dict(cmax=-1), dict(d_ref=None), dict(d_grid=None), dict(d_count=None), dict(d_status=None)):
            with pytest.raises(engine.EngineError, match=r"\(-1\)"):
                eng.friction_gen_device(**dict(ok, **bad))
        with pytest.raises(engine.EngineError, match=r"\(-3\)"):
            eng.friction_gen_device(**dict(ok, tracks=40000))
        eng.friction_gen_device(**dict(ok, cmax=-1, d_cells=None))        # a counting call does not read cmax
    for name in ("mcq_points_in_path_device", "mcq_friction_gen_device"):
        assert name in engine.EXPORTED_SYMBOLS and hasattr(eng.lib, name)


# ---- 3. the reference's names ---------------------------------------------------------------------------------------------------------------------
def check_dropin(eng, tmp, berlin=False):
    """gen_friction_map and write_friction_map: the bytes of the two files the reference's own script wrote; load_friction_map reads them back."""
    z = rec()
    ref = z["rounded_rectangle/reftrack"]
    cells, mue = friction.gen_friction_map(ref, 2.0, 0.8, fc.INSIDE["rounded_rectangle"], engine=eng)
    assert cells.shape == (1048, 2) and mue.shape == (1048,) and (mue == 0.8).all()
    p_map, p_data = os.path.join(tmp, "rr_tpamap.csv"), os.path.join(tmp, "rr_tpadata.json")
    friction.write_friction_map(cells, mue, p_map, p_data)
    with open(p_map, "rb") as a, open(p_data, "rb") as b:
        assert a.read() == z["script/rr_csv"].tobytes() and b.read() == z["script/rr_json"].tobytes()
    back, mue_back = friction.load_friction_map(p_map, p_data)
    assert _bits(back, np.round(cells, 4)) and _bits(mue_back, mue)
    with eng.friction_map(back, mue_back) as fmap:
        assert fmap.info["cells"] == 1048
    empty = friction.gen_friction_map(ref, 2.0, 0.8, "right", engine=eng)
    assert empty[0].shape == (0, 2) and empty[1].shape == (0,)
    br, bl = friction.calc_trackboundaries(ref, engine=eng)
    assert _bits(br, z["rounded_rectangle/bound_right"]) and _bits(bl, z["rounded_rectangle/bound_left"])
    bad = fc.refused_tracks()
    for k in bad:
        with pytest.raises(ValueError):
            friction.gen_friction_map(bad[k][0], 2.0, 0.8, "left", engine=eng)
    big, cw = fc.grid_refused()
    with pytest.raises(ValueError, match="2\\^31"):
        friction.gen_friction_map(big, cw, 0.8, "left", engine=eng)
    assert eng.friction_gen_batch([big], cw, "left")["status"][0] == engine.FGEN_GRID
    # calc_trackboundaries: the boundaries-only form; a zero gradient gives the reference's NaN row, not an error
    zr, zl = friction.calc_trackboundaries(bad["zero_gradient"][0], engine=eng)
    fr_r, fr_l = fr.calc_trackboundaries(bad["zero_gradient"][0])
    for got, want in ((zr, fr_r), (zl, fr_l)):     # (a NaN's sign and payload are the arithmetic unit's: where they are, and every finite bit)
        assert np.array_equal(np.isnan(got), np.isnan(want)) and _bits(np.nan_to_num(got, nan=0.0), np.nan_to_num(want, nan=0.0))
    assert np.isnan(zr[12]).all() and np.isfinite(zr[:12]).all() and np.isfinite(zr[13:]).all()
    with pytest.raises(ValueError):
        friction.calc_trackboundaries(bad["two_rows"][0], engine=eng)
    rr, ll, st3 = eng.track_boundaries_batch([ref, bad["nan"][0], big])
    assert st3.tolist() == [0, engine.FGEN_NONFINITE, 0] and _bits(rr[0], br) and _bits(ll[0], bl) and np.isnan(rr[1]).all()
    assert _bits(rr[2], fr.calc_trackboundaries(big)[0])
    for kw in (dict(cellwidth_m=0.0), dict(cellwidth_m=math.nan), dict(inside_trackbound="inner")):
        with pytest.raises(ValueError):
            friction.gen_friction_map(**dict(dict(reftrack=ref, cellwidth_m=2.0, initial_mue=0.8, inside_trackbound="left", engine=eng), **kw))
    with pytest.raises(ValueError):
        eng.friction_gen_batch([ref, ref], 2.0, ["left"])
    both = eng.friction_gen_batch([ref, z["small/open_arc/reftrack"]], 2.0, ["left", "right"])
    assert _bits(both["cells"][0], cells) and both["counts"].tolist() == [1048, 453] and both["grids"].shape == (2, 6)
    cut = eng.friction_gen_batch([ref], 2.0, "left", cmax=1000)
    assert cut["status"][0] == engine.FGEN_OVERFLOW and cut["counts"][0] == 1048 and _bits(cut["cells"][0], cells[:1000])
    if berlin:
        cells, mue = friction.gen_friction_map(z["berlin_2018/reftrack"], 2.0, 0.8, fc.INSIDE["berlin_2018"], engine=eng)
        assert cells.shape[0] == int(z["script/berlin_cells"]) == 7468
        friction.write_friction_map(cells, mue, p_map, p_data)
        with open(p_map, "rb") as a, open(p_data, "rb") as b:
            assert [hashlib.sha256(a.read()).hexdigest(), hashlib.sha256(b.read()).hexdigest()] == z["script/berlin_sha256"].tolist()


def check_end_to_end(eng, golden_berlin):
    """gen_friction_map -> Engine.friction_map -> friction_query_batch at the optimised raceline of tests/golden/berlin_2018: every query's
    nearest cell lies within half a cell's diagonal -- the raceline runs between the boundaries, and the map covers the track."""
    cw = 2.0
    cells, mue = friction.gen_friction_map(rec()["berlin_2018/reftrack"], cw, 0.8, fc.INSIDE["berlin_2018"], engine=eng)
    race = golden_berlin["reftrack"][:, :2] + golden_berlin["alpha"][:, None] * golden_berlin["normvec"]
    with eng.friction_map(cells, mue) as fmap:
        got, idx, dist = eng.friction_query_batch(fmap, race, want_idx=True, want_dist=True)
    assert (got == 0.8).all() and (idx >= 0).all()
    assert dist.max() <= cw * math.sqrt(2.0) / 2.0, "a raceline point lies %.3f m from its nearest cell" % dist.max()
    return float(dist.max())
