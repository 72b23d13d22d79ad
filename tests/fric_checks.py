"""The bodies of the friction tests, shared by the SIMT interpreter's run (tests/test_emu_fric.py) and the MI355X's (tests/test_gpu_fric.py):
every body takes the engine under test.  Cases: tests/fric_cases.py; reference: tests/fric_ref.py; what a result is held to: tests/fric_guard.py."""
import json
import os

import numpy as np
import pytest

import fric_cases as fc
import fric_guard as fg
import fric_ref as fr
from global_racetrajectory_optimization_amd import engine, friction

OK, BAD = 0, 4         # MCQ_OK, MCQ_BAD_INPUT
LD = np.longdouble
FILL = 7.25         # what outputs are pre-filled with: nothing of it may be left


def _bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def query_prefilled(eng, fmap, q):
    """mcq_fmap_query_device on pre-filled outputs: (mue, idx, dist)."""
    q = np.ascontiguousarray(q, dtype=np.float64).reshape(-1, 2)
    k = q.shape[0]
    with eng.scope() as dev:
        d_q = dev.up(q if k else np.zeros((1, 2)))
        d_m, d_i, d_d = dev.up(np.full(max(k, 1), FILL)), dev.up(np.full(max(k, 1), 77, dtype=np.int32)), dev.up(np.full(max(k, 1), FILL))
        eng.friction_query_device(fmap, k, d_q, d_m, d_i, d_d)
        m, i, d = eng.download(d_m, (max(k, 1),), np.float64), eng.download(d_i, (max(k, 1),), np.int32), eng.download(d_d, (max(k, 1),), np.float64)
    if k == 0:
        assert m[0] == FILL and i[0] == 77 and d[0] == FILL, "count == 0 wrote something"
    return m[:k], i[:k], d[:k]


# ---- 1. maps and queries ------------------------------------------------------------------------------------------------------------------------
def check_map(eng, name):
    """One map of the case table: every count of the table, against the brute force; then the same queries alone, reversed and beside others."""
    cells, mue, side = fc.maps()[name]
    q_all = fc.queries(name)
    ref_all = fr.nearest(cells, q_all)
    with eng.friction_map(cells, mue, bin_side=side) as fmap:
        info = fmap.info
        assert info["cells"] == cells.shape[0] and info["bins_x"] >= 1 and info["bins_y"] >= 1 and info["bin_side"] > 0 and info["device_bytes"] > 0
        if name == "line3":
            assert info["bins_y"] == 1
        if name == "one":
            assert info["bins_x"] == 1 and info["bins_y"] == 1
        if name == "onebin":
            assert info["bins_x"] * info["bins_y"] == 1
        if name == "sparse":
            assert info["bins_x"] * info["bins_y"] > 100 * cells.shape[0]
        singles = 0
        for count in fc.COUNTS:
            m, i, d = query_prefilled(eng, fmap, q_all[:count])
            singles += fg.accept_indices(cells, mue, q_all[:count], i, m, d, ref=tuple(r[:count] for r in ref_all), label="%s/%d" % (name, count))
        assert singles > 0 or cells.shape[0] == 1
        m, i, d = query_prefilled(eng, fmap, q_all)
        for k in (0, 5, len(q_all) - 1):
            assert all(_bits(a[k:k + 1], b) for a, b in zip((m, i, d), query_prefilled(eng, fmap, q_all[k:k + 1]))), "%s: query %d alone" % (name, k)
        assert all(_bits(a[::-1], b) for a, b in zip((m, i, d), query_prefilled(eng, fmap, q_all[::-1]))), "%s: reversed" % name
        both = query_prefilled(eng, fmap, np.vstack((q_all[100:], q_all)))
        assert all(_bits(a, b[len(q_all) - 100:]) for a, b in zip((m, i, d), both)), "%s: beside others" % name
        # the Python surface: shapes, and the entries asked for
        out = eng.friction_query_batch(fmap, q_all.reshape(-1, 1, 2)[:12].reshape(3, 4, 2), want_idx=True, want_dist=True)
        assert [o.shape for o in out] == [(3, 4)] * 3 and _bits(out[0].reshape(-1), m[:12]) and _bits(out[1].reshape(-1), i[:12])
        assert _bits(eng.friction_query_batch(fmap, q_all[:12]), m[:12])
        assert eng.friction_query_batch(fmap, np.zeros((0, 2))).shape == (0,)
    if name == "nanmue":
        assert np.isnan(m[i == 5]).all() and (i == 5).any(), "a NaN mue is handed through"


def check_exact_ties(eng):
    """Dyadic coordinates, every product exact: the lowest of the tied indices -- and the reference agrees that they are ties."""
    for name, q, want in fc.exact_ties():
        cells, mue, side = fc.maps()[name]
        r_idx, _, r_gap = fr.nearest(cells, [q])
        assert r_idx[0] == want, (name, q, r_idx[0], want)
        with eng.friction_map(cells, mue, bin_side=side) as fmap:
            m, i, d = query_prefilled(eng, fmap, [q])
        assert i[0] == want and _bits(m[0], mue[want]), "%s %r: index %d, the lowest tied one is %d (gap %r)" % (name, q, i[0], want, r_gap[0])


def check_nonfinite(eng):
    cells, mue, side = fc.maps()["c257"]
    q = fc.queries("c257")[:70].copy()
    bad = {3: (np.nan, 1.0), 17: (1.0, np.nan), 33: (np.inf, 0.0), 34: (0.0, -np.inf), 63: (np.nan, np.nan), 64: (-np.inf, np.inf)}
    for k, v in bad.items():
        q[k] = v
    with eng.friction_map(cells, mue) as fmap:
        m, i, d = query_prefilled(eng, fmap, q)
        for k in bad:
            assert i[k] == -1 and np.isnan(m[k]) and np.isnan(d[k])
            m1, i1, d1 = query_prefilled(eng, fmap, q[k:k + 1])
            assert i1[0] == -1 and np.isnan(m1[0]) and np.isnan(d1[0]), "alone"
        fg.accept_indices(cells, mue, q, i, m, d, label="nonfinite")


def check_map_arguments(eng):
    cells, mue, _ = fc.maps()["lattice"]
    for c in (np.nan, np.inf, -np.inf):
        bad = cells.copy()
        bad[7, 1] = c
        with pytest.raises(engine.EngineError, match=r"\(-1\)"):
            eng.friction_map(bad, mue)
    with pytest.raises(engine.EngineError, match=r"\(-1\)"):
        eng.friction_map(np.zeros((0, 2)), np.zeros(0))
    with pytest.raises(ValueError):
        eng.friction_map(cells, mue[:-1])
    fm = eng.friction_map(cells, mue)
    fm.close()
    fm.close()
    with pytest.raises(engine.EngineError, match="closed"):
        eng.friction_query_batch(fm, cells)
    with eng.friction_map(cells, mue, bin_side=1e-9) as fmap:        # more bins than the cap: the side grows
        assert fmap.info["bins_x"] * fmap.info["bins_y"] <= 1 << 22 and fmap.info["bin_side"] > 1e-9
        fg.accept_indices(cells, mue, fc.queries("lattice")[:40], query_prefilled(eng, fmap, fc.queries("lattice")[:40])[1], label="capped")


def check_recorded_queries(eng, track):
    """The 2 000 recorded queries in and around the track's box against the brute force, cKDTree's indices and the reference's own mue."""
    g = fg.recorded(track)
    with eng.friction_map(g["cells"], g["mue"]) as fmap:
        m, i, d = query_prefilled(eng, fmap, g["q"])
    singles = fg.accept_indices(g["cells"], g["mue"], g["q"], i, m, d, ref=fg.recorded_nearest(track), ckd=g["q_idx"], label=track)
    assert singles >= 1990
    same = i == g["q_idx"]
    assert _bits(m[same], g["q_mue"][same])


# ---- 2. grids ------------------------------------------------------------------------------------------------------------------------------------
def run_grid(eng, fmap, case, width=None, tracks=None, idx=True):
    tracks = case["tracks"] if tracks is None else tracks
    return eng.friction_grid_batch(fmap, [t[0] for t in tracks], [t[1] for t in tracks], case["width"] if width is None else width, fc.WB_F, fc.WB_R,
                                   case["dn"], jmax=case["jmax"], want_idx=idx)


def hold_track(out, t, cells, mue, track, width, dn, label, expect_bad=False, recorded=None):
    """One track of a grid result against the restatement: counts and positions bitwise, every query an accepted index, the lines under the guard."""
    ref, nv = track
    if expect_bad:
        assert out["status"][t] == BAD
        assert np.isnan(out["n"][t]).all() and np.isnan(out["mue"][t]).all() and np.all(out["idx"][t] == -1) and np.isnan(out["w_mue"][t]).all()
        return
    assert out["status"][t] == OK, label
    R = fr.grid(ref, nv, width, fc.WB_F, fc.WB_R, dn)
    assert out["rows"][t] == len(R)
    assert list(out["cnt"][t, :len(R)]) == [r["cnt"] for r in R] and not np.any(out["cnt"][t, len(R):]), "%s: counts" % label
    assert np.isnan(out["n"][t, len(R):]).all() and np.isnan(out["mue"][t, :, len(R):]).all() and np.all(out["idx"][t, :, len(R):] == -1)
    assert np.isnan(out["w_mue"][t, :, len(R):]).all()
    guard = fg.w_guard()
    worst = 0.0
    for i, r in enumerate(R):
        c = max(r["cnt"], 0)
        assert _bits(out["n"][t, i, :c], r["n"]), "%s: row %d is not numpy.linspace's bits" % (label, i)
        assert np.isnan(out["n"][t, i, c:]).all() and np.isnan(out["mue"][t, :, i, c:]).all() and np.all(out["idx"][t, :, i, c:] == -1)
        for k in range(4):
            got_m, got_i = out["mue"][t, k, i, :c], out["idx"][t, k, i, :c]
            if recorded is None:
                fg.accept_indices(cells, mue, r["xy"][k], got_i, got_m, label="%s row %d %s" % (label, i, fr.WHEELS[k]))
            else:       # a whole track: the recording decides (the brute force serves the undecided queries only)
                assert np.all((got_i >= 0) & (got_i < len(cells))) and _bits(got_m, mue[got_i])
                dec = recorded["decided"][k, i, :c]
                assert _bits(got_m[dec], recorded["mue4"][k, i, :c][dec]), "%s row %d %s: differs from the reference's own grid" % (label, i, fr.WHEELS[k])
                if not dec.all():
                    fg.accept_indices(cells, mue, r["xy"][k][~dec], got_i[~dec], label=label)
            w = out["w_mue"][t, k, i]
            if c < 2:
                assert np.isnan(w).all(), "%s: a row of %d positions has a line" % (label, c)
                continue
            lines = [fr.line(r["n"], got_m)]
            if recorded is not None and dec.all():
                lines.append(fr.line(r["n"], recorded["mue4"][k, i, :c]))
            for s, ic in lines:
                if np.isnan(float(s)):
                    assert np.isnan(w).all()
                    continue
                dev = max(abs(LD(w[0]) - s), abs(LD(w[1]) - ic))
                worst = max(worst, float(dev))
                assert dev <= guard, "%s row %d %s: line off by %.3e (guard %.3e)" % (label, i, fr.WHEELS[k], float(dev), guard)
    return worst


def check_grid_case(eng, name):
    case = fc.grid_cases()[name]
    cells, mue = fc.grid_map()
    widths = fc.widths_of(case)
    with eng.friction_map(cells, mue) as fmap:
        out = run_grid(eng, fmap, case)
        for t, track in enumerate(case["tracks"]):
            bad = not np.all(np.isfinite(track[0]))
            over = case["jmax"] is not None and max(r["cnt"] for r in fr.grid(*track, widths[t], fc.WB_F, fc.WB_R, case["dn"])) > case["jmax"] \
                if not bad else False
            hold_track(out, t, cells, mue, track, widths[t], case["dn"], "%s[%d]" % (name, t), expect_bad=bad or over)
            if over:        # the counts the track needs
                want = [r["cnt"] for r in fr.grid(*track, widths[t], fc.WB_F, fc.WB_R, case["dn"])]
                assert list(out["cnt"][t, :len(want)]) == want
            elif bad:
                assert not np.any(out["cnt"][t])
        # every track alone, and the launch in reversed order: the same bits
        keys = ("n", "cnt", "mue", "idx", "w_mue")
        jmax = out["n"].shape[2]
        for t, track in enumerate(case["tracks"]):
            alone = run_grid(eng, fmap, dict(case, jmax=jmax), width=widths[t], tracks=[track])
            rows = alone["n"].shape[1]
            for q in keys:
                b = out[q][t][:, :rows] if q in ("mue", "idx", "w_mue") else out[q][t][:rows]
                assert _bits(alone[q][0], np.ascontiguousarray(b)), "%s[%d]: %s alone differs" % (name, t, q)
            assert alone["status"][0] == out["status"][t]
        if len(case["tracks"]) > 1:
            rev = run_grid(eng, fmap, dict(case, width=widths[::-1]), tracks=case["tracks"][::-1])
            assert all(_bits(rev[q][::-1], out[q]) for q in keys + ("status",)), "%s: reversed launch" % name
        # without the optional outputs
        lean = eng.friction_grid_batch(fmap, [t[0] for t in case["tracks"]], [t[1] for t in case["tracks"]], case["width"], fc.WB_F, fc.WB_R, case["dn"],
                                       fit=False, jmax=case["jmax"])
        assert lean["w_mue"] is None and lean["idx"] is None and all(_bits(lean[q], out[q]) for q in ("n", "cnt", "mue", "status"))


def check_grid_prefilled(eng):
    """Pre-filled outputs are overwritten whole: no entry keeps what it held."""
    case = fc.grid_cases()["nan_track"]
    cells, mue = fc.grid_map()
    ns, ref = engine._pad_rows([t[0] for t in case["tracks"]], 4)
    nv = engine._pad_like([t[1] for t in case["tracks"]], ns, (2,))
    tracks, nmax = ref.shape[:2]
    rows, jmax = nmax + 1, 12
    with eng.friction_map(cells, mue) as fmap, eng.scope() as dev:
        shapes = dict(n=(tracks, rows, jmax), cnt=(tracks, rows), mue=(tracks, 4, rows, jmax), idx=(tracks, 4, rows, jmax), w=(tracks, 4, rows, 2),
                      st=(tracks,))
        d = {k: dev.up(np.full(s, 77 if k in ("cnt", "idx", "st") else FILL, dtype=np.int32 if k in ("cnt", "idx", "st") else np.float64))
             for k, s in shapes.items()}
        eng.friction_grid_device(fmap, tracks, nmax, dev.up(ns), dev.up(ref), dev.up(nv), case["width"], None, fc.WB_F, fc.WB_R, case["dn"], jmax,
                                 d["n"], d["cnt"], d["mue"], d["idx"], d["w"], d["st"])
        got = {k: eng.download(d[k], s, np.int32 if k in ("cnt", "idx", "st") else np.float64) for k, s in shapes.items()}
    assert list(got["st"]) == [OK, BAD, OK]
    assert not np.any(got["n"] == FILL) and not np.any(got["mue"] == FILL) and not np.any(got["w"] == FILL)
    assert not np.any(got["cnt"] == 77) and not np.any(got["idx"] == 77)
    with eng.friction_map(cells, mue) as fmap:
        ref_out = eng.friction_grid_batch(fmap, [t[0] for t in case["tracks"]], [t[1] for t in case["tracks"]], case["width"], fc.WB_F, fc.WB_R,
                                          case["dn"], jmax=jmax, want_idx=True)
    assert _bits(got["n"], ref_out["n"]) and _bits(got["mue"], ref_out["mue"]) and _bits(got["w"], ref_out["w_mue"]) and _bits(got["idx"], ref_out["idx"])


def check_width_list(eng):
    """width_list against repeated scalar calls, bitwise."""
    case = fc.grid_cases()["widths"]
    cells, mue = fc.grid_map()
    with eng.friction_map(cells, mue) as fmap:
        jmax = max(max(r["cnt"] for r in fr.grid(*t, w, fc.WB_F, fc.WB_R, case["dn"])) for t, w in zip(case["tracks"], case["width"]))
        both = eng.friction_grid_batch(fmap, [t[0] for t in case["tracks"]], [t[1] for t in case["tracks"]], case["width"], fc.WB_F, fc.WB_R,
                                       case["dn"], jmax=jmax, want_idx=True)
        assert not np.any(both["status"])
        for t, w in enumerate(case["width"]):
            one = eng.friction_grid_batch(fmap, [x[0] for x in case["tracks"]], [x[1] for x in case["tracks"]], w, fc.WB_F, fc.WB_R, case["dn"],
                                          jmax=jmax, want_idx=True)
            assert all(_bits(one[q][t], both[q][t]) for q in ("n", "cnt", "mue", "idx", "w_mue")), "track %d with width %r" % (t, w)
        with pytest.raises(ValueError):
            eng.friction_grid_batch(fmap, [t[0] for t in case["tracks"]], [t[1] for t in case["tracks"]], case["width"][:2], fc.WB_F, fc.WB_R, 0.25)


def check_grid_arguments(eng):
    case = fc.grid_cases()["n3"]
    cells, mue = fc.grid_map()
    refs, nvs = [case["tracks"][0][0]], [case["tracks"][0][1]]
    with eng.friction_map(cells, mue) as fmap:
        for kw in (dict(dn=0.0), dict(dn=-0.25), dict(dn=float("nan")), dict(dn=float("inf")), dict(jmax=0)):
            a = dict(dn=0.25, jmax=None)
            a.update(kw)
            with pytest.raises(engine.EngineError, match=r"\(-1\)"):
                eng.friction_grid_batch(fmap, refs, nvs, 3.4, fc.WB_F, fc.WB_R, a["dn"], jmax=a["jmax"] if a["dn"] == 0.25 else 8)
        with eng.scope() as dev:
            p = dev.new(4096)
            for miss in range(5):
                args = [p, p, p, p, p]         # n_out, cnt_out, mue_out, status_out, reftrack
                args[miss] = None
                rc = eng.lib.mcq_friction_grid_device(eng.h, fmap.ptr, 1, 3, None, args[4], p, 3.4, None, 1.6, 1.4, 0.25, 4, args[0], args[1], args[2],
                                                      None, None, args[3])
                assert rc == -1, miss
            assert eng.lib.mcq_fmap_query_device(eng.h, fmap.ptr, -1, p, p, None, None) == -1
            assert eng.lib.mcq_fmap_query_device(eng.h, fmap.ptr, 1, None, p, None, None) == -1
            assert eng.lib.mcq_fmap_query_device(eng.h, fmap.ptr, 0, None, None, None, None) == 0
        out = eng.friction_grid_batch(fmap, refs, nvs, float("nan"), fc.WB_F, fc.WB_R, 0.25, jmax=8)
        assert out["status"][0] == BAD and np.isnan(out["mue"]).all() and not np.any(out["cnt"])


def check_recorded_grid(eng, track):
    """A whole track: the reference's OWN extract_friction_coeffs and approx_friction_map("linear"), recorded."""
    g = fg.recorded(track)
    z = np.load(os.path.join(os.path.dirname(fg.PATH), "..", track + ".npz"))
    ref, nv = z["reftrack"], z["normvec"]
    with eng.friction_map(g["cells"], g["mue"]) as fmap:
        out = eng.friction_grid_batch(fmap, [ref], [nv], g["width"], g["wb_f"], g["wb_r"], g["dn"], want_idx=True)
    assert out["n"].shape[2] == g["n"].shape[1] and _bits(out["cnt"][0], g["cnt"]) and _bits(out["n"][0], g["n"])
    worst = hold_track(out, 0, g["cells"], g["mue"], (ref, nv), g["width"], g["dn"], track, recorded=g)
    dev = float(np.nanmax(np.abs(out["w_mue"][0] - g["w"])))
    assert dev <= fg.w_guard() + float(fg.fixture()["w_floor"]), "%s: %.3e from numpy's own polyfit" % (track, dev)
    return worst, dev


# ---- 3. the reference's names ------------------------------------------------------------------------------------------------------------------
def write_map_files(d, cells, mue, drop=(), bad_value=None):
    p_map, p_data = os.path.join(d, "t_tpamap.csv"), os.path.join(d, "t_tpadata.json")
    with open(p_map, "w") as fh:
        fh.write("# x_m;y_m\n")
        for x, y in cells:
            fh.write("%.4f;%.4f\n" % (x, y))
    data = {str(i): [float(m)] for i, m in enumerate(mue) if i not in drop}
    if bad_value is not None:
        data["3"] = bad_value
    with open(p_data, "w") as fh:
        json.dump(data, fh)
    return p_map, p_data


def check_dropin(eng, tmp):
    cells, mue = fc.grid_map()
    case = fc.grid_cases()["ragged"]
    ref, nv = case["tracks"][2]
    pars = dict(optim_opts=dict(width_opt=3.4, var_friction="linear"), vehicle_params_mintime=dict(wheelbase_front=fc.WB_F, wheelbase_rear=fc.WB_R))
    p_map, p_data = write_map_files(tmp, cells, mue)
    c2, m2 = friction.load_friction_map(p_map, p_data)
    assert _bits(c2, cells) and _bits(m2, mue)
    iface = friction.FrictionMapInterface(tpamap_path=p_map, tpadata_path=p_data, engine=eng)
    q = fc.queries("lattice")[:9] + 2.0
    got = iface.get_friction_singlepos(q)
    assert isinstance(got, np.ndarray) and got.shape == (9, 1) and _bits(got[:, 0], mue[fr.nearest(cells, q)[0]])
    empty = iface.get_friction_singlepos(np.asarray([]))
    assert isinstance(empty, np.ndarray) and empty.shape == (0,)
    iface.close()
    n, *grids = friction.extract_friction_coeffs(ref, nv, p_map, p_data, pars, 0.25, False, False, engine=eng)
    R = fr.grid(ref, nv, 3.4, fc.WB_F, fc.WB_R, 0.25)
    assert isinstance(n, list) and len(n) == len(grids[0]) == ref.shape[0] + 1 and len(grids) == 4
    assert all(_bits(a, r["n"]) for a, r in zip(n, R)) and all(g[i].shape == (R[i]["cnt"], 1) for g in grids for i in range(len(R)))
    w = friction.approx_friction_map(ref, nv, p_map, p_data, pars, 0.25, 5, False, False, engine=eng)
    assert len(w) == 5 and all(a.shape == (len(R), 2) for a in w[:4]) and w[4].shape == (len(R), 1) and not np.any(w[4])
    for k in range(4):
        for i, r in enumerate(R):
            pf = np.polyfit(r["n"], grids[k][i].T[0], 1)
            assert np.max(np.abs(w[k][i] - pf)) <= fg.w_guard() + float(fg.fixture()["w_floor"])
    # the error paths
    with pytest.raises(NotImplementedError):
        friction.approx_friction_map(ref, nv, p_map, p_data, dict(pars, optim_opts=dict(width_opt=3.4, var_friction="gauss")), 0.25, 5, engine=eng)
    with pytest.raises(ValueError, match="Unknown method for friction map approximation!"):
        friction.approx_friction_map(ref, nv, p_map, p_data, dict(pars, optim_opts=dict(width_opt=3.4, var_friction="cubic")), 0.25, 5, engine=eng)
    hit = int(fr.nearest(cells, ref[:1, :2])[0][0])
    sub = os.path.join(tmp, "missing")
    os.makedirs(sub)
    p_map2, p_data2 = write_map_files(sub, cells, mue, drop=(hit,))
    assert np.isnan(friction.load_friction_map(p_map2, p_data2)[1][hit])
    iface = friction.FrictionMapInterface(p_map2, p_data2, engine=eng)
    with pytest.raises(KeyError):
        iface.get_friction_singlepos(ref[:1, :2])
    iface.close()
    sub = os.path.join(tmp, "badvalue")
    os.makedirs(sub)
    with pytest.raises(ValueError):
        friction.load_friction_map(*write_map_files(sub, cells, mue, bad_value=[1.0, 2.0]))
    import helper_checks
    helper_checks.check_abi_table()
    for name in ("mcq_fmap_create", "mcq_fmap_destroy", "mcq_fmap_info", "mcq_fmap_query_device", "mcq_friction_grid_device"):
        assert name in engine.EXPORTED_SYMBOLS and hasattr(eng.lib, name)


# ---- 4. end to end -------------------------------------------------------------------------------------------------------------------------------
def check_end_to_end(eng, golden):
    """prep_track_batch -> solve_batch -> raceline_batch -> the resident query -> vel_profile_batch(mu=...) on Berlin with the varmue data, against
    oracle/vel_ref.py fed the reference lookup's mu."""
    import fit_cases
    from test_emu_kernels import _check_vel_profiles, _vehicle_variants
    g = fg.recorded("berlin_2018")
    c = fit_cases.case("berlin_2018")
    track = np.load(fit_cases.TRACKS)["berlin_2018.track"]
    prep = eng.prep_track_batch([track], tcks=[(c["t"], list(c["c"]), c["k"])])
    assert prep["status"][0] == OK
    ref, nv = prep["reftrack"][0], prep["normvec"][0]
    al, _, st, _ = eng.solve_batch([dict(reftrack=ref, normvec=nv, scaling=prep["scaling"][0], kappa_bound=float(golden["kappa_bound"]),
                                         w_veh=float(golden["w_veh"]))])
    assert st[0] == OK
    race = eng.raceline_batch([ref], [nv], [al[0]], 2.0)
    m, mmax = int(race["m"][0]), race["xy"].shape[1]
    assert race["status"][0] == OK and m < mmax
    xy = race["xy"].copy()
    xy[0, m:] = np.nan          # (the raceline entry leaves the rows behind m unwritten)
    with eng.friction_map(g["cells"], g["mue"]) as fmap, eng.scope() as dev:
        d_xy, d_mu = dev.up(xy), dev.up(np.full((1, mmax), FILL))
        eng.friction_query_device(fmap, mmax, d_xy, d_mu)           # [batch][mmax][2] in, [batch][mmax] out: the mu of the profile entries
        mu = eng.download(d_mu, (1, mmax), np.float64)
    assert np.isnan(mu[0, m:]).all() and np.all(np.isfinite(mu[0, :m])), "padding rows are NaN in and NaN out"
    r_idx, _, r_gap = fr.nearest(g["cells"], race["xy"][0, :m])
    dec = r_gap > fg.INDEX_TOL
    assert dec.sum() >= m - 2 and _bits(mu[0, :m][dec], g["mue"][r_idx][dec]), "the resident query differs from the reference lookup"
    mu_ref = np.where(dec, g["mue"][r_idx], mu[0, :m])
    assert mu_ref.min() < 0.95 and mu_ref.max() > 1.05
    kappa, el = race["kappa"][0, :m], race["el_lengths"][0, :m]
    var = _vehicle_variants()[:2]
    _check_vel_profiles(eng, kappa, el, var, 1.0, mu=mu_ref)
    args = (np.stack([v[0] for v in var]), np.stack([v[1] for v in var]), [v[2] for v in var], [v[3] for v in var], [v[4] for v in var])
    _, lap_mu = eng.vel_profile_batch(kappa[None, :], el[None, :], *args, track_of=np.zeros(2, dtype=np.int32), mu=mu[:, :m])
    _, lap_one = eng.vel_profile_batch(kappa[None, :], el[None, :], *args, track_of=np.zeros(2, dtype=np.int32), mu=np.ones((1, m)))
    assert np.all(np.isfinite(lap_mu)) and np.all(np.abs(lap_mu - lap_one) > 1e-3), "the lap time does not see the friction map"
