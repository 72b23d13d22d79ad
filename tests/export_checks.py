"""The shared bodies of tests/test_emu_export.py (SIMT interpreter) and tests/test_gpu_export.py (MI355X): mcq_export_device through
Engine.export_device on outputs PRE-FILLED with a pattern (every entry must be written, NaN or -1), and through Engine.export_batch, on the cases
of tests/export_cases.py against the longdouble reference of tests/export_ref.py under the guards of tests/export_guard.py.  Copied columns are
bitwise; decided indices are the reference's, undecided ones one of its two candidates; every launch is repeated in reversed order and must return
the same bits."""
import math
import os
import tempfile

import numpy as np

import export_cases as xc
import export_guard as xg
import export_ref as xr
import glue_cases as gc
from global_racetrajectory_optimization_amd import engine, export

LD = np.longdouble
OK, BAD_INPUT = xc.OK, xc.BAD_INPUT
PAT_D, PAT_I = 777.25, 12345          # what the outputs hold before the call


def _bits(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def run_raw(eng, P, optional=True):
    """mcq_export_device on the padded arrays of xc.pack (or any dict of that form), outputs pre-filled with the pattern."""
    T, B, nmax, mmax = len(P["ns"]), len(P["track_of"]), P["nmax"], P["mmax"]
    with eng.scope() as dev:
        up = dev.up
        d_in = [up(P[k]) for k in ("ns", "ref", "nv", "al")]
        d_m, d_t, d_tj = up(P["ms"]), up(P["track_of"]), up(P["traj"])
        d_tab = up(np.full((B, nmax + 1, 12), PAT_D))
        d_idx = up(np.full((B, nmax), PAT_I, dtype=np.int32)) if optional else None
        d_len = up(np.full((T, nmax), PAT_D)) if optional else None
        d_s = up(np.full((T, nmax + 1), PAT_D)) if optional else None
        d_tot, d_st = up(np.full(T, PAT_D)), up(np.full(B, PAT_I, dtype=np.int32))
        eng.export_device(T, nmax, d_in[0], d_in[1], d_in[2], d_in[3], B, mmax, d_m, d_t, d_tj, d_tab, d_idx, d_len, d_s, d_tot, d_st)
        out = dict(ltpl=eng.download(d_tab, (B, nmax + 1, 12), np.float64), total=eng.download(d_tot, (T,), np.float64),
                   status=eng.download(d_st, (B,), np.int32))
        if optional:
            out.update(idx=eng.download(d_idx, (B, nmax), np.int32), lengths=eng.download(d_len, (T, nmax), np.float64),
                       s_ref=eng.download(d_s, (T, nmax + 1), np.float64))
    for k, a in out.items():
        assert not np.any(a == (PAT_I if a.dtype == np.int32 else PAT_D)), "%s keeps entries the call did not write" % k
    return out


def hold_track(worst, key, out, t, n, r0, what, live=None):
    """spline_lengths / s_ref / spline_total of track t against the reference's front r0."""
    g_s, g_l, g_t = xg.guards(key, live)
    for q, dev, g in (("s_ref", xg.dmax(out["s_ref"][t, :n + 1], r0["s_ref"]), g_s), ("lengths", xg.dmax(out["lengths"][t, :n], r0["lengths"]), g_l),
                      ("total", xg.dmax(out["total"][t], r0["total"]), g_t)):
        worst.add("%s.%s" % (what.split("/")[0], q), dev, g)
        assert dev <= g, "%s: %s deviates by %.3e, guard %.3e" % (what, q, dev, g)
    assert out["s_ref"][t, 0] == 0.0 and _bits(out["s_ref"][t, n], out["total"][t])
    assert np.all(np.isnan(out["s_ref"][t, n + 1:])) and np.all(np.isnan(out["lengths"][t, n:])), what + ": entries behind n are not NaN"
    return g_s


def hold_variant(out, v, t, track, traj, R, g_s, what, cap=True):
    """Variant v (track t) of a result against the reference table R."""
    ref, nv, al = track
    n, m = ref.shape[0], traj.shape[0]
    tab, idx = out["ltpl"][v], out["idx"][v]
    assert out["status"][v] == OK, what + ": status %d" % out["status"][v]
    assert _bits(tab[:n, :4], ref[:, :4]) and _bits(tab[:n, 4:6], nv) and _bits(tab[:n, 6], al), what + ": a copied input column differs"
    assert _bits(tab[:n, 7], out["s_ref"][t, :n]), what + ": column 7 is not s_ref"
    closing = tab[0].copy()
    closing[7] = out["total"][t]
    assert _bits(tab[n], closing), what + ": row n is not row 0 with the total"
    assert np.all(np.isnan(tab[n + 1:])) and np.all(idx[n:] == -1), what + ": rows behind n are not NaN / -1"
    und = xg.undecided(R["margin"], g_s)
    dec = ~und
    assert np.array_equal(idx[:n][dec], R["idx"][dec]), what + ": %d decided indices differ from the reference" % int(np.sum(idx[:n][dec] != R["idx"][dec]))
    for i in np.nonzero(und)[0]:
        assert idx[i] in (R["c1"][i], R["c2"][i]) and idx[i] >= 0, what + ": waypoint %d took station %d, candidates %d / %d" % (i, idx[i], R["c1"][i], R["c2"][i])
    assert np.all((idx[:n] >= 0) & (idx[:n] < m))
    assert _bits(tab[:n, 8:12], traj[idx[:n], 3:7]), what + ": columns 8 .. 11 are not the bits of the station idx names"
    if cap:
        assert np.mean(und) <= xc.UNDECIDED_CAP, what + ": %d of %d waypoints undecided" % (int(np.sum(und)), n)
    return int(np.sum(und))


def check_launch(eng, L, worst, alone=False):
    P = xc.pack(L)
    out = run_raw(eng, P)
    family, name = L["name"].split("/")
    g_of = {}
    for t, track in enumerate(L["tracks"]):
        n = track[0].shape[0]
        g_of[t] = hold_track(worst, "%s/%d" % (family, n), out, t, n, xr.front(*track), "%s track %d (n=%d)" % (L["name"], t, n))
    for v, t in enumerate(L["track_of"]):
        hold_variant(out, v, t, L["tracks"][t], L["trajs"][v], xc.reference(family, name, v), g_of[t],
                     "%s variant %d (n=%d, m=%d)" % (L["name"], v, P["ns"][t], P["ms"][t]))
    order = np.arange(len(L["track_of"]))[::-1]
    rev = run_raw(eng, xc.pack(L, order))
    for q in ("ltpl", "idx", "status"):
        assert _bits(out[q], rev[q][::-1]), "%s: the reversed launch returns other bits (%s)" % (L["name"], q)
    for q in ("lengths", "s_ref", "total"):
        assert _bits(out[q], rev[q])
    bare = run_raw(eng, P, optional=False)           # without the optional outputs: the same table
    assert _bits(bare["ltpl"], out["ltpl"]) and _bits(bare["total"], out["total"]) and _bits(bare["status"], out["status"])
    if alone:                                        # every member alone, at its own nmax / mmax: the bits it has in the mixed launch
        for v, t in enumerate(L["track_of"]):
            one = dict(L, tracks=[L["tracks"][t]], ms=L["ms"][t:t + 1], track_of=np.zeros(1, dtype=np.int32), trajs=[L["trajs"][v]])
            o = run_raw(eng, xc.pack(one))
            n, m = P["ns"][t], P["ms"][t]
            assert _bits(o["ltpl"][0, :n + 1], out["ltpl"][v, :n + 1]) and _bits(o["idx"][0, :n], out["idx"][v, :n]) and \
                _bits(o["s_ref"][0, :n + 1], out["s_ref"][t, :n + 1]) and _bits(o["lengths"][0, :n], out["lengths"][t, :n]) and \
                _bits(o["total"][0], out["total"][t]), "%s variant %d: alone it has other bits" % (L["name"], v)
    return out


def _one(eng, track, traj):
    P = xc.pack(dict(tracks=[track], ms=np.array([traj.shape[0]], dtype=np.int32), track_of=np.zeros(1, dtype=np.int32), trajs=[traj]))
    return run_raw(eng, P)


def check_handmade(eng):
    """Hand-made s columns around the s_ref the entry itself returns for the ring: the expected idx of the case table, exactly."""
    track = gc.ring(*xc.HAND_RING)
    n = track[0].shape[0]
    q = _one(eng, track, xc.make_traj(xc.total64(*xc.HAND_RING), 5, "hand0"))["s_ref"][0, :n]
    assert np.all(np.diff(q) > 0.5)
    for name, col, expected in xc.handmade(q):
        col = np.array(col, dtype=np.float64)
        assert [int(np.abs(col - s).argmin()) for s in q] == expected and [xr.rule(col, s) for s in q] == expected, name
        traj = xc.hand_traj(col, name)
        out = _one(eng, track, traj)
        assert out["status"][0] == OK and list(out["idx"][0, :n]) == expected, "%s: idx %s, expected %s" % (name, list(out["idx"][0, :n]), expected)
        assert _bits(out["ltpl"][0, :n, 8:12], traj[expected, 3:7]) and _bits(out["ltpl"][0, n, 8:12], traj[expected[0], 3:7])


def check_ties(eng, worst):
    """The regular polygon: no cap on the undecided waypoints, each must take one of its two candidates and copy that station."""
    track, traj = xc.ties()
    n = track[0].shape[0]
    out = _one(eng, track, traj)
    g_s = hold_track(worst, "ties", out, 0, n, xr.front(*track), "ties")
    und = hold_variant(out, 0, 0, track, traj, xr.table(*track, traj), g_s, "ties", cap=False)
    assert und >= n // 4, "the ties case has only %d undecided waypoints" % und


REFUSAL_ROWS = [(48, 47), (257, 1500), (47, 60)]
REFUSAL_TRACK_OF = [0, 1, 1, 2]


def check_refusals(eng, family="peanut"):
    """Each MCQ_BAD_INPUT cause alone, on track 1 (variants 1 and 2) or on one of its variants, in a batch whose other members keep their bits."""
    L = xc._launch("refusals", family, REFUSAL_ROWS, REFUSAL_TRACK_OF)
    P0 = xc.pack(L)
    clean = run_raw(eng, P0)
    assert list(clean["status"]) == [OK] * 4
    nmax, mmax = P0["nmax"], P0["mmax"]

    def edit(key, fn):
        P = dict(P0, **{key: P0[key].copy()})
        fn(P[key])
        return P

    def put(*index_value):
        *index, value = index_value
        def fn(a):
            a[tuple(index)] = value
        return fn
    track_causes = [("n = 2", edit("ns", put(1, 2))), ("n = nmax + 1", edit("ns", put(1, nmax + 1))), ("n = -1", edit("ns", put(1, -1))),
                    ("m = 1", edit("ms", put(1, 1))), ("m = mmax + 1", edit("ms", put(1, mmax + 1))),
                    ("a NaN coordinate", edit("ref", put(1, 200, 1, np.nan))), ("an infinite width", edit("ref", put(1, 256, 3, np.inf))),
                    ("a NaN normal", edit("nv", put(1, 0, 0, np.nan))), ("an infinite alpha", edit("al", put(1, 130, -np.inf)))]
    variant_causes = [("a NaN in the s column", edit("traj", put(1, 1400, 0, np.nan)), [1]),
                      ("a NaN in the last station's s", edit("traj", put(2, 1499, 0, np.nan)), [2]),
                      ("s descends inside a tile", edit("traj", put(2, 700, 0, 0.0)), [2]),
                      ("s descends across the tile's edge", edit("traj", put(1, 1024, 0, P0["traj"][1, 1023, 0] - 1e-9)), [1]),
                      ("track_of beyond the tracks", edit("track_of", put(2, 3)), [2]), ("track_of negative", edit("track_of", put(1, -1)), [1])]
    for what, P, hit in [(w, p, [1, 2]) for w, p in track_causes] + variant_causes:
        out = run_raw(eng, P)
        for v in range(4):
            if v in hit:
                assert out["status"][v] == BAD_INPUT and np.all(np.isnan(out["ltpl"][v])) and np.all(out["idx"][v] == -1), \
                    "%s: variant %d is not refused whole" % (what, v)
            else:
                assert all(_bits(out[q][v], clean[q][v]) for q in ("ltpl", "idx", "status")), "%s: a refusal disturbed variant %d" % (what, v)
        track_bad = len(hit) == 2 and not what.startswith("m =")
        for t in range(3):
            if t == 1 and track_bad:
                assert np.all(np.isnan(out["lengths"][t])) and np.all(np.isnan(out["s_ref"][t])) and np.isnan(out["total"][t]), \
                    "%s: the refused track returns lengths" % what
            else:
                assert all(_bits(out[q][t], clean[q][t]) for q in ("lengths", "s_ref", "total")), "%s: track %d changed" % (what, t)
    # a NaN or a descent BEHIND the m stations is not the variant's business
    P = edit("traj", put(0, 47, 0, -5.0))
    assert _bits(run_raw(eng, P)["ltpl"][0], clean["ltpl"][0])


def check_arguments(eng):
    buf = eng.alloc(1 << 16)
    try:
        good = dict(tracks=1, nmax=8, d_n=None, d_ref=buf, d_nv=buf, d_alpha=buf, batch=1, mmax=8, d_m_of_track=None, d_track_of=None, d_traj=buf,
                    d_ltpl=buf, d_idx=None, d_lengths=None, d_s_ref=None, d_total=buf, d_status=buf)
        eng.export_device(**good)                # (zero-filled buffers: a legal call, refused on the device)
        for key, val in (("tracks", 0), ("batch", 0), ("batch", -1), ("nmax", 2), ("mmax", 1), ("d_ref", None), ("d_nv", None), ("d_alpha", None),
                         ("d_traj", None), ("d_ltpl", None), ("d_total", None), ("d_status", None)):
            try:
                eng.export_device(**dict(good, **{key: val}))
            except engine.EngineError as e:
                assert "(-1)" in str(e), str(e)           # MCQ_E_ARG
            else:
                raise AssertionError("mcq_export_device accepted %s = %r" % (key, val))
    finally:
        eng.sync()
        eng.free(buf)


def check_export_batch(eng, worst, family="peanut"):
    """Engine.export_batch, the list form: the raw entry's bits cut to lists, and the closed race table under the guard against numpy.sum."""
    L = next(q for q in xc.launches(family) if q["name"].endswith("/variants"))
    P = xc.pack(L)
    raw = run_raw(eng, P)
    refs, nvs, als = zip(*L["tracks"])
    for form in (dict(traj=P["traj"], m=P["ms"]), P["traj"]):      # with the station counts, and counted from the NaN rows
        out = eng.export_batch(list(refs), list(nvs), list(als), form, track_of=L["track_of"])
        assert _bits(out["status"], raw["status"]) and _bits(out["spline_total"], raw["total"])
        for t, n in enumerate(P["ns"]):
            assert _bits(out["spline_lengths"][t], raw["lengths"][t, :n]) and _bits(out["s_ref"][t], raw["s_ref"][t, :n + 1])
        for v, t in enumerate(L["track_of"]):
            n, m = P["ns"][t], P["ms"][t]
            assert out["ltpl"][v].shape == (n + 1, 12) and _bits(out["ltpl"][v], raw["ltpl"][v, :n + 1]) and _bits(out["idx"][v], raw["idx"][v, :n])
            rc = out["race_cl"][v]
            assert rc.shape == (m + 1, 7) and _bits(rc[:m], L["trajs"][v]) and _bits(rc[m, 1:], L["trajs"][v][0, 1:]) and _bits(rc[m, 0], raw["total"][t])
            summed = np.sum(xr.front(*L["tracks"][t])["lengths"])
            g = xg.guards("%s/%d" % (family, n))[2]
            worst.add("%s.race_cl" % family, xg.dmax(rc[m, 0], summed), g)
            assert xg.dmax(rc[m, 0], summed) <= g
    try:
        eng.export_batch(list(refs), list(nvs), list(als), P["traj"])
    except ValueError:
        pass
    else:
        raise AssertionError("export_batch took 3 tracks for 7 variants without track_of")


# ---- end to end: solve -> raceline -> profile -> trajectory -> export --------------------------------------------------------------------------
E2E_STEP = 6.0


def run_resident(eng, g, vehicle):
    """solve -> raceline -> profile -> trajectory -> export as ONE chain of device entries on resident arrays: the inputs go up once, nothing comes
    back before the last launch.  Returns the downloaded arrays."""
    ref, nv = np.ascontiguousarray(g["reftrack"]), np.ascontiguousarray(g["normvec"])
    ggv, axm, drag, mass, vmax = vehicle
    n = ref.shape[0]
    poly = np.vstack((ref[:, :2], ref[:1, :2]))
    mmax = int(1.25 * np.sum(np.hypot(*np.diff(poly, axis=0).T)) / E2E_STEP) + 16
    lib, h = eng.lib, eng.h
    with eng.scope() as dev:
        up, new = dev.up, dev.new
        d_ref, d_nv, d_sc = up(ref), up(nv), up(np.ascontiguousarray(g["scaling"]))
        d_al, d_curv, d_qst = new(n * 8), new(8), new(4)
        d_xy, d_psi, d_k, d_el, d_m, d_rst = new(mmax * 16), new(mmax * 8), new(mmax * 8), new(mmax * 8), new(4), new(4)
        d_g, d_a, d_s3 = up(ggv), up(axm), [up(np.array([x], dtype=np.float64)) for x in (drag, mass, vmax)]
        d_vx, d_lap = new(mmax * 8), new(8)
        d_traj, d_t, d_len, d_lim, d_fl = new(mmax * 56), new((mmax + 1) * 8), new(8), new(48), new(4)
        d_tab, d_idx, d_sl, d_s, d_tot, d_xst = new((n + 1) * 96), new(n * 4), new(n * 8), new((n + 1) * 8), new(8), new(4)
        eng.solve_device(1, n, d_ref, d_nv, d_sc, float(g["kappa_bound"]), float(g["w_veh"]), d_al, d_curv, d_qst)
        eng._check(lib.mcq_raceline_device(h, 1, n, None, d_ref, d_nv, d_al, E2E_STEP, mmax, d_xy, d_psi, d_k, d_el, d_m, d_rst), "mcq_raceline_device")
        eng._check(lib.mcq_vel_profile_device_ragged(h, 1, mmax, d_m, None, d_k, d_el, d_g, ggv.shape[0], d_a, axm.shape[0], d_s3[0], d_s3[1], d_s3[2],
                                                     1.0, d_vx, d_lap), "mcq_vel_profile_device_ragged")
        eng.trajectory_device(1, 0, mmax, d_m, None, d_xy, d_psi, d_k, d_el, d_vx, True, d_s3[0], d_s3[1], d_s3[2], d_g, ggv.shape[0], d_a,
                              axm.shape[0], float(g["kappa_bound"]), d_traj, d_t, d_len, d_lim, d_fl)
        eng.export_device(1, n, None, d_ref, d_nv, d_al, 1, mmax, d_m, None, d_traj, d_tab, d_idx, d_sl, d_s, d_tot, d_xst)
        st = [int(eng.download(p, (1,), np.int32)[0]) for p in (d_qst, d_rst, d_fl, d_xst)]
        return dict(statuses=st, alpha=eng.download(d_al, (n,), np.float64), m=int(eng.download(d_m, (1,), np.int32)[0]), mmax=mmax,
                    traj=eng.download(d_traj, (1, mmax, 7), np.float64), lap=eng.download(d_lap, (1,), np.float64),
                    t=eng.download(d_t, (mmax + 1,), np.float64), ltpl=eng.download(d_tab, (1, n + 1, 12), np.float64),
                    idx=eng.download(d_idx, (1, n), np.int32), lengths=eng.download(d_sl, (1, n), np.float64),
                    s_ref=eng.download(d_s, (1, n + 1), np.float64), total=eng.download(d_tot, (1,), np.float64),
                    status=eng.download(d_xst, (1,), np.int32))


def check_end_to_end(eng, golden, worst):
    """The Berlin golden through the engine's own stages on resident arrays; the export is held to the reference ON THE DEVICE'S OWN TRAJECTORY,
    and Engine.export_batch on the downloaded arrays returns the chain's bits."""
    g = golden
    ref, nv = g["reftrack"], g["normvec"]
    n = ref.shape[0]
    vehicle = gc._vehicle(gc._seed("export", "e2e"), 19, on_grid=False)
    res = run_resident(eng, g, vehicle)
    assert res["statuses"][0] == OK and res["statuses"][1] == OK and res["statuses"][2] >= 0 and res["statuses"][3] == OK, res["statuses"]
    assert float(np.max(np.abs(res["alpha"] - g["alpha"]))) < 1e-6
    m = res["m"]
    assert _bits(res["t"][m], res["lap"][0]) and np.isfinite(res["lap"][0])
    track = (ref, nv, res["alpha"])
    traj = res["traj"][0, :m]
    assert np.all(np.isfinite(traj)) and np.all(np.isnan(res["traj"][0, m:]))
    live = xg.compute_spread(track)
    R = xr.table(*track, traj)
    g_s = hold_track(worst, None, res, 0, n, xr.front(*track), "e2e", live=live)
    hold_variant(res, 0, 0, track, traj, R, g_s, "e2e")
    assert m == math.ceil(res["total"][0] / E2E_STEP), "m_out %d, spline_total / stepsize %r" % (m, res["total"][0] / E2E_STEP)
    out = eng.export_batch([ref], [nv], [res["alpha"]], dict(traj=res["traj"], m=np.array([m], dtype=np.int32)))
    assert out["status"][0] == OK and _bits(out["ltpl"][0], res["ltpl"][0]) and _bits(out["idx"][0], res["idx"][0]) and \
        _bits(out["spline_total"], res["total"]) and _bits(out["race_cl"][0][:m], traj)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "traj_ltpl.csv")
        export.write_traj_ltpl(path, out["ltpl"][0])
        _, digest, names, rows = export.read_table(path)
        assert names == export.LTPL_COLUMNS and digest == export.ggv_digest(None) and rows.shape == (n, 12)
        assert np.max(np.abs(rows - out["ltpl"][0][:n])) <= 0.5000001e-7, "the file does not parse back to the table at 7 decimals"
        export.write_traj_race(path, out["race_cl"][0])
        _, _, names, rows = export.read_table(path)
        assert names == export.RACE_COLUMNS and rows.shape == (m + 1, 7) and np.max(np.abs(rows - out["race_cl"][0])) <= 0.5000001e-7
