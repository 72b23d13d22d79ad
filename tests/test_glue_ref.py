"""tests/glue_ref.py, tests/glue_cases.py and tests/glue_guard.py on their own (no engine, no GPU): the reference agrees with what the project already
trusts (the dense oracle/tph_ref.py, oracle/vel_ref.py's crossing check, the engine's numpy statement of the fp32 layouts); the case tables meet the
conditions that make exact comparisons of point counts and verdicts legitimate; the guards stay within caps, so that none can hide a failure; the stored
spreads are what tests/glue_guard.py computes."""
import numpy as np
import pytest

import glue_cases as gc
import glue_guard as gg
import glue_ref
from global_racetrajectory_optimization_amd import engine
from oracle import tph_ref, vel_ref

LD = np.longdouble


def _blob(n):
    rng = np.random.default_rng(n)
    th = np.linspace(0.0, 2.0 * np.pi, n, endpoint=False)
    r = 30.0 + 5.0 * np.cos(3 * th) + rng.uniform(-1.0, 1.0, n) * min(1.0, 30.0 / n)       # rough, but no cusps at n = 333
    return np.column_stack((r * np.cos(th) + 100.0, 0.7 * r * np.sin(th) - 50.0))


@pytest.mark.parametrize("n", [3, 4, 7, 40, 97, 333])
@pytest.mark.parametrize("dtype", [np.float64, LD])
def test_reference_matches_the_dense_oracle(n, dtype):
    xy = _blob(n)
    scale = float(np.max(np.abs(xy)))
    tol = 1e-11 * scale
    for dist in (True, False):
        cx, cy, A, nv_d = tph_ref.calc_splines(np.vstack((xy, xy[0])), use_dist_scaling=dist)
        coef, s = glue_ref.closed_spline(xy, dtype, dist_scaling=dist)
        C = np.stack(coef, axis=2)
        assert gg.dmax(C[:, 0, :], cx) < tol and gg.dmax(C[:, 1, :], cy) < tol
        assert gg.dmax(glue_ref.normals_of(coef), nv_d) < 1e-11
        s_A = np.array([-A[4 * i + 2, 4 * i + 5] for i in range(n - 1)] + [A[4 * n - 2, 1]])
        assert gg.dmax(s, s_A) < 1e-11
    th = np.linspace(0.0, 2.0 * np.pi, n, endpoint=False)
    alpha = 0.5 * np.sin(2 * th)
    ref = np.column_stack((xy, 3.0 + 0.3 * np.cos(th), 3.0 + 0.3 * np.sin(th)))
    for step in (2.0, 3.0, 0.77):
        rl, _, cx, cy, inds, tv, s_interp, lengths, el = tph_ref.create_raceline(xy, nv_d, alpha, step)
        r = glue_ref.raceline(ref, nv_d, alpha, step, dtype)
        assert r["m"] == rl.shape[0]
        assert gg.dmax(r["xy"], rl) < tol and gg.dmax(r["el_lengths"], el) < tol and abs(float(r["total"]) - float(np.sum(lengths))) < tol
        # heading and curvature from the oracle's coefficients at the oracle's own (segment, t): values, not indices
        xd = cx[inds, 1] + 2 * cx[inds, 2] * tv + 3 * cx[inds, 3] * tv ** 2
        yd = cy[inds, 1] + 2 * cy[inds, 2] * tv + 3 * cy[inds, 3] * tv ** 2
        xdd = 2 * cx[inds, 2] + 6 * cx[inds, 3] * tv
        ydd = 2 * cy[inds, 2] + 6 * cy[inds, 3] * tv
        assert gg.dpsi(r["psi"], np.arctan2(yd, xd) - np.pi / 2) < 1e-11
        assert gg.dmax(r["kappa"], (xd * ydd - yd * xdd) / (xd ** 2 + yd ** 2) ** 1.5) < 1e-11 * max(1.0, float(np.max(np.abs(r["kappa"]))))
        assert np.all(r["psi"] >= -np.pi) and np.all(r["psi"] < np.pi)
        # the re-linearisation: interp_track_widths on the shifted widths, normals of the unit-scaling spline through the new ring
        q = glue_ref.relinearise(ref, nv_d, alpha, 1.0, step, dtype)
        w = tph_ref.interp_track_widths(np.column_stack((ref[:, 2] - alpha, ref[:, 3] + alpha)), inds, tv)
        _, _, _, nv_new = tph_ref.calc_splines(np.vstack((rl, rl[0])), use_dist_scaling=False)
        assert q["m"] == rl.shape[0] and gg.dmax(q["rows"][:, :2], rl) < tol and gg.dmax(q["rows"][:, 2:], w) < 1e-11
        assert gg.dmax(q["normals"], nv_new) < 1e-11
    nv_p, s_p = glue_ref.prep(ref, dtype)
    _, _, A, nv_d = tph_ref.calc_splines(np.vstack((xy, xy[0])))
    assert gg.dmax(nv_p, nv_d) < 1e-11


def test_crossing_reference_matches_the_oracle(golden):
    from test_emu_kernels import _crossing_cases
    for trk, nv in _crossing_cases(golden)[:3]:
        for hz in (1, 5, 10):
            assert glue_ref.normals_crossing(trk, nv, hz, LD)[0] == int(vel_ref.check_normals_crossing(trk, nv, hz))
            assert glue_ref.normals_crossing(trk, nv, hz, np.float64)[0] == int(vel_ref.check_normals_crossing(trk, nv, hz))
    trk, nv = _crossing_cases(golden)[3]
    assert glue_ref.normals_crossing(trk, nv, 10, LD)[0] == -1
    for name, trk, nv, _ in gc.crossing_cases():             # every new case, n = 600 included; the longest horizon where the oracle's loops allow
        n = trk.shape[0]
        for hz in (10,) + ((n - 1, n - 2) if n <= 12 or name == "wrap_only255" else ()):
            assert glue_ref.normals_crossing(trk, nv, hz, LD)[0] == int(vel_ref.check_normals_crossing(trk, nv, hz)), (name, hz)
        with pytest.raises(RuntimeError, match="too large"):
            vel_ref.check_normals_crossing(trk, nv, n)
        assert glue_ref.normals_crossing(trk, nv, n, LD)[0] == -1


def test_fp32_layouts_match_the_engine_helpers():
    for batch, n in gc.F32_SHAPES:
        ref = gc.f32_tracks(batch, n)
        inc32, org = engine.rows_to_increments(ref)
        for dtype in (np.float64, LD):
            for origin in (None, org):
                assert gg.dmax(glue_ref.rows_increments(inc32, origin, dtype), engine.increments_to_rows(inc32, origin)) < 1e-12 * max(1.0, float(np.max(np.abs(ref[..., :2]))))
        assert gg.dmax(glue_ref.rows_increments(inc32, org, LD)[..., :2], ref[..., :2]) < 1e-3          # the float increments carry the ring
        assert np.array_equal(glue_ref.rows_absolute(ref.astype(np.float32), None, np.float64), ref.astype(np.float32).astype(np.float64))
    assert sorted((b * n) % 4 for b, n in gc.F32_SHAPES) == [0, 1, 2, 3, 3, 3, 3]


# ---- the conditions of the case tables ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", tuple(gc.FAMILIES))
def test_point_counts_are_decided(family):
    """total / stepsize of every row of every launch is at least 1e-6 away from every integer in the longdouble reference (and the float64 run and
    every perturbed run count the same points: glue_guard.compute_* assert that when the spreads are made); the aimed launches hit their counts."""
    hit = {}
    for name, sizes, step, mmax in gc.raceline_launches(family):
        for n in sizes:
            r = gg.raceline_ref(family, n, step)
            assert abs(r["ratio"] - np.rint(r["ratio"])) >= gc.INTEGER_GAP, (name, n)
            hit.setdefault(name, []).append(r["m"] - mmax)
        if "@" in name:
            K = int(name.split("@")[1])
            m = gg.raceline_ref(family, K, step)["m"]
            want = {"m==mmax": mmax, "m==mmax+1": mmax + 1, "m==3": 3, "m==2": 2, "m==1": 1}[name.split("@")[0]]
            assert m == want, (name, m)
    assert all(0 in v or "+1" in k or "m==1" in k for k, v in hit.items())          # every generous launch has a ring AT mmax
    for name, sizes, sc, step, nmax in gc.relin_launches(family):
        ms = []
        for n in sizes:
            r = gg.relin_ref(family, n, sc, step)
            assert abs(r["ratio"] - np.rint(r["ratio"])) >= gc.INTEGER_GAP, (name, n)
            ms.append(r["m"])
        if "@" in name:
            assert ms[sizes.index(int(name.split("@")[1]))] == int(name.split("@")[0][3:])
    assert set(gc.SIZES) >= {3, 97, 2048, 2049, 4096, 4097} and len(gc.SIZES) == 30


def test_crossing_cases_are_decided():
    cases = gc.crossing_cases()
    assert {c[1].shape[0] for c in cases} == set(gc.CROSS_N)
    for name, trk, nv, exact in cases:
        n = trk.shape[0]
        for hz in gc.crossing_horizons():
            v, margin = glue_ref.normals_crossing(trk, nv, hz, LD)
            assert v == (-1 if hz >= n else v)
            if hz < n and not exact:
                assert margin > gc.MARGIN_MIN, (name, hz, margin)
        hz = 10
        v = glue_ref.normals_crossing(trk, nv, hz, LD)[0]
        if name.startswith("wrap_only"):            # only the pairs that reach across the end of the arrays find it
            assert v == 1 and glue_ref.normals_crossing(trk, nv, hz, LD, wrap=False)[0] == 0
            assert glue_ref.normals_crossing(trk, nv, 2, LD)[0] == 0 and glue_ref.normals_crossing(trk, nv, 3, LD)[0] == 1
        if name.startswith("parallel"):             # the same pair on either side of the collinearity skip
            assert v == (1 if "2e-8" in name else 0)
        if name.startswith("on_bound"):
            assert v == 1 and glue_ref.normals_crossing(trk, nv, hz, LD)[1] == 0.0
        if name.startswith("ulp_inside"):
            assert v == 0
        if name.startswith("narrow"):
            assert v == 0
        if name.startswith("wide"):
            assert v == 1


def test_velocity_case_table_covers_what_it_says():
    Ls = gc.vel_launches()
    assert gc.vel_case_count() >= 300
    assert {L["kappa"].shape[1] for L in Ls if L["n_of_track"] is None} >= set(gc.VEL_N)
    assert {L["ggv"].shape[0] for L in Ls} >= {1, 63, 64, 65, 129, 1000}
    assert {L["ggv"].shape[1] for L in Ls} == {1, 2, 19} and {L["exp"] for L in Ls} == {1.0, 1.5, 2.0}
    assert any(L["n_of_track"] is not None and L["mu"] is not None and (L["filt_window"] or 0) > 1 for L in Ls)
    assert {L["filt_window"] for L in Ls} >= {None, 1, 3, 7} and all(L["filt_window"] == L["kappa"].shape[1] for L in Ls if L["name"].startswith("fw==n"))
    clipped = zeros = on_grid = 0
    for L in Ls:
        for v in range(min(L["ggv"].shape[0], 40)):
            r = gg.vel_ref_case(L, v)
            t, n = gg.vel_row(L, v)
            if r is None:
                assert n == 1 or n > L["kappa"].shape[1]
                continue
            clipped += bool(np.any(r[0] >= L["vmax"][v] * (1 - 1e-12)))
            zeros += bool(np.any(L["kappa"][t, :n] == 0.0))
            on_grid += bool(np.any(L["ggv"][v][:, 0] == L["vmax"][v]))
    assert clipped > 50 and zeros > 50 and on_grid > 50


# ---- the guards ----------------------------------------------------------------------------------------------------------------------------
def test_stored_spreads_are_complete_and_reproducible():
    ent = gg.entries()
    z = np.load(gg.PATH)
    assert sorted(z.files) == sorted(ent)
    for key in ("raceline/stadium/2.0", "raceline/trefoil/m==mmax@97", "relin/peanut/0.61h", "prep/stadium", "vel/n63", "vel/ragged_fw3"):
        if key.startswith("vel/"):
            L = [x for x in gc.vel_launches() if x["name"] == key[4:]][0]
            only = list(range(0, L["ggv"].shape[0], 9))
            new, old = gg.compute_vel_spread(L, only=only)[only], gg.spread(key)[only]
        else:
            new, old = ent[key](), gg.spread(key)
        assert new.shape == old.shape
        assert np.allclose(np.maximum(4 * new, 1e-13), np.maximum(4 * old, 1e-13), rtol=1e-3, atol=0.0), key


def test_velocity_guards_are_capped():
    """At most 2 % of the cases carry a guard above the floor, none above 1e-7 (a sweep's flipped `<` moves a profile by far more: such a case is
    regenerated from another seed, glue_cases.VEL_SEEDS, not kept under a wide guard)."""
    S = np.vstack([gg.spread("vel/" + L["name"]) for L in gc.vel_launches()])
    assert S.shape == (gc.vel_case_count(), 2)
    for qi, q in enumerate(gg.VEL_Q):
        g = np.maximum(gg.FLOOR[q], 4.0 * S[:, qi])
        assert np.mean(g > gg.FLOOR[q]) <= 0.02 and np.max(g) <= 1e-7, (q, float(np.mean(g > gg.FLOOR[q])), float(np.max(g)))


@pytest.mark.parametrize("family", tuple(gc.FAMILIES))
def test_geometry_guards_are_capped(family):
    """Per family and quantity: at most 5 % of the cases above 100 x the floor, none above 1e4 x, rings up to 513 waypoints on the floor.

    One quantity cannot meet the last clause for any ring, and is held to its derivation instead: a scaling l_i / l_(i+1) moves by
    (dl_i + dl_(i+1)) / l under a perturbation of the coordinates, dl <= 2 sqrt(2) X rel |r| for coordinates up to X and normal draws r; with
    |r| <= 5 that is 4 x 2 x 2 sqrt(2) x 5 x 1e-15 X / l = 1.1e-13 X / l for the guard: on the 1e-12 floor only while X / l < 9, and a closed ring
    of n waypoints has X / l >= n / (2 pi).  So prep_scalings is asserted against that bound (the floor where the bound is below it) AND against
    what the generator achieves: on the floor up to 257 waypoints and within 2.5 x at 513 for the families around the origin, within 30 x the
    floor everywhere (the family at (1000, -2000) m starts at 5 x: X / l = 200 at any size)."""
    tables = [("raceline", gc.raceline_launches(family), gg.RACE_Q), ("relin", gc.relin_launches(family), gg.RELIN_Q)]
    for kind, launches, Q in tables:
        S = np.vstack([gg.spread("%s/%s/%s" % (kind, family, L[0])) for L in launches])
        ns = np.concatenate([np.array(L[1]) for L in launches])
        for qi, q in enumerate(Q):
            g = np.maximum(gg.FLOOR[q], 4.0 * S[:, qi]) / gg.FLOOR[q]
            assert np.mean(g > 100.0) <= 0.05 and np.max(g) <= 1e4 and np.all(g[ns <= 513] == 1.0), (kind, q, float(np.max(g)), float(np.max(g[ns <= 513])))
    S = gg.spread("prep/" + family)
    ns = np.array(gc.SIZES)
    g = np.maximum(gg.FLOOR["prep_normals"], 4.0 * S[:, 0]) / gg.FLOOR["prep_normals"]
    assert np.max(g) <= 1e4 and np.mean(g > 100.0) <= 0.05 and np.all(g[ns <= 513] == 1.0)
    g = np.maximum(gg.FLOOR["prep_scalings"], 4.0 * S[:, 1]) / gg.FLOOR["prep_scalings"]
    assert np.max(g) <= 30.0                                    # what the generator achieves: far inside the general caps (100 x, 1e4 x)
    if family != "stadium":                                     # around the origin X / l = n / (2 pi) is as small as a ring allows
        assert np.all(g[ns <= 257] == 1.0) and np.all(g[ns <= 513] <= 2.5)
    for k, n in enumerate(gc.SIZES):
        xy = gc.ring(family, n)[0][:, :2]
        l = np.hypot(*(np.roll(xy, -1, axis=0) - xy).T)
        bound = 4.0 * 2.0 * 2.0 * np.sqrt(2.0) * 5.0 * gg.SPREAD_REL * float(np.max(np.abs(xy))) / float(np.min(l)) * float(np.max(l) / np.min(l))
        assert g[k] * gg.FLOOR["prep_scalings"] <= max(gg.FLOOR["prep_scalings"], bound), (n, g[k], bound)
