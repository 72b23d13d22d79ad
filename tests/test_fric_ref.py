"""The friction reference (tests/fric_ref.py) held to arrays recorded from the reference's OWN get_friction_singlepos, extract_friction_coeffs and
approx_friction_map("linear") (tests/golden/friction/reference.npz, scripts/make_golden_friction.py), on rounded_rectangle whole and Berlin with
the varmue08-12 data -- on the CPU, no engine.  What the engine is then held to (tests/test_emu_fric.py, tests/test_gpu_fric.py) is this reference."""
import os

import numpy as np
import pytest

import fric_cases as fc
import fric_guard as fg
import fric_ref as fr


def test_the_case_table_is_what_its_names_say():
    fc.check_case_table()
    assert set(fc.maps()) >= {"one", "two", "line3", "lattice", "ring", "dup", "c255", "c256", "c257", "onebin", "sparse", "edges", "nanmue"}
    for name, q, want in fc.exact_ties():
        idx, _, gap = fr.nearest(fc.maps()[name][0], [q])
        assert idx[0] == want and (gap[0] == 0 or name in ("dup", "edges", "lattice") and gap[0] >= 0), (name, q)


def test_fixture_size_and_map_expansion():
    assert os.path.getsize(fg.PATH) < 1000000
    g = fg.recorded("berlin_2018")
    assert g["cells"].shape == (104191, 2) and 0.80 < g["mue"].min() < 0.82 and 1.18 < g["mue"].max() < 1.20
    assert np.array_equal(g["cells"] * 2.0, np.round(g["cells"] * 2.0))
    r = fg.recorded("rounded_rectangle")
    assert r["cells"].shape == (13252, 2) and np.all(r["mue"] == 1.0)


@pytest.mark.parametrize("track", fg.TRACKS)
def test_nearest_against_ckdtree_and_the_reference_lookup(track):
    g = fg.recorded(track)
    idx, dist, gap = fg.recorded_nearest(track)
    single = gap > fg.INDEX_TOL
    assert single.sum() >= 1990 and np.array_equal(idx[single], g["q_idx"][single])
    assert np.all(fr.dists_to(g["cells"], g["q"], g["q_idx"]) - dist <= fg.INDEX_TOL)
    assert np.array_equal(g["mue"][idx][single], g["q_mue"][single])


@pytest.mark.parametrize("track", fg.TRACKS)
def test_grid_rows_against_the_reference_extraction(track):
    g = fg.recorded(track)
    z = np.load(os.path.join(os.path.dirname(fg.PATH), "..", track + ".npz"))
    R = fr.grid(z["reftrack"], z["normvec"], g["width"], g["wb_f"], g["wb_r"], g["dn"])
    assert [r["cnt"] for r in R] == list(g["cnt"]) and g["decided"][~np.isnan(g["mue4"])].all()
    if track == "berlin_2018":
        assert len(R) == 777 and min(g["cnt"]) == 10 and max(g["cnt"]) == 75 and 4 * int(g["cnt"].sum()) == 74228
    rng = np.random.default_rng(5)
    worst = 0.0
    for i, r in enumerate(R):
        assert r["n"].tobytes() == g["n"][i, :r["cnt"]].tobytes()
        for k in range(4):
            s, c = fr.line(r["n"], g["mue4"][k, i, :r["cnt"]])
            worst = max(worst, float(abs(s - g["w"][k, i, 0])), float(abs(c - g["w"][k, i, 1])))
    assert worst <= float(fg.fixture()["w_floor"]) and fg.w_guard() < 1e-13
    for i in rng.choice(len(R), 6, replace=False):      # the lookups of a few rows (every row: the engine's tests)
        for k in range(4):
            idx = fr.nearest(g["cells"], R[i]["xy"][k])[0]
            assert np.array_equal(g["mue"][idx], g["mue4"][k, i, :R[i]["cnt"]])
