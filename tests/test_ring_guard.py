"""The spread data behind the GPU ring tests' guards (tests/ring_guard.py, tests/golden/ring_spread.npz written by
scripts/make_golden_ring_spread.py): every ring fixture has a finite entry, and the entries of the two smallest tracks recompute."""
import glob
import os

import numpy as np

import ring_guard
from conftest import GOLDEN_DIR, load_golden


def test_every_ring_fixture_has_a_spread_entry():
    z = np.load(ring_guard.PATH)
    have = list(zip((str(s) for s in z["name"]), (str(s) for s in z["what"]), (int(k) for k in z["k"])))
    assert len(set(have)) == len(have)
    assert set(have) == set(ring_guard.expected_entries())
    assert np.all(np.isfinite(z["spread"])) and np.all(z["spread"] > 0.0)
    assert np.array_equal(z["spread"], np.maximum(z["perturb_spread"], z["route_gap"]))
    # a new ring golden cannot land without an entry: every fixture file in tests/golden/ but the open chains and the recorded runs
    names = {str(s) for s in z["name"]}
    for path in glob.glob(os.path.join(GOLDEN_DIR, "*.npz")):
        name = os.path.basename(path)[:-4]
        if name.startswith("open_") or name in ("harness_runs", "ring_spread", "glue_spread"):      # (glue_spread: tests/glue_guard.py's table)
            continue
        if name == "gi_edges":      # (the Goldfarb-Idnani edge cases carry their spread per case, by the same draws and the same rule:
            continue                #  tests/gi_cases.guard, held finite and positive by tests/test_gi_ref.py::test_case_is_decided)
        assert name in names, "ring fixture %s has no entry in ring_spread.npz (scripts/make_golden_ring_spread.py)" % name
    # the guard rule of tests/open_ref.py
    for name, what, k in have[:5]:
        assert ring_guard.guard(name, None if k < 0 else k, what) == max(1e-8, 4.0 * ring_guard.spread(name, None if k < 0 else k, what))


def test_spread_of_the_smallest_tracks_recomputes():
    """The perturbation spread of rounded_rectangle and handling_track, recomputed with the generator's draws: within a factor of 2 of the
    stored value (bitwise where the BLAS runs as it did there)."""
    from oracle import tph_ref
    for name in ("rounded_rectangle", "handling_track"):
        g = load_golden(name)
        ref = g["reftrack"]
        A = tph_ref.calc_splines(np.vstack((ref[:, :2], ref[0, :2])))[2]
        worst = 0.0
        for draw in range(ring_guard.SPREAD_DRAWS):
            rng = ring_guard.draw_rng(name, "alpha", -1, draw)
            a = tph_ref.opt_min_curv(ref, g["normvec"], A, float(g["kappa_bound"]), float(g["w_veh"]), solver=ring_guard.perturbed_solver(rng))[0]
            worst = max(worst, ring_guard.dmax(a, g["alpha"]))
        z = np.load(ring_guard.PATH)
        j = [k for k in range(len(z["name"])) if str(z["name"][k]) == name and str(z["what"][k]) == "alpha"][0]
        stored = float(z["perturb_spread"][j])
        assert stored / 2.0 <= worst <= 2.0 * stored, (name, worst, stored)
