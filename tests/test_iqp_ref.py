"""tests/iqp_ref.py, tests/iqp_cases.py and tests/iqp_guard.py on their own (no engine, no GPU): the reference loop IS oracle/tph_ref.iqp_handler; every
case of the table is decided -- round count and every ring's waypoint count, with room, on every route -- and reaches the branch it is in the table
for; the guards stay under their cap; the stored spreads are what tests/iqp_guard.py computes.  An undecided case fails here, before anything
reaches an engine."""
import numpy as np
import pytest

import iqp_cases as ic
import iqp_guard as ig
import iqp_ref
from oracle import tph_ref


@pytest.mark.parametrize("name", ["golden/rounded_rectangle", "ladder/5/7"])
def test_loop_is_the_oracles_bit_for_bit(name):
    c = ic.CASES[name]
    t = ic.track(c["track"])
    tr = []
    al, ref, nv = tph_ref.iqp_handler(t["reftrack"], t["normvectors"], t["A"], c["kappa_bound"], c["w_veh"], c["stepsize"], c["iters_min"],
                                      c["allowed"], trace=tr)
    R = iqp_ref.run(t["reftrack"], t["normvectors"], t["A"], c["kappa_bound"], c["w_veh"], c["stepsize"], c["iters_min"], c["allowed"])
    assert len(R) == len(tr) == c["rounds"] and R[-1]["stopped"]
    assert np.array_equal(al, R[-1]["alpha"]) and np.array_equal(ref, R[-1]["reftrack"]) and np.array_equal(nv, R[-1]["normvec"])
    for a, b in zip(tr, R):
        assert a["n"] == b["n"] and a["curv_error_max"] == b["curv_error_max"]
        assert np.array_equal(a["alpha"], b["alpha"]) and np.array_equal(a["reftrack"], b["reftrack"]) and np.array_equal(a["normvec"], b["normvec"])
    # a capped run is the uncapped run's first rounds
    m = len(R) - 1
    C = iqp_ref.run(t["reftrack"], t["normvectors"], t["A"], c["kappa_bound"], c["w_veh"], c["stepsize"], c["iters_min"], c["allowed"], max_rounds=m)
    assert len(C) == m and not C[-1]["stopped"] and all(np.array_equal(a["alpha"], b["alpha"]) for a, b in zip(C, R))


@pytest.mark.parametrize("name", tuple(ic.CASES))
def test_case_is_decided(name):
    """On every route: the rounds the table states; in every round where the error decides, it is at least ROUND_GAP x allowed away from allowed;
    length / stepsize of every re-sampling at least INTEGER_GAP away from every integer (tests/test_glue_ref.py::test_point_counts_are_decided);
    the routes count the same waypoints."""
    c = ic.CASES[name]
    runs = {route: ic.reference(name, route) for route in ("gi",) + ig.routes(name)}
    for route, R in runs.items():
        assert len(R) == c["rounds"] <= ic.MAX_ROUNDS and R[-1]["stopped"], (route, len(R))
        assert [r["n"] for r in R] == [r["n"] for r in runs["gi"]], route
        for r in R:
            assert 3 <= r["n"] <= ic.MAX_N
            if r["iter"] >= c["iters_min"]:
                assert abs(r["curv_error_max"] - c["allowed"]) >= ic.ROUND_GAP * c["allowed"], (route, r["iter"], r["curv_error_max"])
            if r["ratio"] is not None:
                assert abs(r["ratio"] - np.rint(r["ratio"])) >= ic.INTEGER_GAP, (route, r["iter"], r["ratio"])


def test_ladder_and_cap_cover_what_they_say():
    lad = [ic.CASES[n] for n in ic.CASES if n.startswith("ladder/")]
    assert {c["iters_min"] for c in lad} == {1, 2, 3, 5}
    for im in (1, 2, 3, 5):
        extra = sorted(c["rounds"] - im for c in lad if c["iters_min"] == im)
        assert extra[0] == 0 and 1 <= extra[1] <= 3, (im, extra)
    c = ic.CASES[ic.CAP_CASE]
    assert c["rounds"] == ic.CAP_ROUNDS > c["iters_min"] and ic.CAP_ROUNDS - 1 in ic.CAP_BELOW and min(ic.CAP_BELOW) < c["iters_min"]
    assert ic.CAP_FREE == (ic.CAP_ROUNDS, ic.CAP_ROUNDS + 1)
    assert ic.CASES["trace/t12"]["rounds"] == 18 and ic.CASES["trace/t12"]["iters_min"] == 18
    assert ic.reference("trace/t12")[0]["n"] == min(ic.reference(n)[0]["n"] for n in ic.CASES)          # the smallest ring of the table


@pytest.mark.parametrize("name", tuple(ic.SWITCHES))
def test_switch_cases_cross_their_switch(name):
    switch, way = int(name.split("/")[1]), name.split("/")[2]
    ns = [r["n"] for r in ic.reference(name)]
    assert tuple(ns[:2]) == ic.SWITCHES[name][4]
    assert (ns[0] < switch <= ns[1]) if way == "up" else (ns[0] >= switch > ns[1]), ns


def test_curvature_rows_are_active_inside_the_loop():
    act = [r["kappa_active"] for r in ic.reference("kappa/k296")]
    assert any(a > 0 for a in act[1:]), act
    for name in ic.CASES:
        if not name.startswith("kappa/"):
            assert not any(r["kappa_active"] for r in ic.reference(name)), name


def test_batches_cover_what_they_say():
    kinds = [k for k, _ in ic.MIXED]
    assert 10 <= len(ic.MIXED) <= 12 and sorted(set(kinds)) == ["empty", "nan", "narrow", "ok", "overflow"]
    ends = [len(ic.reference("batch/" + t)) for k, t in ic.MIXED if k == "ok"]
    assert set(ends) == {3, 4, 5} and len({ic.reference("batch/" + t)[-1]["n"] for k, t in ic.MIXED if k == "ok"}) == len(ends)
    assert {len(ic.reference("batch/" + t)) for _, t in ic.SAME_ROUND} == {3}
    for k, t in ic.MIXED + ic.SAME_ROUND:
        if k == "ok":
            assert all(r["n"] <= ic.BATCH_NMAX for r in ic.reference("batch/" + t))
    # the overflowing track: it fits on entry, its first re-sampling does not (and is decided)
    t = ic.track("coarse100")
    R = iqp_ref.run(t["reftrack"], t["normvectors"], t["A"], ic.KAPPA, ic.W_VEH, ic.BATCH_STEP, ic.BATCH_ITERS_MIN, ic.BATCH_ALLOWED, max_rounds=2)
    assert R[0]["n"] <= ic.BATCH_NMAX < R[1]["n"] and abs(R[0]["ratio"] - np.rint(R[0]["ratio"])) >= ic.INTEGER_GAP
    # the narrow track is what the oracle refuses
    with pytest.raises(RuntimeError, match="Problem not solvable"):
        b = ic.batch_track("narrow", "o75")
        tph_ref.constraints_dense(b["reftrack"], np.zeros((75, 75)), np.zeros(75), ic.KAPPA, ic.W_VEH)


def test_guards_are_capped():
    """No guard above CAP x its floor (tests/iqp_guard.py); prints which are above the floor at all."""
    above = []
    for name in ic.CASES:
        for q, g in ig.guards(name).items():
            assert g <= ig.CAP * ig.FLOOR[q], (name, q, g)
            if g > ig.FLOOR[q]:
                above.append((name, q, g))
    print("guards above their floor: %s" % (above or "none -- every guard is its floor"))


def test_stored_spreads_are_complete_and_reproducible():
    """The file holds exactly the table's cases; a sample recomputed gives the same guards.  (The spreads are differences of two solvers' rounding:
    their own last digits move with the linear-algebra library's threading, so the GUARDS are compared, to 25 %.)"""
    z = np.load(ig.PATH)
    assert sorted(str(n) for n in z["name"]) == sorted(ic.CASES) and z["spread"].shape == (len(ic.CASES), len(ig.Q))
    for name in ("ladder/3/6", "switch/48/up", "switch/20/down", "trace/t12", "batch/c120", "cap/o60", "kappa/k296"):
        new, old = ig.compute_spread(name), ig.spread(name)
        floor = np.array([ig.FLOOR[q] for q in ig.Q])
        assert np.allclose(np.maximum(floor, 4 * new), np.maximum(floor, 4 * old), rtol=0.25, atol=0.0), (name, new, old)
