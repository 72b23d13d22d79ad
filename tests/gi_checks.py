"""The bodies of the Goldfarb-Idnani edges suite, shared by the SIMT interpreter's run (tests/test_emu_gi_edges.py) and the MI355X's
(tests/test_gpu_gi_edges.py).  Every case of tests/gi_cases.py goes through Engine.solve_batch(..., algorithm=ALG_GI) and is held to what the dense
restatement (tests/gi_ref.py, engine's rule) wrote into tests/golden/gi_edges.npz -- STEP COUNTS and working sets, not only alpha: the polish after
gi_solve repairs a wrong vertex, so alpha alone meets 1e-9 m over a wrong back-substitution, rotation or projection.  What gives those away is the
number of steps, as_iters == 1 (the polish had nothing to exchange) and second_attempt bit 3 (the polish was rejected).

Every figure is printed before it is asserted.  Nothing here reads outside the repository or calls a live oracle."""
import numpy as np

import gi_cases as gc
import gi_ref
from global_racetrajectory_optimization_amd import engine
from ring_guard import dmax

CONTRACT = 1e-6          # north_star's fp64 tolerance
ON_BOUND = 1e-12         # |alpha - bound| below which a waypoint counts as on its bound (the engine pins active rows; decided cases keep the rest millimetres off)
INFO = ("gi_iters", "n_active_box", "n_active_kappa", "as_iters", "second_attempt", "ipm_iters")


def solve(eng, names, **kw):
    al, curv, st, info = eng.solve_batch([gc.problem(n) for n in names], **kw)
    return [dict(alpha=al[k], curv=float(curv[k]), status=int(st[k]), info=info[k]) for k in range(len(names))]


def box_sets(name, alpha):
    """(waypoints on lo, waypoints on hi) read off alpha."""
    c = gc.case(name)
    ref, w_veh = c["reftrack"], float(c["w_veh"])
    lo, hi = -(ref[:, 3] - w_veh / 2), ref[:, 2] - w_veh / 2
    return set(np.where(np.abs(alpha - lo) <= ON_BOUND)[0].tolist()), set(np.where(np.abs(alpha - hi) <= ON_BOUND)[0].tolist())


def expected_box_sets(name):
    codes = gc.case(name)["codes"]
    box = codes[((codes >> 1) & 1) == 0]
    return set((box[(box & 1) == 0] >> 2).tolist()), set((box[(box & 1) == 1] >> 2).tolist())


def check_result(name, r, worst):
    """One case's result against its stored trace."""
    c, i = gc.case(name), r["info"]
    sa = i["second_attempt"]
    print("%s: status %d, gi_iters %d (trace: %d adds + %d drops, %d steps), active box %d (%d) kappa %d (%d), as_iters %d, second_attempt %#x, "
          "ipm_iters %d" % (name, r["status"], i["gi_iters"], int(c["adds"]), int(c["drops"]), int(c["steps"]), i["n_active_box"], int(c["n_active_box"]),
                            i["n_active_kappa"], int(c["n_active_kappa"]), i["as_iters"], sa, i["ipm_iters"]))
    assert sa & 4, "the Goldfarb-Idnani path did not run"
    assert i["ipm_iters"] == 0
    if str(c["status"]) == "inconsistent":
        assert r["status"] == engine.STATUS_KAPPA_INFEASIBLE, r["status"]
        assert i["gi_iters"] == int(c["steps"])
        return
    assert r["status"] == 0, r["status"]
    assert int(c["steps"]) == int(c["adds"]) + int(c["drops"])
    assert i["gi_iters"] == int(c["adds"]) + int(c["drops"])
    assert i["n_active_box"] == int(c["n_active_box"]) and i["n_active_kappa"] == int(c["n_active_kappa"])
    on_lo, on_hi = box_sets(name, r["alpha"])
    want_lo, want_hi = expected_box_sets(name)
    assert on_lo == want_lo and on_hi == want_hi, (sorted(on_lo ^ want_lo), sorted(on_hi ^ want_hi))
    assert i["as_iters"] == 1, "the polish exchanged rows: gi_solve's vertex was not the vertex"
    assert not sa & 8, "the polish was rejected"
    d, g = dmax(r["alpha"], c["alpha"]), gc.guard(name)
    dc = abs(r["curv"] - float(c["curv_error"]))
    print("%s: |d alpha| %.2e (guard %.1e, contract %.0e), |d curv_error| %.2e" % (name, d, g, CONTRACT, dc))
    assert d < CONTRACT
    assert worst.add(name.split("/")[0], d, g) < g
    assert dc < 1e-9


def check_case(eng, name, worst):
    r = solve(eng, [name], algorithm=engine.ALG_GI)[0]
    check_result(name, r, worst)
    return r


def outgrows(name):
    c = gc.case(name)
    return int(c["q_max"]) > gi_ref.small_qcap(c["reftrack"].shape[0])


GROWN = tuple(n for n in gc.SPECS if n in gc.names() and outgrows(n) and str(gc.case(n)["status"]) == "ok")


def check_slot_edge(name):
    """The cases at qcap - 1, qcap, qcap + 1 sit where they claim, by the trace's largest working set."""
    c = gc.case(name)
    n = c["reftrack"].shape[0]
    qcap = gi_ref.small_qcap(n)
    print("%s: n %d, small slot %d constraints, largest working set %d" % (name, n, qcap, int(c["q_max"])))
    assert qcap < n and int(c["q_max"]) == qcap + gc.SLOT_EDGE[name]
    assert outgrows(name) == (gc.SLOT_EDGE[name] > 0)


def check_routes(eng, name, worst, grown=None):
    """The grown route (ALG_GI: a small slot, gi_grow on the way) against the route that starts in a FULL slot: the default algorithm with
    max_as_iter = 1, so that block pivoting ends after one round and hands over -- and with max_ipm_iter = 1, without which the interior point
    delivers the all-active rings' working set whole and that one round settles (nothing would be compared).  The same gi_solve from scratch,
    differing only in R's leading dimension and in where Q and R lie: the same steps and the same bits.  Returns whether the fallback ran."""
    assert outgrows(name)
    a = grown or solve(eng, [name], algorithm=engine.ALG_GI)[0]
    b = solve(eng, [name], max_as_iter=1, max_ipm_iter=1)[0]
    ran = bool(b["info"]["second_attempt"] & 4)
    same = np.array_equal(a["alpha"], b["alpha"])
    print("%s: full-slot route ran %s (second_attempt %#x), gi_iters grown %d / full %d, alpha bitwise %s (|d| %.2e)" % (
        name, ran, b["info"]["second_attempt"], a["info"]["gi_iters"], b["info"]["gi_iters"], same, dmax(a["alpha"], b["alpha"])))
    assert ran, "block pivoting settled in one round: nothing is compared"
    assert (b["info"]["second_attempt"] >> 4) == engine.STATUS_ITER_CAP and not b["info"]["second_attempt"] & 8
    if ran:
        assert b["status"] == 0 and a["status"] == 0
        assert a["info"]["gi_iters"] == b["info"]["gi_iters"]
        assert same
        assert b["info"]["n_active_box"] == a["info"]["n_active_box"] and b["info"]["n_active_kappa"] == a["info"]["n_active_kappa"]
    return ran


def check_ragged(eng, worst):
    """One launch of rings of 130, 300 and 5 waypoints (Q's column stride is the longest ring's): every member bitwise what it is alone."""
    batch = solve(eng, list(gc.RAGGED), algorithm=engine.ALG_GI)
    assert len(set(gc.case(n)["reftrack"].shape[0] for n in gc.RAGGED)) == len(gc.RAGGED)
    for name, r in zip(gc.RAGGED, batch):
        check_result(name, r, worst)
        alone = solve(eng, [name], algorithm=engine.ALG_GI)[0]
        print("%s: batch %s / alone %s" % (name, [r["info"][k] for k in INFO], [alone["info"][k] for k in INFO]))
        assert r["status"] == alone["status"]
        assert np.array_equal(r["alpha"], alone["alpha"]), dmax(r["alpha"], alone["alpha"])
        for k in INFO:
            assert r["info"][k] == alone["info"][k], k
    return batch
