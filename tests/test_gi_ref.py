"""Pins the dense restatement of the Goldfarb-Idnani path (tests/gi_ref.py) and the committed case table (tests/gi_cases.py,
tests/golden/gi_edges.npz) on the CPU, without the engine:

  * under qpgen2's rule the restatement reproduces oracle/gi_dense.c on every case -- its `iters` pair, its final iact as a set, its x to 1e-9 m
    (and its "constraints are inconsistent") --, and on every box-only case it takes the stored trace of the engine's rule event for event;
  * under the engine's rule it reproduces the stored trace, the stored edges and the stored margins (cases of up to 520 waypoints: the large ring
    is covered by the line above), and takes the number of steps tests/golden/CHECK_r6.json records for the two small reference tracks;
  * every edge of gi_ref.EDGES is reached by the stored trace of at least one case, every case reaches the edges it is there for, every case is
    decided.  A case that stops reaching its edge fails here, not silently on the GPU.

Left out (docs/NOTEBOOK.md, the Goldfarb-Idnani edges section): gi_ref.SHARPEST -- 121 ... 128 curvature rows in a small slot that never grew."""
import json
import os

import numpy as np
import pytest

import gi_cases as gc
import gi_ref
from oracle import qp_ref

NAMES = gc.names()


@pytest.fixture(scope="module")
def dense():
    cache = {}

    def get(name):
        if name not in cache:
            p = gc.problem(name)
            cache[name] = gi_ref.problem_dense(p["reftrack"], p["normvec"], p["kappa_bound"], p["w_veh"])
        return cache[name]
    return get


def test_the_table_is_complete():
    assert set(NAMES) == set(gc.SPECS), sorted(set(gc.SPECS) - set(NAMES))
    for name in NAMES:
        c = gc.case(name)
        assert int(c["candidates"]) <= gc.MAX_CANDIDATES
        assert all(v.nbytes < (1 << 20) for v in c.values())
    assert os.path.getsize(gc.GOLDEN) < (1 << 20)


def test_every_listed_edge_is_covered():
    covered = {e: [n for n in NAMES if e in gc.edges(n)] for e in gi_ref.EDGES}
    print("\n".join("%-34s %s" % (e, ", ".join(ns)) for e, ns in covered.items()))
    assert not [e for e, ns in covered.items() if not ns]
    for name in NAMES:
        assert set(gc.SPECS[name]["want"]) <= set(gc.edges(name)), name
    assert gi_ref.SHARPEST not in gi_ref.EDGES and not any(gi_ref.SHARPEST in gc.edges(n) for n in NAMES)
    # the ragged batch: Q's column stride (the longest ring) differs from the length of two of its rings
    ns = [gc.case(n)["reftrack"].shape[0] for n in gc.RAGGED]
    assert sorted(ns) == [5, 130, 300]
    for name, d in gc.SLOT_EDGE.items():
        n = gc.case(name)["reftrack"].shape[0]
        assert gi_ref.small_qcap(n) < n and int(gc.case(name)["q_max"]) == gi_ref.small_qcap(n) + d
    # partially active cases exist, so the guard compares something
    assert sum(1 for n in NAMES if 0 < int(gc.case(n)["q_max"]) < gc.case(n)["reftrack"].shape[0] // 4) >= 2


@pytest.mark.parametrize("name", NAMES)
def test_case_is_decided(name):
    c = gc.case(name)
    print(name, dict(zip(("violation", "t1_t2", "blocking", "dependence"), c["margins"])))
    assert float(c["margin"]) >= gi_ref.DECIDED and float(np.min(c["margins"])) == float(c["margin"])
    if str(c["status"]) == "ok":
        assert float(c["ref_vs_dense"]) < 1e-9 and 0.0 < float(c["spread"]) < 1e-7          # (every case has its spread: tests/test_ring_guard.py relies on it)
        assert gc.guard(name) == max(1e-8, 4.0 * float(c["spread"]))


@pytest.mark.parametrize("name", NAMES)
def test_qpgen2_rule_reproduces_the_dense_oracle(dense, name):
    c, P = gc.case(name), dense(name)
    kb = float(c["kappa_bound"])
    tr = gi_ref.solve(P["E"], P["k_ref"], P["lo"], P["hi"], kb, rule="qpgen2")
    if str(c["status"]) == "inconsistent":
        with pytest.raises(ValueError, match="inconsistent"):
            qp_ref.solve_qp_gi(P["H"], P["f"], P["G"], P["h"])
        assert tr.status == "inconsistent" and tr.q_final > 0
        return
    info = {}
    x = qp_ref.solve_qp_gi(P["H"], P["f"], P["G"], P["h"], info)
    n = x.shape[0]
    assert tr.status == "ok"
    assert (tr.adds + 1, tr.drops) == tuple(int(v) for v in info["iters"])
    assert sorted(gi_ref.dense_code(int(j), n) for j in info["iact"]) == tr.codes.tolist()
    assert np.max(np.abs(tr.alpha - x)) < 1e-9
    assert np.max(np.abs(x - c["alpha"])) < gc.guard(name)          # the stored answer is this oracle's (another BLAS, another thread count: its spread)
    if kb == gc.KB_OFF:
        # box-only: both rules divide every violation by the same number -- the same trace
        assert np.array_equal(tr.events, c["events"])


@pytest.mark.parametrize("name", [n for n in NAMES if gc.SPECS[n]["n"] <= 520])
def test_engine_rule_reproduces_the_stored_trace(dense, name):
    c, P = gc.case(name), dense(name)
    tr = gi_ref.solve(P["E"], P["k_ref"], P["lo"], P["hi"], float(c["kappa_bound"]), rule="engine")
    assert tr.status == str(c["status"]) and np.array_equal(tr.events, c["events"])
    assert (tr.adds, tr.drops, tr.steps, tr.q_max) == tuple(int(c[k]) for k in ("adds", "drops", "steps", "q_max"))
    assert np.array_equal(tr.codes, c["codes"]) and gi_ref.edges_hit(tr) == list(gc.edges(name))
    assert gi_ref.decided(tr)
    if tr.status == "ok":
        assert np.max(np.abs(tr.alpha - c["ref_alpha"])) < 1e-11


@pytest.mark.parametrize("track", ["rounded_rectangle", "handling_track"])
def test_engine_rule_takes_the_steps_the_goldens_record(golden, track):
    """tests/golden/CHECK_r6.json holds the dense oracle's `iters` pair of the reference's tracks (qpgen2's: main iterations = adds + 1, drops;
    SUMMARY.json's older pair is the earlier oracle variant's, which counted otherwise): the steps tests/test_emu_gi.py holds the engine to."""
    with open(os.path.join(os.path.dirname(gc.GOLDEN), "CHECK_r6.json")) as fh:
        it = json.load(fh)[track]["iters"]
    g = golden[track]
    P = gi_ref.problem_dense(g["reftrack"], g["normvec"], float(g["kappa_bound"]), float(g["w_veh"]))
    tr = gi_ref.solve(P["E"], P["k_ref"], P["lo"], P["hi"], float(g["kappa_bound"]), rule="engine")
    assert tr.status == "ok" and tr.steps == it[0] - 1 + it[1] and (tr.adds + 1, tr.drops) == tuple(it)
    assert np.max(np.abs(tr.alpha - g["alpha"])) < 1e-9
