"""
Generates tests/golden/gi_edges.npz: the committed table of the Goldfarb-Idnani edges suite (tests/gi_cases.py) -- data only.

Per case of gi_cases.SPECS: candidates gi_cases.build(name, seed), seed = 0, 1, ... (at most gi_cases.MAX_CANDIDATES), each through the dense
restatement tests/gi_ref.py under the engine's rule; the first one that REACHES the edges the case is there for and is DECIDED (gi_ref.decided)
is kept.  Stored: the inputs (reftrack, normvec, scaling, kappa_bound, w_veh), the reference's expectations (status, adds, drops, steps, q_max,
final codes, active box / curvature rows, every event, the edges the trace hits, its margins), the dense oracle's answer (oracle/gi_dense.c: alpha,
curv_error, its `iters` pair and iact) and the spread of that answer under four draws of ring_guard.perturbed (the guard's input), the seed and the
number of candidates tried.  A case no candidate satisfies is reported and left out; tests/test_gi_ref.py then names the edges nobody covers.

`python scripts/make_golden_gi_edges.py [case ...]` (no arguments: every case; with arguments: those cases are replaced in the existing file).
A quarter of an hour on one core, most of it the dense oracle on the large ring.  Never run by a test.
"""
import os

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ.setdefault(_v, "4")

import sys  # noqa: E402
import time  # noqa: E402

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import gi_cases  # noqa: E402
import gi_ref  # noqa: E402
import ring_guard  # noqa: E402
from oracle import qp_ref, tph_ref  # noqa: E402


def search(name):
    spec = gi_cases.SPECS[name]
    for seed in range(gi_cases.MAX_CANDIDATES):
        p = gi_cases.build(name, seed)
        P = gi_ref.problem_dense(p["reftrack"], p["normvec"], p["kappa_bound"], p["w_veh"])
        tr = gi_ref.solve(P["E"], P["k_ref"], P["lo"], P["hi"], p["kappa_bound"], rule="engine")
        hit = gi_ref.edges_hit(tr)
        missing = [e for e in spec["want"] if e not in hit]
        ok = gi_ref.decided(tr) and not missing
        print("  %s seed %d: %s adds %d drops %d q_max %d margins %s window %s missing %s -> %s" % (
            name, seed, tr.status, tr.adds, tr.drops, tr.q_max, {k: "%.1e" % v for k, v in tr.margins.items()}, tr.window, missing,
            "kept" if ok else "next"), flush=True)
        if ok:
            return seed, p, P, tr, hit
    return None


def record(name, seed, p, P, tr, hit):
    out = dict(p)
    n = tr.n
    info = {}
    if tr.status == "ok":
        x = qp_ref.solve_qp_gi(P["H"], P["f"], P["G"], P["h"], info)
        spread = 0.0
        for draw in range(ring_guard.SPREAD_DRAWS):
            Hp, fp = ring_guard.perturbed(P["H"], P["f"], ring_guard.draw_rng("gi_edges/" + name, "alpha", -1, draw))
            spread = max(spread, float(np.max(np.abs(qp_ref.solve_qp_gi(Hp, fp, P["G"], P["h"]) - x))))
        out.update(alpha=x, curv_error=tph_ref.curv_error(x, P["aux"]), dense_iters=np.asarray(info["iters"]),
                   dense_codes=np.sort([gi_ref.dense_code(int(j), n) for j in info["iact"]]), spread=spread,
                   ref_vs_dense=float(np.max(np.abs(tr.alpha - x))))
    else:
        out.update(alpha=np.full(n, np.nan), curv_error=np.nan, dense_iters=np.zeros(2, dtype=np.int32), dense_codes=np.zeros(0, dtype=np.int64),
                   spread=np.nan, ref_vs_dense=np.nan)
    out.update(status=tr.status, adds=tr.adds, drops=tr.drops, steps=tr.steps, q_max=tr.q_max, codes=tr.codes, n_active_box=tr.n_active_box,
               n_active_kappa=tr.n_active_kappa, events=tr.events.astype(np.int32), edges=np.array(hit), margin=gi_ref.min_margin(tr),
               margins=np.array([tr.margins[k] for k in ("violation", "t1_t2", "blocking", "dependence")]), seed=seed, candidates=seed + 1,
               ref_alpha=tr.alpha)
    return out


def main(argv):
    todo = argv or list(gi_cases.SPECS)
    table = {}
    if argv and os.path.exists(gi_cases.GOLDEN):
        z = np.load(gi_cases.GOLDEN)
        table = {k: z[k] for k in z.files if k.split("|")[0] not in todo}
    for name in todo:
        t0 = time.time()
        found = search(name)
        if found is None:
            print("%s: NO decided candidate that reaches %s among %d -- left out" % (name, gi_cases.SPECS[name]["want"], gi_cases.MAX_CANDIDATES))
            continue
        rec = record(name, *found)
        for k, v in rec.items():
            table["%s|%s" % (name, k)] = np.asarray(v)
        print("%s: seed %d, n %d, adds %d, drops %d, q_max %d, margin %.1e, spread %s, ref vs dense %s, edges %s  (%.0f s)" % (
            name, rec["seed"], found[3].n, rec["adds"], rec["drops"], rec["q_max"], rec["margin"], rec["spread"], rec["ref_vs_dense"],
            list(rec["edges"]), time.time() - t0), flush=True)
    np.savez_compressed(gi_cases.GOLDEN, **table)
    print("wrote %s: %d bytes" % (gi_cases.GOLDEN, os.path.getsize(gi_cases.GOLDEN)))


if __name__ == "__main__":
    main(sys.argv[1:])
