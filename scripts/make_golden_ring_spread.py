"""
Generates tests/golden/ring_spread.npz and tests/golden/SUMMARY_ring_spread.json: how far every closed-ring (ring) oracle answer in
tests/golden/ is determined, from which tests/ring_guard.py derives the tight guard max(1e-8, 4 x spread) the GPU ring tests hold on top of
the 1e-6 m contract.

Per entry (a fixture, the golden key compared, a problem index for kappa_tight_fuzz.npz):
  perturb_spread  the largest |delta| against the stored golden value over four draws of a relative 1e-15 perturbation of H (symmetrised)
                  and f (ring_guard.perturbed, the constants of scripts/make_golden_open_edges.py), re-solved by the dense GI of
                  oracle.qp_ref.solve_qp_gi.  Minimum-curvature fixtures are assembled by oracle.tph_ref.opt_min_curv, shortest-path ones
                  by tph_ref.shortest_path_dense; the IQP chains (iqp_alpha / iqp_reftrack, harness iqp_oracle_*) re-run
                  tph_ref.iqp_handler with every pass's H and f perturbed and record the end state's alpha and reftrack.
  route_gap       every inter-route difference already on record for the entry: tests/golden/CHECK_r6.json (the previous oracle against
                  the qpgen2 rewrite: d_alpha, d_reftrack; kappa_tight_fuzz's worst_d_alpha for its worst problem) and SUMMARY*.json's
                  second_route_max_diff / bvls_max_diff.
  spread          max(perturb_spread, route_gap).

Deterministic: each draw is seeded by its entry and draw index alone (ring_guard.draw_rng) and runs with single-threaded BLAS, so the
pool's order does not matter.  Tens of CPU-minutes (a dense GI solve at N >= 2000 takes 25-55 s, the N = 2000 IQP chain about 220 s):
`python scripts/make_golden_ring_spread.py [workers [output directory]]`.  Never run by a test.
"""
import os

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[_v] = "1"              # bitwise-reproducible BLAS: one thread in every worker

import json  # noqa: E402
import math  # noqa: E402
import multiprocessing  # noqa: E402
import sys  # noqa: E402
import time  # noqa: E402

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ring_guard  # noqa: E402
from global_racetrajectory_optimization_amd.trajectory_planning_helpers import calc_splines as cs  # noqa: E402
from oracle import qp_ref, tph_ref  # noqa: E402

GOLD = ring_guard.GOLDEN_DIR
CHAIN_BASE = {"berlin_2018_iqp": "berlin_2018", "modena_2019_iqp": "modena_2019"}      # IQP chain fixture -> the file with its input
KAPPA_BOUND, W_VEH, STEP, ITERS_MIN, CURV_ALLOWED = 0.12, 3.4, 3.0, 3, 0.01


def load(name):
    z = np.load(os.path.join(GOLD, name + ".npz"))
    return {k: z[k] for k in z.files}


def les_matrix(ref, unit):
    """A of calc_splines on the closed reference line (distance scaling unless unit), as scripts/check_goldens_r6.py builds it."""
    return tph_ref.calc_splines(np.vstack((ref[:, :2], ref[0, :2])), use_dist_scaling=not unit)[2]


def maxdiff(a, b):
    """(a None: the perturbed QP turned "inconsistent", or a chain changed its length -- the entry is not determined at all)"""
    if a is None or np.shape(a) != np.shape(b):
        return math.inf
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))))


def inconsistent_as_none(fn):
    def wrapped(*args):
        try:
            return fn(*args)
        except ValueError as e:
            assert "inconsistent" in str(e), e
            return None
    return wrapped


@inconsistent_as_none
def mincurv_draw(ref, nv, A, kb, wv, rng):
    return tph_ref.opt_min_curv(ref, nv, A, kb, wv, solver=ring_guard.perturbed_solver(rng))[0]


def shortest_draw(ref, nv, wv, rng):
    H, f, G, h = tph_ref.shortest_path_dense(ref, nv, wv)
    Hp, fp = ring_guard.perturbed(H, f, rng)
    return qp_ref.solve_qp_gi(Hp, fp, G, h)


def chain_draw(ref, nv, A, kb, wv, step, iters_min, allowed, rng):
    try:
        a, rt, _ = tph_ref.iqp_handler(ref, nv, A, kb, wv, step, iters_min=iters_min, curv_error_allowed=allowed,
                                       solver=ring_guard.perturbed_solver(rng))
    except ValueError as e:
        assert "inconsistent" in str(e), e
        return None, None
    return a, rt


def job(spec):
    """One draw of one entry (or of every entry sharing its solve).  spec: (kind, name, k, draw) -> [((name, what, k), |delta|), ...]."""
    kind, name, k, draw = spec
    t0 = time.perf_counter()
    if kind == "mincurv":
        g = load(name)
        rng = ring_guard.draw_rng(name, "alpha", k, draw)
        a = mincurv_draw(g["reftrack"], g["normvec"], les_matrix(g["reftrack"], name in ring_guard.UNIT_SCALING),
                         float(g["kappa_bound"]), float(g["w_veh"]), rng)
        out = [((name, "alpha", k), maxdiff(a, g["alpha"]))]
    elif kind == "fuzz":
        z = load("kappa_tight_fuzz")
        r = slice(int(z["offsets"][k]), int(z["offsets"][k + 1]))
        ref, nv = z["reftrack"][r], z["normvec"][r]
        rng = ring_guard.draw_rng(name, "alpha", k, draw)
        a = mincurv_draw(ref, nv, les_matrix(ref, False), float(z["kappa_bound"][k]), float(z["w_veh"][k]), rng)
        out = [((name, "alpha", k), maxdiff(a, z["alpha"][r]))]
    elif kind == "chain":
        g = load(name)
        b = load(CHAIN_BASE.get(name, name))
        rng = ring_guard.draw_rng(name, "iqp_alpha", k, draw)
        a, rt = chain_draw(b["reftrack"], b["normvec"], les_matrix(b["reftrack"], False), KAPPA_BOUND, W_VEH, STEP, ITERS_MIN,
                           CURV_ALLOWED, rng)
        out = [((name, "iqp_alpha", k), maxdiff(a, g["iqp_alpha"])), ((name, "iqp_reftrack", k), maxdiff(rt, g["iqp_reftrack"]))]
    elif kind == "shortest":
        if name == "shortest_path_n2100":
            g = load(name)
            ref, nv, wv, want, what = g["reftrack"], g["normvec"], float(g["w_veh"]), g["alpha"], "alpha"
        else:
            z, b = load("shortest_path"), load(k)
            ref, nv, wv, want, what = b["reftrack"], b["normvec"], float(z["w_veh"]), z[k + "_alpha"], k + "_alpha"
        rng = ring_guard.draw_rng(name, what, -1, draw)
        out = [((name, what, -1), maxdiff(shortest_draw(ref, nv, wv, rng), want))]
    else:                                   # harness_calls_berlin: the oracle outputs of the recorded calls
        z = load("harness_calls_berlin")
        call = k
        ref, nv = z[call + "_reftrack"], z[call + "_normvectors"]
        kw = json.loads(str(z[call + "_kwargs"]))
        if call != "shortest":
            A = les_matrix(ref, False)
            assert np.max(np.abs(cs.scalings_from_les_matrix(A) - z[call + "_A_scalings"])) < 1e-13, call
        if call == "iqp":
            rng = ring_guard.draw_rng(name, "iqp_oracle_alpha", -1, draw)
            a, rt = chain_draw(ref, nv, A, kw["kappa_bound"], kw["w_veh"], kw["stepsize_interp"], kw["iters_min"],
                               kw["curv_error_allowed"], rng)
            out = [((name, "iqp_oracle_alpha", -1), maxdiff(a, z["iqp_oracle_alpha"])),
                   ((name, "iqp_oracle_reftrack", -1), maxdiff(rt, z["iqp_oracle_reftrack"]))]
        elif call == "shortest":
            rng = ring_guard.draw_rng(name, "shortest_oracle_alpha", -1, draw)
            out = [((name, "shortest_oracle_alpha", -1), maxdiff(shortest_draw(ref, nv, kw["w_veh"], rng), z["shortest_oracle_alpha"]))]
        else:
            what = call + "_oracle_alpha"
            rng = ring_guard.draw_rng(name, what, -1, draw)
            out = [((name, what, -1), maxdiff(mincurv_draw(ref, nv, A, kw["kappa_bound"], kw["w_veh"], rng), z[what]))]
    print("%-9s %-22s %-8s draw %d  %s  %.1f s" % (kind, name, k, draw, " ".join("%.1e" % d for _, d in out), time.perf_counter() - t0),
          flush=True)
    return out


def route_gaps():
    """(name, what, k) -> the largest inter-route difference on record."""
    gaps = {}

    def put(key, v):
        if v is not None and np.isfinite(v):
            gaps[key] = max(gaps.get(key, 0.0), float(v))

    chk = json.load(open(os.path.join(GOLD, "CHECK_r6.json")))
    for name in ring_guard.FIRST_PASS + ring_guard.UNIT_SCALING:
        put((name, "alpha", -1), chk[name]["d_alpha"])
    for fix in ring_guard.IQP_CHAINS:
        rec = chk["iqp_chain_" + CHAIN_BASE.get(fix, fix)]
        put((fix, "iqp_alpha", -1), rec.get("d_alpha"))
        put((fix, "iqp_reftrack", -1), rec.get("d_reftrack"))
    sp = chk["shortest_path"]
    for t in ring_guard.SHORTEST:
        put(("shortest_path", t + "_alpha", -1), sp[t])
    put(("shortest_path_n2100", "alpha", -1), sp["n2100"])
    kf = chk["kappa_tight_fuzz"]
    put(("kappa_tight_fuzz", "alpha", int(kf["worst_problem"])), kf["worst_d_alpha"])
    for fname in ("SUMMARY.json", "SUMMARY_r3.json"):
        for name, rec in json.load(open(os.path.join(GOLD, fname))).items():
            if isinstance(rec, dict):
                for key in ("second_route_max_diff", "bvls_max_diff"):
                    put((name, "alpha", -1), rec.get(key))
    put(("oval_n2000", "alpha", -1), json.load(open(os.path.join(GOLD, "SUMMARY_n2000.json")))["second_route_max_diff"])
    for t, rec in json.load(open(os.path.join(GOLD, "SUMMARY_shortest_path.json"))).items():
        put(("shortest_path", t + "_alpha", -1), rec.get("bvls_max_diff"))
    return gaps


def main(argv):
    workers = int(argv[0]) if argv else min(8, os.cpu_count() or 1)
    out = argv[1] if len(argv) > 1 else GOLD           # (another directory: to check that a rerun reproduces the committed files)
    fuzz = load("kappa_tight_fuzz")
    specs = [("mincurv", n, -1) for n in ring_guard.FIRST_PASS + ring_guard.UNIT_SCALING]
    specs += [("chain", n, -1) for n in ring_guard.IQP_CHAINS]
    specs += [("fuzz", "kappa_tight_fuzz", k) for k in range(len(fuzz["status_ref"])) if int(fuzz["status_ref"][k]) == 0]
    specs += [("shortest", "shortest_path", t) for t in ring_guard.SHORTEST] + [("shortest", "shortest_path_n2100", -1)]
    specs += [("harness", "harness_calls_berlin", c) for c in ("mincurv", "iqp", "shortest", "reopt")]
    jobs = [s + (d,) for s in specs for d in range(ring_guard.SPREAD_DRAWS)]

    def cost(s):                                # the largest first: chains, then by size
        kind, name, k, _ = s
        if kind == "chain":
            return 1e9 if name == "oval_n2000" else 3e6
        if kind == "harness" and k == "iqp":
            return 3e6
        if kind == "mincurv":
            return load(name)["alpha"].shape[0] ** 2
        return 0
    jobs.sort(key=lambda s: -cost(s))
    t0 = time.perf_counter()
    with multiprocessing.get_context("fork").Pool(workers) as pool:
        res = pool.map(job, jobs, chunksize=1)
    perturb = {}
    for rec in res:
        for key, d in rec:
            perturb[key] = max(perturb.get(key, 0.0), d)
    want = ring_guard.expected_entries()
    missing = [e for e in want if e not in perturb]
    extra = [e for e in perturb if e not in set(want)]
    assert not missing and not extra, (missing, extra)
    gaps = route_gaps()
    assert set(gaps) <= set(want), set(gaps) - set(want)
    pspread = np.array([perturb[e] for e in want])
    gap = np.array([gaps.get(e, 0.0) for e in want])
    spread = np.maximum(pspread, gap)
    np.savez_compressed(os.path.join(out, "ring_spread.npz"), name=np.array([e[0] for e in want]), what=np.array([e[1] for e in want]),
                        k=np.array([e[2] for e in want], dtype=np.int32), perturb_spread=pspread, route_gap=gap, spread=spread)
    summary = dict(rule="guard = max(1e-8, 4 x spread); spread = max(perturb_spread, route_gap)", draws=ring_guard.SPREAD_DRAWS,
                   relative_perturbation=ring_guard.SPREAD_REL,
                   entries={"%s/%s%s" % (n, w, "" if k < 0 else "/%d" % k): dict(perturb_spread=float(p), route_gap=float(r), spread=float(s))
                            for (n, w, k), p, r, s in zip(want, pspread, gap, spread) if n != "kappa_tight_fuzz"},
                   kappa_tight_fuzz=dict(problems=int(sum(1 for e in want if e[0] == "kappa_tight_fuzz")),
                                         max_spread=float(max(s for e, s in zip(want, spread) if e[0] == "kappa_tight_fuzz")),
                                         median_spread=float(np.median([s for e, s in zip(want, spread) if e[0] == "kappa_tight_fuzz"]))))
    with open(os.path.join(out, "SUMMARY_ring_spread.json"), "w") as fh:
        json.dump(summary, fh, indent=1, sort_keys=True)
    print("done in %.0f s; largest spread %.2e (%s)" % (time.perf_counter() - t0, float(spread.max()), want[int(np.argmax(spread))]))


if __name__ == "__main__":
    main(sys.argv[1:])
