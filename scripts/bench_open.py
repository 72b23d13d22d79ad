"""Open chains against rings at the headline size: 1024 problems of 2000 waypoints through mcq_solve_batch_ends (chains: the first 2000
waypoints of the config-3 generator's rings of 2400, end headings from their end chords) and through mcq_solve_batch (the rings of 2000
themselves), same engine, same host entry.  Prints one JSON line: wall time per launch and solves per second of each, their ratio, and
per problem the mean interior-point / active-set iterations, active box rows and device time of its workgroup (the two sets are different
problems: the work per waypoint is the same, the iteration counts need not be)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from global_racetrajectory_optimization_amd import engine, synthetic  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--n", type=int, default=2000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    B, n = a.batch, a.n
    rr, rn, rs = synthetic.oval_batch(B, n)
    rings = [dict(reftrack=rr[k], normvec=rn[k], scaling=rs[k], kappa_bound=0.12, w_veh=3.4) for k in range(B)]
    cr, cn, _ = synthetic.oval_batch(B, n + 400)
    cr, cn = np.ascontiguousarray(cr[:, :n]), np.ascontiguousarray(cn[:, :n])
    chains, ends = [], []
    for k in range(B):
        el = np.sqrt(np.sum(np.diff(cr[k, :, :2], axis=0) ** 2, axis=1))
        chains.append(dict(reftrack=cr[k], normvec=cn[k], scaling=np.concatenate((el[:-1] / el[1:], [1.0, 1.0])), kappa_bound=0.12, w_veh=3.4))
        d0, d1 = cr[k, 1, :2] - cr[k, 0, :2], cr[k, -1, :2] - cr[k, -2, :2]
        ends.append(dict(psi_s=float(np.arctan2(d0[1], d0[0]) - np.pi / 2), psi_e=float(np.arctan2(d1[1], d1[0]) - np.pi / 2)))
    eng = engine.Engine(0)
    res = {}
    for name, call in (("rings", lambda: eng.solve_batch(rings)), ("chains", lambda: eng.solve_batch(chains, ends=ends))):
        for _ in range(a.warmup):
            _, _, st, info = call()
        t = []
        for _ in range(a.steps):
            t0 = time.perf_counter()
            _, _, st, info = call()
            t.append(time.perf_counter() - t0)
        ms = 1e3 * float(np.median(t))
        res[name] = dict(ms_per_launch=ms, ms_min=1e3 * float(np.min(t)), ms_max=1e3 * float(np.max(t)), solves_per_s=B / (ms / 1e3),
                         status_ok=int(np.sum(st == 0)), mean_ipm_iters=float(np.mean([i["ipm_iters"] for i in info])),
                         mean_as_iters=float(np.mean([i["as_iters"] for i in info])),
                         mean_active_box=float(np.mean([i["n_active_box"] for i in info])),
                         kernel_ms_per_problem=float(np.mean([i["ticks"][3] for i in info])) / 1e5)
    res["chains_over_rings"] = res["chains"]["ms_per_launch"] / res["rings"]["ms_per_launch"]
    res.update(batch=B, n=n, steps=a.steps, warmup=a.warmup)
    print(json.dumps(res))
    eng.close()


if __name__ == "__main__":
    main()
