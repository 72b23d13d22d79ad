"""The regularised primal-dual Newton step of the minimum-time problem on the device (mcq_mintime_step_device), timed on the MI355X beside the
Jacobian and the Hessian of the same run (GPU only: without one the engine cannot be created and the script fails), at the shapes of
scripts/bench_mintime_hess.py:

    berlin    one problem of N = 776 intervals (Berlin's recorded reference line; w from the engine's own minimum-curvature flow)
    sweep     a batch of problems of N = 2000 intervals (seeded random track data and w, the same problem tiled): the largest of 1024 / 256 whose
              blocks and workspace (mcq_mintime_step_bytes) fit in --memory-gb

nvec = 1, refine = 2.  The diagonals make K quasi-definite: dw = the largest absolute row sum of H (Gershgorin) + 1e-3, dg = 1e-6 on equality rows
and 1 on inequality rows.  Every kernel is warmed up, then timed as a span of its own between device events (mcq_timing_begin / mcq_timing_end): the
launch repeated until the span lasts about --window seconds.  For the step: microseconds per interval, the bytes it must move (blocks read by the
factorisation, by the check and by each of the three residuals; the factor written once and read by six sweeps) and the rate.  Beside it
scipy.sparse.linalg.splu of mintime.kkt_matrix and one solve for ONE problem (host time).  No pass / fail threshold.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_friction import span  # noqa: E402
from global_racetrajectory_optimization_amd import engine, mintime  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5, help="seconds a timed span should last")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--intervals", type=int, default=2000)
    ap.add_argument("--memory-gb", type=float, default=200.0, help="device memory the sweep may take")
    ap.add_argument("--refine", type=int, default=2)
    a = ap.parse_args()
    import mintime_cases as mc
    import mintime_ref as mr
    import scipy.sparse.linalg as sla
    eng = engine.Engine(0)          # (EngineError without a device)
    z = np.load(os.path.join(ROOT, "tests", "golden", "berlin_2018.npz"))
    berlin, _ = mc.flow_problem(eng, z["reftrack"], mc.PARS, float(z["kappa_bound"]), float(z["w_veh"]), stepsize=2.0)
    res = dict(window_s=a.window, warmup=a.warmup, nvec=1, refine=a.refine, shapes=[])
    opts = eng.mintime_opts()
    rng = np.random.default_rng(4)
    for name, prob in (("berlin", berlin), ("sweep", mc.problem(a.intervals))):
        N = prob["h"].shape[0]
        nw, ng = eng.mintime_sizes(N, opts)
        per_problem = eng.mintime_step_bytes(N, 1) + (2 * N * 1089 + 6 * (nw + ng)) * 8
        batch = 1 if name == "berlin" else next((b for b in (1024, 256) if b * per_problem <= a.memory_gb * 1e9), 0)
        if batch == 0:
            raise SystemExit("the sweep does not fit in --memory-gb")
        lam = rng.uniform(-1.0, 1.0, ng)
        # one problem through the chained call: its blocks for the diagonals and for the host's sparse factorisation
        first = eng.mintime_step_batch([prob], [lam], [np.ones(nw)], [np.ones(ng)], [np.zeros((1, nw + ng))], refine=0)
        H = mintime.hessian_coo(first["hblocks"][0], N).tocsr()
        dw = np.full(nw, float(np.max(abs(H).sum(axis=1))) + 1e-3)
        _, _, _, lbg, ubg = mr.bounds(prob, {})
        dg = np.where(lbg == ubg, 1e-6, 1.0)
        rhs = rng.uniform(-1.0, 1.0, nw + ng)
        with eng.scope() as dev:
            one = {k: np.ascontiguousarray(prob[k], dtype=np.float64) for k in ("h", "kappa_cl", "w_tr_right_cl", "w_tr_left_cl", "w")}
            one.update(lam=lam, dw=dw, dg=dg, rhs=rhs)
            pars = np.array([prob["pars"][k] for k in engine.MINTIME_PARS])
            d = {k: dev.new(batch * x.nbytes) for k, x in one.items()}
            d_p = dev.new(batch * pars.nbytes)
            for b in range(batch):
                for k, x in one.items():
                    eng.upload(d[k], x, offset_bytes=b * x.nbytes)
                eng.upload(d_p, pars, offset_bytes=b * pars.nbytes)
            data = eng.mintime_data(batch, N, None, d["h"], d["kappa_cl"], d["w_tr_right_cl"], d["w_tr_left_cl"], d_p, d["w"])
            d_blk, d_gJ, d_gE = dev.new(batch * N * 1089 * 8), dev.new(batch * nw * 8), dev.new(batch * nw * 8)
            d_hb = dev.new(batch * N * 1089 * 8)
            d_sol, d_res, d_in, d_st = dev.new(batch * (nw + ng) * 8), dev.new(batch * 8), dev.new(batch * 12), dev.new(batch * 4)
            inputs = batch * (nw + N + 3 * (N + 1)) * 8
            blocks_b, factor_b, vec_b = batch * 2 * N * 1089 * 8, batch * (N * 94 * 57 + 37 * 37) * 8, batch * (nw + ng) * 8
            sweeps = 2 * (a.refine + 1)
            step_bytes = blocks_b * (2 + a.refine + 1) + factor_b * (1 + sweeps) + vec_b * (4 * (a.refine + 1) + 4)
            kernels = (("jac", lambda: eng.mintime_jac_device(data, opts, d_blk, d_gJ, d_gE), inputs + batch * (N * 1089 + 2 * nw) * 8),
                       ("hess", lambda: eng.mintime_hess_device(data, opts, d["lam"], None, d_hb), inputs + batch * (ng + N * 1089) * 8),
                       ("step", lambda: eng.mintime_step_device(data, opts, d_hb, d_blk, None, d["dw"], d["dg"], d["rhs"], 1, a.refine, d_sol, d_res,
                                                                d_in, d_st), step_bytes))
            shape = dict(name=name, batch=batch, intervals=N, workspace_bytes_per_problem=eng.mintime_step_bytes(N, 1), kernels=[])
            for kname, call, nbytes in kernels:
                ms, reps, total = span(eng, call, a.window, a.warmup)
                shape["kernels"].append(dict(kernel=kname, ms_per_call=ms, calls_in_span=reps, span_ms=total, bytes_moved=nbytes,
                                             GB_per_s=nbytes / (ms * 1e-3) / 1e9, us_per_interval=ms * 1e3 / N,
                                             intervals_per_s=batch * N / (ms * 1e-3)))
            st, inertia = eng.download(d_st, (batch,), np.int32), eng.download(d_in, (batch, 3), np.int32)
            resid = eng.download(d_res, (batch,), np.float64)
            shape.update(status_ok=bool(np.all(st == 0)), inertia=inertia[0].tolist(), quasi_definite=bool(np.all(inertia == [nw, ng, 0])),
                         res_max=float(np.max(resid)))
            K = mintime.kkt_matrix(first["hblocks"][0], first["blocks"][0], N, dw, dg)
            t0 = time.perf_counter()
            lu = sla.splu(K)
            t1 = time.perf_counter()
            x = lu.solve(rhs)
            t2 = time.perf_counter()
            got = eng.download(d_sol, (batch, nw + ng), np.float64)[0]
            shape["host_one_problem"] = dict(splu_s=t1 - t0, solve_s=t2 - t1, max_abs_difference_from_device=float(np.max(np.abs(x - got))),
                                             max_abs_solution=float(np.max(np.abs(got))))
            res["shapes"].append(shape)
    print(json.dumps(res))
    eng.close()


if __name__ == "__main__":
    main()
