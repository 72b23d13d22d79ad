"""The Hessian of the minimum-time Lagrangian and H v on the device, timed on the MI355X beside the Jacobian and the certificate of the same run (GPU
only: without one the engine cannot be created and the script fails), at the shapes of scripts/bench_mintime_eval.py:

    berlin    one problem of N = 776 intervals (Berlin's recorded reference line; w from the engine's own minimum-curvature flow, tests/mintime_cases.py)
    sweep     1024 problems of N = 2000 intervals (seeded random track data and w inside tests/mintime_cases.py's ranges, the same problem tiled)

Every kernel is warmed up, then timed as a span of its own between device events (mcq_timing_begin / mcq_timing_end): the launch repeated until the
span lasts about --window seconds.  Per kernel the bytes it must move (inputs read once, outputs written once), the rate reached, and for the two
differentiating kernels the model evaluations per second (the Jacobian: 36 one-tangent evaluations per interval; the Hessian: 180 hyper-dual ones).
Beside them the float64 numpy restatement of the Hessian blocks (tests/mintime_hess_ref.py) for ONE problem (host time).  No pass / fail threshold.
Prints one JSON line."""
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
from global_racetrajectory_optimization_amd import engine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5, help="seconds a timed span should last")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--intervals", type=int, default=2000)
    ap.add_argument("--nvec", type=int, default=1)
    a = ap.parse_args()
    import mintime_cases as mc
    import mintime_hess_ref as hr
    eng = engine.Engine(0)          # (EngineError without a device)
    z = np.load(os.path.join(ROOT, "tests", "golden", "berlin_2018.npz"))
    berlin, _ = mc.flow_problem(eng, z["reftrack"], mc.PARS, float(z["kappa_bound"]), float(z["w_veh"]), stepsize=2.0)
    res = dict(window_s=a.window, warmup=a.warmup, nvec=a.nvec, shapes=[])
    opts = eng.mintime_opts()
    rng = np.random.default_rng(3)
    for name, prob, batch in (("berlin", berlin, 1), ("sweep", mc.problem(a.intervals), a.batch)):
        N = prob["h"].shape[0]
        nw, ng = eng.mintime_sizes(N, opts)
        lam, v = rng.uniform(-1.0, 1.0, ng), rng.uniform(-1.0, 1.0, a.nvec * nw)
        with eng.scope() as dev:
            one = {k: np.ascontiguousarray(prob[k], dtype=np.float64) for k in ("h", "kappa_cl", "w_tr_right_cl", "w_tr_left_cl", "w")}
            one.update(lam=lam, v=v)
            pars = np.array([prob["pars"][k] for k in engine.MINTIME_PARS])
            d = {k: dev.new(batch * x.nbytes) for k, x in one.items()}
            d_p = dev.new(batch * pars.nbytes)
            for b in range(batch):
                for k, x in one.items():
                    eng.upload(d[k], x, offset_bytes=b * x.nbytes)
                eng.upload(d_p, pars, offset_bytes=b * pars.nbytes)
            data = eng.mintime_data(batch, N, None, d["h"], d["kappa_cl"], d["w_tr_right_cl"], d["w_tr_left_cl"], d_p, d["w"])
            bw = [dev.new(batch * nw * 8) for _ in range(3)]
            bg = [dev.new(batch * ng * 8) for _ in range(2)]
            d_g, d_J, d_st = dev.new(batch * ng * 8), dev.new(batch * 8), dev.new(batch * 4)
            d_blk, d_gJ, d_gE = dev.new(batch * N * 1089 * 8), dev.new(batch * nw * 8), dev.new(batch * nw * 8)
            d_hb, d_y = dev.new(batch * N * 1089 * 8), dev.new(batch * a.nvec * nw * 8)
            d_lx, d_r, d_k = dev.new(batch * nw * 8), dev.new(batch * nw * 8), dev.new(batch * 24)
            eng.mintime_bounds_device(data, opts, bw[0], bw[1], bw[2], bg[0], bg[1])
            eng.mintime_eval_device(data, opts, d_g, d_J, d_st)
            eng.upload(d_lx, np.zeros(batch * nw))
            inputs = batch * (nw + N + 3 * (N + 1)) * 8
            kernels = (("jac", lambda: eng.mintime_jac_device(data, opts, d_blk, d_gJ, d_gE), inputs + batch * (N * 1089 + 2 * nw) * 8, 36),
                       ("kkt", lambda: eng.mintime_kkt_device(data, opts, d_g, d_blk, d_gJ, None, d["lam"], d_lx, bw[1], bw[2], bg[0], bg[1], d_r, d_k),
                        batch * (N * 1089 + 6 * nw + 4 * ng) * 8, 0),
                       ("hess", lambda: eng.mintime_hess_device(data, opts, d["lam"], None, d_hb), inputs + batch * (ng + N * 1089) * 8, 180),
                       ("hessvec", lambda: eng.mintime_hessvec_device(data, opts, d_hb, d["v"], a.nvec, d_y),
                        batch * (N * 1089 + 2 * a.nvec * nw) * 8, 0))
            shape = dict(name=name, batch=batch, intervals=N, kernels=[])
            for kname, call, nbytes, evals in kernels:
                ms, reps, total = span(eng, call, a.window, a.warmup)
                row = dict(kernel=kname, ms_per_call=ms, calls_in_span=reps, span_ms=total, bytes_moved=nbytes, GB_per_s=nbytes / (ms * 1e-3) / 1e9,
                           intervals_per_s=batch * N / (ms * 1e-3))
                if evals:
                    row.update(model_evaluations=batch * N * evals, ns_per_model_evaluation=ms * 1e6 / (batch * N * evals))
                shape["kernels"].append(row)
            y = eng.download(d_y, (batch, a.nvec, nw), np.float64)
            shape["outputs_finite"] = bool(np.all(np.isfinite(y)) and np.all(np.isfinite(eng.download(d_k, (batch, 3), np.float64))))
            t0 = time.perf_counter()
            hr.blocks(prob, prob["w"], {}, lam, 1.0, np.float64)
            shape["host_one_problem"] = dict(numpy_hess_blocks_s=time.perf_counter() - t0)
            res["shapes"].append(shape)
    print(json.dumps(res))
    eng.close()


if __name__ == "__main__":
    main()
