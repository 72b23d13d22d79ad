"""The minimum-time NLP's evaluation, Jacobian and certificate on the device, timed on the MI355X (GPU only: without one the engine cannot be created
and the script fails).

    berlin    one problem of N = 776 intervals (Berlin's recorded reference line; w from the engine's own minimum-curvature flow, tests/mintime_cases.py)
    sweep     1024 problems of N = 2000 intervals (seeded random track data and w inside tests/mintime_cases.py's ranges, the same problem tiled)

Every shape is warmed up, then timed as a span of its own between device events (mcq_timing_begin / mcq_timing_end): the launch repeated until the
span lasts about --window seconds.  Per kernel the bytes it must move (inputs read once, outputs written once) and the rate reached.  Beside them
the float64 numpy restatement on the same machine (tests/mintime_ref.py: g and the sums; the blocks by 33 dual passes) for ONE problem (host time).
No pass / fail threshold.  Prints one JSON line."""
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
    a = ap.parse_args()
    import mintime_cases as mc
    import mintime_ref as mr
    eng = engine.Engine(0)          # (EngineError without a device)
    z = np.load(os.path.join(ROOT, "tests", "golden", "berlin_2018.npz"))
    ref = z["reftrack"]
    berlin, _ = mc.flow_problem(eng, ref, mc.PARS, float(z["kappa_bound"]), float(z["w_veh"]), stepsize=2.0)
    res = dict(window_s=a.window, warmup=a.warmup, shapes=[])
    opts = eng.mintime_opts()
    for name, prob, batch in (("berlin", berlin, 1), ("sweep", mc.problem(a.intervals), a.batch)):
        N = prob["h"].shape[0]
        nw, ng = eng.mintime_sizes(N, opts)
        with eng.scope() as dev:
            one = {k: np.ascontiguousarray(prob[k], dtype=np.float64) for k in ("h", "kappa_cl", "w_tr_right_cl", "w_tr_left_cl", "w")}
            pars = np.array([prob["pars"][k] for k in engine.MINTIME_PARS])
            d = {k: dev.new(batch * v.nbytes) for k, v in one.items()}
            d_p = dev.new(batch * pars.nbytes)
            for b in range(batch):
                for k, v in one.items():
                    eng.upload(d[k], v, offset_bytes=b * v.nbytes)
                eng.upload(d_p, pars, offset_bytes=b * pars.nbytes)
            data = eng.mintime_data(batch, N, None, d["h"], d["kappa_cl"], d["w_tr_right_cl"], d["w_tr_left_cl"], d_p, d["w"])
            bw = [dev.new(batch * nw * 8) for _ in range(3)]
            bg = [dev.new(batch * ng * 8) for _ in range(2)]
            d_g, d_J, d_lap, d_st = dev.new(batch * ng * 8), dev.new(batch * 8), dev.new(batch * 8), dev.new(batch * 4)
            d_x, d_u, d_tf = dev.new(batch * (N + 1) * 40), dev.new(batch * N * 32), dev.new(batch * N * 96)
            d_dt, d_ax, d_ay, d_ec = (dev.new(batch * N * 8) for _ in range(4))
            d_blk, d_gJ, d_gE = dev.new(batch * N * 1089 * 8), dev.new(batch * nw * 8), dev.new(batch * nw * 8)
            d_lg, d_lx, d_r, d_k = dev.new(batch * ng * 8), dev.new(batch * nw * 8), dev.new(batch * nw * 8), dev.new(batch * 24)
            eng.mintime_bounds_device(data, opts, bw[0], bw[1], bw[2], bg[0], bg[1])
            eng.upload(d_lg, np.zeros(batch * ng))
            eng.upload(d_lx, np.zeros(batch * nw))
            inputs = batch * (nw + N + 3 * (N + 1)) * 8
            kernels = (("eval", lambda: eng.mintime_eval_device(data, opts, d_g, d_J, d_st, d_lap, None, d_x, d_u, d_tf, d_dt, d_ax, d_ay, d_ec),
                        inputs + batch * (ng + (N + 1) * 5 + N * (4 + 12 + 4)) * 8, "arithmetic (fp64 sin / cos / atan library code)"),
                       ("jac", lambda: eng.mintime_jac_device(data, opts, d_blk, d_gJ, d_gE), inputs + batch * (N * 1089 + 2 * nw) * 8,
                        "arithmetic at one wave per SIMD (its stores reach a fraction of the memory system's rate)"),
                       ("kkt", lambda: eng.mintime_kkt_device(data, opts, d_g, d_blk, d_gJ, None, d_lg, d_lx, bw[1], bw[2], bg[0], bg[1], d_r, d_k),
                        batch * (N * 1089 + 6 * nw + 4 * ng) * 8, "loads"))
            shape = dict(name=name, batch=batch, intervals=N, kernels=[])
            for kname, call, nbytes, bound in kernels:
                ms, reps, total = span(eng, call, a.window, a.warmup)
                shape["kernels"].append(dict(kernel=kname, ms_per_call=ms, calls_in_span=reps, span_ms=total, bytes_moved=nbytes,
                                             GB_per_s=nbytes / (ms * 1e-3) / 1e9, intervals_per_s=batch * N / (ms * 1e-3), bound_by=bound))
            assert not np.any(eng.download(d_st, batch, np.int32)) and np.all(np.isfinite(eng.download(d_k, (batch, 3), np.float64)))
            t0 = time.perf_counter()
            mr.nlp(prob, prob["w"], {}, np.float64)
            t1 = time.perf_counter()
            mr.blocks(prob, prob["w"], {}, np.float64)
            t2 = time.perf_counter()
            shape["host_one_problem"] = dict(numpy_eval_s=t1 - t0, numpy_blocks_s=t2 - t1)
            res["shapes"].append(shape)
    print(json.dumps(res))
    eng.close()


if __name__ == "__main__":
    main()
