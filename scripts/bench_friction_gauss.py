"""The Gaussian-basis friction fit on the device, timed on the MI355X (GPU only: without one the engine cannot be created and the script fails).

    fit       mcq_friction_gauss_device with n_gauss = 5 on Berlin's recorded grids (tests/golden/friction/reference.npz: 777 rows of 10 .. 75
              positions, friction 0.81 .. 1.19), {1, 256} tracks resident on the device
    model     mcq_friction_model_device on the fitted weights at every row's own positions (both centre forms), 256 tracks

Every shape is warmed up, then timed as a span of its own between device events (mcq_timing_begin / mcq_timing_end): the launch repeated until the
span lasts about --window seconds.  Beside them the host loop on the same machine: sklearn's LinearRegression on the same features, four fits per
row in a Python loop as the reference runs it, for ONE track (host time; null where sklearn is not installed), and this project's float64
restatement (tests/fgauss_ref.py, numpy, a batch of rows at a time).  Prints one JSON line."""
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


def sklearn_loop(ns, mues, N):
    """Seconds of the reference's loop for one track with sklearn's own regression (features by tests/fgauss_ref.design), or None."""
    try:
        from sklearn.linear_model import LinearRegression
    except ImportError:
        return None
    import fgauss_ref as gr
    t0 = time.perf_counter()
    for n, m in zip(ns, mues):
        X = gr.design(n, N)
        for k in range(4):
            LinearRegression().fit(X, m[k][:, None])
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.6, help="seconds a timed span should last")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tracks", type=int, nargs="+", default=[1, 256])
    ap.add_argument("--n-gauss", type=int, default=5)
    a = ap.parse_args()
    import fgauss_guard as gg
    import fgauss_ref as gr
    import fric_guard as fg
    eng = engine.Engine(0)          # (EngineError without a device)
    g = fg.recorded("berlin_2018")
    ng, N = a.n_gauss, 2 * a.n_gauss + 1
    P = N + 1
    cnt = g["cnt"].astype(np.int32)
    rows, jmax = len(cnt), g["n"].shape[1]
    res = dict(track="berlin_2018", rows=rows, jmax=jmax, n_gauss=ng, problems_per_track=4 * rows, window_s=a.window, warmup=a.warmup, fit=[], model=[])
    for tracks in a.tracks:
        d_n, d_c, d_m = eng.alloc(tracks * rows * jmax * 8), eng.alloc(tracks * rows * 4), eng.alloc(tracks * 4 * rows * jmax * 8)
        for t in range(tracks):
            eng.upload(d_n, g["n"], offset_bytes=t * rows * jmax * 8)
            eng.upload(d_c, cnt, offset_bytes=t * rows * 4)
            eng.upload(d_m, g["mue4"], offset_bytes=t * 4 * rows * jmax * 8)
        d_st = eng.alloc(tracks * 4)            # (zeroed: MCQ_OK)
        d_w, d_cd, d_rk, d_sw = eng.alloc(tracks * 4 * rows * P * 8), eng.alloc(tracks * rows * 8), eng.alloc(tracks * rows * 4), eng.alloc(tracks * rows * 4)
        ms, reps, total = span(eng, lambda: eng.friction_gauss_device(tracks, rows - 1, jmax, d_n, d_c, d_m, d_st, ng, None, d_w, d_cd, d_rk, d_sw),
                               a.window, a.warmup)
        rk, sw = eng.download(d_rk, (tracks, rows), np.int32), eng.download(d_sw, (tracks, rows), np.int32)
        assert rk.min() >= 0 and np.array_equal(rk[0], rk[-1])
        res["fit"].append(dict(tracks=tracks, ms_per_call=ms, calls_in_span=reps, span_ms=total, fits_per_s=4 * rows * tracks / (ms * 1e-3),
                               sweeps_max=int(sw.max()), ranks={int(k): int(v) for k, v in zip(*np.unique(rk[0], return_counts=True))}))
        if tracks == max(a.tracks):
            d_q, d_out = eng.alloc(tracks * rows * jmax * 8), eng.alloc(tracks * 4 * rows * jmax * 8)
            for t in range(tracks):
                eng.upload(d_q, np.where(np.isnan(g["n"]), 0.0, g["n"]), offset_bytes=t * rows * jmax * 8)
            for name, kw in (("gauss, the fit's centres", dict(model=engine.FRIC_GAUSS, centres=engine.FRIC_CENTRES_FIT)),
                             ("gauss, the consumer's centres", dict(model=engine.FRIC_GAUSS, centres=engine.FRIC_CENTRES_MINTIME))):
                ms, reps, total = span(eng, lambda: eng.friction_model_device(tracks, rows - 1, jmax, d_q, d_c, kw["model"], d_w, d_out, ng, kw["centres"],
                                                                              d_cd, d_n, d_c, jmax), a.window, a.warmup)
                evals = 4 * int(cnt.sum()) * tracks
                res["model"].append(dict(form=name, tracks=tracks, evaluations=evals, ms_per_call=ms, calls_in_span=reps, span_ms=total,
                                         evaluations_per_s=evals / (ms * 1e-3)))
            assert np.all(np.isfinite(eng.download(d_out, (4, rows, jmax), np.float64)[:, 0, :cnt[0]]))
            eng.free(d_q)
            eng.free(d_out)
        for p in (d_n, d_c, d_m, d_st, d_w, d_cd, d_rk, d_sw):
            eng.free(p)
    ns, mues = gg.track_rows("berlin_2018")
    t0 = time.perf_counter()
    gr.fit_rows(ns, mues, ng)
    t1 = time.perf_counter()
    res["host"] = dict(tracks=1, numpy_restatement_s=t1 - t0, sklearn_loop_s=sklearn_loop(ns, mues, N))
    print(json.dumps(res))
    eng.close()


if __name__ == "__main__":
    main()
