"""Friction maps on the device, timed on the MI355X (GPU only: without one the engine cannot be created and the script fails).

    query     mcq_fmap_query_device on Berlin's map (tests/golden/friction/reference.npz, varmue08-12): the 74 228 wheel positions of Berlin's own
              extraction with the ini's defaults, x {1, 256, 1024} (every copy shifted by a seeded offset below 0.25 m)
    grid      mcq_friction_grid_device (positions, lookups, lines) on {1, 256} Berlin tracks
    chain     mcq_raceline_device -> mcq_fmap_query_device on its resident xy -> mcq_vel_profile_device_opts(mu = that result) for 1024 racelines of
              about 3003 stations (Berlin's reference line shifted by 1024 scalings of the golden alpha), nothing leaving the device

Every shape is warmed up, then timed as a span of its own between device events (mcq_timing_begin / mcq_timing_end): the launch repeated until the
span lasts about --window seconds.  Reported per shape: milliseconds per call, queries per second, and the bytes the entry must move (queries in,
results out) over its time -- a byte count computed from the shapes, not a measured traffic.  Beside them the host loop: this project's own numpy +
cKDTree restatement of the reference's loop over waypoints and lateral positions (tests/fric_ref.py's rows, scipy's tree, numpy.polyfit) for ONE
Berlin track, host time.  Prints one JSON line."""
import argparse
import ctypes
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from global_racetrajectory_optimization_amd import engine  # noqa: E402


def span(eng, launch, window, warmup):
    """Milliseconds per call of launch(): warmed up, one call timed to size the span, then `reps` calls in one span of about `window` seconds."""
    for _ in range(warmup):
        launch()
    eng.timing_begin()
    launch()
    one = max(eng.timing_end()[0], 1e-3)
    reps = int(min(max(math.ceil(window * 1e3 / one), 3), 20000))
    eng.timing_begin()
    for _ in range(reps):
        launch()
    ms = eng.timing_end()[0]
    return ms / reps, reps, ms


def host_loop(g, ref, nv):
    """The reference's loop restated with numpy and scipy's cKDTree, for one track: seconds (tree construction apart)."""
    import fric_ref as fr
    from scipy.spatial import cKDTree
    t0 = time.perf_counter()
    tree = cKDTree(g["cells"])
    t1 = time.perf_counter()
    queries = 0
    for r in fr.grid(ref, nv, g["width"], g["wb_f"], g["wb_r"], g["dn"]):
        for k in range(4):
            mue = g["mue"][tree.query(r["xy"][k])[1]]
            np.polyfit(r["n"], mue, 1)
            queries += r["cnt"]
    return time.perf_counter() - t1, t1 - t0, queries


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.6, help="seconds a timed span should last")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--copies", type=int, nargs="+", default=[1, 256, 1024])
    ap.add_argument("--grid-tracks", type=int, nargs="+", default=[1, 256])
    ap.add_argument("--racelines", type=int, default=1024)
    ap.add_argument("--stations", type=int, default=3003)
    a = ap.parse_args()
    import fric_guard as fg
    import fric_ref as fr
    eng = engine.Engine(0)          # (EngineError without a device)
    g = fg.recorded("berlin_2018")
    z = np.load(os.path.join(ROOT, "tests", "golden", "berlin_2018.npz"))
    ref, nv, alpha = z["reftrack"], z["normvec"], z["alpha"]
    n = ref.shape[0]
    fmap = eng.friction_map(g["cells"], g["mue"])
    res = dict(map=fmap.info, window_s=a.window, warmup=a.warmup, note="bytes: computed from shapes (queries in, results out), not measured traffic")
    base = np.vstack([r["xy"].reshape(-1, 2) for r in fr.grid(ref, nv, g["width"], g["wb_f"], g["wb_r"], g["dn"])])
    rng = np.random.default_rng(11)
    # ---- the query entry
    res["query"] = []
    for copies in a.copies:
        count = base.shape[0] * copies
        d_q, d_m = eng.alloc(count * 16), eng.alloc(count * 8)
        for c in range(copies):
            eng.upload(d_q, base + (rng.uniform(-0.25, 0.25, 2) if c else 0.0), offset_bytes=c * base.shape[0] * 16)
        ms, reps, total = span(eng, lambda: eng.friction_query_device(fmap, count, d_q, d_m), a.window, a.warmup)
        first = eng.download(d_m, (base.shape[0],), np.float64)
        assert np.all(np.isfinite(first))
        nbytes = count * 24.0
        res["query"].append(dict(queries=count, ms_per_call=ms, calls_in_span=reps, span_ms=total, queries_per_s=count / (ms * 1e-3),
                                 bytes=nbytes, bytes_per_s=nbytes / (ms * 1e-3)))
        eng.free(d_q)
        eng.free(d_m)
    # ---- the grid entry
    res["grid"] = []
    jmax = engine.Engine.friction_jmax([ref], [g["width"]], g["dn"])
    for tracks in a.grid_tracks:
        rows = n + 1
        d_ref, d_nv = eng.alloc(tracks * n * 32), eng.alloc(tracks * n * 16)
        for t in range(tracks):
            eng.upload(d_ref, ref, offset_bytes=t * n * 32)
            eng.upload(d_nv, nv, offset_bytes=t * n * 16)
        d_no, d_cnt, d_mu = eng.alloc(tracks * rows * jmax * 8), eng.alloc(tracks * rows * 4), eng.alloc(tracks * 4 * rows * jmax * 8)
        d_w, d_st = eng.alloc(tracks * 4 * rows * 16), eng.alloc(tracks * 4)
        ms, reps, total = span(eng, lambda: eng.friction_grid_device(fmap, tracks, n, None, d_ref, d_nv, g["width"], None, g["wb_f"], g["wb_r"], g["dn"],
                                                                     jmax, d_no, d_cnt, d_mu, None, d_w, d_st), a.window, a.warmup)
        assert not np.any(eng.download(d_st, (tracks,), np.int32))
        cnt = eng.download(d_cnt, (rows,), np.int32)
        queries = 4 * int(cnt.sum()) * tracks
        nbytes = tracks * (n * 48.0 + rows * jmax * 8.0 + rows * 4.0 + 4.0 * rows * jmax * 8.0 + 4.0 * rows * 16.0 + 4.0)
        res["grid"].append(dict(tracks=tracks, rows=rows, jmax=jmax, queries=queries, ms_per_call=ms, calls_in_span=reps, span_ms=total,
                                queries_per_s=queries / (ms * 1e-3), bytes=nbytes, bytes_per_s=nbytes / (ms * 1e-3)))
        for p in (d_ref, d_nv, d_no, d_cnt, d_mu, d_w, d_st):
            eng.free(p)
    # ---- raceline -> mu -> profile, resident
    B, m_want = a.racelines, a.stations
    length = float(np.sum(np.hypot(*np.diff(np.vstack((ref[:, :2] + nv * alpha[:, None], ref[:1, :2] + nv[:1] * alpha[0])), axis=0).T)))
    step, mmax = length / (m_want - 0.5), m_want + 64
    scale = np.linspace(0.9, 1.0, B)
    d_ref, d_nv, d_al = eng.alloc(B * n * 32), eng.alloc(B * n * 16), eng.alloc(B * n * 8)
    for b in range(B):
        eng.upload(d_ref, ref, offset_bytes=b * n * 32)
        eng.upload(d_nv, nv, offset_bytes=b * n * 16)
        eng.upload(d_al, alpha * scale[b], offset_bytes=b * n * 8)
    d_xy, d_psi, d_k, d_el = eng.alloc(B * mmax * 16), eng.alloc(B * mmax * 8), eng.alloc(B * mmax * 8), eng.alloc(B * mmax * 8)
    d_m, d_st, d_mu, d_vx, d_lt = eng.alloc(B * 4), eng.alloc(B * 4), eng.alloc(B * mmax * 8), eng.alloc(B * mmax * 8), eng.alloc(B * 8)
    eng.upload(d_xy, np.full((B, mmax, 2), np.nan))          # rows behind m stay NaN: NaN in, NaN out
    v = np.arange(0.0, 72.1, 4.0)
    ggv = np.tile(np.column_stack((v, np.full(v.size, 12.0), np.full(v.size, 12.0))), (B, 1, 1))
    axm = np.tile(np.column_stack((v, np.interp(v, [0.0, 20.0, 72.0], [5.3, 5.3, 1.2]))), (B, 1, 1))
    ptrs = []

    def up(arr):
        arr = np.ascontiguousarray(arr)
        ptrs.append(eng.alloc(arr.nbytes))
        eng.upload(ptrs[-1], arr)
        return ptrs[-1]
    d_g, d_a, d_drag, d_mass, d_vmax = up(ggv), up(axm), up(np.full(B, 0.75)), up(np.full(B, 1200.0)), up(np.full(B, 70.0))
    d_to = up(np.arange(B, dtype=np.int32))
    vo = engine.McqVelOpts(1.0, 0, 0, d_mu)

    def raceline():
        eng._check(eng.lib.mcq_raceline_device(eng.h, B, n, None, d_ref, d_nv, d_al, step, mmax, d_xy, d_psi, d_k, d_el, d_m, d_st), "mcq_raceline_device")

    def mu():
        eng.friction_query_device(fmap, B * mmax, d_xy, d_mu)

    def profile():
        eng._check(eng.lib.mcq_vel_profile_device_opts(eng.h, B, mmax, mmax, d_m, d_to, d_k, d_el, d_g, v.size, d_a, v.size, d_drag, d_mass, d_vmax,
                                                       ctypes.byref(vo), d_vx, d_lt), "mcq_vel_profile_device_opts")

    def chain():
        raceline()
        mu()
        profile()
    chain()
    ms_of = {name: span(eng, fn, a.window, a.warmup) for name, fn in (("raceline", raceline), ("mu", mu), ("profile", profile), ("chain", chain))}
    m = eng.download(d_m, (B,), np.int32)
    lap = eng.download(d_lt, (B,), np.float64)
    assert not np.any(eng.download(d_st, (B,), np.int32)) and np.all(np.isfinite(lap))
    q = int(m.sum())
    res["chain"] = dict(racelines=B, stations_min=int(m.min()), stations_max=int(m.max()), mmax=mmax, lap_s_first=float(lap[0]),
                        **{k + "_ms": v[0] for k, v in ms_of.items()}, **{k + "_calls_in_span": v[1] for k, v in ms_of.items()},
                        mu_queries_per_s=q / (ms_of["mu"][0] * 1e-3), mu_bytes=B * mmax * 24.0, mu_bytes_per_s=B * mmax * 24.0 / (ms_of["mu"][0] * 1e-3))
    # ---- the host loop, one track
    loop_s, tree_s, queries = host_loop(g, ref, nv)
    res["host"] = dict(tracks=1, queries=queries, loop_s=loop_s, tree_build_s=tree_s, queries_per_s=queries / loop_s)
    print(json.dumps(res))
    fmap.close()
    eng.close()


if __name__ == "__main__":
    main()
