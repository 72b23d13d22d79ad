"""Friction map generation on the device, timed on the MI355X (GPU only: without one the engine cannot be created and the script fails), beside the
reference's matplotlib path on the same machine.

    device    mcq_friction_gen_device on Berlin's track file (tests/golden/friction_gen/reference.npz: 2366 waypoints) at cell widths 2.0, 1.0 and
              0.5, one track, and 256 copies of the track at 2.0 in one launch; inputs and outputs resident on the device.  Per shape a counting
              call (cells_out NULL) and a call that writes the cells into buffers of the counted size.
    host      main_gen_frictionmap.py's statements for one track: numpy.arange's grid, the coordinates array, two Path.contains_points calls with a
              radius, the mask (null where matplotlib is not installed).

The entry waits once inside (it reads the grids' sizes back), so a call is timed with the host's clock around the call and a synchronise of the
handle's stream: warmed up, then --runs repetitions, of which the median and the extremes are reported.  `pairs` is the number of (grid point,
contour edge) crossing tests the all-pairs kernel makes per call.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from global_racetrajectory_optimization_amd import engine  # noqa: E402


def host_path(ref, cw, inside):
    """Seconds of the reference's statements with matplotlib, and the cells found; (None, None) without matplotlib."""
    try:
        import matplotlib.path as mpl_path
    except ImportError:
        return None, None
    import fgen_ref as fr
    right, left = fr.calc_trackboundaries(ref)
    b_in, b_out, sign = (right, left, -1) if inside == "right" else (left, right, 1)
    t0 = time.perf_counter()
    x0, x1, y0, y1 = fr.grid_range(ref)
    xg, yg = np.arange(x0, x1 + 0.1, cw), np.arange(y0, y1 + 0.1, cw)
    pts = np.empty((xg.shape[0] * yg.shape[0], 2))
    pts[:, 0], pts[:, 1] = np.repeat(xg, yg.shape[0]), np.tile(yg, xg.shape[0])
    d = cw * 1.1
    mask = mpl_path.Path(b_out).contains_points(pts, radius=d * sign) & ~mpl_path.Path(b_in).contains_points(pts, radius=-(d * sign))
    cells = pts[mask]
    return time.perf_counter() - t0, int(cells.shape[0])


def timed(eng, launch, runs, warmup):
    for _ in range(warmup):
        launch()
    eng.sync()
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        launch()
        eng.sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return dict(ms_median=ts[len(ts) // 2], ms_min=ts[0], ms_max=ts[-1], runs=runs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--widths", type=float, nargs="+", default=[2.0, 1.0, 0.5])
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--host-runs", type=int, default=3)
    a = ap.parse_args()
    import fgen_cases as fc
    import fgen_ref as fr
    eng = engine.Engine(0)          # (EngineError without a device)
    ref = fc.raw_tracks()["berlin_2018"]
    inside = fc.INSIDE["berlin_2018"]
    n = ref.shape[0]
    res = dict(track="berlin_2018", waypoints=n, runs=a.runs, warmup=a.warmup, device=[], host=[])
    for tracks, cw in [(1, w) for w in a.widths] + [(a.batch, 2.0)]:
        polys, _ = fr.polygons(ref, cw, inside == "right")
        edges = sum(fr.contour(v, r).shape[0] for v, r in polys)
        d_ref = eng.alloc(tracks * n * 32)
        for t in range(tracks):
            eng.upload(d_ref, ref, offset_bytes=t * n * 32)
        d_side = eng.alloc(tracks * 4)
        eng.upload(d_side, np.full(tracks, inside == "right", dtype=np.int32))
        d_grid, d_cnt, d_st = eng.alloc(tracks * 48), eng.alloc(tracks * 4), eng.alloc(tracks * 4)
        count_only = lambda: eng.friction_gen_device(tracks, n, None, d_ref, cw, d_side, 0, None, None, d_grid, d_cnt, None, d_st)     # noqa: E731
        t_count = timed(eng, count_only, a.runs, a.warmup)
        counts, grids = eng.download(d_cnt, (tracks,), np.int32), eng.download(d_grid, (tracks, 6), np.float64)
        cmax = int(counts.max())
        d_cells = eng.alloc(tracks * max(cmax, 1) * 16)
        full = lambda: eng.friction_gen_device(tracks, n, None, d_ref, cw, d_side, cmax, None, None, d_grid, d_cnt, d_cells, d_st)      # noqa: E731
        t_full = timed(eng, full, a.runs, a.warmup)
        st = eng.download(d_st, (tracks,), np.int32)
        assert (st == 0).all() and (counts == counts[0]).all() and counts[0] > 0
        points = int(grids[0, 4] * grids[0, 5])
        res["device"].append(dict(tracks=tracks, cellwidth=cw, points_per_track=points, cells_per_track=int(counts[0]), contour_edges=edges,
                                  pairs=tracks * points * edges, count_only=t_count, with_cells=t_full,
                                  pairs_per_s=tracks * points * edges / (t_full["ms_median"] * 1e-3)))
        for p in (d_ref, d_side, d_grid, d_cnt, d_st, d_cells):
            eng.free(p)
        if tracks == 1 and a.host_runs > 0:
            hs = sorted(host_path(ref, cw, inside) for _ in range(a.host_runs))
            if hs[0][0] is not None:
                assert hs[0][1] == int(counts[0]), "the host path finds %d cells, the device %d" % (hs[0][1], int(counts[0]))
            res["host"].append(dict(cellwidth=cw, s_median=hs[len(hs) // 2][0], s_min=hs[0][0], runs=a.host_runs, cells=hs[0][1]))
    print(json.dumps(res))
    eng.close()


if __name__ == "__main__":
    main()
