"""The export tables on the device: mcq_export_device timed at two shapes, inputs and outputs resident.

    bench     1024 racelines of --n waypoints and ~3000 stations, one variant each
    config4   BASELINE config 4's shape: 256 tracks x 64 variants = 16 384 tables (the variants of a track share its s column, as the flow's do)

Tracks: synthetic.oval_batch with a smooth alpha per track; a variant's trajectory is an array with s_j = j total / m and seeded values in the
other columns (the entry copies them; it computes nothing from them).  The entry is timed on the device between events (mcq_timing_begin /
mcq_timing_end around the entry alone), --steps times after --warmup: that is BOTH kernels.  The two kernels separately come from a run of this
script under `rocprofv3 --kernel-trace --stats` with --profile (no timing, the same launches).  Reported per shape: milliseconds per call, the bytes
the rows kernel must move -- the table out, the s column and the gathered columns of the trajectory in, the seven copied input columns in -- and,
with the rows kernel's own time (--rows-ms, from the trace; else the whole entry's), their rate as a fraction of the 6.29 TB/s a float4 copy
reaches on the MI355X.  Beside it: the numpy restatement of the reference's loop (cumsum, n argmins over m stations, the column stack) for ONE
track on one core, with the spline lengths' restatement timed apart.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from global_racetrajectory_optimization_amd import engine, synthetic  # noqa: E402

COPY_RATE = 6.29e12         # B/s, float4 copy on the MI355X
STATIONS = 3000


def tracks_of(count, n):
    ref, nv, _ = synthetic.oval_batch(count, n)
    i = np.arange(n)
    al = np.stack([0.8 * np.sin(2.0 * np.pi * (3 + k % 5) * i / n + 0.1 * k) for k in range(count)])
    return ref, nv, al


def shape(eng, tracks, per_track, n, steps, warmup, profile, rows_ms):
    import export_ref as xr
    ref, nv, al = tracks_of(tracks, n)
    B = tracks * per_track
    total0 = float(xr.front(ref[0], nv[0], al[0], np.float64)["total"])
    m = STATIONS
    track_of = np.repeat(np.arange(tracks, dtype=np.int32), per_track)
    ptrs = []

    def new(nbytes):
        ptrs.append(eng.alloc(nbytes))
        return ptrs[-1]

    def up(a):
        a = np.ascontiguousarray(a)
        p = new(a.nbytes)
        eng.upload(p, a)
        return p
    d_ref, d_nv, d_al, d_to = up(ref), up(nv), up(al), up(track_of)
    d_tj = new(B * m * 7 * 8)
    rng = np.random.default_rng(7)
    chunk = max(1, min(B, 64))
    first = None
    for b0 in range(0, B, chunk):                  # uploaded chunk by chunk: the whole array is 2.75 GB at config 4's shape
        t = rng.standard_normal((chunk, m, 7))
        t[:, :, 0] = np.arange(m) * (total0 / m)   # (every track's own length differs from total0 in the per-mille: the lookup does not care)
        eng.upload(d_tj, t, offset_bytes=b0 * m * 56)
        if first is None:
            first = t[0].copy()
    d_tab, d_idx = new(B * (n + 1) * 96), new(B * n * 4)
    d_len, d_s, d_tot, d_st = new(tracks * n * 8), new(tracks * (n + 1) * 8), new(tracks * 8), new(B * 4)

    def launch():
        eng.export_device(tracks, n, None, d_ref, d_nv, d_al, B, m, None, d_to, d_tj, d_tab, d_idx, d_len, d_s, d_tot, d_st)
    out = dict(tracks=tracks, variants=B, waypoints=n, stations=m)
    if profile:
        for _ in range(warmup + steps):
            launch()
        eng.sync()
    else:
        t = []
        for s in range(warmup + steps):
            eng.timing_begin()
            launch()
            ms = eng.timing_end()[0]
            if s >= warmup:
                t.append(ms)
        out.update(entry_ms_median=float(np.median(t)), entry_ms_min=float(np.min(t)), entry_ms_max=float(np.max(t)))
    status = eng.download(d_st, (B,), np.int32)
    assert np.all(status == 0), "refused variants: %d" % int(np.sum(status != 0))
    idx0 = eng.download(d_idx, (n,), np.int32)
    s_ref0 = eng.download(d_s, (n + 1,), np.float64)
    tab0 = eng.download(d_tab, (n + 1, 12), np.float64)
    want = np.array([int(np.abs(first[:, 0] - s).argmin()) for s in s_ref0[:n]])
    assert np.array_equal(idx0, want) and np.array_equal(tab0[:n, 8:12].view(np.uint64), first[idx0, 3:7].view(np.uint64))
    for p in ptrs:
        eng.free(p)
    nbytes = B * ((n + 1) * 96.0 + m * 8.0 + n * 32.0 + n * 56.0)
    out.update(rows_kernel_bytes=nbytes)
    if not profile:
        ms = rows_ms if rows_ms else out["entry_ms_median"]
        out.update(rows_ms_used=ms, rows_ms_source="kernel trace" if rows_ms else "whole entry", bytes_per_s=nbytes / (ms * 1e-3),
                   share_of_copy_rate=nbytes / (ms * 1e-3) / COPY_RATE)
    return out, (ref[0], nv[0], al[0], first)


def host_one_track(ref, nv, al, traj):
    """The reference's loop in numpy for one track, on one core: (ms of the spline lengths' restatement, ms of the loop and the stack)."""
    import export_ref as xr
    t0 = time.perf_counter()
    lengths = np.float64(xr.front(ref, nv, al, np.float64)["lengths"])
    t1 = time.perf_counter()
    s = np.insert(np.cumsum(lengths), 0, 0.0)
    cols = [[], [], [], []]
    for q in list(s[:-1]):
        i = (np.abs(traj[:, 0] - q)).argmin()
        for c in range(4):
            cols[c].append(traj[i, 3 + c])
    tab = np.column_stack((ref, nv, al, s[:-1], *cols))
    tab = np.vstack((tab, tab[0]))
    tab[-1, 7] = s[-1]
    t2 = time.perf_counter()
    return 1e3 * (t1 - t0), 1e3 * (t2 - t1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--bench-batch", type=int, default=1024)
    ap.add_argument("--config4-tracks", type=int, default=256)
    ap.add_argument("--profile", action="store_true", help="launch only (for a kernel trace); no event timing")
    ap.add_argument("--rows-ms", type=float, nargs=2, default=None, help="mcq_export_rows_kernel's average time per launch at the two shapes (from the trace)")
    a = ap.parse_args()
    eng = engine.Engine(0)
    res = dict(n=a.n, steps=a.steps, warmup=a.warmup, copy_rate=COPY_RATE, profile=a.profile)
    res["bench"], one = shape(eng, a.bench_batch, 1, a.n, a.steps, a.warmup, a.profile, a.rows_ms[0] if a.rows_ms else None)
    res["config4"], _ = shape(eng, a.config4_tracks, 64, a.n, a.steps, a.warmup, a.profile, a.rows_ms[1] if a.rows_ms else None)
    if not a.profile:
        res["host_spline_lengths_one_track_ms"], res["host_loop_one_track_ms"] = host_one_track(*one)
    print(json.dumps(res))
    eng.close()


if __name__ == "__main__":
    main()
