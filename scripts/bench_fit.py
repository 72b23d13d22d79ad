"""FITPACK's periodic smoothing fit, host against device, in one run on one machine, on the Berlin rows of
tests/golden/spline_approx/cases.npz (k = 3, s = 10, stepsize_prep = 1: 2328 closed points, 78 knots):

    device entry   mcq_spline_fit_device alone (re-sampling, parameter, fit), inputs and outputs resident, timed on the device with
                   mcq_timing_begin / mcq_timing_end, the median of --steps after --warmup: one track, and --batch copies (default 256, each
                   shifted by its index so that no two are the same rows) in one launch
    host loop      the parent's route for the same tracks: interp_track and scipy.interpolate.splprep, one track after the other
    end to end     Engine.prep_track_batch(fit="device") against Engine.prep_track_batch(fit="host") on the batch, wall clock, uploads and
                   downloads included, the median of --e2e-steps after one warm-up

Reads nothing outside the repository.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from global_racetrajectory_optimization_amd import engine  # noqa: E402

CASES = os.path.join(ROOT, "tests", "golden", "spline_approx", "cases.npz")
K, S, STEP = 3, 10.0, 1.0


def device_ms(eng, tracks, steps, warmup):
    bsz, n = len(tracks), tracks[0].shape[0]
    trk = np.ascontiguousarray(np.stack(tracks))
    total = float(np.sum(np.hypot(*np.diff(np.vstack((tracks[0][:, :2], tracks[0][:1, :2])), axis=0).T)))
    mimax = int(np.ceil(total / STEP)) + 3
    nkmax = mimax + 2 * K
    ptrs = []

    def up(a):
        p = eng.alloc(a.nbytes)
        ptrs.append(p)
        eng.upload(p, a)
        return p
    try:
        d_trk = up(trk)
        d_nk, d_kn, d_cf, d_fp, d_ier, d_mi, d_st = [up(np.zeros(sz, dtype=np.uint8)) for sz in (
            bsz * 4, bsz * nkmax * 8, bsz * 2 * nkmax * 8, bsz * 8, bsz * 4, bsz * 4, bsz * 4)]
        t = []
        for s in range(warmup + steps):
            eng.timing_begin()
            eng.spline_fit_device(bsz, n, None, d_trk, STEP, mimax, K, S, nkmax, d_nk, d_kn, d_cf, d_fp, d_ier, d_mi, None, d_st)
            ms = eng.timing_end()[0]
            if s >= warmup:
                t.append(ms)
        st, nk = eng.download(d_st, (bsz,), np.int32), eng.download(d_nk, (bsz,), np.int32)
        ier, mi = eng.download(d_ier, (bsz,), np.int32), eng.download(d_mi, (bsz,), np.int32)
        assert np.all(st == 0) and np.all(ier == 0), (st, ier)
        return float(np.median(t)), int(nk[0]), int(mi[0])
    finally:
        for p in ptrs:
            eng.free(p)


def host_loop_seconds(tracks):
    try:
        from scipy import interpolate
    except ImportError:
        return None
    from global_racetrajectory_optimization_amd.trajectory_planning_helpers import interp_track as it
    t0 = time.perf_counter()
    for trk in tracks:
        ti = it.interp_track(track=trk, stepsize=STEP)
        cl = np.vstack((ti, ti[0]))
        interpolate.splprep([cl[:, 0], cl[:, 1]], k=K, s=S, per=1)
    return time.perf_counter() - t0


def wall(fn, steps):
    fn()
    t = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--e2e-steps", type=int, default=3)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    track = np.load(CASES)["berlin_2018.track"]
    tracks = [track + np.array([float(b), -0.5 * b, 0.0, 0.0]) for b in range(a.batch)]
    eng = engine.Engine(0)
    try:
        one_ms, nk, mi = device_ms(eng, [track], a.steps, a.warmup)
        batch_ms, _, _ = device_ms(eng, tracks, a.steps, a.warmup)
        e2e_dev = wall(lambda: eng.prep_track_batch(tracks, k_reg=K, s_reg=S, stepsize_prep=STEP, fit="device"), a.e2e_steps)
        e2e_host = None if a.no_host else wall(lambda: eng.prep_track_batch(tracks, k_reg=K, s_reg=S, stepsize_prep=STEP, fit="host"), a.e2e_steps)
    finally:
        eng.close()
    host_one = None if a.no_host else host_loop_seconds([track])
    host_all = None if a.no_host else host_loop_seconds(tracks)
    r = lambda v, d=4: None if v is None else round(v, d)      # noqa: E731
    print(json.dumps(dict(metric="periodic_smoothing_fit", raw_waypoints=int(track.shape[0]), closed_points=mi, knots=nk, batch=a.batch,
                          device_single_ms=r(one_ms), device_batch_ms=r(batch_ms), device_batch_ms_per_track=r(batch_ms / a.batch, 5),
                          host_single_s=r(host_one), host_loop_s=r(host_all),
                          host_loop_over_device_batch=None if host_all is None else r(host_all * 1e3 / batch_ms, 2),
                          prep_track_batch_device_fit_s=r(e2e_dev), prep_track_batch_host_fit_s=r(e2e_host))))


if __name__ == "__main__":
    main()
