"""Track preparation behind FITPACK's fit, host against device, in one run on one machine:

    single    one Berlin-sized track (the raw rows and the recorded spline of tests/golden/spline_approx/cases.npz: 2366 raw waypoints, 776 rows):
              the host route, if scipy is there -- one whole call of trajectory_planning_helpers.spline_approximation (which fits its own
              spline) MINUS one separately timed call of FITPACK's fit on the same points: an estimate of the body behind the fit, off by
              the two fits' difference, a hundredth of the figure -- against mcq_spline_approx_device on the recorded spline, inputs and
              outputs resident
    batch     --batch copies of that track (default 256, each shifted by its index so that no two are the same rows) in one launch

The device entry is timed on the device (mcq_timing_begin / mcq_timing_end around the entry alone), --steps times after --warmup; the median
is reported.  Reads nothing outside the repository.  Prints one JSON line."""
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


def load(name="berlin_2018"):
    z = np.load(CASES)
    c = z[name + ".c"]
    return z[name + ".track"], (z[name + ".t"], (c[0], c[1]), int(z[name + ".k"])), float(z[name + ".step"])


def device_ms(eng, tracks, tcks, step, steps, warmup):
    bsz = len(tracks)
    n = tracks[0].shape[0]
    trk = np.ascontiguousarray(np.stack(tracks))
    k, nk, knots, coef = eng.pack_tcks(tcks)
    mmax = int(2.0 * n / step) + 8
    ptrs = []

    def up(a):
        p = eng.alloc(a.nbytes)
        ptrs.append(p)
        eng.upload(p, a)
        return p
    try:
        d_trk, d_nk, d_kn, d_cf = up(trk), up(nk), up(knots), up(coef)
        d_ref, d_m, d_ct, d_ds, d_dev, d_nm, d_st = [up(np.zeros(sz, dtype=np.uint8)) for sz in (
            bsz * mmax * 32, bsz * 4, bsz * (n + 1) * 8, bsz * (n + 1) * 8, bsz * 16, bsz * 4, bsz * 4)]
        t = []
        for s in range(warmup + steps):
            eng.timing_begin()
            eng.spline_approx_device(bsz, n, None, d_trk, k, knots.shape[1], d_nk, d_kn, d_cf, step, mmax, d_ref, d_m, d_ct, d_ds, d_dev, d_nm, d_st)
            ms = eng.timing_end()[0]
            if s >= warmup:
                t.append(ms)
        st = eng.download(d_st, (bsz,), np.int32)
        m = eng.download(d_m, (bsz,), np.int32)
        assert np.all(st == 0), st
        return float(np.median(t)), int(m[0])
    finally:
        for p in ptrs:
            eng.free(p)


def host_seconds(track, tck, step):
    """(seconds of one whole call of the shim minus the seconds of one separate splprep call, those seconds), or (None, None) without scipy."""
    try:
        from scipy import interpolate
    except ImportError:
        return None, None
    from global_racetrajectory_optimization_amd.trajectory_planning_helpers import interp_track as it
    from global_racetrajectory_optimization_amd.trajectory_planning_helpers import spline_approximation as sa
    ti = it.interp_track(track=track, stepsize=1.0)
    cl = np.vstack((ti, ti[0]))
    t0 = time.perf_counter()
    interpolate.splprep([cl[:, 0], cl[:, 1]], k=tck[2], s=10, per=1)
    t_fit = time.perf_counter() - t0
    t0 = time.perf_counter()
    sa.spline_approximation(track, k_reg=tck[2], s_reg=10, stepsize_prep=1.0, stepsize_reg=step)
    return time.perf_counter() - t0 - t_fit, t_fit


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    track, tck, step = load()
    eng = engine.Engine(0)
    try:
        one_ms, m = device_ms(eng, [track], [tck], step, a.steps, a.warmup)
        tracks, tcks = [], []
        for b in range(a.batch):        # the same shape moved by b metres: other rows, other coefficients, the same search
            sh = np.array([float(b), -0.5 * b, 0.0, 0.0])
            tracks.append(track + sh)
            tcks.append((tck[0], (tck[1][0] + sh[0], tck[1][1] + sh[1]), tck[2]))
        batch_ms, _ = device_ms(eng, tracks, tcks, step, a.steps, a.warmup)
    finally:
        eng.close()
    host_s, fit_s = (None, None) if a.no_host else host_seconds(track, tck, step)
    print(json.dumps(dict(metric="prep_track_behind_the_fit", raw_waypoints=int(track.shape[0]), rows=m, knots=int(tck[0].shape[0]),
                          device_single_ms=round(one_ms, 4), device_batch_ms=round(batch_ms, 4), batch=a.batch,
                          device_batch_ms_per_track=round(batch_ms / a.batch, 5),
                          host_search_s=None if host_s is None else round(host_s, 3), host_fit_s=None if fit_s is None else round(fit_s, 4))))


if __name__ == "__main__":
    main()
