"""The last row of the post-QP flow on the device: mcq_bound_dists_device (check_traj's distance check, the one compute-bound piece) and
mcq_trajectory_device (ax, t, rows, limits, verdicts), timed at two shapes:

    config4   BASELINE config 4's shape: 4 tracks x 64 vehicle widths = 256 racelines (solve -> raceline), the distance check on all 256 with the
              width list, then 64 ggv / top-speed variants per raceline = 16 384 profiles and trajectory_batch's entry on them
    bench     the bench workload's shape: 1024 rings of 2000 waypoints, the distance check on their racelines

Each entry is timed on the device (mcq_timing_begin / mcq_timing_end around the entry alone, inputs and outputs resident), --steps times after
--warmup.  Reported per shape: milliseconds per launch, point pairs per second, and the share of the vector issue rate the all-pairs kernel reaches:
VALU_PER_PAIR x pairs / 64 lanes wave instructions against CUS x SIMDS x CLOCK / 2 issue slots per second (a SIMD-32 issues a wave64 vector
instruction in 2 cycles; VALU_PER_PAIR is counted in the ISA of mcq_bound_dists_kernel's inner loop: 80 arithmetic instructions and 2 canonicalising
v_max per 16 pairs).  Beside it: the float64 host restatement (tests/traj_check_ref.py) of ONE track on one core.  Prints one JSON line."""
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

STEP_OUT, STEP_BOUND = 2.0, 1.0         # stepsize_interp_after_opt [REF params/racecar.ini:15]; check_traj's boundary step
LENGTH_VEH = 4.7
VALU_PER_PAIR = 82.0 / 16.0
CUS, SIMDS, CLOCK = 256, 4, 2.4e9


class Resident:
    def __init__(self, eng):
        self.eng, self.ptrs = eng, []

    def up(self, a):
        a = np.ascontiguousarray(a)
        p = self.eng.alloc(a.nbytes)
        self.ptrs.append(p)
        self.eng.upload(p, a)
        return p

    def new(self, nbytes):
        p = self.eng.alloc(nbytes)
        self.ptrs.append(p)
        return p

    def free(self):
        for p in self.ptrs:
            self.eng.free(p)


def _timed(eng, fn, steps, warmup):
    t = []
    for s in range(warmup + steps):
        eng.timing_begin()
        fn()
        ms = eng.timing_end()[0]
        if s >= warmup:
            t.append(ms)
    return dict(ms_median=float(np.median(t)), ms_min=float(np.min(t)), ms_max=float(np.max(t)))


def racelines(eng, refs, nvs, scs, w_veh):
    probs = [dict(reftrack=refs[k], normvec=nvs[k], scaling=scs[k], kappa_bound=0.12, w_veh=float(w_veh[k])) for k in range(len(refs))]
    al, _, st, _ = eng.solve_batch(probs)
    assert np.all(st == 0)
    race = eng.raceline_batch(list(refs), list(nvs), al, STEP_OUT)
    assert np.all(race["status"] == 0)
    return race


def bound_check(eng, refs, nvs, race, widths, steps, warmup):
    """The distance check of every raceline, resident; returns (stats, results)."""
    B, n, mmax = refs.shape[0], refs.shape[1], race["xy"].shape[1]
    R = Resident(eng)
    d_ref, d_nv, d_xy, d_psi, d_m, d_w = R.up(refs), R.up(nvs), R.up(race["xy"]), R.up(race["psi"]), R.up(race["m"]), R.up(widths)
    d_md, d_mn, d_nb, d_st = R.new(B * mmax * 8), R.new(B * 8), R.new(B * 8), R.new(B * 4)

    def launch():
        eng.bound_dists_device(B, n, None, d_ref, d_nv, mmax, d_m, d_xy, d_psi, LENGTH_VEH, 0.0, None, d_w, STEP_BOUND, engine.BOUNDS_ALL, d_md,
                               d_mn, d_nb, None, d_st)
    st = _timed(eng, launch, steps, warmup)
    nb, status = eng.download(d_nb, (B, 2), np.int32), eng.download(d_st, (B,), np.int32)
    mind = eng.download(d_mn, (B,), np.float64)
    R.free()
    assert np.all(status == 0)
    pairs = float(np.sum(4.0 * race["m"] * nb.sum(axis=1)))
    st.update(pairs=pairs, pairs_per_s=pairs / (st["ms_median"] * 1e-3),
              valu_issue_share=VALU_PER_PAIR * pairs / 64.0 / (st["ms_median"] * 1e-3 * CUS * SIMDS * CLOCK / 2.0),
              mean_stations=float(np.mean(race["m"])), mean_samples_per_side=float(np.mean(nb)), min_dist_min=float(np.min(mind)))
    return st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--bench-batch", type=int, default=1024)
    a = ap.parse_args()
    eng = engine.Engine(0)
    res = dict(n=a.n, steps=a.steps, warmup=a.warmup, stepsize=STEP_OUT, stepsize_bound=STEP_BOUND, valu_per_pair=VALU_PER_PAIR)

    # ---- config 4's shape ----------------------------------------------------------------------------------------------------------------
    tr, tn, ts = synthetic.oval_batch(4, a.n)
    widths = np.tile(np.linspace(1.6, 2.4, 64), 4)
    refs, nvs = np.repeat(tr, 64, axis=0), np.repeat(tn, 64, axis=0)
    race = racelines(eng, refs, nvs, np.repeat(ts, 64, axis=0), widths + 1.4)
    res["config4_bound_dists"] = dict(bound_check(eng, refs, nvs, race, widths, a.steps, a.warmup), racelines=256)
    V = 16384
    track_of = np.repeat(np.arange(256, dtype=np.int32), 64)
    v = np.arange(0.0, 72.1, 4.0)
    scale = np.tile(np.linspace(0.8, 1.2, 64), 256)
    ggv = np.repeat(np.column_stack((v, np.full(v.size, 12.0), np.full(v.size, 12.0)))[None], V, axis=0)
    ggv[:, :, 1:] *= scale[:, None, None]
    axm = np.repeat(np.column_stack((v, np.interp(v, [0.0, 20.0, 72.0], [5.3, 5.3, 1.2])))[None], V, axis=0)
    vmax = np.tile(np.linspace(50.0, 70.0, 64), 256)
    vx, lap = eng.vel_profile_batch(race["kappa"], race["el_lengths"], ggv, axm, 0.75, 1200.0, vmax, 1.0, track_of=track_of, n_of_track=race["m"])
    assert np.all(np.isfinite(lap))
    mmax = race["xy"].shape[1]
    R = Resident(eng)
    d = [R.up(race[k]) for k in ("xy", "psi", "kappa", "el_lengths", "m")]
    d_vx, d_to, d_g, d_a = R.up(vx), R.up(track_of), R.up(ggv), R.up(axm)
    d_dr, d_ms, d_vm = R.up(np.full(V, 0.75)), R.up(np.full(V, 1200.0)), R.up(vmax)
    d_traj, d_t, d_len, d_lim, d_fl = R.new(V * mmax * 56), R.new(V * (mmax + 1) * 8), R.new(V * 8), R.new(V * 48), R.new(V * 4)

    def launch():
        eng.trajectory_device(V, 0, mmax, d[4], d_to, d[0], d[1], d[2], d[3], d_vx, True, d_dr, d_ms, d_vm, d_g, ggv.shape[1], d_a, axm.shape[1],
                              0.12, d_traj, d_t, d_len, d_lim, d_fl)
    st = _timed(eng, launch, a.steps, a.warmup)
    flags = eng.download(d_fl, (V,), np.int32)
    t_last = eng.download(d_t, (V, mmax + 1), np.float64)[np.arange(V), race["m"][track_of]]
    R.free()
    assert np.all(flags >= 0) and np.array_equal(t_last.view(np.uint64), lap.view(np.uint64))
    res["config4_trajectory"] = dict(st, variants=V, stations=float(np.mean(race["m"])), flagged=int(np.sum(flags != 0)),
                                     last_time_is_lap_time_bitwise=True)

    # ---- the bench workload's shape ----------------------------------------------------------------------------------------------------------
    br, bn, bs = synthetic.oval_batch(a.bench_batch, a.n)
    race_b = racelines(eng, br, bn, bs, np.full(a.bench_batch, 3.4))
    res["bench_bound_dists"] = dict(bound_check(eng, br, bn, race_b, np.full(a.bench_batch, 2.0), a.steps, a.warmup), racelines=a.bench_batch)

    # ---- the host restatement of one track on one core ----------------------------------------------------------------------------------------
    import traj_check_ref as tcr
    m0 = int(race_b["m"][0])
    t0 = time.perf_counter()
    h = tcr.bound_dists(br[0], bn[0], race_b["xy"][0, :m0], race_b["psi"][0, :m0], LENGTH_VEH, 2.0, STEP_BOUND, False, np.float64)
    res["host_restatement_one_track_ms"] = 1e3 * (time.perf_counter() - t0)
    res["host_restatement_pairs"] = float(4 * m0 * sum(h["nb"]))
    print(json.dumps(res))
    eng.close()


if __name__ == "__main__":
    main()
