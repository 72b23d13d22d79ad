"""The batched post-QP flow for OPEN tracks at the headline size: 1024 chains of 2000 waypoints (the first 2000 waypoints of the config-3
generator's rings of 2400, end headings from their end chords, as scripts/bench_open.py) through

    chain solve (mcq_solve_batch_ends)  ->  open raceline (mcq_raceline_device_ends)  ->  unclosed velocity profile (mcq_vel_profile_device_forms)

and, in the same run, the RING raceline entry (mcq_raceline_device) on rings of the same size next to the open entry.  The two raceline entries
are timed on the device (mcq_timing_begin / mcq_timing_end around the entry alone, inputs and outputs resident), alternating, --steps times each
after --warmup.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from global_racetrajectory_optimization_amd import engine, synthetic  # noqa: E402

STEP_OUT = 2.0          # stepsize_interp_after_opt [REF params/racecar.ini:15]


class Resident:
    """Inputs and outputs of one raceline launch, resident on an engine's device."""

    def __init__(self, eng, refs, nvs, als, mmax, ends=None):
        self.eng, self.bsz, self.n, self.mmax = eng, refs.shape[0], refs.shape[1], mmax
        self.ptrs = []
        self.d_ref, self.d_nv, self.d_al = self.up(refs), self.up(nvs), self.up(np.ascontiguousarray(als))
        self.d_n = self.up(np.full(self.bsz, self.n, dtype=np.int32))
        self.d_closed = self.d_psi = None
        if ends is not None:
            self.d_closed = self.up(np.zeros(self.bsz, dtype=np.int32))
            self.d_psi = self.up(np.array([[e["psi_s"], e["psi_e"]] for e in ends]))
        self.d_xy, self.d_ps, self.d_k, self.d_el = (self.new(self.bsz * mmax * w) for w in (16, 8, 8, 8))
        self.d_m, self.d_st = self.new(self.bsz * 4), self.new(self.bsz * 4)

    def up(self, a):
        p = self.eng.alloc(a.nbytes)
        self.ptrs.append(p)
        self.eng.upload(p, a)
        return p

    def new(self, nbytes):
        p = self.eng.alloc(nbytes)
        self.ptrs.append(p)
        return p

    def launch(self):
        e = self.eng
        if self.d_psi is None:
            rc = e.lib.mcq_raceline_device(e.h, self.bsz, self.n, self.d_n, self.d_ref, self.d_nv, self.d_al, STEP_OUT, self.mmax, self.d_xy,
                                           self.d_ps, self.d_k, self.d_el, self.d_m, self.d_st)
            e._check(rc, "mcq_raceline_device")
        else:
            e.raceline_device_ends(self.bsz, self.n, self.d_n, self.d_ref, self.d_nv, self.d_al, self.d_closed, self.d_psi, STEP_OUT, self.mmax,
                                   self.d_xy, self.d_ps, self.d_k, self.d_el, self.d_m, self.d_st)

    def timed(self):
        self.eng.timing_begin()
        self.launch()
        return self.eng.timing_end()[0]

    def results(self):
        e = self.eng
        return dict(kappa=e.download(self.d_k, (self.bsz, self.mmax), np.float64), el_lengths=e.download(self.d_el, (self.bsz, self.mmax), np.float64),
                    m=e.download(self.d_m, (self.bsz,), np.int32), status=e.download(self.d_st, (self.bsz,), np.int32))

    def free(self):
        for p in self.ptrs:
            self.eng.free(p)


def _stats(t):
    return dict(ms_median=float(np.median(t)), ms_min=float(np.min(t)), ms_max=float(np.max(t)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--n", type=int, default=2000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    B, n = a.batch, a.n
    rr, rn, rs = synthetic.oval_batch(B, n)
    rings = [dict(reftrack=rr[k], normvec=rn[k], scaling=rs[k], kappa_bound=0.12, w_veh=3.4) for k in range(B)]
    cr, cn, _ = synthetic.oval_batch(B, n + 400)
    cr, cn = np.ascontiguousarray(cr[:, :n]), np.ascontiguousarray(cn[:, :n])
    chains, ends = [], []
    for k in range(B):
        el = np.sqrt(np.sum(np.diff(cr[k, :, :2], axis=0) ** 2, axis=1))
        chains.append(dict(reftrack=cr[k], normvec=cn[k], scaling=np.concatenate((el[:-1] / el[1:], [1.0, 1.0])), kappa_bound=0.12, w_veh=3.4))
        d0, d1 = cr[k, 1, :2] - cr[k, 0, :2], cr[k, -1, :2] - cr[k, -2, :2]
        ends.append(dict(psi_s=float(np.arctan2(d0[1], d0[0]) - np.pi / 2), psi_e=float(np.arctan2(d1[1], d1[0]) - np.pi / 2)))
    eng = engine.Engine(0)
    res = dict(batch=B, n=n, steps=a.steps, warmup=a.warmup, stepsize=STEP_OUT)

    # ---- the QPs: chains (timed: the flow's first stage) and rings (their alpha feeds the ring entry) --------------------------------------------
    t = []
    for k in range(a.warmup + min(a.steps, 5)):
        t0 = time.perf_counter()
        al_c, _, st_c, _ = eng.solve_batch(chains, ends=ends)
        if k >= a.warmup:
            t.append(1e3 * (time.perf_counter() - t0))
    al_r, _, st_r, _ = eng.solve_batch(rings)
    res["chain_solve_host_entry"] = dict(_stats(t), status_ok=int(np.sum(st_c == 0)))
    assert np.all(st_c == 0) and np.all(st_r == 0)

    # ---- the two raceline entries, alternating, on the device --------------------------------------------------------------------------------
    per = float(np.max(np.sum(np.hypot(*np.diff(rr[:, :, :2], axis=1, append=rr[:, :1, :2]).transpose(2, 0, 1)), axis=1)))
    mmax = int(per / STEP_OUT * 1.25) + 16
    runs = {"ring_entry": Resident(eng, rr, rn, np.stack(al_r), mmax), "open_entry": Resident(eng, cr, cn, np.stack(al_c), mmax, ends=ends)}
    times = {k: [] for k in runs}
    for s in range(a.warmup + a.steps):
        for k, r in runs.items():
            ms = r.timed()
            if s >= a.warmup:
                times[k].append(ms)
    for k in runs:
        res[k] = _stats(times[k])
    out_r, out_c = runs["ring_entry"].results(), runs["open_entry"].results()
    assert np.all(out_r["status"] == 0) and np.all(out_c["status"] == 0)
    res["ring_entry"]["mean_points"] = float(np.mean(out_r["m"]))
    res["open_entry"]["mean_points"] = float(np.mean(out_c["m"]))
    res["open_over_ring"] = res["open_entry"]["ms_median"] / res["ring_entry"]["ms_median"]

    # ---- unclosed velocity profiles on the open entry's own kappa / el_lengths rows: one vehicle per chain -----------------------------------------
    v = np.arange(0.0, 72.1, 4.0)
    ggv = np.repeat(np.column_stack((v, np.full(v.size, 12.0), np.full(v.size, 12.0)))[None], B, axis=0)
    axm = np.repeat(np.column_stack((v, np.interp(v, [0.0, 20.0, 72.0], [5.3, 5.3, 1.2])))[None], B, axis=0)
    t = []
    for k in range(a.warmup + min(a.steps, 5)):
        vx, lap, ms = eng.vel_profile_batch(out_c["kappa"], out_c["el_lengths"], ggv, axm, 0.75, 1200.0, 70.0, 1.0, n_of_track=out_c["m"],
                                            closed=False, v_start=10.0, timed=True)
        if k >= a.warmup:
            t.append(ms)
    assert np.all(np.isfinite(lap))
    res["unclosed_profile_device"] = _stats(t)
    res["flow_ms"] = res["chain_solve_host_entry"]["ms_median"] + res["open_entry"]["ms_median"] + res["unclosed_profile_device"]["ms_median"]
    res["timings"] = "chain solve: wall time of the host entry (packing + PCIe); raceline entries and profile: device time of the entry alone"
    print(json.dumps(res))
    for r in runs.values():
        r.free()
    eng.close()


if __name__ == "__main__":
    main()
