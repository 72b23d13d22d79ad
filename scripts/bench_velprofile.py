#!/usr/bin/env python
"""Measurement for row f-3: ggv velocity profile + lap time of 16384 (track, vehicle) variants -- BASELINE config 4's sweep
size -- on the racelines of the committed reference tracks; the host chain timed on a sample beside it.  One JSON line.

  python scripts/bench_velprofile.py [--variants 16384] [--cpu-sample 16] [--form closed|open|locgg|open_locgg] [--kernel-runs 3]

--form: the same variants on the other forms of tph.calc_vel_profile (mcq_vel_profile_device_forms) -- open: the raceline cut open (its closing
element dropped), v_start = 0, no v_end; locgg: a synthetic per-waypoint loc_gg (12 m/s^2 +- 10 % along the lap, scaled per variant as the
diagram is) in place of the diagram.  kernel_ms: the launch alone, timed on the device (no copies, no allocation), one entry per run.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from global_racetrajectory_optimization_amd import engine                                                              # noqa: E402
from global_racetrajectory_optimization_amd.trajectory_planning_helpers import (calc_ax_profile as ca, calc_head_curv_an as ch,  # noqa: E402
                                                                                calc_t_profile as ct, calc_vel_profile as cv,
                                                                                create_raceline as cr)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variants", type=int, default=16384)
    ap.add_argument("--cpu-sample", type=int, default=16)
    ap.add_argument("--form", choices=("closed", "open", "locgg", "open_locgg"), default="closed")
    ap.add_argument("--kernel-runs", type=int, default=3)
    args = ap.parse_args()
    closed, local = args.form in ("closed", "locgg"), "locgg" in args.form
    eng = engine.Engine(0)
    g = np.load(os.path.join(ROOT, "tests", "golden", "berlin_2018.npz"))
    out = cr.create_raceline(refline=g["reftrack"][:, :2], normvectors=g["normvec"], alpha=g["alpha"], stepsize_interp=3.0)
    _, kappa = ch.calc_head_curv_an(coeffs_x=out[2], coeffs_y=out[3], ind_spls=out[4], t_spls=out[5])
    el = out[8]
    n = kappa.size
    v = np.arange(0.0, 72.1, 4.0)
    ggv0 = np.column_stack((v, np.full(v.size, 12.0), np.full(v.size, 12.0)))
    axm = np.column_stack((v, np.interp(v, [0.0, 20.0, 72.0], [5.3, 5.3, 1.2])))
    bsz = args.variants
    scales = 0.3 + 0.7 * (np.arange(bsz) % 128) / 127.0
    tops = 100.0 / 3.6 + (50.0 / 3.6) * ((np.arange(bsz) // 128) % 128) / 127.0
    ggv = np.repeat(ggv0[None], bsz, axis=0)
    ggv[:, :, 1:] *= scales[:, None, None]
    axms = np.repeat(axm[None], bsz, axis=0)
    tr = np.zeros(bsz, dtype=np.int32)
    kap_rows, el_rows, kw = kappa[None], el[None], {}
    if not closed:
        kw.update(closed=False, v_start=0.0)            # (el keeps its shape: entry n - 1, the closing element, is not read)
    if local:
        # one row of local limits per scale (128 of them), the raceline repeated under each: the variants of the diagram's sweep
        lg_row = 12.0 * (1.0 + 0.1 * np.column_stack((np.sin(0.05 * np.arange(n)), np.cos(0.03 * np.arange(n)))))
        loc_gg = lg_row[None] * (0.3 + 0.7 * np.arange(128) / 127.0)[:, None, None]
        kap_rows, el_rows, tr = np.repeat(kappa[None], 128, axis=0), np.repeat(el[None], 128, axis=0), (np.arange(bsz) % 128).astype(np.int32)
        ggv = None
        kw.update(loc_gg=loc_gg)

    def launch(sl=slice(None), **more):
        return eng.vel_profile_batch(kap_rows, el_rows, None if local else ggv[sl], axms[sl], 0.75, 1200.0, tops[sl], 1.0, tr[sl], **kw, **more)
    launch(slice(0, 64))                                # warm-up
    t0 = time.perf_counter()
    vx, lt = launch()
    t_gpu = time.perf_counter() - t0                    # includes the PCIe copies of the tables and of the profiles
    kernel_ms = [launch(timed=True)[2] for _ in range(args.kernel_runs)]
    ks = np.linspace(0, bsz - 1, args.cpu_sample).astype(int)
    t0 = time.perf_counter()
    worst, worst_t_host = 0.0, 0.0
    el_h = el if closed else el[:-1]
    for k in ks:
        vx_h = cv.calc_vel_profile(ggv=None if local else ggv[k], loc_gg=loc_gg[tr[k]] if local else None, ax_max_machines=axm, v_max=tops[k],
                                   kappa=kappa, el_lengths=el_h, closed=closed, filt_window=None, dyn_model_exp=1.0, drag_coeff=0.75,
                                   m_veh=1200.0, v_start=None if closed else 0.0)
        vx_cl = np.append(vx_h, vx_h[0]) if closed else vx_h
        ax_h = ca.calc_ax_profile(vx_profile=vx_cl, el_lengths=el_h, eq_length_output=False)
        t_h = ct.calc_t_profile(vx_profile=vx_h, ax_profile=ax_h, el_lengths=el_h)
        worst = max(worst, float(np.max(np.abs(vx[k] - vx_h))), abs(float(lt[k] - np.sum(2.0 * el_h / (vx_cl[:-1] + vx_cl[1:])))))
        worst_t_host = max(worst_t_host, abs(float(lt[k] - t_h[-1])))
    t_cpu = (time.perf_counter() - t0) / len(ks)
    print(json.dumps({"variants": bsz, "n": int(n), "track": "berlin_2018 raceline", "form": args.form, "gpu_seconds_incl_pcie": t_gpu,
                      "variants_per_s_gpu": bsz / t_gpu, "kernel_ms": kernel_ms,
                      "variants_per_s_kernel": (bsz / (1e-3 * min(kernel_ms))) if kernel_ms else None, "cpu_seconds_per_variant": t_cpu, "variants_per_s_cpu_1core": 1.0 / t_cpu,
                      "cpu_sample": len(ks), "max_abs_diff_vs_host": worst, "max_lap_time_diff_vs_host_unstable_formula_s": worst_t_host,
                      "lap_time_range_s": [float(lt.min()), float(lt.max())]}))


if __name__ == "__main__":
    main()
