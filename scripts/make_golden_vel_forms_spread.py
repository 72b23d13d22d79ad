#!/usr/bin/env python
"""Writes tests/golden/vel_forms/vel_forms_spread.npz: how far oracle/vel_ref.py's answer is determined on every case of tests/vel_forms_cases.py that is
compared with it (tests/vel_forms_guard.py says how: its movement under four draws of a relative 1e-15 on kappa, el_lengths, mu and loc_gg).  One
[batch, 2] array (vx, time) per kind and launch; arrays of spreads only.  Python loops over the points of every profile: minutes, over a pool.

  python scripts/make_golden_vel_forms_spread.py [--jobs 8]
"""
import argparse
import multiprocessing as mp
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vel_forms_cases as fc            # noqa: E402
import vel_forms_guard as fg            # noqa: E402


def _one(job):
    k, lo, hi = job
    F = [F for _, F in fc.all_launches() if fg.key(F) == k][0]
    only = list(range(lo, hi))
    return k, lo, hi, fg.compute_spread(F, only=only)[lo:hi]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=8)
    args = ap.parse_args()
    jobs, out = [], {}
    for _, F in fc.all_launches():
        if not F["parity"]:
            continue
        bsz = F["ggv"].shape[0]
        out[fg.key(F)] = np.zeros((bsz, 2))
        step = 4 if F["kappa"].shape[1] > 256 else 16
        jobs += [(fg.key(F), lo, min(lo + step, bsz)) for lo in range(0, bsz, step)]
    with mp.Pool(args.jobs) as pool:
        for k, lo, hi, s in pool.imap_unordered(_one, jobs):
            out[k][lo:hi] = s
    os.makedirs(os.path.dirname(fg.PATH), exist_ok=True)
    np.savez_compressed(fg.PATH, **out)
    S = np.vstack([out[k] for k in sorted(out)])
    for qi, q in enumerate(fg.VEL_Q):
        g = np.maximum(fg.FLOOR[q], 4.0 * S[:, qi])
        print("%s: %d cases, %d above the floor, largest guard %.2e, largest spread %.2e" % (q, S.shape[0], int(np.sum(g > fg.FLOOR[q])), float(np.max(g)),
                                                                                        float(np.max(S[:, qi]))))
    for k in sorted(out):
        bad = np.nonzero((4.0 * out[k] > np.array([fg.FLOOR[q] for q in fg.VEL_Q])).any(axis=1))[0]
        if bad.size:
            print("  above the floor: %s variants %s spreads %s" % (k, bad.tolist(), out[k][bad].tolist()))


if __name__ == "__main__":
    main()
