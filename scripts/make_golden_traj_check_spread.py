#!/usr/bin/env python3
"""Writes tests/golden/traj_check/traj_check_spread.npz: how far the reference answers of the trajectory / check_traj tests
(tests/traj_check_cases.py) are determined -- one [rows, quantities] array per family and launch, tests/traj_check_guard.py's
compute_bound_spread / compute_traj_spread (float64 against longdouble, and SPREAD_DRAWS draws of a relative SPREAD_REL perturbation of every
input array).  No GPU, no engine: tests/traj_check_ref.py alone.  Prints the largest spread per quantity and the measured
float64-against-longdouble deviations that tests/traj_check_guard.py's floors for ax, t, ay and a_tot are derived from (next power of ten
above four times the value).  --jobs N spreads the entries over N processes."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import traj_check_cases as tc  # noqa: E402
import traj_check_guard as tg  # noqa: E402


def _entry(key):
    return key, tg.entries()[key]()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=1)
    ap.add_argument("--out", default=tg.PATH)
    a = ap.parse_args()
    t0 = time.time()
    keys = sorted(tg.entries())
    if a.jobs > 1:
        import multiprocessing as mp
        with mp.Pool(a.jobs) as pool:
            res = dict(pool.map(_entry, keys, chunksize=1))
    else:
        res = dict(_entry(k) for k in keys)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    np.savez_compressed(a.out, **{k: res[k] for k in keys})
    B = np.vstack([res[k] for k in keys if "/bound/" in k])
    T = np.vstack([res[k] for k in keys if "/traj/" in k])
    for qi, q in enumerate(("min_dists", "min_dist", "bound")):
        print("%-10s largest spread %.3e, floor %.0e" % (q, B[:, qi].max(), tg.FLOOR[tg.BOUND_Q[qi]]))
    for qi, q in enumerate(("s", "ax", "t", "length", "lim kappa", "lim ay", "lim ax+", "lim ax-", "lim a_tot", "lim vx")):
        print("%-10s largest spread %.3e, floor %.0e" % (q, T[:, qi].max(), tg.FLOOR[tg.TRAJ_Q[qi]]))
    for q, d in sorted(tg.measure_f64_deviation().items()):
        print("float64 against longdouble, %-5s: %.2e -> floor %.0e (guard module: measured %.1e, floor %.0e)"
              % (q, d, tc.next_power_of_ten(4.0 * d), tg.MEASURED[q], tg.FLOOR[q]))
    print("%d entries -> %s (%.0f s)" % (len(res), a.out, time.time() - t0))


if __name__ == "__main__":
    main()
