#!/usr/bin/env python3
"""Writes tests/golden/race_open/race_open_spread.npz: how far the reference answers of the open-chain raceline tests (tests/race_open_cases.py)
are determined -- one [rows, 4] array per family and launch, tests/race_open_guard.py's compute_spread (float64 against longdouble, and
SPREAD_DRAWS draws of a relative SPREAD_REL perturbation of rows, normals, alpha and the two headings).  No GPU, no engine:
tests/race_open_ref.py alone.  Prints the largest spread per quantity, and the float64-against-longdouble part of it.  --jobs N spreads the
families over N processes."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import race_open_cases as oc  # noqa: E402
import race_open_guard as og  # noqa: E402
import race_open_ref as ror  # noqa: E402


def _family(family):
    """Every launch of one family in one process: the stepsize-independent half of the reference is cached per (arc, run)."""
    out, f64 = {}, np.zeros(4)
    for L in oc.launches(family):
        out[og.key(family, L)] = og.compute_spread(family, L)
        for n in L[1]:
            f64 = np.maximum(f64, og.deviations(ror.stations(og.front(family, n, 1), L[2]), og.reference(family, n, L[2])))
    return out, f64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=1)
    ap.add_argument("--out", default=og.PATH)
    a = ap.parse_args()
    t0 = time.time()
    fams = list(oc.FAMILIES)
    if a.jobs > 1:
        import multiprocessing as mp
        with mp.Pool(min(a.jobs, len(fams))) as pool:
            parts = pool.map(_family, fams)
    else:
        parts = [_family(f) for f in fams]
    res = {}
    for p, _ in parts:
        res.update(p)
    assert sorted(res) == sorted(og.entries())
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    np.savez_compressed(a.out, **{k: res[k] for k in sorted(res)})
    S = np.vstack([res[k] for k in sorted(res)])
    f64 = np.max([q for _, q in parts], axis=0)
    for qi, q in enumerate(og.RACE_Q):
        print("%-5s largest spread %.3e (float64 against longdouble alone %.3e), floor %.0e" % (q, S[:, qi].max(), f64[qi], og.FLOOR[q]))
    print("%d entries -> %s (%.0f s)" % (len(res), a.out, time.time() - t0))


if __name__ == "__main__":
    main()
