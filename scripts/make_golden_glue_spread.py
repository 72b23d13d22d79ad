#!/usr/bin/env python3
"""Writes tests/golden/glue_spread.npz: how far the reference answers of the helper-kernel tests (tests/glue_cases.py) are determined -- one
array per launch, tests/glue_guard.py's compute_* functions (float64 against longdouble, and SPREAD_DRAWS draws of a relative SPREAD_REL
perturbation of the inputs).  No GPU, no engine: tests/glue_ref.py and oracle/vel_ref.py alone.  About two minutes on one core; --jobs N
spreads the launches over N processes."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import glue_guard  # noqa: E402


def _one(key):
    return key, glue_guard.entries()[key]()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=1)
    ap.add_argument("--out", default=glue_guard.PATH)
    a = ap.parse_args()
    t0 = time.time()
    keys = sorted(glue_guard.entries())
    if a.jobs > 1:
        import multiprocessing as mp
        with mp.Pool(a.jobs) as pool:
            res = dict(pool.imap_unordered(_one, keys))
    else:
        res = dict(_one(k) for k in keys)
    np.savez_compressed(a.out, **{k: res[k] for k in keys})
    print("%d entries -> %s (%.0f s)" % (len(keys), a.out, time.time() - t0))


if __name__ == "__main__":
    main()
