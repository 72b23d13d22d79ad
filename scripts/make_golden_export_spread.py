#!/usr/bin/env python3
"""Writes tests/golden/export/export_spread.npz: how far the reference answers of the export tests (tests/export_cases.py) are determined -- per
ring one [3] array (s_ref, spline_lengths, spline_total): the largest deviation of the float64 restatements of tests/export_ref.front_variants
(other evaluation and summation orders) from the longdouble run.  No GPU, no engine: tests/export_ref.py alone.  Prints the largest spreads."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import export_guard as xg  # noqa: E402


def main():
    res = {k: xg.compute_spread(t) for k, t in sorted(xg.rings().items())}
    os.makedirs(os.path.dirname(xg.PATH), exist_ok=True)
    np.savez_compressed(xg.PATH, **res)
    worst = np.max(np.vstack(list(res.values())), axis=0)
    print("%d rings; largest spread: s_ref %.3e, lengths %.3e, total %.3e (floor %.0e) -> %s" % (len(res), *worst, xg.FLOOR, xg.PATH))


if __name__ == "__main__":
    main()
