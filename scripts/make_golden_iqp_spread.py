#!/usr/bin/env python3
"""Writes tests/golden/iqp_edges/iqp_spread.npz: per case of tests/iqp_cases.py the distance between the two routes of tests/iqp_ref.py (alpha, ring
rows, normals, curvature error; the largest over the case's rounds), from which tests/iqp_guard.py derives the guards of the IQP edges suite.
CPU only, a few minutes.  Usage: scripts/make_golden_iqp_spread.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import iqp_cases as ic          # noqa: E402
import iqp_guard as ig          # noqa: E402


def main():
    names = sorted(ic.CASES)
    S = np.zeros((len(names), len(ig.Q)))
    for k, name in enumerate(names):
        S[k] = ig.compute_spread(name)
        print("%-26s rounds %2d  " % (name, len(ic.reference(name))) + "  ".join("%s %.2e" % (q, s) for q, s in zip(ig.Q, S[k])), flush=True)
    os.makedirs(os.path.dirname(ig.PATH), exist_ok=True)
    np.savez(ig.PATH, name=np.array(names), spread=S)
    g = np.maximum(4.0 * S, [ig.FLOOR[q] for q in ig.Q])
    print("guards above their floor: %d of %d" % (int(np.sum(g > [ig.FLOOR[q] for q in ig.Q])), g.size))


if __name__ == "__main__":
    main()
