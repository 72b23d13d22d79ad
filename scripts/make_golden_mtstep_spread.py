"""Writes tests/golden/mintime/mtstep_spread.npz: per case key of tests/mtstep_cases.py and refine count, the largest deviation -- relative to
max |x_ref| -- of the float64 restatement of the static-order LDL^T with that many float64 refinements, in two stage orders, from the longdouble
reference (tests/mtstep_guard.py measure()).  CPU only; nothing here runs the code under test.  Usage: python scripts/make_golden_mtstep_spread.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mtstep_cases as sc      # noqa: E402
import mtstep_guard as sg      # noqa: E402


def main():
    out = {}
    for key in sc.all_keys():
        for r in (0, 1, 2) if key in sc.REFINE_KEYS else (2,):
            out["%s/r%d" % (key, r)] = sg.measure(key, r)
            print("%-20s refine %d  spread %.3e  floor %.3e" % (key, r, out["%s/r%d" % (key, r)], sg.floor(key)), flush=True)
    os.makedirs(os.path.dirname(sg.PATH), exist_ok=True)
    np.savez(sg.PATH, **out)


if __name__ == "__main__":
    main()
