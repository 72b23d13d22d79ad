"""Writes tests/golden/mintime/mintime_hess_spread.npz: per case key of tests/mintime_hess_cases.py, the largest deviation of the float64
second-order restatement (tests/mintime_hess_ref.py, both operation orders) from the longdouble one -- the spread of tests/mintime_hess_guard.py.
CPU only; the code under test is not involved."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import mintime_hess_cases as hc  # noqa: E402
import mintime_hess_guard as hg  # noqa: E402

out = {}
for key in hc.keys():
    out[key + "/hblocks"] = np.float64(hg.measure(key))
    print("%-24s spread %.2e  largest entry %.2e" % (key, out[key + "/hblocks"], hg.scale(hg.restated(key))))
np.savez(hg.PATH, **out)
print("wrote", hg.PATH, len(out), "entries")
