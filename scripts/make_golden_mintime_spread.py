"""Writes tests/golden/mintime/mintime_spread.npz: per case of tests/mintime_cases.py and per quantity, the largest deviation of the float64
restatement (tests/mintime_ref.py, both operation orders) from the longdouble restatement -- the spread of tests/mintime_guard.py.  CPU only; the
code under test is not involved."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import mintime_cases as mc  # noqa: E402
import mintime_guard as mg  # noqa: E402

out = {}
for name in sorted(mc.cases()):
    for q, v in mg.measure(name).items():
        out["%s/%s" % (name, q)] = np.float64(v)
    print(name, {q: "%.2e" % out["%s/%s" % (name, q)] for q in ("g", "J", "blocks")})
os.makedirs(os.path.dirname(mg.PATH), exist_ok=True)
np.savez(mg.PATH, **out)
print("wrote", mg.PATH, len(out), "entries")
