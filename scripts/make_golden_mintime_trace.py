"""Writes tests/golden/mintime/trace.npz: per case of tests/mintime_trace_cases.py, the engine-side problem and what the reference's own
opt_mintime.py builds at the case's w -- traced by oracle/mintime_trace.py on the numeric CasADi stand-in, in longdouble, rounded once to float64
(the bounds: from the float64 run) -- with the ingredients of the guards of tests/mintime_trace_checks.py, which come from the restatements alone.
Recorded numbers only.  CPU only; needs the reference tree ($MCQ_REFERENCE_DIR); the code under test is not involved."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import mintime_trace_cases as tc  # noqa: E402
import mintime_trace_checks as tk  # noqa: E402

out = {}
for name in tc.TABLE:
    fix = tk.live(name)["fix"]
    out.update({"%s/%s" % (name, k): np.asarray(v) for k, v in fix.items()})
    print("%-10s %3d arrays, %7d bytes" % (name, len(fix), sum(np.asarray(v).nbytes for v in fix.values())))
np.savez(tc.FIXTURE, **out)
print("wrote", tc.FIXTURE, len(out), "arrays,", os.path.getsize(tc.FIXTURE), "bytes")
