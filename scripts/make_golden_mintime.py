"""Writes tests/golden/mintime/export_n8.npz: the bytes (and SHA-256) of the seven files the REFERENCE's own export_mintime_solution writes for the
N = 8 case of tests/mintime_cases.py, from the longdouble restatement's arrays (tests/mintime_ref.py) rounded to float64 and post-processed as the
reference does, with seeded multipliers.  Data only; run at generation time with the reference checkout's path as the one argument:
    python scripts/make_golden_mintime.py /path/to/reference"""
import hashlib
import importlib.util
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import mintime_cases as mc  # noqa: E402
import mintime_guard as mg  # noqa: E402

spec = importlib.util.spec_from_file_location("ref_export", os.path.join(sys.argv[1], "opt_mintime_traj", "src", "export_mintime_solution.py"))
ref_export = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ref_export)

name = "N8"
p = mc.cases()[name][1]
r = {k: np.asarray(v, dtype=np.float64) for k, v in mg.restated(name).items()}
N = 8
last_first = np.arange(-1, N) % N          # the lap closes: row 0 is the last interval's
tf, ax, ay = r["tf_opt"][last_first], r["ax_opt"][last_first], r["ay_opt"][last_first]
t = np.zeros(N + 1)
t[1:] = np.cumsum(r["dt_opt"])
rng = np.random.default_rng(8)
lam_x, lam_g = rng.normal(size=5 + 24 * N), rng.normal(size=r["g"].shape[0])
out = dict(lam_x0=lam_x, lam_g0=lam_g)
with tempfile.TemporaryDirectory() as d:
    ref_export.export_mintime_solution(d, {"pwr_params_mintime": {"pwr_behavior": False}}, np.append(0.0, np.cumsum(p["h"])), t, r["x_opt"], r["u_opt"],
                                       tf, ax, ay, np.sqrt(ax ** 2 + ay ** 2), p["w"], lam_x, lam_g)
    for f in ("states.csv", "controls.csv", "tire_forces.csv", "accelerations.csv", "w0.csv", "lam_x0.csv", "lam_g0.csv"):
        b = open(os.path.join(d, f), "rb").read()
        out[f] = np.frombuffer(b, dtype=np.uint8)
        out[f + ".sha256"] = np.array(hashlib.sha256(b).hexdigest())
        print(f, len(b), out[f + ".sha256"])
np.savez(os.path.join(ROOT, "tests", "golden", "mintime", "export_n8.npz"), **out)
