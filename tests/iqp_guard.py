"""What the IQP loop is held to: guard = max(floor, 4 x spread) per case and quantity -- the rule of tests/ring_guard.py and tests/glue_guard.py.

floor: 1e-8 for alpha (m), ring rows (m), normals and the curvature trace (1/m) -- what the suite already asserts for these quantities
  (tests/test_emu_kernels.py::test_iqp_device_resident_with_warm_started_passes, tests/test_harness.py's default flow); nobody picked a number here.
spread: how far the REFERENCE is determined -- the distance between the routes of tests/iqp_ref.py (dense Goldfarb-Idnani against
  trust-region-reflective least squares / CPU-B, and against its own perturbed draws where curvature rows are active), per quantity the largest
  over every round of the case: any round is an end state under some round
  cap, and the last one is where the error of the rounds before it has accumulated.
scripts/make_golden_iqp_spread.py writes the spreads into tests/golden/iqp_edges/iqp_spread.npz (a subfolder: tests/test_ring_guard.py takes every .npz
directly under tests/golden/ for a ring fixture); the expected values are computed live.  tests/test_iqp_ref.py recomputes a sample and caps every
guard at CAP x its floor: a case whose reference is undetermined beyond that leaves the table, it does not stay in behind a wide guard."""
import os

import numpy as np

import iqp_cases as ic
from ring_guard import SPREAD_DRAWS

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "iqp_edges", "iqp_spread.npz")
Q = ("alpha", "ring", "normals", "curv")
FLOOR = dict(alpha=1e-8, ring=1e-8, normals=1e-8, curv=1e-8)
CAP = 100.0


def dmax(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b))) if a.size else 0.0


def round_dev(a, b):
    """[4] (Q): one round of one run against the same round of another (dicts of tests/iqp_ref.py, or anything with its keys)."""
    return np.array([dmax(a["alpha"], b["alpha"]), dmax(a["reftrack"], b["reftrack"]), dmax(a["normvec"], b["normvec"]),
                     abs(float(a["curv_error_max"]) - float(b["curv_error_max"]))])


def compute_spread(name):
    """[4] (Q) of one case: the two routes must agree on the round count and on every ring's waypoint count."""
    r0 = ic.reference(name, "gi")
    out = np.zeros(len(Q))
    for route in routes(name):
        r1 = ic.reference(name, route)
        assert [r["n"] for r in r0] == [r["n"] for r in r1], (name, route, [r["n"] for r in r0], [r["n"] for r in r1])
        out = np.maximum(out, np.max([round_dev(a, b) for a, b in zip(r0, r1)], axis=0))
    return out


def routes(name):
    """The routes "gi" is compared with: the second route, and the SPREAD_DRAWS perturbed draws where a pass of the case has a curvature row active
    (there the second route has no solver of its own, tests/iqp_ref.py)."""
    kappa = any(r["kappa_active"] for r in ic.reference(name, "gi"))
    return ("second",) + (tuple(("draw", d) for d in range(SPREAD_DRAWS)) if kappa else ())


_Z = None


def spread(name):
    global _Z
    if _Z is None:
        z = np.load(PATH)
        _Z = {str(n): np.array(s) for n, s in zip(z["name"], z["spread"])}
    return _Z[name]


def guards(name):
    """{quantity: guard} of one case."""
    s = spread(name)
    return {q: max(FLOOR[q], 4.0 * float(s[k])) for k, q in enumerate(Q)}
