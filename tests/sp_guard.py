"""What a shortest-path solve is held to: guard = max(FLOOR, 4 x spread), the rule of tests/ring_guard.py, tests/open_ref.py and tests/glue_guard.py.

FLOOR = 1e-9 m: what tests/test_emu_kernels.py already asserts for this objective against the dense oracle.
spread (per case): how far the REFERENCE's alpha is determined -- the larger of (i) tests/sp_ref.py's float64 run against its longdouble run and
(ii) the longdouble run's movement under SPREAD_DRAWS draws of a relative SPREAD_REL perturbation of rows and normals.
scripts/make_golden_sp_spread.py writes the spreads into tests/golden/sp_edges/sp_spread.npz (a subfolder: tests/test_ring_guard.py takes every .npz
directly under tests/golden/ for a ring fixture); the expected alphas are computed live.  tests/test_sp_ref.py asserts that every stored spread is at
most FLOOR / 4 -- the guard IS the floor on every case -- and that every case's margin (distance of the optimum to the next change of its
working set) is at least MARGIN_MIN, so that comparing working sets row by row is legitimate.  A case that misses one gets another seed
(sp_cases.SEEDS)."""
import functools
import os

import numpy as np

import sp_cases as sc
import sp_ref
from ring_guard import SPREAD_DRAWS, SPREAD_REL, draw_rng

LD = np.longdouble
PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sp_edges", "sp_spread.npz")
FLOOR = 1e-9
MARGIN_MIN = 1e-6


@functools.lru_cache(maxsize=None)
def reference(name):
    """tests/sp_ref.py's longdouble solve of a case (of the case it shares its problem with); computed once, not to be written to."""
    name = sc.base_name(name)
    r = sp_ref.solve(*sc.case(name), dt=LD)
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


def _perturb(a, rng):
    a = np.asarray(a, dtype=LD)
    return a * (LD(1) + LD(SPREAD_REL) * rng.standard_normal(a.shape).astype(LD))


def compute_spread(name):
    """Of a case or of a derived input (sp_cases.derived_names)."""
    ref, nv, w_veh = sc.case(name)
    a0 = reference(name)["alpha"]
    s = float(np.max(np.abs(sp_ref.solve(ref, nv, w_veh, dt=np.float64)["alpha"].astype(LD) - a0)))
    for draw in range(SPREAD_DRAWS):
        rng = draw_rng("sp_edges/" + name, "alpha", sc.size(name), draw)
        a = sp_ref.solve(_perturb(ref, rng), _perturb(nv, rng), w_veh, dt=LD)["alpha"]
        s = max(s, float(np.max(np.abs(a - a0))))
    return s


_Z = None


def spread(name):
    global _Z
    if _Z is None:
        z = np.load(PATH)
        _Z = {str(n): float(s) for n, s in zip(z["name"], z["spread"])}
    return _Z[sc.base_name(name)]


def guard(name):
    return max(FLOOR, 4.0 * spread(name))
