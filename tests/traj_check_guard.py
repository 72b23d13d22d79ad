"""What the trajectory / check_traj kernels are held to: guard = max(floor, 4 x spread) per row and quantity, the rule of tests/glue_guard.py.

spread: how far the REFERENCE's answer is determined -- the larger of (i) the float64 run of tests/traj_check_ref.py against its longdouble run and
(ii) the longdouble run's movement under SPREAD_DRAWS draws of a relative SPREAD_REL perturbation (tests/ring_guard.py) of its inputs.  Spreads are
written by scripts/make_golden_traj_check_spread.py into tests/golden/traj_check/traj_check_spread.npz (one [rows, quantities] array per family
and launch); the expected VALUES are computed live.  tests/test_traj_check_ref.py recomputes entries.

Floors.  Distances, boundary points, s and the length: the project's 1e-9 m (glue_guard.FLOOR['xy'] / ['el']); the curvature limit FLOOR['kappa'],
the speed limit FLOOR['vx'].  For ax, t, ay and a_tot the project had no floor: MEASURED below is the largest float64-against-longdouble
deviation of the reference over all cases (scripts/make_golden_traj_check_spread.py prints it, tests/test_traj_check_ref.py re-measures it),
and the floor is the next power of ten above four times it.  Counts (nb), statuses and flags are exact; the copied columns of a trajectory row
(x, y, psi, kappa, vx) are exact too."""
import functools
import os

import numpy as np

import glue_guard as gg
import traj_check_cases as tc
from ring_guard import SPREAD_DRAWS, SPREAD_REL, draw_rng

LD = np.longdouble
PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "traj_check", "traj_check_spread.npz")
MEASURED = dict(ax=5.91e-14, t=5.67e-13, ay=2.04e-14, a_tot=3.63e-14)   # largest float64-against-longdouble deviation over all cases
FLOOR = dict(dist=gg.FLOOR["xy"], bound=gg.FLOOR["xy"], s=gg.FLOOR["el"], length=gg.FLOOR["el"], kappa=gg.FLOOR["kappa"], vx=gg.FLOOR["vx"],
             ax=1e-12, t=1e-11, ay=1e-13, a_tot=1e-12)
BOUND_Q = ("dist", "dist", "bound")                                     # min_dists, min_dist, the raw boundaries
TRAJ_Q = ("s", "ax", "t", "length", "kappa", "ay", "ax", "ax", "a_tot", "vx")     # rows' s and ax, t, length, the six limits
dmax = gg.dmax
N_RUNS = 2 + SPREAD_DRAWS       # 0 = longdouble (THE reference), 1 = float64, 2 .. = longdouble on perturbed inputs


def guard(quantity, spread):
    return max(FLOOR[quantity], 4.0 * float(spread))


def _perturber(rng):
    def p(a):
        a = np.asarray(a, dtype=LD)
        return a * (LD(1) + LD(SPREAD_REL) * rng.standard_normal(a.shape).astype(LD))
    return p


def bound_deviations(a, b):
    """BOUND_Q of two results with the same sample counts."""
    return [dmax(a["min_dists"], b["min_dists"]), dmax(a["min_dist"], b["min_dist"]),
            max(dmax(a["bound_r"], b["bound_r"]), dmax(a["bound_l"], b["bound_l"]))]


def traj_deviations(a, b):
    """TRAJ_Q of two (trajectory dict, limits) pairs."""
    (Ta, la), (Tb, lb) = a, b
    return [dmax(Ta["traj"][:, 0], Tb["traj"][:, 0]), dmax(Ta["traj"][:, 6], Tb["traj"][:, 6]), dmax(Ta["t"], Tb["t"]),
            dmax(Ta["length"], Tb["length"])] + [dmax(la[q], lb[q]) for q in range(6)]


def bound_runs(family, launch, k):
    """The runs 1 .. of row k (run 0 is tc.bound_ref_cached)."""
    yield tc.bound_reference(launch, k, np.float64)
    for draw in range(SPREAD_DRAWS):
        yield tc.bound_reference(launch, k, LD, _perturber(draw_rng("traj_check/" + family, launch["name"], k, draw)))


def compute_bound_spread(family, launch):
    """[rows, 3] (BOUND_Q) of one launch of tc.bound_launches(family)."""
    out = np.zeros((len(launch["rows"]), len(BOUND_Q)))
    for k in range(len(launch["rows"])):
        r0 = tc.bound_ref_cached(family, launch["name"], k)
        for r in bound_runs(family, launch, k):
            assert r["nb"] == r0["nb"]
            out[k] = np.maximum(out[k], bound_deviations(r, r0))
    return out


def traj_runs(family, name, L, v):
    yield tc.traj_reference(L, v, np.float64)[:2]
    for draw in range(SPREAD_DRAWS):
        yield tc.traj_reference(L, v, LD, _perturber(draw_rng("traj_check/" + family, name, v, draw)))[:2]


def compute_traj_spread(family, name, L):
    """[variants, 10] (TRAJ_Q) of one trajectory launch."""
    out = np.zeros((len(L["track_of"]), len(TRAJ_Q)))
    for v in range(len(L["track_of"])):
        r0 = tc.traj_reference(L, v)[:2]
        for r in traj_runs(family, name, L, v):
            out[v] = np.maximum(out[v], traj_deviations(r, r0))
    return out


def traj_named_launches(family):
    """[(name, launch)]: the closed and the unclosed launch and the flag cases."""
    return [("closed", tc.traj_launch(family, True)), ("unclosed", tc.traj_launch(family, False))] + \
           [("flag_" + name, L) for name, L, _ in tc.flag_launches(family)]


def entries():
    """{key: function that recomputes the array} of everything traj_check_spread.npz must hold."""
    out = {}
    for f in tc.FAMILIES:
        for L in tc.bound_launches(f):
            out["%s/bound/%s" % (f, L["name"])] = functools.partial(compute_bound_spread, f, L)
        for name, L in traj_named_launches(f):
            out["%s/traj/%s" % (f, name)] = functools.partial(compute_traj_spread, f, name, L)
    return out


def measure_f64_deviation():
    """{ax, t, ay, a_tot}: the largest float64-against-longdouble deviation of the reference over every trajectory case."""
    worst = dict(ax=0.0, t=0.0, ay=0.0, a_tot=0.0)
    for f in tc.FAMILIES:
        for name, L in traj_named_launches(f):
            for v in range(len(L["track_of"])):
                d = traj_deviations(tc.traj_reference(L, v, np.float64)[:2], tc.traj_reference(L, v)[:2])
                worst["ax"] = max(worst["ax"], d[1], d[6], d[7])
                worst["t"] = max(worst["t"], d[2])
                worst["ay"] = max(worst["ay"], d[5])
                worst["a_tot"] = max(worst["a_tot"], d[8])
    return worst


_Z = None


def spread(k):
    global _Z
    if _Z is None:
        z = np.load(PATH)
        _Z = {q: z[q] for q in z.files}
    return _Z[k]
