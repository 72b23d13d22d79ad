"""Cases of the traced reference NLP (oracle/mintime_trace.py; tests/test_mintime_trace_ref.py holds tests/mintime_ref.py to them, and
tests/mintime_trace_checks.py the kernels to their recorded results in tests/golden/mintime/trace.npz).

Interval counts N = 2 (one actuator row; the regularisation wraps between two intervals), 3, 8 (the Jacobian kernel's first interval across two
workgroups) and one N = 65 (the evaluation kernel's first workgroup edge; values only).  Options: plain at every N; safe, energy, linear and gauss1
alone at N = 3; everything on at N = 3, 8 and 65; one plain case of non-regular sampling, 8 kept points of 20, so that h is non-uniform and the
lap closes at the original point count.  w* is mintime_cases.random_w and the 40 parameters mintime_cases.vary: no two of them equal.

The engine's problem of a case is made from the SAME nested dictionary that the reference receives, by mintime.pars_from_ini and
mintime.problem_from_track: those two mappings are under test with the kernels.

Conditions (tests/test_mintime_trace_ref.py asserts them): every case is DECIDED (mintime_checks.undecided), keeps |ax| >= 1e-3 m/s^2 at every path
point where safe_traj is on, and across the cases both signs of ax occur.  A seed that fails one is replaced by the next (SEEDS)."""
import functools
import os
import sys

import numpy as np

import mintime_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from global_racetrajectory_optimization_amd import mintime  # noqa: E402
from oracle import mintime_trace as mt  # noqa: E402

FIXTURE = os.path.join(mc.GOLDEN, "mintime", "trace.npz")
# name: (N, option of mintime_cases.OPTIONS, non-regular sampling)
TABLE = {"N2 plain": (2, "plain", False), "N3 plain": (3, "plain", False), "N8 plain": (8, "plain", False), "N8 nonreg": (8, "plain", True),
         "N3 safe": (3, "safe", False), "N3 energy": (3, "energy", False), "N3 linear": (3, "linear", False), "N3 gauss1": (3, "gauss1", False),
         "N3 all": (3, "all", False), "N8 all": (8, "all", False), "N65 all": (65, "all", False)}
SEEDS = {name: 0 for name in TABLE}
VALUES_ONLY = ("N65 all",)
SMALL = tuple(n for n in TABLE if n not in VALUES_ONLY)
SENSITIVITY_CASE = "N3 all"            # every option on: each of the 40 parameters is read
NONREG_ORIG = 20
# launches of the kernel tests: the cases of equal options, ragged under a wider nmax
LAUNCHES = {"plain": (("N2 plain", "N3 plain", "N8 plain", "N8 nonreg"), 9), "safe": (("N3 safe",), 4), "energy": (("N3 energy",), 4),
            "linear": (("N3 linear",), 4), "gauss1": (("N3 gauss1",), 4), "all": (("N3 all", "N8 all"), 10)}
SIGMAS = (1.0, 0.3)
AX_MARGIN = 1e-3


def options(name):
    return dict(mc.OPTIONS[TABLE[name][1]])


@functools.lru_cache(maxsize=None)
def setup(name):
    """What the runner needs for one case (oracle/mintime_trace.run): seeded track data, parameters, w*, weights, multipliers for the export."""
    N, option, nonreg = TABLE[name]
    opts = options(name)
    seed = SEEDS[name]
    rng = np.random.default_rng(90000 + 1009 * sorted(TABLE).index(name) + seed)
    flat = mc.vary(500 + 17 * sorted(TABLE).index(name) + seed)
    # vary() moves 7 of the 40 and leaves c_roll == penalty_F: every parameter gets 2 % of its own here, so that no two are equal
    flat = {k: float(v * (1.0 + 0.02 * rng.uniform(-1, 1))) for k, v in flat.items()}
    assert len(set(flat.values())) == 40, "two of the 40 parameters are equal"
    n = NONREG_ORIG if nonreg else N
    stepsize = float(rng.uniform(2.5, 3.5))
    ang = 2 * np.pi * np.arange(n) / n
    radius = n * stepsize / (2 * np.pi)
    reftrack = np.column_stack((radius * np.cos(ang), radius * np.sin(ang), rng.uniform(3.5, 6.0, n), rng.uniform(3.5, 6.0, n)))
    kap = 0.02 * np.sin(np.linspace(0.0, 2 * np.pi, N, endpoint=False) + rng.uniform(0, 6)) + rng.uniform(-0.003, 0.003, N)
    out = dict(flat=flat, opts=opts, stepsize=stepsize, reftrack=reftrack, kappa=kap, sampled=None, discr_points=None)
    if nonreg:
        keep = np.concatenate(([0], np.sort(rng.choice(np.arange(1, n), N - 1, replace=False))))
        out.update(sampled=reftrack[keep], discr_points=keep)
    wm, cd = mc.friction_weights(rng, N, opts)
    out.update(w_mue=wm, center_dist=cd, w=mc.random_w(rng, N))
    ng = mintime.g_rows(N, opts.get("safe_traj"), opts.get("limit_energy"))[1]
    out.update(lam_x=rng.uniform(-1, 1, 5 + 24 * N), lam_g=rng.uniform(-1, 1, ng))
    return out


@functools.lru_cache(maxsize=None)
def problem(name):
    """(the engine's problem, its option keywords) of a case: from the reference's nested dictionary through mintime.pars_from_ini, and from the
    track the NLP runs on through mintime.problem_from_track.  Cached: shared, not to be changed."""
    s = setup(name)
    nonreg = s["sampled"] is not None
    block, opts = mintime.pars_from_ini(mt.nested_pars(s["flat"], s["opts"], s["stepsize"], nonreg))
    if nonreg:
        prob = mintime.problem_from_track(s["sampled"], s["kappa"], s["stepsize"], discr_points=s["discr_points"], no_points_orig=s["reftrack"].shape[0])
    else:
        prob = mintime.problem_from_track(s["reftrack"], s["kappa"], s["stepsize"])
    prob.update(pars=block, w=s["w"], w_mue=s["w_mue"], center_dist=s["center_dist"])
    return prob, opts


@functools.lru_cache(maxsize=None)
def multipliers(name):
    """(lam_g [ng], sigmas) of a case's Lagrangian: mintime_hess_cases.multipliers' recipe (lam_g uniform in [-1, 1], seeded by the case's place in
    the table) with the two sigmas every case is held at"""
    prob, opts = problem(name)
    N = prob["h"].shape[0]
    ng = mintime.g_rows(N, opts["safe_traj"], opts["limit_energy"])[1]
    return np.random.default_rng(424200 + 100 + sorted(TABLE).index(name)).uniform(-1.0, 1.0, ng), SIGMAS


@functools.lru_cache(maxsize=None)
def directions(name):
    """three seeded directions v [3, nw], entries uniform in [-1, 1]"""
    nw = setup(name)["w"].shape[0]
    return np.random.default_rng(616100 + sorted(TABLE).index(name)).uniform(-1.0, 1.0, (3, nw))


def pairs(name, ax):
    """The (u, v) of the second derivatives [P, nw] each, with their labels: three seeded pairs; unit pairs on the wrap entries (U_N-1 with U_0: the
    steer angles, and a drive with a brake force); an actuator entry X_k+1 with U_k-1 (k = 1: the speed of X_2 with the steer angle of U_0); with
    safe_traj on, the drive force of an interval with ax > 0 against itself (row 31's branch) and of one with ax < 0 (row 32's).  ax: the path
    points' accelerations, from the trace or the fixture."""
    N, nw = TABLE[name][0], setup(name)["w"].shape[0]
    rng = np.random.default_rng(717100 + sorted(TABLE).index(name))
    U, V, labels = list(rng.uniform(-1.0, 1.0, (3, nw))), list(rng.uniform(-1.0, 1.0, (3, nw))), ["seeded 0", "seeded 1", "seeded 2"]

    def unit(i):
        e = np.zeros(nw)
        e[i] = 1.0
        return e
    u_last, u_0 = 24 * (N - 1) + 5, 5
    for (a, b, what) in ((u_last, u_0, "wrap delta"), (u_last + 1, u_0 + 2, "wrap drive-brake"), (24 * 2, u_0, "actuator X_2 U_0")):
        U.append(unit(a)), V.append(unit(b)), labels.append(what)
    if options(name).get("safe_traj"):
        for sign, what in ((1, "safe ax > 0"), (-1, "safe ax < 0")):
            ks = np.flatnonzero(np.sign(ax) == sign)
            if ks.size:
                i = 24 * int(ks[0]) + 6
                U.append(unit(i)), V.append(unit(i)), labels.append(what)
    return np.array(U), np.array(V), labels
