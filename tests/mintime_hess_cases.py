"""Cases for mcq_mintime_hess_device and mcq_mintime_hessvec_device (include/mcq.h "Hessian blocks").

Problems: tests/mintime_cases.py's cases() and LAUNCHES, unchanged -- N = 2 (both blocks hold one of the regularisation's two equal terms; interval 0's
slots 29 .. 32 are U_1), 3, 7 / 8, 63 / 64 / 65, 255 .. 257, 1025, every option at N = 5, "N3 all" / "N65 all".  The Hessian kernel's lane mapping adds no
edge of its own: a workgroup holds exactly ONE interval, so no interval straddles a wave or a workgroup, and its waves' shares are the same at every
N.  The H v kernel packs the entries of w 256 to a workgroup: its first edge (entry 256) falls inside interval 10, the next ones every 10.7
intervals -- N = 63 .. 1025 cross them; N = 2 (53 entries) and N = 257 (6173 = 24 workgroups and 29 entries) are its smallest and an uneven end.
Multipliers: seeded, lam_g uniform in [-1, 1], sigma in [0.5, 1.5], per case.
Localising cases at "N5 all": lam_g non-zero on ONE row kind at a time with sigma = 0 (KINDS), and lam_g = 0 with sigma = 1 ("objective"), where the
controls' part is the regularisation's constant cyclic stencil.
DECIDED, beyond mintime_cases' denominators: every safe-row case keeps |ax| >= AX_MARGIN at every path point, so that float64 and longdouble take
the same branch of max(ax, 0) / min(ax, 0) (tests/test_mintime_hess_ref.py asserts it, and that both signs occur)."""
import functools

import numpy as np

import mintime_cases as mc
import mintime_hess_ref as hr
import mintime_ref as mr

AX_MARGIN = 1e-3          # m/s^2
LOCAL_CASE = "N5 all"
KINDS = tuple(hr.ROW_KINDS) + ("energy",)
SAFE_CASES = ("N65 all", "N3 all", "N5 all", "N5 safe")


def ng_of(name):
    option, prob = mc.cases()[name]
    o = mc.OPTIONS[option]
    N = prob["h"].shape[0]
    return N * (27 + 2 * bool(o.get("safe_traj"))) + 4 * (N - 1) + 5 + bool(o.get("limit_energy"))


@functools.lru_cache(maxsize=None)
def multipliers(name):
    """(lam_g [ng], sigma) of a case: seeded by the case's place in the table.  Cached: shared, not to be changed."""
    rng = np.random.default_rng(424200 + sorted(mc.cases()).index(name))
    return rng.uniform(-1.0, 1.0, ng_of(name)), float(rng.uniform(0.5, 1.5))


@functools.lru_cache(maxsize=None)
def localising(kind):
    """(lam_g, sigma) at LOCAL_CASE with the multipliers of one row kind alone (every interval that has the row), or of the objective alone"""
    option, prob = mc.cases()[LOCAL_CASE]
    N, ng = prob["h"].shape[0], ng_of(LOCAL_CASE)
    lam = np.zeros(ng)
    if kind == "objective":
        return lam, 1.0
    rng = np.random.default_rng(515100 + KINDS.index(kind))
    if kind == "energy":
        lam[ng - 1] = rng.uniform(0.5, 1.0)
        return lam, 0.0
    for k in range(N):
        for r in hr.ROW_KINDS[kind]:
            i = mr.row_of(N, k, r, 1)
            if i >= 0:
                lam[i] = rng.uniform(0.5, 1.0) * rng.choice((-1.0, 1.0))
    return lam, 0.0


def setting(key):
    """a case key -- a case name, or "N5 all@kind" -- as (case name, option, problem, lam_g, sigma)"""
    name, _, kind = key.partition("@")
    option, prob = mc.cases()[name]
    lam, sigma = localising(kind) if kind else multipliers(name)
    return name, option, prob, lam, sigma


def keys():
    return sorted(mc.cases()) + ["%s@%s" % (LOCAL_CASE, k) for k in KINDS + ("objective",)]
