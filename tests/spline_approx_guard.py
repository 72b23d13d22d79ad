"""What mcq_spline_approx_device is held to (tests/spline_approx_checks.py), the rule of tests/traj_check_guard.py.

closest_t.  A waypoint is DECIDED if the smallest |f1 - f2| over every comparison the float64 reference's search made (tests/spline_approx_ref.py)
exceeds 64 eps max(|x|, |y|) of the track: two evaluations of f = |s(t) - p| differ between implementations by a few roundings of quantities of
the coordinates' size, so no decision of such a waypoint can fall the other way, and given the decisions the parameter is a rounding-exact function
of x0.  Decided waypoints return the reference's closest_t BITWISE; the others are held to finiteness and dist <= f(t_guess) (fmin never returns a
point worse than its start).  At most UNDECIDED_CAP of a case's waypoints may be undecided (tests/test_spline_approx_ref.py asserts it).

Everything behind the search is compared with the LONGDOUBLE finish of the reference on the closest_t under test, each quantity to
max(FLOOR, 4 x spread): spread = the larger of the float64 finish against the longdouble one and the longdouble finish's movement under
SPREAD_DRAWS draws of a relative SPREAD_REL perturbation of the raw rows, knots and coefficients, stored per case in
tests/golden/spline_approx/cases.npz by scripts/make_golden_spline_approx.py and capped at SPREAD_CAP, so that no guard exceeds 4e-8 m: the
smallest structural mistake (a neighbouring interval, a flipped side of a real deviation, a row off by one) moves a quantity by far more.
m, statuses, nonmono and the inflation flags are exact; every case keeps len_smoothed / stepsize_reg at least RATIO_GAP from an integer."""
import numpy as np

import spline_approx_ref as sr
from ring_guard import SPREAD_DRAWS, SPREAD_REL, draw_rng

LD = np.longdouble
Q = ("xy", "w", "dist", "dev")      # path rows, widths, distances to the closest points, (mean, max) deviation
FLOOR = 1e-9                        # m: the project's floor for lengths (tests/glue_guard.py)
SPREAD_CAP = 1e-8
UNDECIDED_CAP = 0.01
RATIO_GAP = 1e-9
EPS = float(np.finfo(np.float64).eps)


def guard(spread):
    return max(FLOOR, 4.0 * min(float(spread), SPREAD_CAP))


def dmax(a, b):
    return float(np.max(np.abs(np.asarray(a, dtype=LD) - np.asarray(b, dtype=LD))))


def decided(track, gap):
    scale = float(np.max(np.abs(np.asarray(track, dtype=np.float64)[:, :2])))
    return np.asarray(gap) > 64.0 * EPS * scale


def deviations(a, b):
    """Q of two finishes with the same row count."""
    return [dmax(a["rows"][:, :2], b["rows"][:, :2]), dmax(a["rows"][:, 2:], b["rows"][:, 2:]), dmax(a["dists"], b["dists"]),
            max(dmax(a["dev"][0], b["dev"][0]), dmax(a["dev"][1], b["dev"][1]))]


def _perturber(rng):
    def p(a):
        a = np.asarray(a, dtype=LD)
        return a * (LD(1) + LD(SPREAD_REL) * rng.standard_normal(a.shape).astype(LD))
    return p


def compute_spread(track, tck, step, name="case"):
    """(spread [4] per Q, dict(m, undecided, ratio_gap)) of one case, on the float64 reference's closest_t."""
    s = sr.search(track, tck, np.float64)
    r0 = sr.finish(track, tck, step, s["t"], LD)
    out = np.asarray(deviations(sr.finish(track, tck, step, s["t"], np.float64, npts=r0["m"] + 1), r0))
    for draw in range(SPREAD_DRAWS):
        p = _perturber(draw_rng("spline_approx/" + name, "finish", 0, draw))
        t, c, k = tck
        out = np.maximum(out, deviations(sr.finish(p(track), (p(t), (p(c[0]), p(c[1])), k), step, s["t"], LD, npts=r0["m"] + 1), r0))
    ratio = float(r0["ratio"])
    return out, dict(m=r0["m"], undecided=int(np.sum(~decided(track, s["gap"]))), ratio_gap=abs(ratio - round(ratio)))
