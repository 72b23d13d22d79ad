"""What mcq_spline_fit_device is held to (tests/fit_checks.py), the rule of tests/spline_approx_guard.py.

Knots, nk and ier.  The interior knots FITPACK returns are bitwise elements of u, the wrapped ones one rounded +-1 away, so on the closed points
themselves (stepsize_prep <= 0) knots, nk and ier are held BITWISE to scipy's recording.  Behind the re-sampling nk and ier are exact and each
knot is held to half the smallest gap of the case's u (a wrong index misses by a whole gap), the points to the length guard.

Coefficients: max(FLOOR, 4 x min(spread, SPREAD_CAP)) against the LONGDOUBLE restatement (tests/fit_ref.py), spread = the largest of the float64
restatement against the longdouble one, the longdouble one's movement under ring_guard's perturbation draws of the points, and scipy against
the longdouble one; measured per case by scripts/make_golden_spline_fit.py and stored in tests/golden/spline_fit/cases.npz.
fp: 4 x its spread, measured the same way, and never less than fp_floor(): fp is a sum of m squared residuals, each the difference of two numbers
of the coordinates' size; 64 roundings of that size per residual is the noise an interpolating fit (fp ~ 1e-27 where scipy reports 0) consists of.
Independently of any spread |fp - s| <= 0.001 s wherever ier == 0: FITPACK's own stopping rule.

DECIDED.  The knot path and the p rounds hang on fp - s against +-acc, the truncation in npl1 and fpknot's largest interval against its
runner-up.  tests/fit_ref.py returns every such comparison; a case is decided if each relative margin exceeds max(MARGIN_FLOOR, 64 x the largest
relative float64-to-longdouble difference of that quantity over the case; fp's difference is taken relative to max(fp, s), the scale of what is
compared; a tie of fpknot that is exact in both number types AND lies between two sums that the same splits made of the
same interval's sum earlier in the round -- its two halves fpmax * j / m with the same j, or equal pieces of those halves, a scaling by a power of two counting with its exponent alone (tests/fit_ref.same_sum) -- is the same float
operations on the same number in every implementation, falls to the lower index everywhere and is no comparison of rounded quantities; any other
exact tie counts with margin 0).  MARGIN_FLOOR = 64 x FP_AGREE, and FP_AGREE = 2e-9 bounds the relative
difference of fp between scipy, the float64 and the longdouble restatement on every case whose search for p ended (the generator measures it,
tests/test_fit_ref.py asserts it; a case with ier 2 or 3 is held to 64 x its own measured difference instead): implementations that agree that well cannot decide a comparison with a larger margin differently.  Every committed case is
decided (UNDECIDED_CAP = 0); one that is not is replaced by a neighbour, never exempted."""
import numpy as np

from ring_guard import SPREAD_DRAWS, SPREAD_REL, draw_rng       # noqa: F401

LD = np.longdouble
FLOOR = 1e-9            # m: the project's floor for lengths (tests/spline_approx_guard.py)
SPREAD_CAP = 1e-8
EPS = float(np.finfo(np.float64).eps)
FP_AGREE = 2e-9
MARGIN_FLOOR = 64.0 * FP_AGREE
UNDECIDED_CAP = 0
RATIO_GAP = 1e-9
FP_STOP = 0.001


def guard(spread):
    return max(FLOOR, 4.0 * min(float(spread), SPREAD_CAP))


def fp_floor(m1, scale):
    return float(m1) * (64.0 * EPS * float(scale)) ** 2


def fp_guard(spread, m1, scale):
    return max(4.0 * float(spread), fp_floor(m1, scale))


def dmax(a, b):
    return float(np.max(np.abs(np.asarray(a, dtype=LD) - np.asarray(b, dtype=LD))))


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return np.inf
    if a.size == 0:
        return 0.0
    den = np.maximum(np.abs(b), np.finfo(np.float64).tiny)
    return float(np.max(np.abs(a - b) / den))


def margins(m64, mld):
    """(smallest margin / threshold over the case, dict per kind of (smallest relative margin, threshold)); decided iff the first is > 1."""
    out, worst = {}, np.inf
    for kind in ("acc", "npl1", "knot"):
        a, b = np.asarray(m64[kind], dtype=np.float64), np.asarray(mld[kind], dtype=np.float64)
        if a.shape != b.shape:
            return 0.0, {kind: (0.0, np.inf)}
        if a.size == 0:
            continue
        if kind == "acc":
            fp, s, acc = a[:, 0], a[:, 1], a[:, 2]
            live = s > 0
            mar = np.minimum(np.abs(fp - s - acc), np.abs(fp - s + acc))[live] / np.maximum(fp, s)[live]
            rel = float(np.max(np.abs(a[live, 0] - b[live, 0]) / np.maximum(fp, s)[live])) if mar.size else 0.0      # (fp - s is what is compared)
        elif kind == "npl1":
            mar = a[:, 1] / np.maximum(np.abs(a[:, 0]), 1.0)
            rel = _rel(a[:, 0], b[:, 0])
        else:
            # an EXACT tie in float64 and in longdouble is structural (fpknot gives both halves of a split interval fpmax * j / m with the same
            # j): every implementation forms the same two numbers, and FITPACK's scan keeps the lower index.  Only such a tie is taken out:
            # tests/fit_ref.py marks (third entry) the comparisons whose two sides came from the same interval of the round by the same
            # splits (j, m), and an exact tie anywhere else stays in with margin 0, which leaves the case undecided
            live = ~((a[:, 0] == a[:, 1]) & (b[:, 0] == b[:, 1]) & (a[:, 2] == 1.0) & (b[:, 2] == 1.0))
            mar = ((a[:, 0] - a[:, 1]) / a[:, 0])[live]
            rel = _rel(a[live, 0], b[live, 0])
        if mar.size == 0:
            continue
        thr = max(MARGIN_FLOOR, 64.0 * rel)
        out[kind] = (float(mar.min()), thr)
        worst = min(worst, float(mar.min()) / thr)
    return worst, out
