"""What the mcq_mintime_* entries are held to.

The reference is the longdouble restatement (tests/mintime_ref.py).  guard = max(floor, 4 x spread), the project's rule (tests/glue_guard.py,
tests/fgauss_guard.py), per case and per quantity.

floor: a row of g (and every other output) is the end of a chain of at most about 60 float64 operations -- the model's sums, products and quotients,
with sin, cos, atan and exp accurate to 2 units in the last place -- in which every quotient's denominator is DECIDED, at least a factor 4 from
zero (tests/mintime_cases.py), so that one rounding is amplified by at most 4 on its way through a quotient.  60 roundings x 4 x 2 ulp, accumulated
linearly (the worst case), is 480 eps, taken as FLOOR_EPS = 512 eps relative to the largest magnitude of the quantity in the case (at least 1: the
rows' terms are scaled variables of order 1).  A derivative's chain is the value's chain differentiated -- about four times as many operations --
so the Jacobian, grad J and grad energy take 2048 eps relative to their largest entry.
spread: the largest deviation from the longdouble restatement of the float64 restatement in its two operation orders, written into
tests/golden/mintime/mintime_spread.npz by scripts/make_golden_mintime_spread.py (measure() below).  Integer outputs (layout, offsets, status) and
the bounds are compared exactly.  Nothing is measured against the code under test."""
import functools
import os

import numpy as np

import mintime_cases as mc
import mintime_ref as mr

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
FLOOR_EPS, FLOOR_EPS_DERIV = 512.0, 2048.0
COLL_POLY1D_EPS = 128.0      # numpy.poly1d's float64 collocation constants: the monomial coefficients' magnitudes sum to about 100 (test_mintime_ref.py)
PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mintime", "mintime_spread.npz")
VALUES = ("g", "J", "lap_time", "energy", "x_opt", "u_opt", "tf_opt", "dt_opt", "ec_opt", "ax_opt", "ay_opt")
DERIVS = ("blocks", "dJ", "dE")


@functools.lru_cache(maxsize=None)
def restated(name, dtype_name="longdouble", order=0):
    """The restatement of a case: computed once, shared, not to be changed."""
    option, prob = mc.cases()[name]
    return mr.nlp(prob, prob["w"], mc.OPTIONS[option], LD if dtype_name == "longdouble" else np.float64, order)


@functools.lru_cache(maxsize=None)
def restated_blocks(name, dtype_name="longdouble", order=0):
    option, prob = mc.cases()[name]
    b, dJ, dE = mr.blocks(prob, prob["w"], mc.OPTIONS[option], LD if dtype_name == "longdouble" else np.float64, order)
    return dict(blocks=b, dJ=dJ, dE=dE)


def measure(name, derivs=True):
    """{quantity: spread} of a case"""
    out = {}
    ld = restated(name)
    for q in VALUES:
        out[q] = max(float(np.max(np.abs(np.asarray(restated(name, "float64", o)[q]).astype(LD) - ld[q]))) for o in (0, 1))
    if derivs:
        ldb = restated_blocks(name)
        for q in DERIVS:
            out[q] = max(float(np.max(np.abs(restated_blocks(name, "float64", o)[q].astype(LD) - ldb[q]))) for o in (0, 1))
    return out


@functools.lru_cache(maxsize=None)
def fixture():
    z = np.load(PATH)
    return {k: float(z[k]) for k in z.files}


def scale(ref):
    return max(1.0, float(np.max(np.abs(np.asarray(ref, dtype=LD)))))


def floor(q, ref):
    return (FLOOR_EPS_DERIV if q in DERIVS or q.startswith("grad") else FLOOR_EPS) * EPS * scale(ref)


def guard(name, q, ref, spread_key=None):
    return max(floor(q, ref), 4.0 * fixture()["%s/%s" % (name, spread_key or q)])
