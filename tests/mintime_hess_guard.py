"""What mcq_mintime_hess_device and mcq_mintime_hessvec_device are held to.

The reference is the longdouble restatement (tests/mintime_hess_ref.py).  guard = max(floor, 4 x spread), the project's rule (tests/mintime_guard.py).

floor, by mintime_guard's counting: a value is the end of a chain of about 60 float64 operations in which every quotient's denominator is DECIDED (a
rounding is amplified by at most 4), with sin, cos, atan and exp to 2 units in the last place: 60 x 4 x 2 = 480, taken as 512 eps.  A derivative's
chain is the value's chain differentiated, about four times as many operations: 2048 eps.  A second derivative's chain is the first's differentiated
again, four times as many once more: FLOOR_EPS_HESS = 8192 eps, relative to the largest entry of the case's blocks (at least 1).  The multipliers
(|lam_g| <= 1, sigma <= 1.5) weigh at most 16 rows into an entry; their sum's roundings are a few eps of the same scale and lie inside the count.
spread: the largest deviation from the longdouble restatement of the float64 restatement in its two operation orders, per case key of
tests/mintime_hess_cases.py, written into tests/golden/mintime/mintime_hess_spread.npz by scripts/make_golden_mintime_hess_spread.py (measure()
below).  Nothing is measured against the code under test.
H v: an entry of y is a sum of at most 66 products (two blocks' rows of 33).  Each product carries the block entry's error times |v| -- at most
66 x guard(blocks) x max |v| in all -- and the 66 products and 66 additions each round a number of at most 66 x max |H| x max |v|: 132 x 66 eps of
that.  guard_y = 66 max|v| (guard(blocks) + 132 eps max|H|), against the longdouble product of the longdouble blocks."""
import functools
import os

import numpy as np

import mintime_cases as mc
import mintime_hess_cases as hc
import mintime_hess_ref as hr

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
FLOOR_EPS_HESS = 8192.0
PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mintime", "mintime_hess_spread.npz")


@functools.lru_cache(maxsize=None)
def restated(key, dtype_name="longdouble", order=0):
    """The restated blocks [N, 33, 33] of a case key: computed once, shared, not to be changed."""
    name, option, prob, lam, sigma = hc.setting(key)
    return hr.blocks(prob, prob["w"], mc.OPTIONS[option], lam, sigma, LD if dtype_name == "longdouble" else np.float64, order)


def measure(key):
    ld = restated(key)
    return max(float(np.max(np.abs(restated(key, "float64", o).astype(LD) - ld))) for o in (0, 1))


@functools.lru_cache(maxsize=None)
def fixture():
    z = np.load(PATH)
    return {k: float(z[k]) for k in z.files}


def scale(ref):
    return max(1.0, float(np.max(np.abs(np.asarray(ref, dtype=LD)))))


def floor(ref):
    return FLOOR_EPS_HESS * EPS * scale(ref)


def guard(key, ref=None):
    ref = restated(key) if ref is None else ref
    return max(floor(ref), 4.0 * fixture()[key + "/hblocks"])


def guard_y(block_guard, ref_blocks, v):
    vmax = float(np.max(np.abs(v)))
    return 66.0 * vmax * (block_guard + 132.0 * EPS * float(np.max(np.abs(np.asarray(ref_blocks, dtype=LD)))))
