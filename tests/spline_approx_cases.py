"""The cases of the spline-approximation tests (tests/spline_approx_checks.py), read from tests/golden/spline_approx/cases.npz (written by
scripts/make_golden_spline_approx.py: raw track, FITPACK's recorded (t, c, k), stepsize_reg, spreads).  No scipy here.

What each case is for -- the smallest shapes at which the kernels can go wrong:
  rounded_rectangle, berlin_2018  the rows the recorded harness runs handed to prep_track (berlin: ten blocks of searches, waypoint 0 ends below 0)
  n3                              the smallest track
  n254, n255, n256                n + 1 = 255, 256, 257 searches: the search kernel's block of 256
  len252, len256, len260          4 ceil(total) length samples around a block: 251, 255 and 259 chords.  (The count is a multiple of 4, so
                                  these are the sizes next to 256.)
  deg1, deg5                      the other degrees (every other smoothing case is cubic)
  metre                           k = 1, s = 0 through points a metre apart, which are the raw rows: every distance 0 to rounding
  nk1024, nk1025                  3 nk doubles on both sides of the LDS budget, exactly (cubic, s = 0 through the raw rows)
  knots_lds, knots_l2             smoothing fits with little smoothing (s = 0.01 / 0.03): 966 knots staged in LDS, 1052 read through L2, and
                                  searches that reflect, expand and contract (every waypoint decided) through both instantiations
  nonmono                         two raw waypoints out of order: closest_t descends
In EVERY case waypoint 0 starts at x0 == 0 (second vertex 0.00025, reflected to -0.00025: below the spline's interval) and waypoint n at x0 == 1
(second vertex 1.05: beyond it).

EXACT_FIT cases: the raw rows lie ON the spline at their first guesses (f(x0) ~ 1e-13 m).  There the search's reflections are symmetric about
the best vertex and the comparison f(xr) < f(b) is a tie to third order at EVERY iteration (measured: gaps down to 1e-15), so the rule of
tests/spline_approx_guard.py calls every waypoint undecided -- but no decision can move the best vertex: every other point the search evaluates
is at least 1e-7 away in parameter, 1e-5 m on the line, and x0 stays the answer whichever way the ties fall.  So these cases are exempt from
the cap on undecided waypoints and held to MORE: closest_t == t_guess bitwise for every waypoint and every distance below the floor
(tests/test_spline_approx_ref.py asserts both of the reference first)."""
import functools
import os

import numpy as np

import spline_approx_guard as sg
import spline_approx_ref as sr

LD = np.longdouble
PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "spline_approx", "cases.npz")
CASES = ("rounded_rectangle", "berlin_2018", "n3", "n254", "n255", "n256", "len252", "len256", "len260", "deg1", "deg5", "metre", "nk1024",
         "nk1025", "knots_lds", "knots_l2", "nonmono")
EXACT_FIT = ("metre", "nk1024", "nk1025")
LENGTH_SAMPLES = dict(len252=252, len256=256, len260=260)
STAGED_IN_LDS = dict(nk1024=True, nk1025=False, knots_lds=True, knots_l2=False)      # 3 nk <= 3072 (MCQ_SPL_LDS of csrc/mcq_kernels.h)
BATCH = ("n3", "rounded_rectangle", "n255", "knots_l2", "nonmono")      # cubic cases of different n and nk (staged in LDS and not) for one launch
BAD_INPUT = 4


@functools.lru_cache(maxsize=None)
def _file():
    z = np.load(PATH)
    return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def case(name):
    z = _file()
    c = z[name + ".c"]
    return dict(name=name, track=z[name + ".track"], tck=(z[name + ".t"], (c[0], c[1]), int(z[name + ".k"])), step=float(z[name + ".step"]),
                spread=z[name + ".spread"])


@functools.lru_cache(maxsize=None)
def reference(name):
    """The float64 search of the reference (computed once, shared, not to be changed): dict(t, calls, gap, f0, x0, decided, m)."""
    c = case(name)
    s = sr.search(c["track"], c["tck"], np.float64)
    s["decided"] = np.ones(s["t"].shape, dtype=bool) if name in EXACT_FIT else sg.decided(c["track"], s["gap"])
    _, _, ratio, cnt = sr.length_and_count(c["track"], c["tck"], c["step"], LD)
    s["m"], s["ratio"] = cnt - 1, float(ratio)
    for v in s.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return s
