"""The cases of the fit tests (tests/fit_checks.py), read from tests/golden/spline_fit/cases.npz (written by scripts/make_golden_spline_fit.py:
raw points, k, s, stepsize_prep, nest; scipy's t, c, u, fp, ier and stage probes; the longdouble restatement's c, fp, stage fp and points; spreads, of the
final fp and of every stage's, and margins).  No scipy here.  The raw rows of rounded_rectangle and berlin_2018 are those of tests/golden/spline_approx/cases.npz.

What each case is for -- the smallest shapes at which the kernel can go wrong:
  lobe_k{1..5}_s{0..5}       the 41-point two-lobe curve (LOBE_POINTS; with 40 it has a mirror axis and fpknot's intervals tie to rounding) at
                             s = 0, 0.05, 0.5, 5, 500, 1e6: interpolation for odd and even k (ier -1), the constant spline (ier -2),
                             everything between (ier 0), n from 2 k + 2 to 41 + 2 k + 1
  k1_mi4, k3_mi4, k3_mi5, k5_mi6, k5_mi7   the smallest closed counts scipy accepts (mi = k + 1, k + 2; k = 1 starts at the smallest track, n = 3),
                             each at s = 0 and s = 0.5: n7 below k + 1, B-splines that fold onto the same coefficient
                             (k3_mi4_s2 is also the case whose p search runs out of its 20 rounds: ier 3, the last spline is returned)
  GROWN_TO_NMAX              "knot growth that ends at nmax": the _s2 cases of the five above.  With s = 0.5 > 0 their knot loop adds knots until
                             n == nmax = mi + 2 k and takes fpclos's branch there: the knots are re-placed as for interpolation and the loop goes
                             round once more.  FITPACK does NOT return ier -1 from there -- the spline on nmax knots interpolates, fp < s, and it
                             goes on to the smoothing step (ier 0, or 3 on k3_mi4_s2); ier -1 out of the loop needs an s at rounding level of fp,
                             which no decided case can have.  So the branch is covered here and ier -1 by the s = 0 cases.
  nest_short, nest_exact     lobe_k3_s1 with nkmax below the n it needs (ier 1: the least-squares spline of that stage) and exactly n
  seam                       a sharp feature at the start point: knots in the first and the last interval, wrapped knots and border columns at work
  pts255, pts256, pts257     255, 256, 257 fitted points: the thread block's edge
  rs255, rs256, rs257        the re-sampling in front, sample counts on both sides of the block
  rs_below, rs_above         total length just below / above a multiple of stepsize_prep (RATIO_GAP is kept)
  lds558, lds559             cubic interpolation with 558 / 559 distinct coefficients: (2 k + 5) n7 = 6138 / 6149 doubles on both sides of
                             MCQ_FIT_LDS = 6144 (csrc/mcq_kernels.h)
  l2_smooth                  a smoothing fit whose knot rounds cross the LDS budget and whose p rounds run beyond it
  rounded_rectangle, berlin_2018   the reference's tracks with its k = 3, s = 10, stepsize_prep = 1 (316 / 2328 points, n = 27 / 78)"""
import functools
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "golden", "spline_fit", "cases.npz")
TRACKS = os.path.join(HERE, "golden", "spline_approx", "cases.npz")
LOBE_POINTS = 41
S_LIST = (0.0, 0.05, 0.5, 5.0, 500.0, 1e6)
LOBE = tuple("lobe_k%d_s%d" % (k, i) for k in (1, 2, 3, 4, 5) for i in range(len(S_LIST)))
BOTTOM = tuple("%s_s%d" % (nm, i) for nm in ("k1_mi4", "k3_mi4", "k3_mi5", "k5_mi6", "k5_mi7") for i in (0, 2))
GROWN_TO_NMAX = tuple(nm for nm in BOTTOM if nm.endswith("_s2"))
EDGES = ("nest_short", "nest_exact", "seam", "pts255", "pts256", "pts257", "rs255", "rs256", "rs257", "rs_below", "rs_above", "lds558", "lds559",
         "l2_smooth")
REFERENCE_TRACKS = ("rounded_rectangle", "berlin_2018")
CASES = LOBE + BOTTOM + EDGES + REFERENCE_TRACKS
IN_LDS = dict(lds558=True, lds559=False, l2_smooth=False)
BATCH = ("k3_mi5_s2", "lobe_k3_s2", "pts256", "seam", "k3_mi4_s2")       # cubic, s = 0.5, no re-sampling: ragged n, different n reached
BAD_INPUT = 4


@functools.lru_cache(maxsize=None)
def _file():
    z = np.load(PATH)
    return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def case(name):
    z = _file()
    g = lambda q: z[name + "." + q]      # noqa: E731
    raw = np.load(TRACKS)[name + ".track"][:, :2] if name in REFERENCE_TRACKS else g("raw")
    c = dict(name=name, raw=np.ascontiguousarray(raw), k=int(g("k")), s=float(g("s")), step=float(g("step")), nest=int(g("nest")) or None,
             t=g("t"), c=g("c"), u=g("u"), fp=float(g("fp")), ier=int(g("ier")), stage_n=g("stage_n"), stage_fp=g("stage_fp"),
             stage_t=g("stage_t"), stage_fp_ld=g("stage_fp_ld"), stage_spread=g("stage_spread"), c_ld=g("c_ld"), fp_ld=float(g("fp_ld")), pts=g("pts"), spread_c=float(g("spread")[0]),
             spread_fp=float(g("spread")[1]), margin=float(g("margin")), fp_agree=float(g("fp_agree")))
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def scipy_version():
    return str(_file()["scipy_version"])
