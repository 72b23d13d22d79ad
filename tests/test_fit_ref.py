"""The restatement of FITPACK's periodic smoothing fit (tests/fit_ref.py) against scipy's recording (tests/golden/spline_fit/cases.npz, written
by scripts/make_golden_spline_fit.py): knots and nk exact stage by stage, ier exact, coefficients and fp within the guards of
tests/fit_guard.py; every committed case decided; and, where scipy is installed, scipy itself against the recording."""
import numpy as np
import pytest

import fit_cases as fc
import fit_guard as fg
import fit_ref as fr

LD = np.longdouble
SLOW_LD = ("berlin_2018", "l2_smooth", "lds558", "lds559")      # (the longdouble restatement of these takes Python tens of seconds: the generator ran it)


@pytest.mark.parametrize("name", fc.CASES)
def test_restatement_against_the_recording(name):
    c = fc.case(name)
    stages = []
    r = fr.fit_track(c["raw"], c["k"], c["s"], c["step"], c["nest"], np.float64, stages)
    assert r["n"] == c["t"].shape[0] and r["ier"] == c["ier"]
    assert np.array_equal(r["t"], c["t"]) and np.array_equal(r["u"], c["u"]), "knots or parameter differ from scipy's"
    assert [s[0] for s in stages] == list(c["stage_n"])
    off = 0
    for (n, t, fp), fps, fld, spread in zip(stages, c["stage_fp"], c["stage_fp_ld"], c["stage_spread"]):
        assert np.array_equal(t, c["stage_t"][off:off + n]), "stage with %d knots" % n
        off += n
        # each stage's fp against the longdouble one's under 4 x the spread measured for THAT stage (fp falls by orders of magnitude along the
        # knot rounds, so the final fp's spread says nothing about an early stage's)
        gs = fg.fp_guard(spread, c["u"].shape[0] - 1, np.max(np.abs(c["pts"])))
        assert abs(float(fp) - fld) <= gs, "stage with %d knots: fp %r, longdouble %r, guard %.3e" % (n, fp, fld, gs)
        if 0.0 < c["s"] and fp - c["s"] < 0.0:
            continue        # (the stage whose fp is below s: scipy's probe goes on to the smoothing spline and returns that one's fp)
        assert abs(fps - fld) <= gs, "stage with %d knots: scipy's fp %r, longdouble %r, guard %.3e" % (n, fps, fld, gs)
    assert off == c["stage_t"].shape[0]
    assert fg.dmax(r["c"], c["c_ld"]) <= fg.guard(c["spread_c"]) and fg.dmax(c["c"], c["c_ld"]) <= fg.guard(c["spread_c"])
    gf = fg.fp_guard(c["spread_fp"], c["u"].shape[0] - 1, np.max(np.abs(c["pts"])))
    assert abs(float(r["fp"]) - c["fp_ld"]) <= gf and abs(c["fp"] - c["fp_ld"]) <= gf
    if c["ier"] == 0:
        assert abs(float(r["fp"]) - c["s"]) <= fg.FP_STOP * c["s"] and abs(c["fp"] - c["s"]) <= fg.FP_STOP * c["s"]
    if name not in SLOW_LD:
        margin, detail = fg.margins(r["margins"], fr.fit_track(c["raw"], c["k"], c["s"], c["step"], c["nest"], LD)["margins"])
        assert margin > 1.0, detail


def test_every_case_is_decided_and_fp_agrees():
    for name in fc.CASES:
        c = fc.case(name)
        assert c["margin"] > 1.0, "%s is not decided (margin / threshold %.3g)" % (name, c["margin"])
        if c["ier"] <= 1:
            assert c["fp_agree"] <= fg.FP_AGREE, "%s: fp differs by %.3e between scipy and the restatements" % (name, c["fp_agree"])
        else:       # the p search was cut off (ier 2, 3): fp moves more; the case's smallest margin still exceeds 64 x its own disagreement
            assert c["margin"] * fg.MARGIN_FLOOR > 64.0 * c["fp_agree"], name
        assert c["spread_c"] <= fg.SPREAD_CAP, name


def test_the_cases_are_what_they_are_for():
    for name, staged in fc.IN_LDS.items():
        c = fc.case(name)
        n7 = c["t"].shape[0] - 2 * c["k"] - 1
        assert ((2 * c["k"] + 5) * n7 <= 6144) == staged, name       # MCQ_FIT_LDS
    assert [fc.case("pts%d" % n)["u"].shape[0] - 1 for n in (255, 256, 257)] == [255, 256, 257]
    assert [fc.case("rs%d" % n)["u"].shape[0] - 1 for n in (255, 256, 257)] == [255, 256, 257]
    assert fc.case("rs_below")["u"].shape[0] + 1 == fc.case("rs_above")["u"].shape[0]
    assert fc.case("nest_short")["ier"] == 1 and fc.case("nest_short")["t"].shape[0] == 20
    assert fc.case("nest_exact")["ier"] == 0 and fc.case("nest_exact")["t"].shape[0] == fc.case("nest_exact")["nest"] == fc.case("lobe_k3_s1")["t"].shape[0]
    for name in fc.GROWN_TO_NMAX:       # knot growth that ends at nmax = mi + 2 k with s > 0: fpclos's re-placement branch, reached through the loop
        c = fc.case(name)
        nmax = c["u"].shape[0] + 2 * c["k"]
        assert c["s"] > 0.0 and c["t"].shape[0] == nmax and c["stage_n"][-1] == nmax and c["stage_n"].shape[0] > 1 and c["ier"] in (0, 3), name
    assert len(fc.GROWN_TO_NMAX) == 5 and {fc.case(nm)["k"] for nm in fc.GROWN_TO_NMAX} == {1, 3, 5}
    seam = fc.case("seam")
    inner = seam["t"][seam["k"] + 1:-seam["k"] - 1]
    assert inner[0] < 0.1 and inner[-1] > 0.9, "the seam case has no knots next to the start point"
    for k in (1, 2, 3, 4, 5):
        assert fc.case("lobe_k%d_s0" % k)["ier"] == -1 and fc.case("lobe_k%d_s5" % k)["ier"] == -2
        assert fc.case("lobe_k%d_s5" % k)["t"].shape[0] == 2 * k + 2
    assert fc.case("rounded_rectangle")["t"].shape[0] == 27 and fc.case("berlin_2018")["t"].shape[0] == 78


def test_refusals_of_the_restatement():
    lobe = fr.two_lobe(41)
    for raw, k in ((lobe[:2], 3), (np.repeat(lobe[:1], 4, axis=0), 3), (lobe[:4], 5)):
        with pytest.raises(fr.Refused):
            fr.fit_track(raw, k, 0.5, 0.0)


@pytest.mark.parametrize("name", fc.LOBE + fc.BOTTOM + ("seam", "pts256"))       # (cases without re-sampling: the recorded points are the raw rows)
def test_scipy_returns_the_recording(name):
    interpolate = pytest.importorskip("scipy.interpolate")
    import warnings
    c = fc.case(name)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        (t, cc, _), u = interpolate.splprep([c["pts"][:, 0], c["pts"][:, 1]], k=c["k"], s=c["s"], per=1, nest=c["nest"])
    assert np.array_equal(t, c["t"]) and np.array_equal(u, c["u"])
    assert fg.dmax(np.asarray(cc), c["c_ld"]) <= fg.guard(c["spread_c"])
