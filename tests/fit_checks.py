"""The shared bodies of tests/test_emu_fit.py (SIMT interpreter) and tests/test_gpu_fit.py (MI355X): mcq_spline_fit_device through
Engine.spline_fit_batch / prep_track_batch on the cases of tests/fit_cases.py against scipy's recording and the longdouble restatement under
the rules of tests/fit_guard.py.  Reads the goldens; never imports scipy."""
import numpy as np

import fit_cases as fc
import fit_guard as fg
from global_racetrajectory_optimization_amd import engine

OK, BAD_INPUT = 0, fc.BAD_INPUT


def _same_bits(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def run(eng, names, raws=None, **kw):
    cs = [fc.case(nm) for nm in names]
    c = cs[0]
    assert all((x["k"], x["s"], x["step"]) == (c["k"], c["s"], c["step"]) for x in cs)
    return eng.spline_fit_batch(raws or [x["raw"] for x in cs], k=c["k"], s=c["s"], stepsize_prep=c["step"], nest=kw.pop("nest", c["nest"]),
                                points=True, **kw)


def hold_track(worst, name, out, b, what):
    """Track b of a result against the recording of case `name`.  Returns the coefficients' deviation."""
    c = fc.case(name)
    k, n = c["k"], c["t"].shape[0]
    assert out["status"][b] == OK, "%s: status %d" % (what, out["status"][b])
    assert out["nk"][b] == n and out["ier"][b] == c["ier"], "%s: n %d ier %d, scipy %d %d" % (what, out["nk"][b], out["ier"][b], n, c["ier"])
    assert out["mi"][b] == c["u"].shape[0], "%s: mi %d, scipy's m %d" % (what, out["mi"][b], c["u"].shape[0])
    t, (cx, cy), _ = out["tcks"][b]
    assert np.all(np.isnan(out["knots"][b, n:])) and np.all(np.isnan(out["coef"][b, :, n - k - 1:])), what + ": entries behind n are not NaN"
    scale = float(np.max(np.abs(c["pts"])))
    if c["step"] > 0.0:
        gap = 0.5 * float(np.min(np.diff(c["u"])))
        dk = fg.dmax(t, c["t"])
        print("%s: knots deviate by %.3e (half the smallest gap of u %.3e)" % (what, dk, gap))
        assert dk <= gap, "%s: a knot misses by %.3e, half a gap is %.3e" % (what, dk, gap)
        dp = fg.dmax(out["pts"][b], c["pts"])
        worst.add(name + ".pts", dp, fg.FLOOR)
        assert dp <= fg.FLOOR, "%s: the re-sampled points deviate by %.3e" % (what, dp)
    else:
        assert _same_bits(t, c["t"]), "%s: knots differ from scipy's at %s" % (what, np.nonzero(t != c["t"])[0][:5].tolist())
        assert _same_bits(out["pts"][b], c["pts"]), what + ": the closed points are not the raw rows"
    cc = np.stack([cx, cy])
    assert cc.shape == c["c_ld"].shape and np.all(np.isfinite(cc))
    assert _same_bits(cc[:, -k:], cc[:, :k]), what + ": the last k coefficients are not the first k"
    dc, g = fg.dmax(cc, c["c_ld"]), fg.guard(c["spread_c"])
    worst.add(name + ".c", dc, g)
    print("%s: coefficients deviate by %.3e (guard %.3e)" % (what, dc, g))
    assert dc <= g, "%s: coefficients deviate by %.3e, guard %.3e" % (what, dc, g)
    df, gf = abs(float(out["fp"][b]) - c["fp_ld"]), fg.fp_guard(c["spread_fp"], c["u"].shape[0] - 1, scale)
    worst.add(name + ".fp", df, gf)
    print("%s: fp deviates by %.3e (guard %.3e)" % (what, df, gf))
    assert df <= gf, "%s: fp %r deviates by %.3e, guard %.3e" % (what, out["fp"][b], df, gf)
    if c["ier"] == 0:
        assert abs(float(out["fp"][b]) - c["s"]) <= fg.FP_STOP * c["s"], "%s: |fp - s| = %.3e" % (what, abs(float(out["fp"][b]) - c["s"]))
    return dc


def check_case(eng, name, worst):
    out = run(eng, [name])
    hold_track(worst, name, out, 0, name)
    return out


def check_mimax(eng, name):
    """mi == mimax is served with the same bits; mi == mimax + 1 is MCQ_BAD_INPUT and mi_out reports the samples needed."""
    mi = fc.case(name)["u"].shape[0]
    free, tight, short = run(eng, [name]), run(eng, [name], mimax=mi), run(eng, [name], mimax=mi - 1)
    assert tight["status"][0] == OK and all(_same_bits(tight[q][0], free[q][0]) for q in ("nk", "fp", "ier", "mi"))
    assert _same_bits(tight["tcks"][0][0], free["tcks"][0][0]) and _same_bits(np.stack(tight["tcks"][0][1]), np.stack(free["tcks"][0][1]))
    assert short["status"][0] == BAD_INPUT and short["mi"][0] == mi and short["nk"][0] == 0 and short["tcks"][0] is None
    assert np.all(np.isnan(short["knots"])) and np.all(np.isnan(short["coef"])) and np.isnan(short["fp"][0])


def check_refusals(eng):
    good = fc.case("lobe_k3_s2")

    def middle(raw, what, k=3):
        out = eng.spline_fit_batch([good["raw"], raw, good["raw"]], k=k, s=0.5, stepsize_prep=0.0)
        assert list(out["status"]) == [OK, BAD_INPUT, OK], "%s: statuses %s" % (what, list(out["status"]))
        assert out["tcks"][1] is None and out["nk"][1] == 0 and np.all(np.isnan(out["knots"][1])) and np.all(np.isnan(out["coef"][1])), what
        assert np.isnan(out["fp"][1])
        assert _same_bits(out["knots"][0], out["knots"][2]) and _same_bits(out["coef"][0], out["coef"][2]), what
    dup = good["raw"].copy()
    dup[7] = dup[6]
    middle(dup, "a zero-length element")
    hurt = good["raw"].copy()
    hurt[5, 1] = np.nan
    middle(hurt, "a NaN row")
    middle(good["raw"][:2], "n = 2")
    middle(np.repeat(good["raw"][:1], 4, axis=0), "total == 0")
    middle(good["raw"][:4], "mi <= k", k=5)
    stepped = eng.spline_fit_batch([dup], k=3, s=0.5, stepsize_prep=1.0)
    assert stepped["status"][0] == BAD_INPUT, "a zero-length element in front of the re-sampling"


def check_arguments(eng):
    buf = eng.alloc(1 << 16)
    try:
        ok = dict(tracks=1, nmax=8, d_n=None, d_track=buf, stepsize_prep=0.0, mimax=9, k=3, s=1.0, nkmax=15, d_nk=buf + 1024, d_knots=buf + 2048,
                  d_coef=buf + 4096, d_fp=None, d_ier=buf + 8192, d_mi=None, d_pts=None, d_status=buf + 8448)
        eng.spline_fit_device(**ok)             # (zero-filled rows: a legal call, refused per track)
        eng.sync()
        assert eng.download(buf + 8448, (1,), np.int32)[0] == BAD_INPUT
        for key, val in (("tracks", 0), ("tracks", 65536), ("nmax", 2), ("mimax", 1), ("k", 0), ("k", 6), ("s", -1.0), ("s", float("nan")),
                         ("s", float("inf")), ("nkmax", 7), ("d_track", None), ("d_nk", None), ("d_knots", None), ("d_coef", None), ("d_ier", None),
                         ("d_status", None)):
            try:
                eng.spline_fit_device(**dict(ok, **{key: val}))
            except engine.EngineError as e:
                assert "(-1)" in str(e), str(e)           # MCQ_E_ARG
            else:
                raise AssertionError("mcq_spline_fit_device accepted %s = %r" % (key, val))
    finally:
        eng.sync()
        eng.free(buf)


def check_batch(eng, worst):
    """Ragged tracks that reach different n in one launch with a refused track in the middle: scipy's answers, each track bitwise itself alone
    and in the reversed launch."""
    names = list(fc.BATCH)
    raws = [fc.case(nm)["raw"] for nm in names]
    hurt = raws[1].copy()
    hurt[3, 0] = np.inf
    mixed = raws[:2] + [hurt] + raws[2:]
    idx = [0, 1, 3, 4, 5][:len(names)]
    out = run(eng, names, raws=mixed)
    rev = run(eng, names, raws=mixed[::-1])
    assert out["status"][2] == BAD_INPUT and out["tcks"][2] is None and np.all(np.isnan(out["knots"][2])) and np.all(np.isnan(out["coef"][2]))
    B = len(mixed)
    for nm, b in zip(names, idx):
        hold_track(worst, nm, out, b, "batch/" + nm)
        one = run(eng, [nm])
        for other, j, tag in ((one, 0, "alone"), (rev, B - 1 - b, "reversed")):
            assert _same_bits(out["tcks"][b][0], other["tcks"][j][0]), "%s: other knots %s" % (nm, tag)
            assert _same_bits(np.stack(out["tcks"][b][1]), np.stack(other["tcks"][j][1])), "%s: other coefficients %s" % (nm, tag)
            assert all(_same_bits(out[q][b], other[q][j]) for q in ("nk", "fp", "ier", "mi", "status")), "%s: other results %s" % (nm, tag)


def check_stale(eng):
    """Outputs that were full of other numbers before the launch: nothing of them survives."""
    c = fc.case("lobe_k3_s2")
    raw = np.concatenate((c["raw"], np.zeros_like(c["raw"])), axis=1)
    n, mimax, nk = raw.shape[0], raw.shape[0] + 6, 60
    with eng.scope() as dev:
        fill = lambda count: dev.up(np.full(count, 12345.678))      # noqa: E731
        d_trk, d_kn, d_cf, d_fp, d_pts = dev.up(raw), fill(nk), fill(2 * nk), fill(1), fill(2 * mimax)
        d_i = dev.up(np.full(4, 77, dtype=np.int32))
        eng.spline_fit_device(1, n, None, d_trk, 0.0, mimax, 3, 0.5, nk, d_i, d_kn, d_cf, d_fp, d_i + 4, d_i + 8, d_pts, d_i + 12)
        ints = eng.download(d_i, (4,), np.int32)
        kn, cf, pts = eng.download(d_kn, (nk,), np.float64), eng.download(d_cf, (2, nk), np.float64), eng.download(d_pts, (mimax, 2), np.float64)
    nn = c["t"].shape[0]
    assert list(ints) == [nn, c["ier"], n + 1, OK]
    assert _same_bits(kn[:nn], c["t"]) and np.all(np.isnan(kn[nn:])) and np.all(np.isfinite(cf[:, :nn - 4])) and np.all(np.isnan(cf[:, nn - 4:]))
    assert np.all(np.isfinite(pts[:n + 1])) and np.all(np.isnan(pts[n + 1:]))


ALPHA_CONTRACT = 1e-6
DECISION_FACTOR = 100.0


def decision_gaps(name, rows):
    """The recorded decision gap of each of the `rows` prepared waypoints of a reference track.  A prepared width is numpy.interp between the
    widths of the two raw waypoints whose closest parameters bracket its grid parameter, and what decides a raw waypoint is its closest-point
    search: tests/spline_approx_cases.reference(name) holds, per raw waypoint, the smallest |f1 - f2| in metres over every comparison that search
    made on the recorded spline (`gap`, the quantity tests/spline_approx_guard.decided judges).  A prepared waypoint's gap is the smaller of
    its two raw waypoints' (of the one it copies, outside their range): while the coefficients move by less than that, both searches take the
    same decisions and return the same parameters bitwise."""
    import spline_approx_cases as sac
    import spline_approx_ref as sr
    ref = sac.reference(name)
    ct, raw_gap = ref["t"], ref["gap"]
    n = ct.shape[0] - 1
    out = np.empty(rows)
    for j, xv in enumerate(sr.linspace01(rows + 1, np.float64)[:-1]):       # (interp_bisect's bracket, tests/spline_approx_ref.py)
        lo, hi = 0, n
        while lo < hi:
            mid = (lo + hi + 1) >> 1
            if ct[mid] <= xv:
                lo = mid
            else:
                hi = mid - 1
        if xv < ct[0]:
            out[j] = raw_gap[0]
        elif xv > ct[n] or lo == n:
            out[j] = raw_gap[n]
        else:
            out[j] = min(raw_gap[lo], raw_gap[lo + 1])
    return out


def check_end_to_end(eng, name, key, golden, runs, worst, dev_c):
    """prep_track_batch(fit="device") -> solve_batch: rows against the recorded prep_track output, alpha against the golden.  x and y within the
    length guard; widths within it at EVERY waypoint whose recorded decision gap (decision_gaps) exceeds DECISION_FACTOR x the fit's measured
    coefficient deviation dev_c; the other waypoints are at most UNDECIDED_CAP of all and held to finiteness."""
    import spline_approx_guard as sg
    c = fc.case(name)
    track = np.load(fc.TRACKS)[name + ".track"]
    out = eng.prep_track_batch([track], k_reg=c["k"], s_reg=c["s"], stepsize_prep=c["step"], fit="device")
    assert out["status"][0] == OK and out["fit_ier"][0] == c["ier"] and out["crossing"][0] == int(runs[key + "_prep_crossing"])
    assert out["tcks"][0][0].shape == c["t"].shape
    want = runs[key + "_prep_reftrack_interp"]
    got = out["reftrack"][0]
    assert got.shape == want.shape
    g = fg.guard(c["spread_c"])
    dxy = fg.dmax(got[:, :2], want[:, :2])
    worst.add("e2e/%s.xy" % name, dxy, g)
    print("%s: prepared x, y deviate by %.3e (guard %.3e)" % (name, dxy, g))
    assert dxy <= g
    dw = np.max(np.abs(got[:, 2:] - want[:, 2:]), axis=1)
    gap = decision_gaps(name, dw.size)
    decided = gap > DECISION_FACTOR * dev_c
    dwd = float(np.max(dw[decided])) if decided.any() else 0.0
    worst.add("e2e/%s.w" % name, dwd, g)
    print("%s: widths deviate by %.3e at the %d decided waypoints (guard %.3e, smallest decided gap %.3e against %.3e), %d of %d undecided" % (
        name, dwd, int(decided.sum()), g, float(np.min(gap[decided])) if decided.any() else 0.0, DECISION_FACTOR * dev_c, int((~decided).sum()), dw.size))
    assert np.all(dw[decided] <= g), "%s: widths of decided waypoints %s deviate by up to %.3e, guard %.3e" % (
        name, np.nonzero(decided & (dw > g))[0][:5].tolist(), dwd, g)
    assert (~decided).sum() <= sg.UNDECIDED_CAP * dw.size, "%s: %d of %d waypoints undecided" % (name, int((~decided).sum()), dw.size)
    assert np.all(np.isfinite(got))
    al, _, st, _ = eng.solve_batch([dict(reftrack=got, normvec=out["normvec"][0], scaling=out["scaling"][0],
                                         kappa_bound=float(golden["kappa_bound"]), w_veh=float(golden["w_veh"]))])
    da = float(np.max(np.abs(al[0] - golden["alpha"])))
    worst.add("e2e/%s.alpha" % name, da, ALPHA_CONTRACT)
    assert st[0] == OK and da < ALPHA_CONTRACT, (st[0], da)
    host = eng.prep_track_batch([track], tcks=[(c["t"], list(c["c"]), c["k"])])
    assert fg.dmax(host["reftrack"][0][:, :2], got[:, :2]) <= g
