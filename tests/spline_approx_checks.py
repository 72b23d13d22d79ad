"""The shared bodies of tests/test_emu_spline_approx.py (SIMT interpreter) and tests/test_gpu_spline_approx.py (MI355X): mcq_spline_approx_device
and mcq_min_width_device through Engine.spline_approx_batch / min_width_batch / prep_track_batch on the cases of tests/spline_approx_cases.py
against tests/spline_approx_ref.py under the rules of tests/spline_approx_guard.py.  Reads the recorded splines; never imports scipy."""
import numpy as np

import spline_approx_cases as sc
import spline_approx_guard as sg
import spline_approx_ref as sr
from global_racetrajectory_optimization_amd import engine

LD = np.longdouble
OK, BAD_INPUT = 0, sc.BAD_INPUT
KEYS = ("closest_t", "dists", "dev", "nonmono", "m", "status")


def _same_bits(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _hold(worst, name, q, dev, spread, what):
    g = sg.guard(spread)
    worst.add("%s.%s" % (name, q), dev, g)
    print("%s: %s deviates by %.3e (guard %.3e)" % (what, q, dev, g))
    assert dev <= g, "%s: %s deviates by %.3e, guard %.3e" % (what, q, dev, g)


def hold_track(worst, name, out, b, what):
    """Track b of a result against the reference of case `name`."""
    c, ref = sc.case(name), sc.reference(name)
    n = c["track"].shape[0]
    assert out["status"][b] == OK, "%s: status %d" % (what, out["status"][b])
    assert out["m"][b] == ref["m"], "%s: m %d, reference %d" % (what, out["m"][b], ref["m"])
    ct, ds = out["closest_t"][b], out["dists"][b]
    assert np.all(np.isfinite(ct[:n + 1])) and np.all(np.isfinite(ds[:n + 1]))
    assert np.all(np.isnan(ct[n + 1:])) and np.all(np.isnan(ds[n + 1:])), what + ": entries behind n + 1 are not NaN"
    dec = ref["decided"]
    wrong = np.nonzero(dec & (ct[:n + 1].view(np.int64) != ref["t"].view(np.int64)))[0]
    assert wrong.size == 0, "%s: closest_t of decided waypoint(s) %s: %r, reference %r" % (what, wrong[:5].tolist(), ct[wrong[:5]], ref["t"][wrong[:5]])
    slack = 8.0 * sg.EPS * float(np.max(np.abs(c["track"][:, :2])))      # (f(t_guess) itself is a rounded quantity of the coordinates' size)
    assert np.all(ds[:n + 1] <= ref["f0"] + slack), what + ": a search returned a point worse than its start"
    if name in sc.EXACT_FIT:
        assert _same_bits(ct[:n + 1], ref["x0"]) and float(np.max(ds[:n + 1])) <= sg.FLOOR, what + ": an exact fit's waypoints moved"
    fin = sr.finish(c["track"], c["tck"], c["step"], ct[:n + 1], LD)
    rows = out["reftrack"][b]
    assert rows.shape == (ref["m"], 4)
    _hold(worst, name, "xy", sg.dmax(rows[:, :2], fin["rows"][:, :2]), c["spread"][0], what)
    _hold(worst, name, "w", sg.dmax(rows[:, 2:], fin["rows"][:, 2:]), c["spread"][1], what)
    _hold(worst, name, "dist", sg.dmax(ds[:n + 1], fin["dists"]), c["spread"][2], what)
    _hold(worst, name, "dev", max(sg.dmax(out["dev"][b, 0], fin["dev"][0]), sg.dmax(out["dev"][b, 1], fin["dev"][1])), c["spread"][3], what)
    assert out["nonmono"][b] == fin["nonmono"], "%s: nonmono %d, reference %d" % (what, out["nonmono"][b], fin["nonmono"])
    return fin


def run(eng, names, mmax=None, tracks=None):
    cs = [sc.case(nm) for nm in names]
    return eng.spline_approx_batch(tracks or [c["track"] for c in cs], [c["tck"] for c in cs], cs[0]["step"], mmax=mmax)


def check_case(eng, name, worst):
    out = run(eng, [name])
    fin = hold_track(worst, name, out, 0, name)
    if name == "nonmono":
        assert out["nonmono"][0] > 0, "the constructed descent is not there"
    else:
        assert fin["nonmono"] == 0
    return out


def check_mmax(eng, name):
    """m == mmax is served with the same bits; m == mmax + 1 is MCQ_BAD_INPUT, m_out reports the rows needed, everything else is NaN."""
    m = sc.reference(name)["m"]
    free, tight, short = run(eng, [name]), run(eng, [name], mmax=m), run(eng, [name], mmax=m - 1)
    assert tight["status"][0] == OK and _same_bits(tight["reftrack"][0], free["reftrack"][0])
    assert all(_same_bits(tight[q], free[q]) for q in KEYS)
    assert short["status"][0] == BAD_INPUT and short["m"][0] == m and short["reftrack"][0] is None
    assert np.all(np.isnan(short["closest_t"])) and np.all(np.isnan(short["dists"])) and np.all(np.isnan(short["dev"])) and short["nonmono"][0] == 0


def check_batch(eng, worst):
    """Tracks of different n and nk in one launch: the reference's answers, bitwise those of each track alone and of the reversed launch; a NaN
    in one track refuses that track alone."""
    names = list(sc.BATCH)
    step = sc.case(names[0])["step"]
    assert all(sc.case(nm)["step"] == step and sc.case(nm)["tck"][2] == 3 for nm in names)
    out = run(eng, names)
    rev = run(eng, names[::-1])
    B = len(names)
    for b, nm in enumerate(names):
        hold_track(worst, nm, out, b, "batch/" + nm)
        n = sc.case(nm)["track"].shape[0]
        one = run(eng, [nm])
        for other, k, tag in ((one, 0, "alone"), (rev, B - 1 - b, "reversed")):
            assert _same_bits(out["reftrack"][b], other["reftrack"][k]), "%s: other rows %s" % (nm, tag)
            assert _same_bits(out["closest_t"][b, :n + 1], other["closest_t"][k, :n + 1]) and _same_bits(out["dists"][b, :n + 1], other["dists"][k, :n + 1])
            assert all(_same_bits(out[q][b], other[q][k]) for q in ("dev", "nonmono", "m", "status")), "%s: other results %s" % (nm, tag)
    tracks = [sc.case(nm)["track"] for nm in names]
    hurt = tracks[1].copy()
    hurt[5, 0] = np.nan
    bad = run(eng, names, tracks=[tracks[0], hurt] + tracks[2:])
    assert list(bad["status"]) == [OK, BAD_INPUT] + [OK] * (B - 2), list(bad["status"])
    assert bad["reftrack"][1] is None and np.all(np.isnan(bad["closest_t"][1])) and np.all(np.isnan(bad["dists"][1])) and np.all(np.isnan(bad["dev"][1]))
    for b in [0] + list(range(2, B)):
        assert _same_bits(bad["reftrack"][b], out["reftrack"][b]) and _same_bits(bad["closest_t"][b], out["closest_t"][b]), "the refused track disturbed track %d" % b


def check_status_and_arguments(eng):
    c = sc.case("n3")
    good = sc.case("rounded_rectangle")
    t, (cx, cy), k = c["tck"]

    def middle(track=None, tck=None, step=None, what=""):
        out = eng.spline_approx_batch([good["track"], c["track"] if track is None else track, good["track"]],
                                      [good["tck"], c["tck"] if tck is None else tck, good["tck"]], step or c["step"])
        assert list(out["status"]) == [OK, BAD_INPUT, OK], "%s: statuses %s" % (what, list(out["status"]))
        assert out["reftrack"][1] is None and np.all(np.isnan(out["dists"][1])) and np.all(np.isnan(out["dev"][1])), what
        assert _same_bits(out["reftrack"][0], out["reftrack"][2])
    middle(track=c["track"][:2], what="n = 2")
    w = c["track"].copy()
    w[1, 3] = np.inf
    middle(track=w, what="an infinite width")
    middle(track=np.repeat(c["track"][:1], 3, axis=0), what="total == 0")
    td = t.copy()
    td[[6, 7]] = td[[7, 6]]
    middle(tck=(td, (cx, cy), k), what="descending knots")
    middle(tck=(t[:2 * k + 1], (cx, cy), k), what="nk < 2 k + 2")
    cn = cx.copy()
    cn[2] = np.nan
    middle(tck=(t, (cn, cy), k), what="a NaN coefficient")
    huge = eng.spline_approx_batch([c["track"]], [c["tck"]], 1e3)
    assert huge["status"][0] == BAD_INPUT and huge["m"][0] < 3, "m < 3"
    buf = eng.alloc(1 << 16)
    try:
        ok = dict(tracks=1, nmax=8, d_n=None, d_track=buf, k=3, nkmax=12, d_nk=None, d_knots=buf + 1024, d_coef=buf + 2048, stepsize_reg=3.0, mmax=8,
                  d_ref=buf + 4096, d_m=buf + 8192, d_ct=None, d_dist=None, d_dev=None, d_nonmono=None, d_status=buf + 8448)
        eng.spline_approx_device(**ok)             # (zero-filled buffers: a legal call, refused per track)
        for key, val in (("tracks", 0), ("tracks", 65536), ("nmax", 2), ("nmax", 16777217), ("k", 0), ("k", 6), ("nkmax", 7), ("stepsize_reg", 0.0), ("stepsize_reg", -1.0),
                         ("stepsize_reg", float("nan")), ("mmax", 2), ("d_track", None), ("d_knots", None), ("d_coef", None), ("d_ref", None),
                         ("d_m", None), ("d_status", None)):
            try:
                eng.spline_approx_device(**dict(ok, **{key: val}))
            except engine.EngineError as e:
                assert "(-1)" in str(e), str(e)           # MCQ_E_ARG
            else:
                raise AssertionError("mcq_spline_approx_device accepted %s = %r" % (key, val))
        for kw in (dict(batch=0), dict(d_ref=None), dict(d_changed=None), dict(min_width=float("nan"))):
            try:
                eng.min_width_device(**dict(dict(batch=1, nmax=8, d_n=None, d_ref=buf, min_width=1.0, d_changed=buf + 8192), **kw))
            except engine.EngineError as e:
                assert "(-1)" in str(e), str(e)
            else:
                raise AssertionError("mcq_min_width_device accepted %r" % (kw,))
    finally:
        eng.sync()
        eng.free(buf)


def check_min_width(eng):
    """min_width just below, at and above a row's width: only rows strictly narrower grow, by half the deficit on both sides (numpy's bits)."""
    a = np.array([[0.0, 0.0, 1.5, 2.0], [1.0, 0.0, 1.25, 1.0], [2.0, 1.0, 3.0, 0.5], [3.0, 1.0, 0.1, 0.2], [4.0, 2.0, 1.7, 1.8]])
    b = a[:3] + 0.125
    width = float(a[0, 2] + a[0, 3])
    for mw in (np.nextafter(width, 0.0), width, np.nextafter(width, 10.0), 0.0, 2.3, 10.0):
        rows, changed = eng.min_width_batch([a, b], float(mw))
        for src, got, ch in zip((a, b), rows, changed):
            want = src.copy()
            hit = False
            for i in range(want.shape[0]):
                cur = want[i, 2] + want[i, 3]
                if cur < mw:
                    hit = True
                    want[i, 2] += (mw - cur) / 2
                    want[i, 3] += (mw - cur) / 2
            assert _same_bits(got, want) and ch == int(hit), "min_width %r: rows %r, expected %r, flag %d" % (mw, got, want, ch)


ALPHA_CONTRACT = 1e-6
ROWS_E2E = 1e-9     # m: the recorded rows are the host route's on the same raw rows; what separates the two is the fit (recorded here from the
#                     same FITPACK) and roundings of the order of the spreads -- the project's floor for lengths


def check_end_to_end(eng, name, key, golden, runs, worst):
    """prep_track_batch (recorded spline) -> solve_batch: the rows against the recorded prep_track output, alpha against the golden."""
    c = sc.case(name)
    out = eng.prep_track_batch([c["track"]], tcks=[c["tck"]], stepsize_reg=c["step"])
    assert out["status"][0] == OK and out["crossing"][0] == int(runs[key + "_prep_crossing"]) and out["inflated"][0] == 0
    want = runs[key + "_prep_reftrack_interp"]
    assert out["reftrack"][0].shape == want.shape
    d = sg.dmax(out["reftrack"][0], want)
    dn = sg.dmax(out["normvec"][0], runs[key + "_prep_normvec"])
    worst.add("e2e/%s.rows" % name, d, ROWS_E2E)
    print("%s: prepared rows deviate by %.3e, normals by %.3e" % (name, d, dn))
    assert d <= ROWS_E2E and dn <= ROWS_E2E
    al, _, st, _ = eng.solve_batch([dict(reftrack=out["reftrack"][0], normvec=out["normvec"][0], scaling=out["scaling"][0],
                                         kappa_bound=float(golden["kappa_bound"]), w_veh=float(golden["w_veh"]))])
    da = float(np.max(np.abs(al[0] - golden["alpha"])))
    worst.add("e2e/%s.alpha" % name, da, ALPHA_CONTRACT)
    assert st[0] == OK and da < ALPHA_CONTRACT, (st[0], da)
    wide, flag = eng.min_width_batch(out["reftrack"], 100.0)
    assert flag[0] == 1 and np.all(wide[0][:, 2] + wide[0][:, 3] >= 100.0 - 1e-12)
