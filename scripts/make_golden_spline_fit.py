#!/usr/bin/env python3
"""Writes tests/golden/spline_fit/cases.npz: per case of tests/fit_cases.py the raw points, k, s, stepsize_prep and nest; what
scipy.interpolate.splprep(..., per=1, full_output=1) returns on the machine that runs this script (t, c, u, fp, ier; its version is recorded)
and its stage probes (nest = N returns the least-squares spline of the stage with N knots: knots and fp of every stage the restatement
passes); the longdouble restatement's coefficients, fp and points; the spreads and the decision margins of tests/fit_guard.py.
Data only.  Needs scipy; the interpreter and GPU tests read the file and never import scipy."""
import os
import sys
import warnings

import numpy as np
import scipy
from scipy import interpolate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fit_cases as fc      # noqa: E402
import fit_guard as fg      # noqa: E402
import fit_ref as fr        # noqa: E402

LD = np.longdouble
OUT = fc.PATH


def lobed(n, size, seed, noise=0.05):
    rng = np.random.default_rng(seed)
    th = 2.0 * np.pi * np.arange(n) / n
    r = size * (1.0 + 0.25 * np.cos(2.0 * th) + 0.1 * np.sin(3.0 * th))
    return np.column_stack((r * np.cos(th), r * np.sin(th))) + noise * rng.standard_normal((n, 2))


def total_of(xy):
    cl = np.vstack((xy, xy[:1]))
    return float(np.cumsum(np.sqrt(np.sum(np.diff(cl, axis=0) ** 2, axis=1)))[-1])


def scaled_to(xy, total):
    return xy * (total / total_of(xy))


def seam_curve(n=60):
    th = 2.0 * np.pi * np.arange(n) / n
    r = 25.0 + 6.0 * np.exp(-(np.minimum(th, 2.0 * np.pi - th) / 0.12) ** 2)      # a spike at the start point
    r = r * (1.0 + 0.15 * np.sin(2.0 * th) + 0.1 * np.cos(3.0 * th + 0.7))         # (no mirror axis: a symmetric curve ties fpknot's intervals)
    return np.column_stack((r * np.cos(th), 0.8 * r * np.sin(th)))


def build():
    cases = {}

    def add(name, raw, k, s, step=0.0, nest=0):
        cases[name] = (None if raw is None else np.ascontiguousarray(raw, dtype=np.float64), int(k), float(s), float(step), int(nest))
    lobe = fr.two_lobe(fc.LOBE_POINTS)
    for k in (1, 2, 3, 4, 5):
        for i, s in enumerate(fc.S_LIST):
            add("lobe_k%d_s%d" % (k, i), lobe, k, s)
    for nm, k, n in (("k1_mi4", 1, 3), ("k3_mi4", 3, 3), ("k3_mi5", 3, 4), ("k5_mi6", 5, 5), ("k5_mi7", 5, 6)):
        for i in (0, 2):
            # (no mirror axis: a symmetric polygon ties fpknot's intervals; the smooth hexagon ties its first two intervals as well -- its
            #  replacement is the neighbour with two metres of noise on the points)
            add("%s_s%d" % (nm, i), lobed(n, 20.0, 2 if n == 6 else n, noise=2.0 if n == 6 else 0.0), k, fc.S_LIST[i])
    add("nest_short", lobe, 3, 0.05, nest=20)
    add("nest_exact", lobe, 3, 0.05, nest=37)        # (the n lobe_k3_s1 reaches)
    add("seam", seam_curve(), 3, 0.5)
    for n in (255, 256, 257):
        add("pts%d" % n, lobed(n, 40.0, n), 3, 0.5)
    for nb in (255, 256, 257):
        add("rs%d" % nb, scaled_to(lobed(30, 10.0, nb, noise=0.0), nb - 0.5), 3, 0.5, step=1.0)
    add("rs_below", scaled_to(lobed(24, 10.0, 5, noise=0.0), 100.0 - 1e-6), 3, 0.5, step=1.0)
    add("rs_above", scaled_to(lobed(24, 10.0, 5, noise=0.0), 100.0 + 1e-6), 3, 0.5, step=1.0)
    for n7 in (558, 559):
        add("lds%d" % n7, lobed(n7, n7 / 7.3, n7, noise=0.0), 3, 0.0)
    add("l2_smooth", lobed(700, 100.0, 700, noise=0.03), 3, 0.02)
    for nm in fc.REFERENCE_TRACKS:
        add(nm, None, 3, 10.0, step=1.0)
    return cases


def scipy_fit(pts, k, s, nest=None):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        r = interpolate.splprep([pts[:, 0], pts[:, 1]], k=k, s=s, per=1, full_output=1, nest=nest)
    (t, c, _), u = r[0]
    return np.asarray(t), np.asarray(c), np.asarray(u), float(r[1]), int(r[2])


def main():
    cases = build()
    tracks = np.load(fc.TRACKS)
    out = {"scipy_version": np.str_(scipy.__version__)}
    undecided = []
    for name, (raw, k, s, step, nest) in cases.items():
        if raw is None:
            raw = tracks[name + ".track"][:, :2]
        stages = []
        r64 = fr.fit_track(raw, k, s, step, nest or None, np.float64, stages)
        stages_ld = []
        rld = fr.fit_track(raw, k, s, step, nest or None, LD, stages_ld)
        pts = r64["pts"]
        t, c, u, fp, ier = scipy_fit(pts, k, s, nest or None)
        if not (r64["n"] == rld["n"] == t.shape[0] and r64["ier"] == rld["ier"] == ier):
            print("%-18s PATHS DIFFER: n %d / %d / %d, ier %d / %d / %d (float64, longdouble, scipy)" % (name, r64["n"], rld["n"], t.shape[0], r64["ier"], rld["ier"], ier))
            undecided.append(name)
            continue
        assert np.array_equal(r64["t"], t) and np.array_equal(r64["u"], u), name
        sc, sf = max(fg.dmax(r64["c"], rld["c"]), fg.dmax(c, rld["c"])), max(abs(float(r64["fp"] - rld["fp"])), abs(float(fp - rld["fp"])))
        moved = []
        for draw in range(fg.SPREAD_DRAWS):
            rng = fg.draw_rng("spline_fit/" + name, "fit", 0, draw)
            p = np.asarray(raw, dtype=LD) * (LD(1) + LD(fg.SPREAD_REL) * rng.standard_normal(raw.shape).astype(LD))
            stages_p = []
            rp = fr.fit_track(p, k, s, step, nest or None, LD, stages_p)
            if rp["n"] == rld["n"]:
                sc, sf = max(sc, fg.dmax(rp["c"], rld["c"])), max(sf, abs(float(rp["fp"] - rld["fp"])))
            moved.append(stages_p)
        margin, detail = fg.margins(r64["margins"], rld["margins"])
        scale = max(float(rld["fp"]), float(s), 1e-300)
        agree = max(abs(float(r64["fp"] - rld["fp"])), abs(float(fp - rld["fp"]))) / scale if s > 0 else 0.0
        # every stage's fp with a spread of its own, measured as the final one's: float64 and scipy's probe against longdouble, and the longdouble
        # one's movement under the draws (a stage whose fp is below s: scipy's probe goes on to the smoothing spline, so it has no say there)
        assert [st[0] for st in stages_ld] == [st[0] for st in stages], name
        st_n, st_fp, st_t, st_ld, st_sp = [], [], [], [], []
        for i, (n, tk, f) in enumerate(stages):
            ts, _, _, fs, _ = scipy_fit(pts, k, s, n)
            assert ts.shape[0] == n and np.array_equal(ts, tk), (name, "stage", n)
            fl = stages_ld[i][2]
            sp = abs(float(LD(f) - fl))
            if not (0.0 < s and f - s < 0.0):
                sp = max(sp, abs(float(LD(fs) - fl)))
            for sp_ in moved:
                if i < len(sp_) and sp_[i][0] == n:
                    sp = max(sp, abs(float(sp_[i][2] - fl)))
            st_n.append(n)
            st_fp.append(fs)
            st_t.append(ts)
            st_ld.append(float(fl))
            st_sp.append(sp)
        print("%-18s k %d s %-8g mi %4d n %4d ier %2d rounds %2d + %2d  spread c %.1e fp %.1e  fp agree %.1e  margin / threshold %.3g %s" % (
            name, k, s, pts.shape[0], t.shape[0], ier, r64["rounds"], r64["prounds"], sc, sf, agree, margin,
            " ".join("%s %.1e/%.1e" % (q, *v) for q, v in detail.items())))
        if not margin > 1.0:
            undecided.append(name)
        g = lambda q, v: out.__setitem__(name + "." + q, v)      # noqa: E731
        if name not in fc.REFERENCE_TRACKS:
            g("raw", raw)
        g("k", np.int32(k)); g("s", np.float64(s)); g("step", np.float64(step)); g("nest", np.int32(nest))
        g("t", t); g("c", c); g("u", u); g("fp", np.float64(fp)); g("ier", np.int32(ier))
        g("stage_n", np.asarray(st_n, dtype=np.int32)); g("stage_fp", np.asarray(st_fp, dtype=np.float64))
        g("stage_t", np.concatenate(st_t) if st_t else np.zeros(0))
        g("stage_fp_ld", np.asarray(st_ld, dtype=np.float64)); g("stage_spread", np.asarray(st_sp, dtype=np.float64))
        g("c_ld", np.asarray(rld["c"], dtype=np.float64)); g("fp_ld", np.float64(rld["fp"])); g("pts", np.asarray(rld["pts"], dtype=np.float64))
        g("spread", np.asarray([sc, sf], dtype=np.float64)); g("margin", np.float64(margin)); g("fp_agree", np.float64(agree))
    assert not undecided, undecided          # (a case that is not decided is replaced by a neighbour in build(), never exempted)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes; undecided:", undecided or "none")


if __name__ == "__main__":
    main()
