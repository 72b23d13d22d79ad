"""The bodies of the Gaussian friction fit's tests, shared by the SIMT interpreter's run (tests/test_emu_fgauss.py) and the MI355X's
(tests/test_gpu_fgauss.py): every body takes the engine under test.  Cases: tests/fgauss_cases.py; reference: tests/fgauss_ref.py (longdouble);
what a result is held to: tests/fgauss_guard.py.  Bodies that compare return their worst deviations for the report line."""
import os

import numpy as np
import pytest

import fgauss_cases as gc
import fgauss_guard as gg
import fgauss_ref as gr
import fric_cases as fc
import fric_checks as fck
import fric_guard as fg
from global_racetrajectory_optimization_amd import engine, friction

LD = np.longdouble
FILL = -1.2345e201  # what outputs are pre-filled with: nothing of it may be left (no weight, no center_dist takes this value)
CAP = 40            # MCQ_FGS_SWEEPS
_bits = fck._bits


# a buffer width per N at which mcq_friction_gauss_device takes another number of rows per workgroup than at the tables' jmax = 65
# (include/mcq.h: min(4, 64 KB / row), a row N (jmax + N + 6) + 384 doubles): 4 -> 3 at N = 3 and 11, 2 -> 1 at N = 31
WIDE_JMAX = {3: 600, 11: 195, 31: 130}


def rows_per_workgroup(jmax, N):
    return min(4, 65536 // (8 * (N * (jmax + N + 6) + 384)))


def run_fit(eng, n, cnt, mue, status, n_gauss, rcond=None, jmax=None):
    """mcq_friction_gauss_device on pre-filled outputs: dict(w [T, 4, rows, N + 1], cd, rank, sweeps [T, rows])."""
    T, rows, j0 = n.shape
    if jmax is not None and jmax > j0:          # the same rows in wider buffers
        n = np.concatenate((n, np.full((T, rows, jmax - j0), np.nan)), axis=2)
        mue = np.concatenate((mue, np.full((T, 4, rows, jmax - j0), np.nan)), axis=3)
    P = 2 * n_gauss + 2
    with eng.scope() as dev:
        d_w, d_cd = dev.up(np.full((T, 4, rows, P), FILL)), dev.up(np.full((T, rows), FILL))
        d_rk, d_sw = dev.up(np.full((T, rows), 77, dtype=np.int32)), dev.up(np.full((T, rows), 77, dtype=np.int32))
        eng.friction_gauss_device(T, rows - 1, n.shape[2], dev.up(n), dev.up(cnt), dev.up(mue), dev.up(status), n_gauss, rcond, d_w, d_cd, d_rk, d_sw)
        out = dict(w=eng.download(d_w, (T, 4, rows, P), np.float64), cd=eng.download(d_cd, (T, rows), np.float64),
                   rank=eng.download(d_rk, (T, rows), np.int32), sweeps=eng.download(d_sw, (T, rows), np.int32))
    assert not np.any(out["w"] == FILL) and not np.any(out["cd"] == FILL) and not np.any(out["rank"] == 77) and not np.any(out["sweeps"] == 77), \
        "a pre-filled output was not overwritten"
    return out


def hold_row(w, cd, rank, sweeps, r, n_gauss, ld_w, ld_fit, rec_rank, decided, g_w, g_f, label, ref_rank=None):
    """One fitted row: w [4, N + 1], against the longdouble restatement's ld_w [4, N + 1], ld_fit [4, cnt].  ref_rank: the float64 restatement's
    rank where IT decides a row that sklearn's recorded values leave undecided.  Returns (weights, fitted) deviations as fractions of their guards."""
    assert 1 <= sweeps < CAP and rank >= 0, "%s: %d sweeps, rank %d" % (label, sweeps, rank)
    if ref_rank is not None:        # sklearn's values leave the row open, the float64 restatement's decide it
        assert rank == ref_rank, "%s: rank %d, the restatement's %d" % (label, rank, ref_rank)
    assert _bits(np.float64(cd), np.float64(gr.center_dist(r["n"], n_gauss))), "%s: center_dist is not the reference's bits" % label
    nan_wheel = np.isnan(r["mue"]).any(axis=1)
    assert np.isnan(w[nan_wheel]).all() and np.isfinite(w[~nan_wheel]).all(), "%s: a NaN stays with its wheel" % label
    ok = ~nan_wheel
    dev_f = float(np.max(np.abs(gr.fitted_values(r["n"], w[ok]) - ld_fit[ok])))
    assert dev_f <= g_f, "%s: fitted values off by %.3e (guard %.3e)" % (label, dev_f, g_f)
    dev_w = 0.0
    if decided:
        assert rank == rec_rank, "%s: rank %d, sklearn's %d" % (label, rank, rec_rank)
        dev_w = float(np.max(np.abs(w[ok].astype(LD) - ld_w[ok])))
        assert dev_w <= g_w, "%s: weights off by %.3e (guard %.3e)" % (label, dev_w, g_w)
    return dev_w / g_w, dev_f / g_f


def hold_unfitted(out, t, i, cnt, label):
    """A row without a fit: NaN weights, rank 0; center_dist 0 for one position (the reference's own value there), NaN otherwise."""
    assert np.isnan(out["w"][t, :, i]).all() and out["rank"][t, i] == 0 and out["sweeps"][t, i] == 0, label
    assert (out["cd"][t, i] == 0.0) if cnt == 1 else np.isnan(out["cd"][t, i]), label


def check_launch(eng, name):
    """One hand-made launch against the restatement and the recording; then every track alone, the launch reversed, beside others and in wider
    buffers chosen so that the number of rows per workgroup changes (WIDE_JMAX): the same bits."""
    L = gc.launches()[name]
    ng = L["n_gauss"]
    N = 2 * ng + 1
    n, cnt, mue, status = gc.arrays(L)
    out = run_fit(eng, n, cnt, mue, status, ng)
    ld, rec, dec = gg.launch_restated(name), gg.fixture(), gg.launch_decided(name)
    f64 = gg.launch_restated(name, "float64")
    g_w, g_f = gg.launch_guards(name)
    fitted = gc.fitted_rows(L)
    worst = [0.0, 0.0]
    seen = set()
    for j, (t, i, r) in enumerate(fitted):
        seen.add((t, i))
        w = out["w"][t, :, i]
        open_by_sklearn_only = not dec[j] and gr.decided(f64["sing"][j], r["cnt"], N)
        dv = hold_row(w, out["cd"][t, i], out["rank"][t, i], out["sweeps"][t, i], r, ng, ld["w"][j], ld["fitted"][j], rec[name + "/rank"][j],
                      dec[j], g_w[j], g_f[j], "%s[%d][%d] %s" % (name, t, i, r["label"]), ref_rank=int(f64["rank"][j]) if open_by_sklearn_only else None)
        assert dec[j] or open_by_sklearn_only, "%s: a row no restatement decides" % r["label"]
        worst = [max(a, b) for a, b in zip(worst, dv)]
        if "const" in r["label"]:
            assert not np.any(w[:, :N]) and np.all(w[:, N] == 1.0), "%s: a constant friction of 1.0 gives weights 0 and intercept 1, exactly" % name
    for t in range(n.shape[0]):
        for i in range(n.shape[1]):
            if (t, i) not in seen:
                hold_unfitted(out, t, i, int(cnt[t, i]) if status[t] == gc.OK else 0, "%s[%d][%d]" % (name, t, i))
    keys = ("w", "cd", "rank", "sweeps")
    T = len(L["tracks"])
    for t in range(T):
        if L["tracks"][t] is gc.REFUSED:
            continue
        a = gc.arrays(L, order=[t])
        alone = run_fit(eng, *a, ng)
        rows = a[0].shape[1]
        for q in keys:
            b = out[q][t][:, :rows] if q == "w" else out[q][t][:rows]
            assert _bits(alone[q][0], np.ascontiguousarray(b)), "%s[%d]: %s alone differs" % (name, t, q)
    rev = run_fit(eng, *gc.arrays(L, order=list(range(T))[::-1]), ng)
    assert all(_bits(rev[q][::-1], out[q]) for q in keys), "%s: reversed launch" % name
    both = run_fit(eng, *gc.arrays(L, order=[T - 1] + list(range(T))), ng)
    assert all(_bits(both[q][1:], out[q]) for q in keys), "%s: beside others" % name
    j_wide = WIDE_JMAX[N]
    assert rows_per_workgroup(j_wide, N) != rows_per_workgroup(n.shape[2], N), "the wider buffers must change the rows per workgroup"
    wide = run_fit(eng, n, cnt, mue, status, ng, jmax=j_wide)
    assert all(_bits(wide[q], out[q]) for q in keys), "%s: in buffers of width %d" % (name, j_wide)
    return tuple(worst)


def check_rcond(eng):
    """An explicit rcond that removes exactly one more singular value, with margin on both sides, against scipy.linalg.lstsq(cond = rcond)'s
    recording on the centred system and the restatement under the same rcond."""
    r, ng, rcond, ratio = gc.rcond_case()
    assert ratio >= 16.0, "the cut needs a factor 4 on both sides"
    N = 2 * ng + 1
    rec = gg.fixture()
    assert _bits(np.float64(rcond), np.float64(rec["rcond/rcond"])), "the recording was made for another rcond"
    L = dict(n_gauss=ng, tracks=[[r, gc.row(0)]])
    a = gc.arrays(L)
    out, plain = run_fit(eng, *a, ng, rcond=rcond), run_fit(eng, *a, ng)
    assert plain["rank"][0, 0] == N and out["rank"][0, 0] == N - 1 == int(rec["rcond/rank"])
    ld = gr.fit_rows([r["n"]], [r["mue"]], ng, rcond=rcond, dtype=LD)
    g_w, g_f = gg.guard(rec["rcond/spread_w"][0]), gg.guard(rec["rcond/spread_f"][0])
    dv = hold_row(out["w"][0, :, 0], out["cd"][0, 0], out["rank"][0, 0], out["sweeps"][0, 0], r, ng, ld["w"][0], ld["fitted"][0], N - 1, True, g_w, g_f,
                  "rcond %.3e" % rcond)
    dev = float(np.max(np.abs(out["w"][0, :, 0] - rec["rcond/w"])))
    assert dev <= g_w + float(rec["rcond/spread_w"][0]), "rcond: %.3e from scipy's own lstsq" % dev
    assert _bits(run_fit(eng, *a, ng, rcond=0.0)["w"], plain["w"]) and _bits(run_fit(eng, *a, ng, rcond=-1.0)["w"], plain["w"]), "rcond <= 0"
    return dv


def check_arguments(eng):
    L = gc.launches()["n1"]
    n, cnt, mue, status = gc.arrays(L)
    with eng.scope() as dev:
        p = dev.new(1 << 16)
        lib, h = eng.lib, eng.h
        for ng in (0, 16, -3):
            assert lib.mcq_friction_gauss_device(h, 1, 3, 4, p, p, p, p, ng, 0.0, p, p, None, None) == -1, ng
        assert lib.mcq_friction_gauss_device(h, 1, 3, 4, p, p, p, p, 1, float("nan"), p, p, None, None) == -1
        for miss in range(6):           # n_out, cnt_out, mue_out, status, w_gauss_out, center_dist_out
            args = [p] * 6
            args[miss] = None
            assert lib.mcq_friction_gauss_device(h, 1, 3, 4, args[0], args[1], args[2], args[3], 1, 0.0, args[4], args[5], None, None) == -1, miss
        for bad in (dict(tracks=0), dict(nmax=0), dict(jmax=0)):
            a = dict(tracks=1, nmax=3, jmax=4)
            a.update(bad)
            assert lib.mcq_friction_gauss_device(h, a["tracks"], a["nmax"], a["jmax"], p, p, p, p, 1, 0.0, p, p, None, None) == -1, bad
        # the LDS refusal: N (jmax + N + 6) + 384 doubles beyond 64 KB -- N = 31 fits up to jmax 214
        assert lib.mcq_friction_gauss_device(h, 1, 3, 215, p, p, p, p, 15, 0.0, p, p, None, None) == -3
        assert "64 KB" in lib.mcq_last_error().decode()
        # the model entry
        assert lib.mcq_friction_model_device(h, 1, 3, 2, p, None, 2, p, 0, 0, None, None, None, 0, p) == -1, "unknown model"
        assert lib.mcq_friction_model_device(h, 1, 3, 2, p, None, engine.FRIC_GAUSS, p, 0, 1, p, None, None, 0, p) == -1, "n_gauss 0"
        assert lib.mcq_friction_model_device(h, 1, 3, 2, p, None, engine.FRIC_GAUSS, p, 16, 1, p, None, None, 0, p) == -1, "n_gauss 16"
        assert lib.mcq_friction_model_device(h, 1, 3, 2, p, None, engine.FRIC_GAUSS, p, 1, 2, p, None, None, 0, p) == -1, "unknown centres"
        assert lib.mcq_friction_model_device(h, 1, 3, 2, p, None, engine.FRIC_GAUSS, p, 1, 1, None, None, None, 0, p) == -1, "no center_dist"
        assert lib.mcq_friction_model_device(h, 1, 3, 2, p, None, engine.FRIC_GAUSS, p, 1, 0, p, None, p, 4, p) == -1, "FIT without n_out"
        assert lib.mcq_friction_model_device(h, 1, 3, 2, None, None, engine.FRIC_LINEAR, p, 0, 0, None, None, None, 0, p) == -1, "no q"
        assert lib.mcq_friction_model_device(h, 1, 3, 0, p, None, engine.FRIC_LINEAR, p, 0, 0, None, None, None, 0, p) == -1, "qmax 0"
    with pytest.raises(engine.EngineError, match=r"\(-1\)"):
        run_fit(eng, n, cnt, mue, status, 16)
    with pytest.raises(engine.EngineError, match=r"\(-3\)"):
        run_fit(eng, n, cnt, mue, status, 15, jmax=215)
    # at the limit itself the launch goes through (one row per workgroup)
    L15 = gc.launches()["n15"]
    a = gc.arrays(L15)
    assert _bits(run_fit(eng, *a, 15, jmax=214)["w"], run_fit(eng, *a, 15)["w"]), "jmax 214: one row per workgroup"


def check_model(eng):
    """mcq_friction_model_device: both models, both centre forms, positions on, between and outside the sampled range.  Returns the worst
    deviation from the recorded predict as a fraction of the fitted-value guard, and the worst deviation from the longdouble evaluation of the
    same weights as a fraction of tests/fgauss_guard.eval_tol (the issue sets no bound there)."""
    name = "n5"
    L = gc.launches()[name]
    ng = L["n_gauss"]
    N = 2 * ng + 1
    n, cnt, mue, status = gc.arrays(L)
    T, rows, jmax = n.shape
    fit = run_fit(eng, n, cnt, mue, status, ng)
    fitted = gc.fitted_rows(L)
    rec = gg.fixture()
    _, g_f = gg.launch_guards(name)
    worst, worst_predict = 0.0, 0.0
    # 1. MCQ_FRIC_CENTRES_FIT at the rows' own positions: the recorded pipeline's predict, within the fitted-value guard
    own = eng.friction_model_batch(np.where(np.isnan(n), 0.0, n), fit["w"], center_dist=fit["cd"], n=n, cnt=cnt, qcnt=np.maximum(cnt, 0) * (status == 0)[:, None])
    assert own.shape == (T, 4, rows, jmax)
    for j, (t, i, r) in enumerate(fitted):
        c = r["cnt"]
        assert np.isnan(own[t, :, i, c:]).all(), "entries beyond qcnt are NaN"
        ok = ~np.isnan(r["mue"]).any(axis=1)
        assert np.isnan(own[t, ~ok, i, :c]).all(), "a NaN weight gives NaN"
        dev = float(np.max(np.abs(own[t, ok, i, :c] - rec[name + "/predict"][j][ok, :c])))
        worst_predict = max(worst_predict, dev / g_f[j])
        assert dev <= g_f[j], "%s: %.3e from the recorded predict (guard %.3e)" % (r["label"], dev, g_f[j])
    for t in range(T):
        for i in range(rows):
            if not any((t, i) == (a, b) for a, b, _ in fitted):
                assert np.isnan(own[t, :, i]).all(), "a row without a fit evaluates to NaN"
    # 2. both centre forms at positions on, between and outside the range, against the longdouble evaluation of the SAME weights
    t0 = 0
    tr = L["tracks"][t0]
    qs = [gc.eval_positions(r) if r["cnt"] >= 2 else np.zeros(1) for r in tr]
    qmax = max(len(q) for q in qs)
    q = np.zeros((1, rows, qmax))
    qcnt = np.zeros((1, rows), dtype=np.int32)
    for i, v in enumerate(qs):
        q[0, i, :len(v)], qcnt[0, i] = v, len(v)
    kw = dict(center_dist=fit["cd"][t0:t0 + 1], qcnt=qcnt)
    e_fit = eng.friction_model_batch(q, fit["w"][t0:t0 + 1], n=n[t0:t0 + 1], cnt=cnt[t0:t0 + 1], **kw)
    e_min = eng.friction_model_batch(q, fit["w"][t0:t0 + 1], centres=engine.FRIC_CENTRES_MINTIME, **kw)
    checked_asym = False
    for i, r in enumerate(tr):
        if r["cnt"] < 2:
            continue
        k, w, cd = qcnt[0, i], fit["w"][t0, :, i], fit["cd"][t0, i]
        ok = ~np.isnan(w).any(axis=1)
        cs, width = gr.centres(r["n"][0], r["n"][-1], N)
        for got, mint, cc, ww in ((e_fit, False, cs, width), (e_min, True, np.linspace(-ng, ng, N) * cd, 2.0 * cd)):
            want = gr.model_gauss(qs[i], w[ok], cd, ng, r["n"][0], r["n"][-1], mintime=mint)
            tol = gg.eval_tol(qs[i], w[ok], cc, ww, ng)
            dev = np.abs(got[0, ok, i, :k].astype(LD) - want)
            worst = max(worst, float(np.max(dev / tol)))
            assert np.all(dev <= tol), "%s (%s centres): %.3e from the longdouble evaluation" % (r["label"], "mintime" if mint else "fit", float(dev.max()))
            assert np.isnan(got[0, :, i, k:]).all() and np.isnan(got[0, ~ok, i]).all()
        sym = (name, t0, i) == gc.SYMMETRIC
        both = gg.eval_tol(qs[i], w[ok], cs, width, ng) + gg.eval_tol(qs[i], w[ok], np.linspace(-ng, ng, N) * cd, 2.0 * cd, ng)
        agree = np.all(np.abs(e_fit[0, ok, i, :k] - e_min[0, ok, i, :k]) <= both)
        if sym:
            assert _bits(np.float64(r["n"][0]), np.float64(-r["n"][-1])) and agree, "on a symmetric row the two centre forms agree"
        elif (name, t0, i) == gc.ASYMMETRIC:        # num_right != num_left: the consumer's bumps sit elsewhere
            checked_asym = True
            assert not agree, "the two centre forms differ on a row that is not symmetric about 0"
    assert checked_asym and (name, t0) == gc.SYMMETRIC[:2] == gc.ASYMMETRIC[:2], "the named rows were not met"
    # 2b. a feature alone (a unit weight): the kernels' own exponential is good to 0.55 units in the last place -- the argument is float64
    #     arithmetic numpy repeats bit for bit, the exponential of it is taken in longdouble
    rng = np.random.default_rng(9)
    qf = rng.uniform(-9.0, 9.0, (1, 2, 64))
    cdf = np.array([[0.65, 0.3]])
    for k in (0, ng, N - 1):
        wu = np.zeros((1, 4, 2, N + 1))
        wu[:, :, :, k] = 1.0
        got = eng.friction_model_batch(qf, wu, center_dist=cdf, centres=engine.FRIC_CENTRES_MINTIME)
        for i in range(2):
            d = qf[0, i] - float(k - ng) * cdf[0, i]
            sigma = 2.0 * cdf[0, i]
            arg = -(d * d) / (2.0 * (sigma * sigma))
            want = np.exp(arg.astype(LD))
            ulp = np.spacing(want.astype(np.float64))
            err = np.abs(got[0, 0, i].astype(LD) - want) / ulp
            assert np.all(err <= 0.55), "feature %d: the exponential is off by %.3f units in the last place" % (k, float(err.max()))
            assert _bits(got[0, 0, i], got[0, 3, i])
    # 3. the linear model: slope * q + intercept in two roundings, bitwise
    rng = np.random.default_rng(5)
    wl = rng.uniform(-0.2, 1.2, (2, 4, rows, 2))
    wl[1, 2, 1, 0] = np.nan
    ql = rng.uniform(-4.0, 4.0, (2, rows, 7))
    qc = rng.integers(0, 8, (2, rows)).astype(np.int32)
    lin = eng.friction_model_batch(ql, wl, qcnt=qc)
    want = np.stack([np.stack([gr.model_linear(ql[t, i], wl[t, :, i]) for i in range(rows)], axis=1) for t in range(2)])       # [2, 4, rows, 7]
    want = np.where(np.arange(7)[None, None, None, :] < qc[:, None, :, None], want, np.nan)
    assert _bits(lin, want), "the linear model is slope * q + intercept in two roundings"
    assert _bits(eng.friction_model_batch(ql, wl), np.where(np.isnan(wl[..., :1] * ql[:, None]), np.nan, wl[..., :1] * ql[:, None] + wl[..., 1:]))
    return worst_predict, worst


def check_whole_track(eng, track, n_gauss):
    """A whole track's recorded grid -> the fit, against the longdouble restatement under the track's guards, sklearn's recorded rank on every
    decided row, the reference's own center_dist bit for bit."""
    g, rec = fg.recorded(track), gg.fixture()
    pre = "%s/g%d/" % (track, n_gauss)
    N = 2 * n_gauss + 1
    cnt = g["cnt"].astype(np.int32)
    R, jmax = len(cnt), g["n"].shape[1]
    n, mue = g["n"][None], g["mue4"][None]
    out = run_fit(eng, np.ascontiguousarray(n), cnt[None], np.ascontiguousarray(mue), np.zeros(1, dtype=np.int32), n_gauss)
    ld, dec = gg.track_restated(track, n_gauss), gg.track_decided(track, n_gauss)
    g_w, g_f = gg.track_guards(track, n_gauss)
    ns, _ = gg.track_rows(track)
    assert _bits(out["cd"][0], rec[pre + "cd"]), "%s: center_dist is not the reference's bits" % track
    assert np.all((out["sweeps"][0] >= 1) & (out["sweeps"][0] < CAP))
    assert np.array_equal(out["rank"][0][dec], rec[pre + "rank"][dec]), "%s: rank differs from sklearn's on a decided row" % track
    w = np.transpose(out["w"][0], (1, 0, 2))            # [rows, 4, N + 1]
    dev_w = float(np.max(np.abs(w.astype(LD) - ld["w"])[dec])) if dec.any() else 0.0
    dev_f = max(float(np.max(np.abs(gr.fitted_values(ns[i], w[i]) - ld["fitted"][i]))) for i in range(R))
    dev_sk = float(np.max(np.abs(out["w"][0] - rec[pre + "w"])[:, dec]))
    assert dev_f <= g_f, "%s n_gauss %d: fitted values off by %.3e (guard %.3e)" % (track, n_gauss, dev_f, g_f)
    assert dev_w <= g_w, "%s n_gauss %d: weights off by %.3e (guard %.3e)" % (track, n_gauss, dev_w, g_w)
    assert dev_sk <= g_w + float(rec[pre + "spread_w"].max()), "%s n_gauss %d: %.3e from sklearn's own weights" % (track, n_gauss, dev_sk)
    return dict(w=dev_w, fitted=dev_f, sklearn=dev_sk, guard_w=g_w, guard_f=g_f, sweeps=int(out["sweeps"].max()), undecided=int((~dec).sum()))


def check_grid_surface(eng):
    """Engine.friction_grid_batch: fit=True and fit=False keep their results, fit="gauss" adds the fit of the same resident grids."""
    case = fc.grid_cases()["ragged"]
    cells, mue = fc.grid_map()
    a = ([t[0] for t in case["tracks"]], [t[1] for t in case["tracks"]], case["width"], fc.WB_F, fc.WB_R, case["dn"])
    with eng.friction_map(cells, mue) as fmap:
        lin = eng.friction_grid_batch(fmap, *a, jmax=case["jmax"], want_idx=True)
        lean = eng.friction_grid_batch(fmap, *a, fit=False, jmax=case["jmax"])
        ga = eng.friction_grid_batch(fmap, *a, fit="gauss", n_gauss=2, jmax=case["jmax"], want_idx=True)
        with pytest.raises(ValueError):
            eng.friction_grid_batch(fmap, *a, fit="cubic")
        for kw in (dict(n_gauss=0), dict(n_gauss=16), dict(n_gauss=15, jmax=215)):      # refused before the grid is launched
            with pytest.raises(ValueError, match="n_gauss|LDS"):
                eng.friction_grid_batch(fmap, *a, fit="gauss", **kw)
        assert eng.friction_grid_batch(fmap, *a, fit=True, n_gauss=99, jmax=case["jmax"])["w_mue"] is not None       # (read with "gauss" only)
    assert sorted(lin) == sorted(lean) == ["cnt", "idx", "mue", "n", "rows", "status", "w_mue"] and lean["w_mue"] is None and lin["w_mue"] is not None
    assert all(_bits(lean[q], lin[q]) for q in ("n", "cnt", "mue", "status", "rows"))
    assert ga["w_mue"] is None and all(_bits(ga[q], lin[q]) for q in ("n", "cnt", "mue", "idx", "status", "rows"))
    T, rows, jmax = ga["n"].shape
    assert ga["w_gauss"].shape == (T, 4, rows, 6) and ga["center_dist"].shape == ga["rank"].shape == ga["sweeps"].shape == (T, rows)
    direct = run_fit(eng, ga["n"], ga["cnt"], ga["mue"], ga["status"], 2)
    assert _bits(direct["w"], ga["w_gauss"]) and _bits(direct["cd"], ga["center_dist"]) and _bits(direct["rank"], ga["rank"])
    assert np.any(ga["rank"] > 0)
    # the lines still evaluate: the linear model on the grid's own positions is slope * n + intercept
    ev = eng.friction_model_batch(np.where(np.isnan(lin["n"]), 0.0, lin["n"]), lin["w_mue"], qcnt=np.maximum(lin["cnt"], 0) * (lin["status"] == 0)[:, None])
    t, i = 0, 0
    c = lin["cnt"][t, i]
    assert _bits(ev[t, :, i, :c], gr.model_linear(lin["n"][t, i, :c], lin["w_mue"][t, :, i]))


def dropin_track():
    """A closed track on tests/fric_cases.py's map with rows of 4 .. 9 positions, and the same with one row too narrow for two positions."""
    case = fc.grid_cases()["ragged"]
    ref, nv = (np.array(a, dtype=np.float64) for a in case["tracks"][2])
    return ref, nv


def check_dropin(eng, tmp, monkeypatch):
    cells, mue = fc.grid_map()
    ref, nv = dropin_track()
    pars = dict(optim_opts=dict(width_opt=3.4, var_friction="gauss"), vehicle_params_mintime=dict(wheelbase_front=fc.WB_F, wheelbase_rear=fc.WB_R))
    p_map, p_data = fck.write_map_files(tmp, cells, mue)
    monkeypatch.delenv("MCQ_GAUSS_DEVICE", raising=False)
    with pytest.raises(NotImplementedError):
        friction.approx_friction_map(ref, nv, p_map, p_data, pars, 0.25, 2, engine=eng)
    monkeypatch.setenv("MCQ_GAUSS_DEVICE", "0")
    with pytest.raises(NotImplementedError):
        friction.approx_friction_map(ref, nv, p_map, p_data, pars, 0.25, 2, engine=eng)
    n, *grids = friction.extract_friction_coeffs(ref, nv, p_map, p_data, pars, 0.25, engine=eng)
    cnts = np.array([len(r) for r in n])
    ng = 2
    N = 2 * ng + 1
    with monkeypatch.context() as m:
        m.setenv("MCQ_GAUSS_DEVICE", "1")
        got = friction.approx_friction_map(ref, nv, p_map, p_data, pars, 0.25, ng, False, False, engine=eng)
    assert os.environ.get("MCQ_GAUSS_DEVICE") == "0"
    direct = friction.approx_friction_map_gauss(ref, nv, p_map, p_data, pars, 0.25, ng, engine=eng)
    rows = ref.shape[0] + 1
    assert len(got) == 5 and all(a.shape == (rows, N + 1) for a in got[:4]) and got[4].shape == (rows, 1)
    assert all(_bits(a, b) for a, b in zip(got, direct))
    if np.all(cnts >= 2):
        mues = [np.stack([grids[k][i][:, 0] for k in range(4)]) for i in range(rows)]
        ld = gr.fit_rows(n, mues, ng, dtype=LD)
        f64, rev = gr.fit_rows(n, mues, ng), gr.fit_rows(n, mues, ng, reverse=True)
        for i in range(rows):
            assert _bits(got[4][i, 0], np.float64(gr.center_dist(n[i], ng)))
            w = np.stack([got[k][i] for k in range(4)])
            spread = max(float(np.max(np.abs(gr.fitted_values(n[i], o["w"][i]) - ld["fitted"][i]))) for o in (f64, rev))
            dev = float(np.max(np.abs(gr.fitted_values(n[i], w) - ld["fitted"][i])))
            assert dev <= gg.guard(spread), "row %d: fitted values off by %.3e (guard %.3e)" % (i, dev, gg.guard(spread))
    # evaluation by the reference's consumer's form, and by the fit's at the rows' own positions
    q = np.array([0.5 * (r[0] + r[-1]) for r in n])
    e = friction.eval_friction_model(q, *got, mintime=True, engine=eng)
    assert len(e) == 4 and all(a.shape == (rows,) and np.all(np.isfinite(a)) for a in e)
    e2 = friction.eval_friction_model(q.reshape(-1, 1), *got, mintime=False, n=n, engine=eng)
    assert all(a.shape == (rows, 1) for a in e2)
    lin = friction.approx_friction_map(ref, nv, p_map, p_data, dict(pars, optim_opts=dict(width_opt=3.4, var_friction="linear")), 0.25, engine=eng)
    el = friction.eval_friction_model(q, *lin, engine=eng)
    assert all(_bits(el[k], lin[k][:, 0] * q + lin[k][:, 1]) for k in range(4))
    # the error paths: a row of one position (the reference's features are NaN there and sklearn raises), n_gauss out of range, a cell without data
    narrow = ref.copy()
    narrow[1, 2:4] = 2.3            # floor((2.3 - 1.7 - 0.5) / 0.25) = 0 steps on either side: one position
    with pytest.raises(ValueError, match="lateral position"):
        friction.approx_friction_map_gauss(narrow, nv, p_map, p_data, pars, 0.25, ng, engine=eng)
    for bad in (0, 16):
        with pytest.raises(ValueError, match="n_gauss"):
            friction.approx_friction_map_gauss(ref, nv, p_map, p_data, pars, 0.25, bad, engine=eng)
    with eng.friction_map(cells, mue) as fmap:
        hit = int(eng.friction_grid_batch(fmap, [ref], [nv], 3.4, fc.WB_F, fc.WB_R, 0.25, fit=False, want_idx=True)["idx"][0, 1, 2, 0])
    sub = os.path.join(tmp, "missing")
    os.makedirs(sub)
    p_map2, p_data2 = fck.write_map_files(sub, cells, mue, drop=(hit,))
    with pytest.raises(KeyError):
        friction.approx_friction_map_gauss(ref, nv, p_map2, p_data2, pars, 0.25, ng, engine=eng)
    import helper_checks
    helper_checks.check_abi_table()
    for name in ("mcq_friction_gauss_device", "mcq_friction_model_device"):
        assert name in engine.EXPORTED_SYMBOLS and hasattr(eng.lib, name)


def check_end_to_end(eng, golden):
    """Berlin with the varmue data: the map -> the grids -> the Gaussian fit (n_gauss 5) in one call, then the friction at the raceline's alpha."""
    track, ng = "berlin_2018", 5
    N = 2 * ng + 1
    g = fg.recorded(track)
    z = np.load(os.path.join(os.path.dirname(fg.PATH), "..", track + ".npz"))
    ref, nv = z["reftrack"], z["normvec"]
    with eng.friction_map(g["cells"], g["mue"]) as fmap:
        out = eng.friction_grid_batch(fmap, [ref], [nv], g["width"], g["wb_f"], g["wb_r"], g["dn"], fit="gauss", n_gauss=ng)
    rows = int(out["rows"][0])
    assert out["status"][0] == 0 and _bits(out["cnt"][0], g["cnt"]) and _bits(out["n"][0], g["n"])
    ld, dec = gg.track_restated(track, ng), gg.track_decided(track, ng)
    _, g_f = gg.track_guards(track, ng)
    ns, mues = gg.track_rows(track)
    same = np.array([_bits(out["mue"][0, :, i, :len(ns[i])], mues[i]) for i in range(rows)])       # rows whose lookups are the recorded ones
    assert same.sum() >= rows - 8
    w = np.transpose(out["w_gauss"][0], (1, 0, 2))
    dev_f = max(float(np.max(np.abs(gr.fitted_values(ns[i], w[i]) - ld["fitted"][i]))) for i in np.flatnonzero(same))
    assert dev_f <= g_f, "fitted values off by %.3e (guard %.3e)" % (dev_f, g_f)
    assert np.array_equal(out["rank"][0][dec & same], gg.fixture()["%s/g%d/rank" % (track, ng)][dec & same])
    alpha = np.append(golden["alpha"], golden["alpha"][0])          # row n is row 0 again
    assert alpha.shape == (rows,)
    q = alpha.reshape(1, rows, 1)
    kw = dict(center_dist=out["center_dist"])
    e_fit = eng.friction_model_batch(q, out["w_gauss"], n=out["n"], cnt=out["cnt"], **kw)
    e_min = eng.friction_model_batch(q, out["w_gauss"], centres=engine.FRIC_CENTRES_MINTIME, **kw)
    assert np.all(np.isfinite(e_fit)) and np.all(np.isfinite(e_min))
    worst = 0.0
    for i in range(rows):
        cd = out["center_dist"][0, i]
        cs, width = gr.centres(ns[i][0], ns[i][-1], N)
        for got, mint, cc, ww in ((e_fit, False, cs, width), (e_min, True, np.linspace(-ng, ng, N) * cd, 2.0 * cd)):
            want = gr.model_gauss(alpha[i:i + 1], w[i], cd, ng, ns[i][0], ns[i][-1], mintime=mint)
            tol = gg.eval_tol(alpha[i:i + 1], w[i], cc, ww, ng)
            dev = np.abs(got[0, :, i, :].astype(LD) - want)
            worst = max(worst, float(np.max(dev / tol)))
            assert np.all(dev <= tol), "row %d (%s centres): %.3e from the longdouble evaluation" % (i, "mintime" if mint else "fit", float(dev.max()))
    # inside the sampled range the fit follows the map: the friction there lies between 0.81 and 1.19, and the fit's residual is small
    inside = np.array([ns[i][0] <= alpha[i] <= ns[i][-1] for i in range(rows)])
    assert inside.sum() > rows // 2 and np.all(np.abs(e_fit[0, :, inside, 0] - 1.0) < 0.3)
    return dict(fitted=dev_f, guard_f=g_f, eval=worst)
