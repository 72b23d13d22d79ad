"""The plain restatement of the Gaussian friction fit (tests/fgauss_ref.py) against the reference's OWN approx_friction_map("gauss") as recorded in
tests/golden/friction_gauss/reference.npz (scripts/make_golden_friction_gauss.py), and the conditions the device tests rely on: which rows are
decided, the margins of tests/fgauss_cases.py's table, the spreads on record.  No GPU, no interpreter, no sklearn."""
import os
import re

import numpy as np
import pytest

import fgauss_cases as gc
import fgauss_guard as gg
import fgauss_ref as gr
from global_racetrajectory_optimization_amd import engine

LD = np.longdouble
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_entries_are_declared():
    header = open(os.path.join(ROOT, "include", "mcq.h")).read()
    for name in ("mcq_friction_gauss_device", "mcq_friction_model_device"):
        assert name in engine.EXPORTED_SYMBOLS
        assert re.search(r"\bint %s\(mcq_handle\* h," % name, header), name
    for k, v in (("MCQ_FRIC_LINEAR", engine.FRIC_LINEAR), ("MCQ_FRIC_GAUSS", engine.FRIC_GAUSS), ("MCQ_FRIC_CENTRES_FIT", engine.FRIC_CENTRES_FIT),
                 ("MCQ_FRIC_CENTRES_MINTIME", engine.FRIC_CENTRES_MINTIME)):
        assert re.search(r"#define %s %d\b" % (k, v), header), k
    import helper_checks
    helper_checks.check_abi_table()


def test_the_fixture_holds_data_of_the_versions_it_names():
    f = gg.fixture()
    assert any(v.startswith("sklearn 1.") for v in f["versions"]) and any(v.startswith("scipy ") for v in f["versions"])
    assert list(f["tracks"]) == list(gg.TRACKS) and tuple(f["n_gauss"]) == gg.N_GAUSS
    assert os.path.getsize(gg.PATH) < 1 << 20


@pytest.mark.parametrize("n_gauss", gg.N_GAUSS)
@pytest.mark.parametrize("track", gg.TRACKS)
def test_whole_tracks_are_decided_and_restated(track, n_gauss):
    """No row of a whole track is undecided -- by sklearn's recorded singular values and by the float64 restatement's -- and on every row the
    restatement has sklearn's rank, the reference's center_dist bit for bit, and weights and fitted values within the recorded spread."""
    f, pre, N = gg.fixture(), "%s/g%d/" % (track, n_gauss), 2 * n_gauss + 1
    ns, _ = gg.track_rows(track)
    dec = gg.track_decided(track, n_gauss)
    assert dec.all(), "%d undecided rows" % int((~dec).sum())
    f64, ld = gg.track_restated(track, n_gauss, "float64"), gg.track_restated(track, n_gauss)
    assert f64["sweeps"] < 40 and np.array_equal(f64["rank"], f[pre + "rank"]) and np.array_equal(ld["rank"], f[pre + "rank"])
    assert all(np.float64(gr.center_dist(n, n_gauss)).tobytes() == np.float64(c).tobytes() for n, c in zip(ns, f[pre + "cd"]))
    rec = np.transpose(f[pre + "w"], (1, 0, 2))
    sw, sf = f[pre + "spread_w"], f[pre + "spread_f"]
    for o in (f64["w"], rec):
        assert np.all(np.max(np.abs(o.astype(LD) - ld["w"]), axis=(1, 2)).astype(np.float64) <= sw), "a deviation above the spread on record"
    assert all(float(np.max(np.abs(gr.fitted_values(ns[i], rec[i]) - ld["fitted"][i]))) <= sf[i] for i in range(0, len(ns), 7))
    gap = min(min(gr.gap_decades(f[pre + "sing"][i, :min(len(n), N)], len(n), N), gr.gap_decades(f64["sing"][i], len(n), N)) for i, n in enumerate(ns))
    assert gap > np.log10(4.0)
    if (track, n_gauss) == ("berlin_2018", 5):
        assert dict(zip(*np.unique(f[pre + "rank"], return_counts=True))) == {9: 2, 10: 13, 11: 762}
        assert 1.6 < gap < 1.8          # the worst row lies 1.68 decades from the cut


@pytest.mark.parametrize("name", sorted(gc.launches()))
def test_hand_made_rows_are_decided_and_restated(name):
    """Every hand-made row is decided, but the one LAPACK's floor leaves open (tests/fgauss_guard.LAPACK_FLOOR); on the decided ones the
    restatement has sklearn's rank -- min(cnt - 1, N) off the lattice -- and the spreads on record are the ones this tree computes."""
    f, L = gg.fixture(), gc.launches()[name]
    ng = L["n_gauss"]
    N = 2 * ng + 1
    rows = gc.fitted_rows(L)
    dec = gg.launch_decided(name)
    assert {(name, r["label"]) for (_, _, r), d in zip(rows, dec) if not d} == {x for x in gg.LAPACK_FLOOR if x[0] == name}
    f64, ld = gg.launch_restated(name, "float64"), gg.launch_restated(name)
    for j, (_, _, r) in enumerate(rows):
        if not dec[j]:      # the restatement itself decides the row; sklearn's value is the floor, within a factor 4 below the cut
            assert gr.decided(f64["sing"][j], r["cnt"], N) and f64["rank"][j] == f[name + "/rank"][j] == N - 1
            s = f[name + "/sing"][j]
            assert 0.25 < s[-1] / (max(r["cnt"], N) * gr.EPS64 * s[0]) < 1.0
            continue
        assert f64["rank"][j] == ld["rank"][j] == f[name + "/rank"][j], r["label"]
        if "smooth" in r["label"] and not (r["label"].startswith("cnt %d A" % (N + 1))):
            assert f64["rank"][j] == min(r["cnt"] - 1, N), r["label"]
        ok = ~np.isnan(r["mue"]).any(axis=1)
        for o in (f64["w"][j], f[name + "/w"][j]):
            assert float(np.max(np.abs(o[ok].astype(LD) - ld["w"][j][ok]))) <= f[name + "/spread_w"][j], r["label"]
            assert float(np.max(np.abs(gr.fitted_values(r["n"], o[ok]) - ld["fitted"][j][ok]))) <= f[name + "/spread_f"][j], r["label"]
        assert np.isnan(f[name + "/w"][j][~ok]).all()
    rev = gr.fit_rows([r["n"] for _, _, r in rows], [r["mue"] for _, _, r in rows], ng, reverse=True)
    for j, (_, _, r) in enumerate(rows):
        ok = ~np.isnan(r["mue"]).any(axis=1)
        assert float(np.max(np.abs(rev["w"][j][ok].astype(LD) - ld["w"][j][ok]))) <= f[name + "/spread_w"][j]
    # the table's own edges are all there
    cnts = {r["cnt"] for t in L["tracks"] if t is not gc.REFUSED for r in t}
    assert {2, 3, N - 1, N, N + 1, N + 2, 64, 65, 1, 0} <= cnts and (name == "n15" or {63, -1} <= cnts)
    n, cnt, mue, status = gc.arrays(L)
    assert cnt.max() == (1000 if gc.REFUSED in L["tracks"] else n.shape[2]) and n.shape[2] == 65, "a row fills the buffer: cnt == jmax"


def test_the_explicit_rcond_lies_between_two_singular_values_with_margin():
    r, ng, rcond, ratio = gc.rcond_case()
    f = gg.fixture()
    N = 2 * ng + 1
    assert ratio >= 16.0 and np.float64(rcond).tobytes() == np.float64(f["rcond/rcond"]).tobytes()
    s = f["rcond/sing"]
    assert s[-1] < rcond * s[0] / 4.0 and s[-2] > 4.0 * rcond * s[0] and int(f["rcond/rank"]) == N - 1
    got = gr.fit_rows([r["n"]], [r["mue"]], ng, rcond=rcond)
    assert got["rank"][0] == N - 1 and gr.fit_rows([r["n"]], [r["mue"]], ng)["rank"][0] == N
    ld = gr.fit_rows([r["n"]], [r["mue"]], ng, rcond=rcond, dtype=LD)
    assert float(np.max(np.abs(got["w"][0].astype(LD) - ld["w"][0]))) <= f["rcond/spread_w"][0]
    assert float(np.max(np.abs(f["rcond/w"].astype(LD) - ld["w"][0]))) <= f["rcond/spread_w"][0]


def test_the_recorded_predict_is_the_fit_evaluated_at_the_rows_positions():
    """The pipeline's predict against the longdouble evaluation of its own recorded weights: what MCQ_FRIC_CENTRES_FIT is compared with."""
    f, name = gg.fixture(), "n5"
    L = gc.launches()[name]
    ng = L["n_gauss"]
    N = 2 * ng + 1
    for j, (_, _, r) in enumerate(gc.fitted_rows(L)):
        ok = ~np.isnan(r["mue"]).any(axis=1)
        w = f[name + "/w"][j][ok]
        cs, width = gr.centres(r["n"][0], r["n"][-1], N)
        want = gr.model_gauss(r["n"], w, gr.center_dist(r["n"], ng), ng, r["n"][0], r["n"][-1])
        dev = np.abs(f[name + "/predict"][j][ok, :r["cnt"]].astype(LD) - want)
        assert np.all(dev <= gg.eval_tol(r["n"], w, cs, width, ng)), r["label"]


def test_the_two_centre_forms_agree_on_a_symmetric_row_only():
    name, t, i = gc.SYMMETRIC
    L = gc.launches()[name]
    ng = L["n_gauss"]
    assert gc.ASYMMETRIC[:2] == (name, t)
    sym, asym = L["tracks"][t][i], L["tracks"][t][gc.ASYMMETRIC[2]]
    assert sym["n"][0] == -sym["n"][-1] and asym["n"][0] != -asym["n"][-1] and asym["cnt"] == 7 + 16 + 1
    for k, r in ((i, sym), (gc.ASYMMETRIC[2], asym)):
        n = r["n"]
        w = gr.fit_rows([n], [r["mue"]], ng, dtype=LD)["w"][0]
        cd = gr.center_dist(n, ng)
        q = gc.eval_positions(r)
        d = np.max(np.abs(gr.model_gauss(q, w, cd, ng, n[0], n[-1]) - gr.model_gauss(q, w, cd, ng, mintime=True)))
        assert (d < 1e-9) == (k == i), "row %d: the forms differ by %.3e" % (k, float(d))
