"""Open chains (opt_min_curv(..., closed=False, psi_s, psi_e, fix_s, fix_e), calc_splines(path, psi_s=, psi_e=)) without a GPU: the host
spline path against the dense open solve of tests/open_ref.py, the open-matrix scalings, and the UNCHANGED kernel sources on the SIMT
interpreter (tests/emu) against the dense oracle."""
import os

import numpy as np
import pytest

import open_ref
from conftest import GOLDEN_DIR
from global_racetrajectory_optimization_amd import engine
from global_racetrajectory_optimization_amd.trajectory_planning_helpers import calc_splines as cs


@pytest.fixture(scope="module")
def emu(emu_lib):
    eng = engine.Engine(0, lib_path=emu_lib)
    yield eng
    eng.close()


_path = open_ref.seeded_path
_chain = open_ref.seeded_chain


def _solve(eng, ref, nv, A, kb, wv, ps, pe, fs=False, fe=False, **kw):
    al, curv, st, info = eng.solve_batch([dict(reftrack=ref, normvec=nv, scaling=open_ref.scalings_of(A), kappa_bound=kb, w_veh=wv)],
                                         ends=[dict(psi_s=ps, psi_e=pe, fix_s=fs, fix_e=fe)], **kw)
    return al[0], float(curv[0]), int(st[0]), info[0]


# ---- host: calc_splines ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("el,dist", [(False, True), (True, True), (False, False)])
def test_calc_splines_open_matches_dense_solve(el, dist):
    xy = _path(41, 3)
    lengths = np.sqrt(np.sum(np.diff(xy, axis=0) ** 2, axis=1)) * 1.01 if el else None
    ps, pe = 0.3, -0.2
    got = cs.calc_splines(xy, el_lengths=lengths, psi_s=ps, psi_e=pe, use_dist_scaling=dist)
    ref = open_ref.calc_splines_open(xy, el_lengths=lengths, psi_s=ps, psi_e=pe, use_dist_scaling=dist)
    assert got[0].shape == (40, 4) and got[2].shape == (160, 160) and got[3].shape == (40, 2)
    for a, b in zip(got, ref):
        assert np.max(np.abs(a - b)) < 1e-12 * max(1.0, np.max(np.abs(b)))
    assert np.count_nonzero(got[2]) == 12 * 41 - 15


def test_calc_splines_open_needs_headings():
    xy = _path(10, 1)
    with pytest.raises(RuntimeError, match="Headings must be provided for unclosed spline calculation!"):
        cs.calc_splines(xy, psi_s=0.1)
    with pytest.raises(RuntimeError, match="Headings must be provided for unclosed spline calculation!"):
        open_ref.calc_splines_open(xy, psi_e=0.1)


def test_les_scalings_open_accepts_the_matrix_and_rejects_a_perturbed_one(emu_lib, monkeypatch):
    monkeypatch.setattr(engine, "_LIB_FOR_HOST_HELPERS", engine.load_library(emu_lib))
    xy = _path(30, 5)
    _, _, A, _ = cs.calc_splines(xy, psi_s=0.0, psi_e=0.1)
    s = engine.les_scalings(A, closed=False)
    el = np.sqrt(np.sum(np.diff(xy, axis=0) ** 2, axis=1))
    assert s.shape == (30,) and np.allclose(s[:-2], el[:-1] / el[1:], rtol=1e-15) and np.all(s[-2:] == 1.0)
    assert np.array_equal(s, cs.scalings_from_open_les_matrix(A))
    for (r, c) in [(5, 17), (A.shape[0] - 1, A.shape[0] - 1), (A.shape[0] - 2, 0), (2, 5)]:
        B = A.copy()
        B[r, c] += 0.5
        with pytest.raises(RuntimeError):
            engine.les_scalings(B, closed=False)
        with pytest.raises(RuntimeError):
            cs.scalings_from_open_les_matrix(B)
    with pytest.raises(RuntimeError):          # a closed system's matrix is not an open one
        engine.les_scalings(cs.build_les_matrix(30, np.ones(30)), closed=False)


# ---- the kernels on the SIMT interpreter -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [7, 20, 33, 64, 70, 300])
def test_chains_match_dense_oracle(emu, n):
    """One to sixteen separators (n >= 48), the heading rows at both ends, fix clamps, box-only and with curvature rows."""
    ref, nv, A, ps, pe = _chain(n, n)
    _, _, _, k_ref, _ = open_ref.assemble_open(ref, nv, A, ps, pe)
    cases = [(1e3, False, False), (1e3, True, True), (0.9 * float(np.max(np.abs(k_ref))), False, True)]
    for kb, fs, fe in cases:
        a_ref, e_ref = open_ref.opt_min_curv_open(ref, nv, A, kb, 2.0, ps, pe, fs, fe)
        al, curv, st, info = _solve(emu, ref, nv, A, kb, 2.0, ps, pe, fs, fe)
        assert st == 0
        assert np.max(np.abs(al - a_ref)) < 1e-9
        assert abs(curv - e_ref) < 1e-10
        if fs:
            assert abs(al[0]) <= engine.FIX_HALF_WIDTH + 1e-12
        if fe:
            assert abs(al[-1]) <= engine.FIX_HALF_WIDTH + 1e-12


def test_curvature_rows_active_on_a_chain(emu):
    ref, nv, A, ps, pe = _chain(64, 11)
    _, _, E, k_ref, _ = open_ref.assemble_open(ref, nv, A, ps, pe)
    a_box, _ = open_ref.opt_min_curv_open(ref, nv, A, 1e3, 2.0, ps, pe)
    kb = 0.8 * float(np.max(np.abs(k_ref + E @ a_box)))
    a_ref, e_ref = open_ref.opt_min_curv_open(ref, nv, A, kb, 2.0, ps, pe)
    al, curv, st, info = _solve(emu, ref, nv, A, kb, 2.0, ps, pe)
    assert st == 0 and info["n_active_kappa"] >= 1
    assert np.max(np.abs(al - a_ref)) < 1e-9 and abs(curv - e_ref) < 1e-10


def test_fixed_narrow_end_solves_and_unfixed_is_infeasible(emu):
    ref, nv, A, ps, pe = _chain(33, 4)
    ref = ref.copy()
    ref[-1, 2:] = 1.0                        # w_r + w_l < w_veh at the last waypoint
    al, curv, st, _ = _solve(emu, ref, nv, A, 1e3, 2.5, ps, pe, False, False)
    assert st == engine.STATUS_INFEASIBLE
    with pytest.raises(RuntimeError, match="too small"):
        open_ref.opt_min_curv_open(ref, nv, A, 1e3, 2.5, ps, pe)
    a_ref, e_ref = open_ref.opt_min_curv_open(ref, nv, A, 1e3, 2.5, ps, pe, False, True)
    al, curv, st, _ = _solve(emu, ref, nv, A, 1e3, 2.5, ps, pe, False, True)
    assert st == 0 and np.max(np.abs(al - a_ref)) < 1e-9 and abs(curv - e_ref) < 1e-10


def test_heading_rows_are_unscaled(emu):
    """tph.opt_min_curv's heading rows are the UNIT heading vectors (calc_splines scales its own by the element lengths): the engine
    reproduces that quirk.  The scaled variant gives a visibly different alpha, so this fails if the heading rows were ever scaled."""
    ref, nv, A, ps, pe = _chain(40, 8)
    a_unit, _ = open_ref.opt_min_curv_open(ref, nv, A, 1e3, 2.0, ps, pe)
    a_scaled, _ = open_ref.opt_min_curv_open(ref, nv, A, 1e3, 2.0, ps, pe, scaled_headings=True)
    al, _, st, _ = _solve(emu, ref, nv, A, 1e3, 2.0, ps, pe)
    assert st == 0
    assert np.max(np.abs(a_unit - a_scaled)) > 1e-3
    assert np.max(np.abs(al - a_unit)) < 1e-9
    assert np.max(np.abs(al - a_scaled)) > 1e-4


def test_mixed_batch_rings_bitwise(emu, golden):
    g = golden["rounded_rectangle"]
    ring = dict(reftrack=g["reftrack"], normvec=g["normvec"], scaling=g["scaling"], kappa_bound=float(g["kappa_bound"]), w_veh=float(g["w_veh"]))
    ref, nv, A, ps, pe = _chain(70, 2)
    ch = dict(reftrack=ref, normvec=nv, scaling=open_ref.scalings_of(A), kappa_bound=1e3, w_veh=2.0)
    a0, c0, s0, _ = emu.solve_batch([ring, ring])
    a1, c1, s1, _ = emu.solve_batch([ring, ch, ring], ends=[None, dict(psi_s=ps, psi_e=pe), dict(closed=True, psi_s=np.nan)])
    assert list(s1) == [0, 0, 0]
    for k, j in ((0, 0), (2, 1)):
        assert a1[k].tobytes() == a0[j].tobytes() and c1[k] == c0[j]
    a_ref, e_ref = open_ref.opt_min_curv_open(ref, nv, A, 1e3, 2.0, ps, pe)
    assert np.max(np.abs(a1[1] - a_ref)) < 1e-9


def test_goldfarb_idnani_route_on_chains(emu):
    for n, seed in ((33, 1), (70, 2)):
        ref, nv, A, ps, pe = _chain(n, seed)
        _, _, _, k_ref, _ = open_ref.assemble_open(ref, nv, A, ps, pe)
        kb = 0.9 * float(np.max(np.abs(k_ref)))
        al, _, st, _ = _solve(emu, ref, nv, A, kb, 2.0, ps, pe, True, False)
        ag, _, sg, ig = _solve(emu, ref, nv, A, kb, 2.0, ps, pe, True, False, algorithm=engine.ALG_GI)
        assert st == 0 and sg == 0 and ig["gi_iters"] > 0
        assert np.max(np.abs(al - ag)) < 1e-9


def test_chain_argument_checks(emu):
    ref, nv, A, ps, pe = _chain(20, 3)
    sc = open_ref.scalings_of(A)
    p = dict(reftrack=ref, normvec=nv, scaling=sc, kappa_bound=1e3, w_veh=2.0)
    _, _, st, _ = emu.solve_batch([p, p], ends=[dict(psi_s=np.nan, psi_e=pe), dict(psi_s=ps, psi_e=np.inf)])
    assert list(st) == [engine.STATUS_BAD_INPUT] * 2
    with pytest.raises(engine.EngineError):
        emu.solve_batch([dict(p, normvec=None)], ends=[dict(psi_s=ps, psi_e=pe)])
    with pytest.raises(engine.EngineError):
        emu.solve_batch([p], ends=[dict(psi_s=ps, psi_e=pe)], objective=engine.OBJ_SHORTEST_PATH)


def test_chain_beyond_lds_route_is_bad_input(emu):
    n = 2049
    xy = _path(n, 9, step=1.0)
    ref = np.column_stack((xy, np.full((n, 2), 3.0)))
    nv = np.tile([0.0, -1.0], (n, 1))
    _, _, st, _ = emu.solve_batch([dict(reftrack=ref, normvec=nv, scaling=None, kappa_bound=1e3, w_veh=2.0)], ends=[dict(psi_s=0.0, psi_e=0.0)])
    assert st[0] == engine.STATUS_BAD_INPUT


@pytest.fixture(scope="module")
def kc_emu(tmp_path_factory):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path_factory.mktemp("kc") / "kc_emu")
    subprocess.run(["g++", "-O2", "-std=c++17", "-x", "c++", "-I", os.path.join(root, "tests", "emu", "include"), "-o", exe,
                    os.path.join(root, "scripts", "kkt_check.hip"), "-Wno-unused-result", "-Wno-attributes"], check=True)
    return exe


@pytest.mark.parametrize("n,fused,pinned", [(20, 0, 0.0), (333, 0, 0.0), (333, 1, 0.3), (1000, 1, 0.9)])
def test_chain_elimination_in_isolation(kc_emu, n, fused, pinned):
    """The saddle-point elimination of csrc/mcq_kkt.inc on OPEN chains (Lo_0 = 0, the last segment's right spike zero, the separators'
    system without its wrap blocks): scripts/kkt_check.hip with its chain switch, against the dense reduced system of the chain's own T and
    R -- one segment (n < 48) and sixteen, fused right-hand side, pinned waypoints."""
    import re
    import subprocess
    out = subprocess.run([kc_emu, str(n), "2", "2", "12", "1", str(fused), str(pinned), "1"], check=True, capture_output=True, text=True).stdout
    m = re.search(r"factor status (\d+), entries differing from the first solution (\d+) .* NaNs (\d+)", out)
    assert m and m.group(1) == "0" and m.group(2) == "0" and m.group(3) == "0", out
    berr = float(re.search(r"backward error .*: ([0-9.e+-]+)", out).group(1))
    assert berr <= 1e-13, out


# ---- the edge fixtures (tests/golden/open_edges.npz, open_kappa_fuzz.npz) on the interpreter: their small members ----------------------
CONTRACT = 1e-6      # the project's parity contract against the oracle (metres); the guard is the fixture's own (OpenFixture.guard)


@pytest.fixture(scope="module")
def edge_fx():
    return open_ref.OpenFixture(os.path.join(GOLDEN_DIR, "open_edges.npz"))


def _fx_solve(eng, fx, ks, **kw):
    return eng.solve_batch([fx.problem(k) for k in ks], ends=[fx.ends(k) for k in ks], **kw)


def test_edge_ladder_against_fixture(emu, edge_fx):
    """The ladder's n = 3 .. 73 (box only, both ends pinned, curvature rows active), the ragged chain n = 49 and the narrow end in one
    ragged launch: statuses as stored, contract + guard (max(1e-8, 4 x the fixture's alpha spread))."""
    ks = edge_fx.select(lambda k: edge_fx.family(k) != "stadium" and edge_fx.n(k) <= 129)
    assert {edge_fx.n(k) for k in ks} >= {3, 4, 5, 16, 47, 48, 49, 63, 64, 65, 71, 72, 73}
    al, curv, st, info = _fx_solve(emu, edge_fx, ks)
    print(open_ref.worst_report("interpreter ladder", open_ref.check_fixture_results(edge_fx, ks, al, curv, st, info, CONTRACT, 1e-9, {})))


def test_edge_reversal_symmetry(emu, edge_fx):
    """Each ladder length n = 4 .. 73 and its mirror in one launch, one case per length in turn (box only, both ends pinned, curvature rows:
    the interpreter runs a solve in about a second): -alpha'[::-1] is alpha within max(guard, 10 x the oracle's own reversal gap); the
    curvature errors agree within 1e-9."""
    ns = sorted({edge_fx.n(k) for k in range(len(edge_fx)) if edge_fx.family(k) == "ladder" and 4 <= edge_fx.n(k) <= 73})
    ks = edge_fx.select(lambda k: edge_fx.family(k) == "ladder" and edge_fx.n(k) in ns and edge_fx["status_ref"][k] == 0
                        and edge_fx.case(k) == "abc"[ns.index(edge_fx.n(k)) % 3])
    assert len(ks) == len(ns)
    probs, ends = [], []
    for k in ks:
        mp, me = edge_fx.mirrored(k)
        probs += [edge_fx.problem(k), mp]
        ends += [edge_fx.ends(k), me]
    al, curv, st, _ = emu.solve_batch(probs, ends=ends)
    assert np.all(st == 0), list(st)
    for j, k in enumerate(ks):
        d = float(np.max(np.abs(-al[2 * j + 1][::-1] - al[2 * j])))
        tol = max(edge_fx.guard(k), 10.0 * float(edge_fx["rev_gap"][k]))
        assert d < tol, (edge_fx.n(k), edge_fx.case(k), d, tol)
        assert abs(curv[2 * j + 1] - curv[2 * j]) < 1e-9, (edge_fx.n(k), edge_fx.case(k))


def test_kappa_fuzz_sample_against_fixture(emu):
    """Ten of the curvature-tight chain fuzz problems (the smallest; three of them the dense GI's "inconsistent"): status 0 /
    MCQ_KAPPA_INFEASIBLE as stored, contract + guard, the active curvature rows.  (The GPU suite runs all 120.)"""
    fx = open_ref.OpenFixture(os.path.join(GOLDEN_DIR, "open_kappa_fuzz.npz"))
    by_n = sorted(range(len(fx)), key=lambda k: (fx.n(k), k))
    bad = [k for k in by_n if fx["status_ref"][k] == 5][:3]
    ks = sorted(bad + [k for k in by_n if fx["status_ref"][k] == 0][:10 - len(bad)])
    assert len(bad) == 3 and len(ks) == 10
    al, curv, st, info = _fx_solve(emu, fx, ks)
    print(open_ref.worst_report("interpreter fuzz", open_ref.check_fixture_results(fx, ks, al, curv, st, info, CONTRACT, 1e-9, {},
                                                                                   n_active=True)))
