"""Open chains on the MI355X: the open goldens (tests/golden/open_handling_*.npz, scripts/make_golden_open.py), the drop-in chain
calc_splines -> opt_min_curv(closed=False, ...), a launch of 1024 chains of 2000 waypoints, and mixed ring + chain batches."""
import numpy as np
import pytest

import open_ref
from conftest import load_golden
from global_racetrajectory_optimization_amd import engine, synthetic
from global_racetrajectory_optimization_amd import trajectory_planning_helpers as tph
from global_racetrajectory_optimization_amd.trajectory_planning_helpers import opt_min_curv as omc

pytestmark = pytest.mark.gpu

OPEN_GOLDENS = ("open_handling_a", "open_handling_fix_s", "open_handling_fix_se", "open_handling_kappa")
CONTRACT = 1e-6      # the project's parity contract against the oracle (metres)
GUARD = 1e-8         # a tight guard on top: what the engine actually achieves on these fixtures


def _prob(g):
    return dict(reftrack=g["reftrack"], normvec=g["normvec"], scaling=g["scaling"], kappa_bound=float(g["kappa_bound"]),
                w_veh=float(g["w_veh"]))


def _ends(g):
    return dict(psi_s=float(g["psi_s"]), psi_e=float(g["psi_e"]), fix_s=bool(g["fix_s"]), fix_e=bool(g["fix_e"]))


@pytest.mark.parametrize("name", OPEN_GOLDENS)
def test_open_goldens(gpu_engine, name):
    g = load_golden(name)
    al, curv, st, _ = gpu_engine.solve_batch([_prob(g)], ends=[_ends(g)])
    d = float(np.max(np.abs(al[0] - g["alpha"])))
    assert st[0] == 0
    assert d < CONTRACT                  # contract
    assert d < GUARD                     # guard
    assert abs(curv[0] - float(g["curv_error_max"])) < 1e-9
    if bool(g["fix_s"]):
        assert abs(al[0][0]) <= engine.FIX_HALF_WIDTH + 1e-12
    if bool(g["fix_e"]):
        assert abs(al[0][-1]) <= engine.FIX_HALF_WIDTH + 1e-12


def test_drop_in_open_chain_against_golden():
    """calc_splines(path, psi_s=, psi_e=) -> opt_min_curv(closed=False, ...) on the handling arc, as a tph user would call it."""
    g = load_golden("open_handling_a")
    ref = g["reftrack"]
    _, _, A, _ = tph.calc_splines.calc_splines(ref[:, :2], psi_s=float(g["psi_s"]), psi_e=float(g["psi_e"]))
    alpha, curv = tph.opt_min_curv.opt_min_curv(ref, g["normvec"], A, float(g["kappa_bound"]), float(g["w_veh"]), closed=False,
                                                psi_s=float(g["psi_s"]), psi_e=float(g["psi_e"]))
    assert np.max(np.abs(alpha - g["alpha"])) < CONTRACT
    assert abs(curv - float(g["curv_error_max"])) < 1e-9
    with pytest.raises(RuntimeError, match="Headings must be provided"):
        tph.opt_min_curv.opt_min_curv(ref, g["normvec"], A, 0.12, 3.4, closed=False, psi_s=0.0)
    with pytest.raises(RuntimeError, match="wrong dimensions"):
        tph.opt_min_curv.opt_min_curv(ref, g["normvec"], np.eye(4 * ref.shape[0]), 0.12, 3.4, closed=False, psi_s=0.0, psi_e=0.0)
    # the batch form with the same keys, mixed with the closed handling track
    h = load_golden("handling_track")
    res = omc.opt_min_curv_batch([dict(reftrack=h["reftrack"], normvectors=h["normvec"], scaling=h["scaling"], kappa_bound=0.12, w_veh=3.4),
                                  dict(reftrack=ref, normvectors=g["normvec"], A=A, kappa_bound=float(g["kappa_bound"]),
                                       w_veh=float(g["w_veh"]), closed=False, psi_s=float(g["psi_s"]), psi_e=float(g["psi_e"]))])
    assert list(res[2]) == [0, 0]
    assert np.max(np.abs(res[0][1] - g["alpha"])) < CONTRACT


def _arcs(count, n=2000):
    """`count` open arcs of n waypoints cut from the config-3 generator's rings: the first n waypoints of rings of n + 400."""
    refs, nvs, _ = synthetic.oval_batch(count, n + 400)
    return np.ascontiguousarray(refs[:, :n]), np.ascontiguousarray(nvs[:, :n])


def _headings(ref):
    d0 = ref[:, 1, :2] - ref[:, 0, :2]
    d1 = ref[:, -1, :2] - ref[:, -2, :2]
    return np.arctan2(d0[:, 1], d0[:, 0]) - np.pi / 2, np.arctan2(d1[:, 1], d1[:, 0]) - np.pi / 2


def test_1024_chains_of_2000(gpu_engine):
    refs, nvs = _arcs(1024)
    ps, pe = _headings(refs)
    probs = []
    for k in range(1024):
        el = np.sqrt(np.sum(np.diff(refs[k, :, :2], axis=0) ** 2, axis=1))
        sc = np.concatenate((el[:-1] / el[1:], [1.0, 1.0]))
        probs.append(dict(reftrack=refs[k], normvec=nvs[k], scaling=sc, kappa_bound=0.12, w_veh=3.4))
    ends = [dict(psi_s=float(ps[k]), psi_e=float(pe[k]), fix_s=k % 3 == 0, fix_e=k % 5 == 0) for k in range(1024)]
    al, curv, st, info = gpu_engine.solve_batch(probs, ends=ends)
    assert np.all(st == 0), np.unique(st, return_counts=True)
    rng = np.random.default_rng(0)
    sample = rng.choice(1024, size=16, replace=False)
    for k in sample:
        a1, c1, s1, _ = gpu_engine.solve_batch([probs[k]], ends=[ends[k]])
        assert s1[0] == 0 and a1[0].tobytes() == al[k].tobytes() and c1[0] == curv[k]
        ag, _, sg, _ = gpu_engine.solve_batch([probs[k]], ends=[ends[k]], algorithm=engine.ALG_GI)
        assert sg[0] == 0 and np.max(np.abs(ag[0] - al[k])) < 1e-9
    # KKT certificate against the dense oracle's E_kappa (two of the sample: an 8000 x 8000 inverse each)
    from oracle import qp_ref
    from global_racetrajectory_optimization_amd.trajectory_planning_helpers import calc_splines as cs
    for k in sample[:2]:
        A = cs.build_open_les_matrix(2000, probs[k]["scaling"][:-2])
        H, f, E, k_ref, _ = open_ref.assemble_open(refs[k], nvs[k], A, float(ps[k]), float(pe[k]))
        hi, lo = open_ref.bounds_open(refs[k], 3.4, ends[k]["fix_s"], ends[k]["fix_e"])
        G = np.vstack((np.eye(2000), -np.eye(2000), E, -E))
        h = np.concatenate((hi, lo, 0.12 - k_ref, 0.12 + k_ref))
        r = qp_ref.kkt_residuals(H, f, G, h, al[k])
        assert r["stationarity"] <= 1e-9 and r["primal"] <= 1e-9


def test_mixed_batch_rings_bitwise(gpu_engine):
    h = load_golden("handling_track")
    b = load_golden("berlin_2018")
    rings = [dict(reftrack=g["reftrack"], normvec=g["normvec"], scaling=g["scaling"], kappa_bound=float(g["kappa_bound"]),
                  w_veh=float(g["w_veh"])) for g in (h, b)]
    chains = [_prob(load_golden(nm)) for nm in OPEN_GOLDENS]
    cends = [_ends(load_golden(nm)) for nm in OPEN_GOLDENS]
    a0, c0, s0, _ = gpu_engine.solve_batch(rings)
    a1, c1, s1, _ = gpu_engine.solve_batch([rings[0], chains[0], chains[1], rings[1], chains[2], chains[3]],
                                           ends=[None, cends[0], cends[1], dict(closed=True), cends[2], cends[3]])
    assert list(s1) == [0] * 6
    for k, j in ((0, 0), (3, 1)):
        assert a1[k].tobytes() == a0[j].tobytes() and c1[k] == c0[j] and s1[k] == s0[j]
    for k, nm in ((1, OPEN_GOLDENS[0]), (2, OPEN_GOLDENS[1]), (4, OPEN_GOLDENS[2]), (5, OPEN_GOLDENS[3])):
        assert np.max(np.abs(a1[k] - load_golden(nm)["alpha"])) < CONTRACT
