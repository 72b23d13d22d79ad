"""BASELINE's full-size shapes as stated, on the MI355X, held to the oracle's precision (tests/ring_guard.py) and not only to the 1e-6 m
contract: config 3 (mcq_iqp_batch of 1024 tracks x N = 2000, three passes, one call), config 5's per-rank shard (8192 tracks through
mcq_solve_batch_f32), the numbers bench.py itself times (--dump-outputs), and the sliced host entries with more slices than problems."""
import multiprocessing
import os
import subprocess
import sys

import numpy as np
import pytest

import ring_guard
from conftest import load_golden
from global_racetrajectory_optimization_amd import engine, synthetic
from ring_guard import dmax, guard

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = ring_guard.FIXED
WORST = ring_guard.Worst()


@pytest.fixture(scope="module", autouse=True)
def _worst_report(request):
    yield
    ring_guard.print_uncaptured(request.config, WORST.report("test_gpu_full_size"))


def _cpu_b(ref, nv, sc, kappa_bound=0.12, w_veh=3.4):
    from oracle import banded_ref
    a, c, st, _, _ = banded_ref.solve_batch(ref, nv, sc, kappa_bound, w_veh)
    assert np.all(st == 0), st
    return a, c


def test_config3_iqp_batch_as_stated(gpu_engine, monkeypatch):
    """BASELINE config 3 as stated (bench.py --full's call): iqp_handler of 1024 tracks x N = 2000 as ONE mcq_iqp_batch call.  Every track
    three rounds to 2002 waypoints; track 0's end state is the oracle chain's (oval_n2000.npz) within its guard; the round-by-round loop
    ($MCQ_IQP_FUSED=0) agrees bitwise on every track; on 16 seeded tracks the host-glue driver agrees, and CPU-B re-solving the final QP from
    the returned reftrack / normvectors (unit scalings: iqp_handler re-splines without distance scaling) returns the returned alpha."""
    from global_racetrajectory_optimization_amd.trajectory_planning_helpers import iqp_handler as iq
    bsz, n = 1024, 2000
    ref, nv, sc = synthetic.oval_batch(bsz, n=n)
    trk = dict(reftrack=ref, normvectors=nv, scaling=sc)
    monkeypatch.delenv("MCQ_IQP_FUSED", raising=False)
    res = gpu_engine.iqp_batch(trk, 0.12, 3.4, 3.0, iters_min=3, curv_error_allowed=0.01)
    assert np.all(res["status"] == 0), np.unique(res["status"])
    assert np.all(res["rounds"] == 3) and np.all(res["n"] == 2002), (np.unique(res["rounds"]), np.unique(res["n"]))
    g = load_golden("oval_n2000")
    assert np.array_equal(ref[0], g["reftrack"]) and np.array_equal(nv[0], g["normvec"]) and np.array_equal(sc[0], g["scaling"])
    d_a, d_r = dmax(res["alpha"][0], g["iqp_alpha"]), dmax(res["reftrack"][0], g["iqp_reftrack"])
    g_a, g_r = guard("oval_n2000", what="iqp_alpha"), guard("oval_n2000", what="iqp_reftrack")
    assert d_a < 1e-6 and d_r < 1e-6                                                               # contract
    assert WORST.add("config 3 vs oracle chain", d_a, g_a) < g_a and d_r < g_r, (d_a, g_a, d_r, g_r)   # guard
    # the round-by-round loop: the same arithmetic, bit for bit
    monkeypatch.setenv("MCQ_IQP_FUSED", "0")
    loop = gpu_engine.iqp_batch(trk, 0.12, 3.4, 3.0, iters_min=3, curv_error_allowed=0.01)
    monkeypatch.delenv("MCQ_IQP_FUSED")
    for key in ("n", "rounds", "status", "curv_trace", "curv_err"):
        assert np.array_equal(loop[key], res[key]), key
    for key in ("alpha", "reftrack", "normvectors"):
        assert all(np.array_equal(x, y) for x, y in zip(loop[key], res[key])), key
    # 16 seeded tracks: the host-glue driver, and CPU-B on the final QP
    pick = np.sort(np.random.default_rng(3).choice(bsz, 16, replace=False))
    stt = {}
    host = iq.iqp_handler_batch([dict(reftrack=ref[k].copy(), normvectors=nv[k], scaling=sc[k]) for k in pick], 0.12, 3.4, 3.0, 3, 0.01,
                                engine=gpu_engine, stats=stt, device_resident=False)
    assert stt["rounds"] == 3
    worst_h = 0.0
    for j, k in enumerate(pick):
        a_h = host[j][0]
        assert a_h.shape == res["alpha"][k].shape == (2002,), k
        worst_h = max(worst_h, WORST.add("host glue vs device glue", dmax(a_h, res["alpha"][k]), GUARD))
    assert worst_h < GUARD, worst_h                                                                # guard
    r_fin = np.stack([res["reftrack"][k] for k in pick])
    n_fin = np.stack([res["normvectors"][k] for k in pick])
    a_cpu, c_cpu = _cpu_b(r_fin, n_fin, np.ones(r_fin.shape[:2]))
    d_cpu = max(dmax(a_cpu[j], res["alpha"][k]) for j, k in enumerate(pick))
    assert d_cpu < 1e-6                                                                            # contract
    assert WORST.add("CPU-B", d_cpu, GUARD) < GUARD, d_cpu                                         # guard
    assert np.max(np.abs(c_cpu - res["curv_err"][pick])) < 1e-8
    print("config 3 as stated (1024 x N = 2000, 3 rounds): track 0 vs oracle chain %.1e m (guard %.1e), host glue %.1e, CPU-B %.1e" % (
        d_a, g_a, worst_h, d_cpu))


def test_config5_shard_as_stated(monkeypatch):
    """BASELINE config 5's per-rank shard as stated: generator indices 0 .. 8191 (perturbed centrelines) as MCQ_F32_INCREMENTS rows through
    mcq_solve_batch_f32 -- a workspace of about 15 GB, on an engine of its own.  Every status 0; every track feasible in the box of the rows
    the device rebuilds (one float rounding of alpha, 3e-7 m); 64 seeded tracks -- 8190 / 8191 and the golden indices among them -- against
    CPU-B on the rebuilt fp64 rows to one float rounding, the curvature error to 1e-8; the golden indices against their goldens."""
    B, n = 8192, 2000
    chunk = 256
    with multiprocessing.get_context("spawn").Pool(min(15, os.cpu_count() or 1)) as pool:          # (fresh interpreters: no GPU in them)
        parts = pool.starmap(synthetic.oval_batch, [(chunk, n, j * chunk, True) for j in range(B // chunk)])
    ref = np.concatenate([p[0] for p in parts])
    del parts
    rows32, org = engine.rows_to_increments(ref)
    eng = engine.Engine(0)
    try:
        a32, curv, st, _ = eng.solve_batch_f32(rows32, org, 0.12, 3.4, layout=engine.F32_INCREMENTS)
    finally:
        eng.close()
    assert a32.dtype == np.float32 and a32.shape == (B, n)
    assert np.all(st == 0), np.unique(st, return_counts=True)
    r64 = engine.increments_to_rows(rows32, org)
    lo, hi = -(r64[:, :, 3] - 1.7), r64[:, :, 2] - 1.7
    assert np.all(a32 >= lo - 3e-7) and np.all(a32 <= hi + 3e-7)
    golden_idx = (5, 9, 13, 21)
    others = np.setdiff1d(np.arange(B), list(golden_idx) + [8190, 8191])
    pick = sorted(list(golden_idx) + [8190, 8191] + [int(k) for k in np.random.default_rng(8192).choice(others, 58, replace=False)])
    nv64 = np.empty((len(pick), n, 2))
    sc64 = np.empty((len(pick), n))
    for j, k in enumerate(pick):
        nv64[j], sc64[j] = synthetic.prepared_track(r64[k, :, :2])
    a_cpu, c_cpu = _cpu_b(r64[pick], nv64, sc64)
    err = max(dmax(a32[k], a_cpu[j]) for j, k in enumerate(pick))
    assert err < 1e-6, err                                                  # one float rounding of |alpha| <= 4 m is 2.4e-7
    assert np.max(np.abs(curv[pick] - c_cpu)) < 1e-8
    worst = 0.0
    for idx in golden_idx:
        g = load_golden("oval_n2000_c%d" % idx)
        assert np.array_equal(g["reftrack"], ref[idx]), idx
        worst = max(worst, dmax(a32[idx], g["alpha"]))
    assert worst < 5e-5, worst
    print("config 5 shard as stated: %d tracks, 64 vs CPU-B (rebuilt rows) %.2e m, golden indices %.2e m" % (B, err, worst))


def test_bench_outputs_against_the_oracle(tmp_path):
    """What bench.py times is the right answer: the arrays of its last timed step (--dump-outputs, after the warm-up and two timed launches into
    the same workspace).  Every status 0; rows 0, 1, 2, 3, 7, 11 -- the generator's tracks whose dense-oracle goldens are committed -- within
    their guards; 32 other seeded rows against CPU-B within 1e-8; the curvature errors to 1e-9."""
    d = tmp_path / "dump"
    cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
           "--dump-outputs", str(d)]
    res = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    assert res.returncode == 0, (res.returncode, res.stdout[-2000:], res.stderr[-4000:])
    out = {k: np.load(d / (k + ".npy")) for k in ("alpha", "curv_error", "status")}
    assert not (d / "sample_rows.npy").exists()
    al, curv = out["alpha"], out["curv_error"]
    assert al.shape == (1024, 2000) and np.all(out["status"] == 0)
    for idx, name in ((0, "oval_n2000"), (1, "oval_n2000_w1"), (2, "oval_n2000_w2"), (3, "oval_n2000_w3"), (7, "oval_n2000_w7"),
                      (11, "oval_n2000_w11")):
        g = load_golden(name)
        ref, nv, sc = synthetic.oval_batch(1, n=2000, first=idx)
        assert np.array_equal(ref[0], g["reftrack"]) and np.array_equal(nv[0], g["normvec"]) and np.array_equal(sc[0], g["scaling"]), name
        dd = dmax(al[idx], g["alpha"])
        assert dd < 1e-6, (name, dd)                                                                       # contract
        assert WORST.add("bench outputs vs goldens", dd, guard(name)) < guard(name), (name, dd, guard(name))   # guard
        assert abs(curv[idx] - float(g["curv_error_max"])) < 1e-9, name
    rng = np.random.default_rng(1024)
    pick = np.sort(rng.choice(np.setdiff1d(np.arange(1024), [0, 1, 2, 3, 7, 11]), 32, replace=False))
    ref, nv, sc = synthetic.oval_batch(1024, n=2000)
    a_cpu, c_cpu = _cpu_b(ref[pick], nv[pick], sc[pick])
    d_cpu = max(dmax(al[k], a_cpu[j]) for j, k in enumerate(pick))
    assert d_cpu < 1e-6                                                                                    # contract
    assert WORST.add("bench outputs vs CPU-B", d_cpu, GUARD) < GUARD, d_cpu                                # guard
    assert np.max(np.abs(curv[pick] - c_cpu)) < 1e-9
    print("bench.py --dump-outputs (1024 x N = 2000, last timed step): 32 rows vs CPU-B %.1e m" % d_cpu)


def test_sliced_host_entries_clamp_the_slice_count(gpu_engine, monkeypatch):
    """$MCQ_HOST_SLICES = 8, $MCQ_HOST_SLICE_MIN = 4 and batches of 4, 5 and 7 problems: no empty slice (a launch of 0 workgroups was
    MCQ_E_DEVICE), bitwise the one launch -- the interpreter suite's check (tests/test_emu_kernels.py), on libmcq.so."""
    from test_emu_kernels import check_slice_count_clamped_to_the_batch
    check_slice_count_clamped_to_the_batch(gpu_engine, monkeypatch)
