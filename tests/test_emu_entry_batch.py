"""The vector loops between the solver's streaming phases issue the loads of several entries before the first dependent use: the spike
correction at the end of solve_kkt<> (MCQ_KKT_CORR_BATCH, csrc/mcq_kkt.inc) takes four -- float records: eight -- of a lane's waypoints
k, k + 16, ... per trip, and the per-entry loops of the assembly, problem_scales, active_set, solve_body, write_outputs and ipm_box's
initialisation (MCQ_ENTRY_BATCH, csrc/mcq_kernels.hip) a thread's up-to-eight entries tid + 256 u.  With the switches at 0 the sources compile to the earlier loops, one
entry per trip.  Both forms run here on the SIMT interpreter, side by side in one process, and must return the same bits: the arithmetic,
its order and every decision are meant to be untouched.  No tolerance anywhere: equality or failure.  The third switch of the same
work, MCQ_IPB_FOLD_P1 (pass 3 of ipm_box ends with pass 1 of the next iteration, computed from the entries it has just updated), is
compared the same way and, because the vertex the solver returns forgives an interior point that is off in its last bits, through the
-DIPM_TRACE text of both forms as well.

The sizes sit at the edges of the batching: one segment of L = n - 1 with one separator (n = 3, 47), sixteen-lane trips around L = 16
(n = 48, 255 .. 273: segments of 15, 16 and 17 waypoints), L at 64 / 65 (n = 1040, 1041, 1057), L at 127 / 128 / 129 (n = 2047 ..
2065: the fp64 batch of 64 waypoints per lane group runs twice or a third time, the float batch of 128 once or twice), `tid + 256 u < n`
at its edges (255 / 256 / 257, 2047 / 2048), and two rings past 2048, where the entry batch runs twice and ipm() and the long-ring
tridiagonal route are in play."""
import os
import subprocess
import sys

import numpy as np
import pytest

import open_ref
from conftest import ROOT, load_golden
from global_racetrajectory_optimization_amd import engine
from test_emu_ipb_resident import EMU, _TRACE_SCRIPT, _both, _build_emu, _oval, degenerate_ring

SWITCHES_OFF = ["-DMCQ_KKT_CORR_BATCH=0", "-DMCQ_ENTRY_BATCH=0", "-DMCQ_IPB_FOLD_P1=0"]


@pytest.fixture(scope="module")
def emu_lib_eb0(emu_lib):
    return _build_emu(os.path.join(EMU, "libmcq_emu_eb0.so"), SWITCHES_OFF, emu_lib)


@pytest.fixture(scope="module")
def pair(emu_lib, emu_lib_eb0):
    """(engine on the batched loops and the folded pass, engine on the earlier form of all three)"""
    a, b = engine.Engine(0, lib_path=emu_lib), engine.Engine(0, lib_path=emu_lib_eb0)
    yield a, b
    a.close()
    b.close()


@pytest.mark.parametrize("n", [3, 47, 48, 255, 256, 257, 272, 273, 1040, 1041, 1057, 2000, 2047, 2048, 2064, 2065])
def test_ovals_at_the_edges_of_the_batching(pair, n):
    ref, nv, sc = _oval(n)
    ra = _both(pair, "oval n=%d" % n, lambda e: e.solve_batch([dict(reftrack=ref, normvec=nv, scaling=sc, kappa_bound=0.12, w_veh=3.4)]))
    assert ra[2][0] == 0


def test_zero_width_waypoints(pair):
    """Pinned rows (state 2): the batched working-set loops read LO / HI of every entry, the plain ones only of those that need them."""
    g = load_golden("handling_track")
    ref = g["reftrack"].copy()
    for i, shift in ((5, 0.2), (40, -0.35), (41, 0.1)):
        ref[i, 2], ref[i, 3] = 1.0 + shift, 1.0 - shift
    ra = _both(pair, "zero width", lambda e: e.solve_batch([dict(reftrack=ref, normvec=g["normvec"], scaling=g["scaling"], kappa_bound=0.12, w_veh=2.0)]))
    assert ra[2][0] == 0 and all(abs(ra[0][0][i] - s) < 1e-12 for i, s in ((5, 0.2), (40, -0.35), (41, 0.1)))


def test_open_chain(pair):
    """The last segment's right separator is waypoint 0 with Lo = 0: the correction folds nothing of X^R there, batched or not."""
    ref, nv, A, ps, pe = open_ref.seeded_chain(300, 300)
    ra = _both(pair, "chain", lambda e: e.solve_batch(
        [dict(reftrack=ref, normvec=nv, scaling=open_ref.scalings_of(A), kappa_bound=1e3, w_veh=2.0)], ends=[dict(psi_s=ps, psi_e=pe, fix_s=True, fix_e=True)]))
    assert ra[2][0] == 0


def test_fp32_row_entry(pair):
    g = load_golden("rounded_rectangle")
    ref = g["reftrack"].copy()
    ref[:, :2] += np.array([1500.0, -900.0])
    rows32, org = engine.rows_to_increments(ref[None])
    ra = _both(pair, "fp32 rows", lambda e: e.solve_batch_f32(rows32, org, 0.12, 3.4, layout=engine.F32_INCREMENTS))
    assert ra[2][0] == 0


def test_two_tracks_through_iqp_batch(pair):
    """mcq_iqp_rounds_kernel: the later passes enter active_set with the carried working set (identify = 0: its first loop loads nothing)."""
    g, h = load_golden("rounded_rectangle"), load_golden("handling_track")
    res = [e.iqp_batch([dict(reftrack=g["reftrack"].copy(), normvectors=g["normvec"], scaling=g["scaling"]),
                        dict(reftrack=h["reftrack"].copy(), normvectors=h["normvec"], scaling=h["scaling"])], 0.12, 3.4, 3.0, 3, 0.01) for e in pair]
    for key in ("alpha", "reftrack", "normvectors"):
        for k in range(2):
            assert np.array_equal(res[0][key][k], res[1][key][k]), (key, k)
    for key in ("n", "curv_err", "status", "rounds", "curv_trace"):
        assert np.array_equal(res[0][key], res[1][key]), key
    assert list(res[0]["status"]) == [0, 0]


def test_resumed_attempt(pair):
    """The ring that runs the first active-set attempt out of its rounds: the copy of X kept for the resumed interior point, the resumed
    ipm_box (whose initialisation loads the bounds but stores no iterate) and the second attempt's identification.  The bit is asserted."""
    p = degenerate_ring(pair[0])
    ra = _both(pair, "resumed attempt", lambda e: e.solve_batch([p]))
    assert ra[3][0]["second_attempt"] & 1, ra[3][0]
    assert ra[2][0] == 0


def test_every_iterate_bit_for_bit(emu_lib, tmp_path):
    """-DIPM_TRACE builds of both forms print, at every evaluation of pass 1 -- explicit or folded into the previous pass 3 -- the
    complementarity mu and the dual residual with all their bits (%a): between them a checksum of X, ZL, ZU and G of every entry.  The
    problems are those of tests/test_emu_ipb_resident.py's trace (the resumed attempt, ovals of 47 / 257 / 2000 waypoints, pinned rows):
    the same line at the same place, so the two traces must be the same text."""
    libs = [_build_emu(os.path.join(EMU, "libmcq_emu_trace_eb%d.so" % r), ["-DIPM_TRACE"] + ([] if r else SWITCHES_OFF), emu_lib) for r in (1, 0)]
    script = tmp_path / "trace.py"
    script.write_text(_TRACE_SCRIPT)
    out = []
    for lib in libs:
        env = dict(os.environ, OMP_NUM_THREADS="1")
        env.pop("MCQ_LIB", None)
        p = subprocess.run([sys.executable, str(script), ROOT, lib], env=env, capture_output=True, text=True, timeout=900)
        assert p.returncode == 0, p.stderr[-2000:]
        out.append([l for l in p.stdout.splitlines() if l.startswith(("ipmb ", "problem", "status "))])
    n_lines = sum(1 for l in out[0] if l.startswith("ipmb "))
    assert n_lines >= 5 * 9 and any("resume 1" in l for l in out[0]), out[0][:40]           # the trace is there, the resumed attempt included
    assert all("[" in l and "nan" not in l for l in out[0] if l.startswith("ipmb "))
    assert out[0] == out[1], [(a, b) for a, b in zip(out[0], out[1]) if a != b][:5]
