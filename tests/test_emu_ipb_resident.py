"""ipm_box (csrc/mcq_kernels.hip) keeps the thread's entries of X, ZL, ZU, G in registers across the factorisation / solve calls, stores
them at the returns only and solves the corrector in V_DXA (MCQ_IPB_RESIDENT, default 1).  -DMCQ_IPB_RESIDENT=0 compiles the earlier form,
in which every pass loads what it needs and stores what it changed.  Both run here on the SIMT interpreter, side by side in one process,
and must return the same bits: the arithmetic, its order and every decision are meant to be untouched.  No tolerance anywhere: equality
or failure."""
import fcntl
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import open_ref
from conftest import ROOT, load_golden
from global_racetrajectory_optimization_amd import engine, synthetic

INFO_KEYS = ("ipm_iters", "as_iters", "refine_rounds", "f32_factorisations", "second_attempt", "kkt_res")
EMU = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "global_racetrajectory_optimization_amd", "csrc")
# tests/emu/build_emu.sh's flags
EMU_FLAGS = ["-O2", "-std=c++17", "-fPIC", "-pthread", "-x", "c++", "-I", os.path.join(EMU, "include"), "-Wno-unused-result", "-Wno-attributes"]


def _build_emu(path, defines, newer_than):
    """TEST-ONLY: an interpreter library next to libmcq_emu.so -- the same sources, build_emu.sh's flags, plus `defines`."""
    def stale():
        return not os.path.exists(path) or os.path.getmtime(newer_than) > os.path.getmtime(path)

    if stale():
        with open(path + ".lock", "w") as lock:             # (pytest-xdist workers: one builds, the others wait)
            fcntl.flock(lock, fcntl.LOCK_EX)
            if stale():
                tmp = tempfile.mkdtemp(dir=EMU)             # (here: the final rename must stay inside one file system)
                try:
                    procs = [subprocess.Popen(["g++"] + EMU_FLAGS + defines + ["-c", "-o", os.path.join(tmp, f + ".o"), os.path.join(CSRC, f + ".hip")],
                                              stderr=subprocess.DEVNULL) for f in ("mcq_kernels", "mcq_api")]
                    assert all(p.wait() == 0 for p in procs), "the interpreter library with %s does not compile" % " ".join(defines)
                    subprocess.run(["g++", "-shared", "-fPIC", "-pthread", "-o", os.path.join(tmp, "lib.so"), os.path.join(tmp, "mcq_kernels.o"),
                                    os.path.join(tmp, "mcq_api.o"), "-ldl"], check=True)
                    os.replace(os.path.join(tmp, "lib.so"), path)
                finally:
                    shutil.rmtree(tmp, ignore_errors=True)
    return path


@pytest.fixture(scope="module")
def emu_lib_ipb0(emu_lib):
    return _build_emu(os.path.join(EMU, "libmcq_emu_ipb0.so"), ["-DMCQ_IPB_RESIDENT=0"], emu_lib)


@pytest.fixture(scope="module")
def pair(emu_lib, emu_lib_ipb0):
    """(engine on the resident form, engine on the earlier form)"""
    a, b = engine.Engine(0, lib_path=emu_lib), engine.Engine(0, lib_path=emu_lib_ipb0)
    yield a, b
    a.close()
    b.close()


def _info(info, k, key):
    return info[k][key] if isinstance(info[k], dict) else getattr(info[k], key)


def _same(ra, rb, what):
    """(alpha, curv_error, status, info) of the two libraries, bit for bit."""
    al_a, curv_a, st_a, info_a = ra
    al_b, curv_b, st_b, info_b = rb
    assert len(al_a) == len(al_b)
    for k in range(len(al_a)):
        assert np.array_equal(al_a[k], al_b[k]), (what, k, "alpha")
        for key in INFO_KEYS:
            assert _info(info_a, k, key) == _info(info_b, k, key), (what, k, key, _info(info_a, k, key), _info(info_b, k, key))
    assert np.array_equal(curv_a, curv_b), (what, "curv_error")
    assert np.array_equal(st_a, st_b), (what, "status")


def _both(pair, what, call, interior_point=True):
    ra, rb = call(pair[0]), call(pair[1])
    _same(ra, rb, what)
    if interior_point:          # the comparison says something about ipm_box only where ipm_box ran
        assert all(_info(ra[3], k, "ipm_iters") > 0 for k in range(len(ra[0]))), what
    return ra


def _oval(n, seed=0):
    """A bench oval of n waypoints (synthetic.widths needs n >= 15: below that, widths drawn directly)."""
    if n >= 15:
        ref, nv, sc = synthetic.oval_batch(1, n=n, first=seed)
        return ref[0], nv[0], sc[0]
    xy = synthetic.oval_centreline(n)
    nv, sc = synthetic.prepared_track(xy)
    return np.column_stack((xy, 5.0 + np.random.default_rng(seed).uniform(-1.5, 1.5, size=(n, 2)))), nv, sc


# the edges of `tid + 256 u < n` (entries a thread owns: 256 threads, up to eight each) and of the LDS routes
@pytest.mark.parametrize("n", [3, 47, 48, 255, 256, 257, 333, 2000, 2047, 2048])
def test_ovals_at_the_ownership_edges(pair, n):
    ref, nv, sc = _oval(n)
    _both(pair, "oval n=%d" % n, lambda e: e.solve_batch([dict(reftrack=ref, normvec=nv, scaling=sc, kappa_bound=0.12, w_veh=3.4)]))


def test_zero_width_waypoints(pair):
    """any_fixed: pinned rows (state 2) ride through the masked factorisation; the resident copies of such entries are never updated."""
    g = load_golden("handling_track")
    ref = g["reftrack"].copy()
    for i, shift in ((5, 0.2), (40, -0.35), (41, 0.1)):
        ref[i, 2], ref[i, 3] = 1.0 + shift, 1.0 - shift
    ra = _both(pair, "zero width", lambda e: e.solve_batch([dict(reftrack=ref, normvec=g["normvec"], scaling=g["scaling"], kappa_bound=0.12, w_veh=2.0)]))
    assert ra[2][0] == 0 and all(abs(ra[0][0][i] - s) < 1e-12 for i, s in ((5, 0.2), (40, -0.35), (41, 0.1)))


def test_open_chain(pair):
    ref, nv, A, ps, pe = open_ref.seeded_chain(300, 300)
    for fs, fe in ((False, False), (True, True)):
        ra = _both(pair, "chain fix %d%d" % (fs, fe), lambda e: e.solve_batch(
            [dict(reftrack=ref, normvec=nv, scaling=open_ref.scalings_of(A), kappa_bound=1e3, w_veh=2.0)], ends=[dict(psi_s=ps, psi_e=pe, fix_s=fs, fix_e=fe)]))
        assert ra[2][0] == 0


def test_fp32_row_entry(pair):
    g = load_golden("rounded_rectangle")
    ref = g["reftrack"].copy()
    ref[:, :2] += np.array([1500.0, -900.0])
    rows32, org = engine.rows_to_increments(ref[None])
    ra = _both(pair, "fp32 rows", lambda e: e.solve_batch_f32(rows32, org, 0.12, 3.4, layout=engine.F32_INCREMENTS))
    assert ra[2][0] == 0


def test_iqp_rounds_kernel_with_warm_started_passes(pair):
    """mcq_iqp_rounds_kernel calls ipm_box through solve_body; the later passes start from the carried working set."""
    g, h = load_golden("rounded_rectangle"), load_golden("handling_track")
    res = [e.iqp_batch([dict(reftrack=g["reftrack"].copy(), normvectors=g["normvec"], scaling=g["scaling"]),
                        dict(reftrack=h["reftrack"].copy(), normvectors=h["normvec"], scaling=h["scaling"])], 0.12, 3.4, 3.0, 3, 0.01) for e in pair]
    for key in ("alpha", "reftrack", "normvectors"):
        for k in range(2):
            assert np.array_equal(res[0][key][k], res[1][key][k]), (key, k)
    for key in ("n", "curv_err", "status", "rounds", "curv_trace"):
        assert np.array_equal(res[0][key], res[1][key]), key
    assert list(res[0]["status"]) == [0, 0] and list(res[0]["rounds"]) == [3, 4]


def degenerate_ring(eng, n=120):
    """A ring on which the first active-set attempt runs out of its rounds: every second upper bound lies 1e-8 m INSIDE the optimum of the
    problem without those bounds -- sixty rows that are active with multipliers of next to nothing, which the pairs at mu = 1e-10 do not
    separate.  The driver then resumes the interior point, ipm_box(c, 1e-13, true)."""
    ref, nv, sc = _oval(n)
    wide = ref.copy()
    wide[:, 2:] = 60.0
    al, _, st, _ = eng.solve_batch([dict(reftrack=wide, normvec=nv, scaling=sc, kappa_bound=5.0, w_veh=2.0)])
    assert st[0] == 0
    wide[::2, 2] = al[0][::2] + 1.0 - 1e-8
    return dict(reftrack=wide, normvec=nv, scaling=sc, kappa_bound=5.0, w_veh=2.0)


def test_resumed_attempt(pair):
    """ipm_box(c, 1e-13, true): starts from the pairs in memory (so the first attempt's returns must have stored them), recomputes the
    gradient before its resident load, and ends on a stalled complementarity or a failed factorisation with the last completed iteration
    in memory.  The bit is asserted: this test must not silently stop covering the path."""
    p = degenerate_ring(pair[0])
    ra = _both(pair, "resumed attempt", lambda e: e.solve_batch([p]))
    assert ra[3][0]["second_attempt"] & 1, ra[3][0]
    assert ra[2][0] == 0


_TRACE_SCRIPT = r'''
import sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import test_emu_ipb_resident as t
from conftest import load_golden
from global_racetrajectory_optimization_amd import engine
eng = engine.Engine(0, lib_path=sys.argv[2])
probs = [t.degenerate_ring(eng)]
for n in (47, 257, 2000):
    ref, nv, sc = t._oval(n)
    probs.append(dict(reftrack=ref, normvec=nv, scaling=sc, kappa_bound=0.12, w_veh=3.4))
g = load_golden("handling_track")
ref = g["reftrack"].copy()
ref[5, 2:], ref[40, 2:] = (1.2, 0.8), (0.65, 1.35)
probs.append(dict(reftrack=ref, normvec=g["normvec"], scaling=g["scaling"], kappa_bound=0.12, w_veh=2.0))
for p in probs:                     # one problem per launch: the lines of two workgroups would interleave
    print("problem", flush=True)
    al, curv, st, info = eng.solve_batch([p])
    print("status %d second_attempt %d" % (st[0], info[0]["second_attempt"]), flush=True)
'''


def test_every_iterate_bit_for_bit(emu_lib, tmp_path):
    """What the solver returns is the vertex the active-set phase ends on, which forgives an interior point that is off in its last bits
    (measured while writing this: with the reload of G after gradient() taken out, every comparison above still passes).  So the iterates
    themselves: -DIPM_TRACE builds of both forms print, at every evaluation of pass 1, the complementarity mu (a sum over X, ZL, ZU of
    every entry) and the dual residual (a maximum over G, ZL, ZU) with all their bits (%a).  The two traces must be the same text."""
    import sys
    libs = [_build_emu(os.path.join(EMU, "libmcq_emu_trace_ipb%d.so" % r), ["-DIPM_TRACE", "-DMCQ_IPB_RESIDENT=%d" % r], emu_lib) for r in (1, 0)]
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
