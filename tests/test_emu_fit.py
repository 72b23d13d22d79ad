"""FITPACK's periodic smoothing fit on the SIMT interpreter (tests/emu), UNCHANGED sources: mcq_spline_fit_kernel behind mcq_spline_fit_device
through Engine.spline_fit_batch / prep_track_batch on every case of tests/fit_cases.py against scipy's recording and the longdouble
restatement under the rules of tests/fit_guard.py.  tests/test_gpu_fit.py runs the same bodies (tests/fit_checks.py) on the MI355X, where the
code object and the device's division and sqrt are what is tested; here the kernel's logic is.  Reads the goldens; the shim test alone needs scipy."""
import pytest

import fit_cases as fc
import fit_checks as ck
from conftest import load_golden
from global_racetrajectory_optimization_amd import engine
from ring_guard import Worst

WORST = Worst()
DEV_C = {}


@pytest.fixture(scope="module")
def emu(emu_lib):
    eng = engine.Engine(0, lib_path=emu_lib)
    assert "mcq_spline_fit_device" in engine.EXPORTED_SYMBOLS and hasattr(eng.lib, "mcq_spline_fit_device")
    yield eng
    eng.close()


@pytest.mark.parametrize("name", fc.CASES)
def test_case_against_the_recording(emu, name):
    out = ck.check_case(emu, name, WORST)
    DEV_C[name] = WORST.w[name + ".c"][0]
    assert out["status"][0] == 0


@pytest.mark.parametrize("name", ("lobe_k3_s2", "rs256"))
def test_mi_at_and_beyond_mimax(emu, name):
    ck.check_mimax(emu, name)


def test_refusals_leave_the_other_tracks_alone(emu):
    ck.check_refusals(emu)


def test_arguments(emu):
    ck.check_arguments(emu)


def test_mixed_launch_alone_reversed_and_a_refused_track(emu):
    ck.check_batch(emu, WORST)


def test_nothing_stale_survives(emu):
    ck.check_stale(emu)


@pytest.mark.parametrize("name,key", (("rounded_rectangle", "rr_mincurv"), ("berlin_2018", "berlin_mincurv")))
def test_prep_track_with_the_device_fit_to_solve(emu, name, key):
    if name not in DEV_C:
        ck.check_case(emu, name, WORST)
        DEV_C[name] = WORST.w[name + ".c"][0]
    ck.check_end_to_end(emu, name, key, load_golden(name), load_golden("harness_runs"), WORST, DEV_C[name])


def test_shim_route_returns_the_host_route_and_prints_its_line(emu, monkeypatch, capsys):
    """MCQ_FIT_DEVICE=1: tph.spline_approximation fits on the device and stays there; default route and print line as before."""
    import numpy as np
    import scipy        # noqa: F401  (the host route's own dependency: its absence is a failure, not a skip)
    from global_racetrajectory_optimization_amd.trajectory_planning_helpers import spline_approximation as sa
    track = np.load(fc.TRACKS)["rounded_rectangle.track"]
    monkeypatch.delenv("MCQ_PREP_DEVICE", raising=False)
    monkeypatch.delenv("MCQ_FIT_DEVICE", raising=False)
    called = []
    monkeypatch.setattr(sa, "_fit_on_device", lambda *a: called.append(a))
    host = sa.spline_approximation(track, debug=True)
    line = capsys.readouterr().out
    assert not called and line.startswith("Spline approximation: mean deviation ")
    monkeypatch.undo()
    monkeypatch.setattr(engine, "_DEFAULT_ENGINE", emu)
    monkeypatch.setenv("MCQ_FIT_DEVICE", "1")
    dev = sa.spline_approximation(track, debug=True)
    assert capsys.readouterr().out == line
    assert dev.shape == host.shape and float(np.max(np.abs(dev - host))) <= 1e-9      # (the project's floor for lengths)
    tri = fc.case("k3_mi4_s2")      # the recorded ier = 3: three raw rows, fitted as they are (stepsize_prep <= 0 is the device entry's form)
    with pytest.warns(RuntimeWarning, match="maximal number of iterations"):
        rows = sa.spline_approximation(np.column_stack((tri["raw"], np.full((3, 2), 3.0))), k_reg=3, s_reg=tri["s"], stepsize_prep=0.0)
    assert rows.shape[1] == 4 and np.all(np.isfinite(rows))


def test_report(emu):
    """The worst deviation per case and quantity next to its guard (what the interpreter achieves; the GPU file prints its own)."""
    print(WORST.report("periodic smoothing fit on the interpreter", what="deviation"))
