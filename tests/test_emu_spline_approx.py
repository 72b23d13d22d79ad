"""The spline-approximation kernels (mcq_spline_length_kernel, mcq_spline_search_kernel, mcq_spline_finish_kernel, mcq_min_width_kernel behind
mcq_spline_approx_device / mcq_min_width_device) on the SIMT interpreter (tests/emu), UNCHANGED sources: every case of
tests/spline_approx_cases.py against the reference of tests/spline_approx_ref.py under the rules of tests/spline_approx_guard.py.
tests/test_gpu_spline_approx.py runs the same bodies (tests/spline_approx_checks.py) on the MI355X, where the code object and the device's
division, sqrt and hypot are what is tested; here the kernels' logic is."""
import pytest

import spline_approx_cases as sc
import spline_approx_checks as ck
from conftest import load_golden
from global_racetrajectory_optimization_amd import engine
from ring_guard import Worst

WORST = Worst()


@pytest.fixture(scope="module")
def emu(emu_lib):
    eng = engine.Engine(0, lib_path=emu_lib)
    for sym in ("mcq_spline_approx_device", "mcq_min_width_device"):
        assert sym in engine.EXPORTED_SYMBOLS and hasattr(eng.lib, sym)
    yield eng
    eng.close()


@pytest.mark.parametrize("name", sc.CASES)
def test_case_against_the_reference(emu, name):
    ck.check_case(emu, name, WORST)


@pytest.mark.parametrize("name", ("n3", "len256"))
def test_m_at_and_beyond_mmax(emu, name):
    ck.check_mmax(emu, name)


def test_mixed_launch_alone_reversed_and_a_nan_track(emu):
    ck.check_batch(emu, WORST)


def test_status_and_arguments(emu):
    ck.check_status_and_arguments(emu)


def test_min_width_below_at_and_above(emu):
    ck.check_min_width(emu)


@pytest.mark.parametrize("name,key", (("rounded_rectangle", "rr_mincurv"), ("berlin_2018", "berlin_mincurv")))
def test_prep_track_to_solve(emu, name, key):
    ck.check_end_to_end(emu, name, key, load_golden(name), load_golden("harness_runs"), WORST)


def test_shim_route_returns_the_host_route_and_prints_its_line(emu, monkeypatch, capsys):
    """MCQ_PREP_DEVICE=1: tph.spline_approximation goes through the device entry behind the fit; default route and print line as before."""
    pytest.importorskip("scipy")
    import numpy as np
    from global_racetrajectory_optimization_amd.trajectory_planning_helpers import spline_approximation as sa
    track = sc.case("rounded_rectangle")["track"]
    monkeypatch.delenv("MCQ_PREP_DEVICE", raising=False)
    host = sa.spline_approximation(track, debug=True)
    line = capsys.readouterr().out
    assert line.startswith("Spline approximation: mean deviation ")
    monkeypatch.setattr(engine, "_DEFAULT_ENGINE", emu)
    monkeypatch.setenv("MCQ_PREP_DEVICE", "1")
    dev = sa.spline_approximation(track, debug=True)
    assert capsys.readouterr().out == line
    assert dev.shape == host.shape and float(np.max(np.abs(dev - host))) <= 1e-9      # (the project's floor for lengths)


def test_report(emu):
    """The worst deviation per case and quantity next to its guard (what the interpreter achieves; the GPU file prints its own)."""
    print(WORST.report("spline approximation on the interpreter", what="deviation"))
