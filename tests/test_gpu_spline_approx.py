"""The spline-approximation kernels on the MI355X (mcq_spline_approx_device, mcq_min_width_device through Engine.spline_approx_batch /
min_width_batch / prep_track_batch) at their structural edges (tests/spline_approx_cases.py), against the reference of
tests/spline_approx_ref.py: decided waypoints return its closest_t bitwise, everything behind the search is held to max(floor, 4 x spread)
(tests/spline_approx_guard.py), counts, statuses and flags are exact.  The bodies are tests/spline_approx_checks.py's, shared with the SIMT
interpreter's run (tests/test_emu_spline_approx.py): agreement there says nothing about the gfx950 code object or the device's division, sqrt
and hypot.  Reads the recorded splines; imports no scipy; reads nothing outside the repository."""
import pytest

import spline_approx_cases as sc
import spline_approx_checks as ck
from conftest import load_golden
from ring_guard import Worst, print_uncaptured

pytestmark = pytest.mark.gpu

WORST = Worst()


@pytest.fixture(scope="module", autouse=True)
def the_entries_exist(gpu_engine):
    assert hasattr(gpu_engine.lib, "mcq_spline_approx_device") and hasattr(gpu_engine.lib, "mcq_min_width_device")


@pytest.mark.parametrize("name", sc.CASES)
def test_case_against_the_reference(gpu_engine, name):
    ck.check_case(gpu_engine, name, WORST)


@pytest.mark.parametrize("name", ("n3", "len256"))
def test_m_at_and_beyond_mmax(gpu_engine, name):
    ck.check_mmax(gpu_engine, name)


def test_mixed_launch_alone_reversed_and_a_nan_track(gpu_engine):
    ck.check_batch(gpu_engine, WORST)


def test_status_and_arguments(gpu_engine):
    ck.check_status_and_arguments(gpu_engine)


def test_min_width_below_at_and_above(gpu_engine):
    ck.check_min_width(gpu_engine)


@pytest.mark.parametrize("name,key", (("rounded_rectangle", "rr_mincurv"), ("berlin_2018", "berlin_mincurv")))
def test_prep_track_to_solve(gpu_engine, name, key):
    ck.check_end_to_end(gpu_engine, name, key, load_golden(name), load_golden("harness_runs"), WORST)


def test_report(gpu_engine, request):
    """Last in the file: the worst deviation per case and quantity next to the guard it was held to, past pytest's capture into the log."""
    assert WORST.w, "no comparison has run"
    print_uncaptured(request.config, WORST.report("spline approximation on the GPU", what="deviation"))
