"""The iterated re-linearisation as ONE engine call on the MI355X -- iqp_step_track, mcq_iqp_step_kernel, mcq_iqp_rounds_kernel and the host's round
loop, round cap and two-buffer download -- at its edges (tests/iqp_cases.py: the damping and termination ladder, the round cap, rings that cross a
kernel switch between two passes, curvature rows active inside the loop, a batch whose tracks end in different rounds next to tracks that fail, the
trace beyond its 16 entries, handle history), against the dense reference loop of tests/iqp_ref.py under the guards of tests/iqp_guard.py.  The
bodies are tests/iqp_checks.py's, shared with the SIMT interpreter's run (tests/test_emu_iqp.py).  Reads nothing outside the repository."""
import pytest

import iqp_cases as ic
import iqp_checks as ck
from global_racetrajectory_optimization_amd import engine
from ring_guard import Worst, print_uncaptured

pytestmark = pytest.mark.gpu

WORST = Worst()
RESULTS = {}
SINGLE = tuple(n for n in ic.CASES if n.startswith(("ladder/", "golden/")))


@pytest.mark.parametrize("name", SINGLE)
def test_damping_and_termination(gpu_engine, name):
    ck.check_case(gpu_engine, name, WORST)


def test_round_cap(gpu_engine):
    ck.check_round_cap(gpu_engine, WORST)


def test_termination_boundary_is_inclusive(gpu_engine):
    ck.check_boundary_is_inclusive(gpu_engine, WORST)


@pytest.mark.parametrize("name", tuple(ic.SWITCHES))
def test_switch_crossing_between_passes(gpu_engine, name):
    ck.check_warm_and_cold(gpu_engine, name, WORST)


def test_curvature_rows_inside_the_loop(gpu_engine):
    ck.check_warm_and_cold(gpu_engine, "kappa/k296", WORST)


def test_mixed_batch(gpu_engine):
    RESULTS["mixed"] = ck.check_mixed_batch(gpu_engine, WORST)


def test_same_round_batch(gpu_engine):
    ck.check_same_round_batch(gpu_engine, WORST)


def test_routes_of_the_mixed_batch(gpu_engine):
    ck.check_routes(gpu_engine, RESULTS.get("mixed") or ck._batch_call(gpu_engine, ic.MIXED), WORST)


def test_trace_beyond_its_length(gpu_engine):
    ck.check_long_trace(gpu_engine, WORST)


def test_handle_history():
    ck.check_handle_history(lambda: engine.Engine(0))


def test_resident_entry_on_own_buffers(gpu_engine):
    ck.check_resident_entry(gpu_engine)


def test_buffer_growth():
    ck.check_buffer_growth(lambda: engine.Engine(0))


def test_report(gpu_engine, request):
    """Last in the file: the worst deviation per family and quantity next to the guard it was held to, past pytest's capture into the log."""
    assert WORST.w, "no comparison has run"
    print_uncaptured(request.config, WORST.report("IQP loop on the GPU", "deviation"))
