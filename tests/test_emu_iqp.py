"""The iterated re-linearisation as ONE engine call -- iqp_step_track, mcq_iqp_step_kernel, mcq_iqp_rounds_kernel and the host's round loop, round cap
and two-buffer download (csrc/mcq_kernels.hip, csrc/mcq_api.hip) -- on the SIMT interpreter (tests/emu), UNCHANGED sources: every case of
tests/iqp_cases.py against the dense reference loop of tests/iqp_ref.py under the guards of tests/iqp_guard.py (the 1e-8 floors on every case).
tests/test_gpu_iqp.py runs the same bodies (tests/iqp_checks.py) on the MI355X."""
import pytest

import iqp_cases as ic
import iqp_checks as ck
from global_racetrajectory_optimization_amd import engine
from ring_guard import Worst

WORST = Worst()
RESULTS = {}
SINGLE = tuple(n for n in ic.CASES if n.startswith(("ladder/", "golden/")))


@pytest.fixture(scope="module")
def emu(emu_lib):
    eng = engine.Engine(0, lib_path=emu_lib)
    yield eng
    eng.close()


@pytest.mark.parametrize("name", SINGLE)
def test_damping_and_termination(emu, name):
    ck.check_case(emu, name, WORST)


def test_round_cap(emu):
    ck.check_round_cap(emu, WORST)


def test_termination_boundary_is_inclusive(emu):
    ck.check_boundary_is_inclusive(emu, WORST)


@pytest.mark.parametrize("name", tuple(ic.SWITCHES))
def test_switch_crossing_between_passes(emu, name):
    ck.check_warm_and_cold(emu, name, WORST)


def test_curvature_rows_inside_the_loop(emu):
    ck.check_warm_and_cold(emu, "kappa/k296", WORST)


def test_mixed_batch(emu):
    RESULTS["mixed"] = ck.check_mixed_batch(emu, WORST)


def test_same_round_batch(emu):
    ck.check_same_round_batch(emu, WORST)


def test_routes_of_the_mixed_batch(emu):
    ck.check_routes(emu, RESULTS.get("mixed") or ck._batch_call(emu, ic.MIXED), WORST)


def test_trace_beyond_its_length(emu):
    ck.check_long_trace(emu, WORST)


def test_handle_history(emu_lib):
    ck.check_handle_history(lambda: engine.Engine(0, lib_path=emu_lib))


def test_resident_entry_on_own_buffers(emu):
    ck.check_resident_entry(emu)


def test_buffer_growth(emu_lib):
    ck.check_buffer_growth(lambda: engine.Engine(0, lib_path=emu_lib))


def test_report(emu):
    """The worst deviation per family and quantity next to its guard (what the interpreter achieves; the GPU file prints its own)."""
    print(WORST.report("IQP loop on the interpreter", "deviation"))
