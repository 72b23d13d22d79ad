"""The shortest-path objective's own kernel path on the MI355X -- mcq_assemble_sp_kernel, factor_sp / sp_solve / sp_chain_solve (csrc/mcq_tri.inc:
Sherman-Morrison for the ring, per-thread blocks, cyclic reduction of the separators; workspace vectors above 2048 waypoints) and the solver kernel's
last resort -- at its structural edges (tests/sp_cases.py), against a plain longdouble reference that certifies itself (tests/sp_ref.py).  Every row is
held to 1e-9 m (tests/sp_guard.py: the floor on every case), to its box exactly, and to the reference's working set row by row.  The bodies are
tests/sp_checks.py's, shared with the SIMT interpreter's run (tests/test_emu_sp.py).  Every launch is repeated reversed and problem by problem, and the
uniform cases through every entry point: the same bits.  Reads nothing outside the repository."""
import pytest

import sp_cases as sc
import sp_checks as ck
from global_racetrajectory_optimization_amd import engine
from ring_guard import Worst, print_uncaptured

pytestmark = pytest.mark.gpu

WORST = Worst()
LAUNCHES = sc.launches()
NOTES = []


@pytest.mark.parametrize("lname", tuple(LAUNCHES))
def test_launch_against_the_reference(gpu_engine, lname):
    rows, opts = LAUNCHES[lname]
    out = ck.check_launch(gpu_engine, lname, rows, opts, WORST)
    if lname.startswith("last_resort"):
        NOTES.append("%s ran at n = %s" % (lname, ck.check_last_resort(lname, rows, out)))
    ck.check_order_and_neighbours(gpu_engine, lname, rows, opts, out)


@pytest.mark.parametrize("n", [257, 2053])
def test_entry_points(gpu_engine, n):
    ck.check_entry_points(gpu_engine, n, WORST)


def test_solve_host_above_the_slicing_threshold(gpu_engine):
    ck.check_solve_host_large_batch(gpu_engine, WORST)


@pytest.mark.parametrize("n", [257, 2053])
def test_fp32_entries(gpu_engine, n):
    ck.check_f32(gpu_engine, n, WORST)


def test_handle_history(golden):
    ck.check_handle_history(lambda: engine.Engine(0), golden["rounded_rectangle"])


def test_report(gpu_engine, request):
    """Last in the file: the worst |d alpha| per family next to the guard it was held to, past pytest's capture into the log."""
    assert WORST.w, "no comparison has run"
    print_uncaptured(request.config, WORST.report("shortest path on the GPU") + "".join("; " + n for n in NOTES))
