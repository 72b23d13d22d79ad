"""The shortest-path objective's own kernel path -- mcq_assemble_sp_kernel, factor_sp / sp_solve / sp_chain_solve (csrc/mcq_tri.inc) and the solver
kernel's last resort -- on the SIMT interpreter (tests/emu), UNCHANGED sources: the launches of tests/sp_cases.py up to EMU_NMAX waypoints against the
longdouble reference of tests/sp_ref.py, every row held to the 1e-9 m floor (tests/sp_guard.py) and to the reference's working set bit for bit.
tests/test_gpu_sp.py runs the same bodies (tests/sp_checks.py) on every case on the MI355X."""
import pytest

import sp_cases as sc
import sp_checks as ck
from global_racetrajectory_optimization_amd import engine
from ring_guard import Worst

WORST = Worst()
EMU_NMAX = 2305
LAUNCHES = sc.launches(EMU_NMAX)
RESULTS = {}


@pytest.fixture(scope="module")
def emu(emu_lib):
    eng = engine.Engine(0, lib_path=emu_lib)
    yield eng
    eng.close()


@pytest.mark.parametrize("lname", tuple(LAUNCHES))
def test_launch_against_the_reference(emu, lname):
    rows, opts = LAUNCHES[lname]
    RESULTS[lname] = ck.check_launch(emu, lname, rows, opts, WORST)


@pytest.mark.parametrize("lname", ["last_resort", "last_resort_cold"])
def test_last_resort_runs(emu, lname):
    rows, opts = LAUNCHES[lname]
    out = RESULTS.get(lname) or emu.solve_batch(sc.launch_problems(rows), objective=ck.SP, **opts)
    print("%s ran at n =" % lname, ck.check_last_resort(lname, rows, out))


def test_order_and_neighbours(emu):
    """The interpreter runs one workgroup after the other, so a launch's rows cannot disturb each other the way they can on the GPU: one launch
    of few rows here (the GPU file repeats every launch)."""
    rows = ["ladder/5", "bad/nan_normal", "corner/257/second", "ladder/2049", "bad/n2", "all_free/64", "corner/514/separators"]
    ck.check_order_and_neighbours(emu, "mixed", rows, {})


@pytest.mark.parametrize("n", [257, 2053])
def test_entry_points(emu, n):
    ck.check_entry_points(emu, n, WORST)


def test_solve_host_above_the_slicing_threshold(emu):
    ck.check_solve_host_large_batch(emu, WORST)


@pytest.mark.parametrize("n", [257, 2053])
def test_fp32_entries(emu, n):
    ck.check_f32(emu, n, WORST)


def test_handle_history(emu_lib, golden):
    ck.check_handle_history(lambda: engine.Engine(0, lib_path=emu_lib), golden["rounded_rectangle"])


def test_report(emu):
    """The worst |d alpha| per family next to its guard (what the interpreter achieves; the GPU file prints its own)."""
    print(WORST.report("shortest path on the interpreter"))
