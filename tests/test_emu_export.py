"""The export kernels (mcq_export_s_kernel, mcq_export_rows_kernel behind mcq_export_device) on the SIMT interpreter (tests/emu), UNCHANGED sources:
every case of tests/export_cases.py against the longdouble reference of tests/export_ref.py under the guards of tests/export_guard.py.
tests/test_gpu_export.py runs the same bodies (tests/export_checks.py) on the MI355X, where the code object and the device's hypot are what is
tested; here the kernels' logic is."""
import pytest

import export_cases as xc
import export_checks as ck
from conftest import load_golden
from global_racetrajectory_optimization_amd import engine
from ring_guard import Worst

WORST = Worst()


@pytest.fixture(scope="module")
def emu(emu_lib):
    eng = engine.Engine(0, lib_path=emu_lib)
    assert "mcq_export_device" in engine.EXPORTED_SYMBOLS and hasattr(eng.lib, "mcq_export_device")
    yield eng
    eng.close()


@pytest.mark.parametrize("name", ("sizes", "rowblock", "tiles", "chunks", "large", "variants"))
@pytest.mark.parametrize("family", xc.FAMILIES)
def test_tables_against_the_reference(emu, family, name):
    L = next(q for q in xc.launches(family) if q["name"] == "%s/%s" % (family, name))
    ck.check_launch(emu, L, WORST, alone=name in ("sizes", "variants"))


def test_hand_made_s_columns(emu):
    ck.check_handmade(emu)


def test_ties(emu):
    ck.check_ties(emu, WORST)


def test_refusals_leave_the_neighbours_alone(emu):
    ck.check_refusals(emu)


def test_arguments(emu):
    ck.check_arguments(emu)


def test_export_batch(emu):
    ck.check_export_batch(emu, WORST)


def test_solve_raceline_profile_trajectory_export_on_berlin(emu):
    ck.check_end_to_end(emu, load_golden("berlin_2018"), WORST)


def test_report(emu):
    """The worst deviation per family and quantity next to its guard (what the interpreter achieves; the GPU file prints its own)."""
    print(WORST.report("export tables on the interpreter", what="deviation"))
