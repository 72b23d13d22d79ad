"""The chain form of the raceline kernel (mcq_raceline_ends_kernel behind mcq_raceline_device_ends / Engine.raceline_batch(ends=...)) on the SIMT
interpreter (tests/emu), UNCHANGED sources: every launch of tests/race_open_cases.py against the longdouble reference of tests/race_open_ref.py
under the guards of tests/race_open_guard.py.  tests/test_gpu_race_open.py runs the same bodies (tests/race_open_checks.py) on the MI355X, where
the code object and the device's hypot / atan2 / sqrt are what is tested; here the kernel's logic is."""
import pytest

import race_open_cases as oc
import race_open_checks as ck
from conftest import load_golden
from global_racetrajectory_optimization_amd import engine
from ring_guard import Worst

WORST = Worst()


@pytest.fixture(scope="module")
def emu(emu_lib):
    eng = engine.Engine(0, lib_path=emu_lib)
    assert "mcq_raceline_device_ends" in engine.EXPORTED_SYMBOLS and hasattr(eng.lib, "mcq_raceline_device_ends")
    yield eng
    eng.close()


@pytest.mark.parametrize("family", tuple(oc.FAMILIES))
def test_open_raceline_against_the_reference(emu, family):
    for launch in oc.launches(family):
        ck.check_launch(emu, family, launch, WORST)


@pytest.mark.parametrize("family", tuple(oc.FAMILIES))
def test_rings_and_chains_in_one_launch(emu, family):
    ck.check_mixed(emu, family)


def test_arguments_and_status(emu):
    ck.check_arguments_and_status(emu, "peanut")


def test_chain_solve_into_open_raceline_into_unclosed_profile(emu):
    ck.check_end_to_end(emu, load_golden("open_handling_a"), WORST)


def test_report(emu):
    """The worst deviation per family and quantity next to its guard (what the interpreter achieves; the GPU file prints its own)."""
    print(WORST.report("open racelines on the interpreter", what="deviation"))
