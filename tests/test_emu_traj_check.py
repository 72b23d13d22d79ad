"""The trajectory / check_traj kernels (mcq_trajectory_kernel, mcq_bound_points_kernel, mcq_bound_dists_kernel, mcq_bound_min_kernel behind
mcq_trajectory_device / mcq_bound_dists_device) on the SIMT interpreter (tests/emu), UNCHANGED sources: every case of tests/traj_check_cases.py
against the longdouble reference of tests/traj_check_ref.py under the guards of tests/traj_check_guard.py.  tests/test_gpu_traj_check.py runs the
same bodies (tests/traj_check_checks.py) on the MI355X, where the code object and the device's sin / cos / sqrt / division are what is tested;
here the kernels' logic is."""
import pytest

import traj_check_cases as tc
import traj_check_checks as ck
import traj_check_guard as tg
from conftest import load_golden
from global_racetrajectory_optimization_amd import engine
from ring_guard import Worst

WORST = Worst()


@pytest.fixture(scope="module")
def emu(emu_lib):
    eng = engine.Engine(0, lib_path=emu_lib)
    for sym in ("mcq_trajectory_device", "mcq_bound_dists_device"):
        assert sym in engine.EXPORTED_SYMBOLS and hasattr(eng.lib, sym)
    yield eng
    eng.close()


@pytest.mark.parametrize("family", tuple(tc.FAMILIES))
def test_bound_dists_against_the_reference(emu, family):
    for launch in tc.bound_launches(family):
        ck.check_bound_launch(emu, family, launch, WORST)


def test_bound_dists_status_and_arguments(emu):
    ck.check_bound_status_and_arguments(emu, "peanut")


@pytest.mark.parametrize("family", tuple(tc.FAMILIES))
def test_trajectories_against_the_reference(emu, family):
    for name, L in tg.traj_named_launches(family)[:2]:
        ck.check_traj_launch(emu, family, name, L, WORST)


@pytest.mark.parametrize("family", tuple(tc.FAMILIES))
def test_every_flag_alone_and_none(emu, family):
    for name, L, bit in tc.flag_launches(family):
        ck.check_traj_launch(emu, family, "flag_" + name, L, WORST, expected_flags=bit)
    ck.check_null_tables(emu, family)


@pytest.mark.parametrize("closed", (True, False))
def test_last_time_is_the_profile_lap_time_bit_for_bit(emu, closed):
    ck.check_lap_time_bitwise(emu, "trefoil", closed)


def test_trajectory_nan_rule_and_arguments(emu):
    ck.check_traj_nan_and_status(emu, "peanut")
    ck.check_traj_arguments(emu)


def test_solve_raceline_profile_trajectory_check_on_berlin(emu):
    ck.check_end_to_end(emu, load_golden("berlin_2018"), WORST)


def test_report(emu):
    """The worst deviation per family and quantity next to its guard (what the interpreter achieves; the GPU file prints its own)."""
    print(WORST.report("trajectory / check_traj on the interpreter", what="deviation"))
