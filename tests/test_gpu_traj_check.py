"""The trajectory / check_traj kernels on the MI355X (mcq_trajectory_device, mcq_bound_dists_device through Engine.trajectory_batch /
Engine.bound_dists_batch) at their structural edges (tests/traj_check_cases.py), against a plain longdouble reference (tests/traj_check_ref.py),
each quantity held to max(floor, 4 x spread) (tests/traj_check_guard.py).  The bodies are tests/traj_check_checks.py's, shared with the SIMT
interpreter's run (tests/test_emu_traj_check.py): agreement there says nothing about the gfx950 code object or the device's sin / cos / sqrt /
division.  Sample counts, statuses and flags are exact; every launch is repeated in reversed order and must return the same bits; the last time of
a trajectory is the velocity kernel's lap time bit for bit.  Reads nothing outside the repository."""
import pytest

import traj_check_cases as tc
import traj_check_checks as ck
import traj_check_guard as tg
from conftest import load_golden
from ring_guard import Worst, print_uncaptured

pytestmark = pytest.mark.gpu

WORST = Worst()


@pytest.fixture(scope="module", autouse=True)
def the_entries_exist(gpu_engine):
    assert hasattr(gpu_engine.lib, "mcq_trajectory_device") and hasattr(gpu_engine.lib, "mcq_bound_dists_device")


@pytest.mark.parametrize("family", tuple(tc.FAMILIES))
def test_bound_dists_against_the_reference(gpu_engine, family):
    for launch in tc.bound_launches(family):
        ck.check_bound_launch(gpu_engine, family, launch, WORST)


def test_bound_dists_status_and_arguments(gpu_engine):
    ck.check_bound_status_and_arguments(gpu_engine, "peanut")


@pytest.mark.parametrize("family", tuple(tc.FAMILIES))
def test_trajectories_against_the_reference(gpu_engine, family):
    for name, L in tg.traj_named_launches(family)[:2]:
        ck.check_traj_launch(gpu_engine, family, name, L, WORST)


@pytest.mark.parametrize("family", tuple(tc.FAMILIES))
def test_every_flag_alone_and_none(gpu_engine, family):
    for name, L, bit in tc.flag_launches(family):
        ck.check_traj_launch(gpu_engine, family, "flag_" + name, L, WORST, expected_flags=bit)
    ck.check_null_tables(gpu_engine, family)


@pytest.mark.parametrize("closed", (True, False))
def test_last_time_is_the_profile_lap_time_bit_for_bit(gpu_engine, closed):
    ck.check_lap_time_bitwise(gpu_engine, "trefoil", closed)


def test_trajectory_nan_rule_and_arguments(gpu_engine):
    ck.check_traj_nan_and_status(gpu_engine, "peanut")
    ck.check_traj_arguments(gpu_engine)


def test_solve_raceline_profile_trajectory_check_on_berlin(gpu_engine):
    ck.check_end_to_end(gpu_engine, load_golden("berlin_2018"), WORST)


def test_report(gpu_engine, request):
    """Last in the file: the worst deviation per family and quantity next to the guard it was held to, past pytest's capture into the log."""
    assert WORST.w, "no comparison has run"
    print_uncaptured(request.config, WORST.report("trajectory / check_traj on the GPU", what="deviation"))
