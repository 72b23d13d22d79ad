"""mcq_vel_profile_device_forms -- unclosed velocity profiles and local gg limits, the three new instantiations of the velocity profile kernel's
body -- on the SIMT interpreter (tests/emu), UNCHANGED sources: every launch of tests/vel_forms_cases.py against oracle/vel_ref.py under the
guards of tests/vel_forms_guard.py, the entry's NaN / +inf / argument rules, and the closed / ggv form through the new entry against the old
ones bit for bit.  tests/test_gpu_vel_forms.py runs the same bodies (tests/vel_forms_checks.py) on the MI355X, where the code object and the
device's pow / sqrt are what is tested; here the kernels' logic is."""
import pytest

import glue_cases as gc
import vel_forms_cases as fc
import vel_forms_checks as ck
from global_racetrajectory_optimization_amd import engine
from ring_guard import Worst

WORST = Worst()


@pytest.fixture(scope="module")
def emu(emu_lib):
    eng = engine.Engine(0, lib_path=emu_lib)
    yield eng
    eng.close()


@pytest.mark.parametrize("k", range(len(fc.all_launches())), ids=fc.launch_ids())
def test_forms_against_the_oracle(emu, k):
    ck.check_launch(emu, fc.all_launches()[k][1], WORST)


@pytest.mark.parametrize("k", range(len(gc.vel_launches())), ids=[L["name"] for L in gc.vel_launches()])
def test_existing_form_through_the_new_entry_is_bitwise_the_old_entries(emu, k):
    ck.check_existing_form_untouched(emu, gc.vel_launches()[k])


def test_unclosed_filter_leaves_the_ends(emu):
    ck.check_filter_ends(emu)


def test_standing_start_to_standstill_over_two_points_is_inf(emu):
    ck.check_standing_two_points(emu)


def test_negative_speeds_count_as_zero(emu):
    ck.check_negative_speeds(emu)


def test_end_speed_null_nan_zero_and_high(emu):
    ck.check_v_end_forms(emu)


def test_start_speed_against_the_lateral_limit(emu):
    ck.check_start_against_the_lateral_limit(emu)


def test_timed_launch_returns_the_same_bits(emu):
    ck.check_timed(emu)


def test_nan_rules(emu):
    ck.check_nan_rules(emu)


def test_argument_errors(emu):
    ck.check_argument_errors(emu)


def test_report(emu):
    """The worst deviation per kind and quantity next to its guard (what the interpreter achieves; the GPU file prints its own)."""
    print(WORST.report("velocity profile forms on the interpreter", what="deviation"))
