"""mcq_vel_profile_device_forms on the MI355X: unclosed velocity profiles (v_start, optional v_end) and local gg limits per waypoint -- the
three new instantiations of the velocity profile kernel's body -- on every launch of tests/vel_forms_cases.py against oracle/vel_ref.py, each
quantity held to max(floor, 4 x spread) (tests/vel_forms_guard.py: the rule and the floors of tests/glue_guard.py); the entry's NaN / +inf /
argument rules; the closed / ggv form through the new entry against the three old entries, bit for bit.  The bodies are
tests/vel_forms_checks.py's, shared with the SIMT interpreter's run (tests/test_emu_vel_forms.py): agreement there says nothing about the gfx950
code object or the device's pow / sqrt.  Every launch is repeated in reversed variant order and must return the same bits.  Reads nothing
outside the repository."""
import pytest

import glue_cases as gc
import vel_forms_cases as fc
import vel_forms_checks as ck
from ring_guard import Worst, print_uncaptured

pytestmark = pytest.mark.gpu

WORST = Worst()


@pytest.mark.parametrize("k", range(len(fc.all_launches())), ids=fc.launch_ids())
def test_forms_against_the_oracle(gpu_engine, k):
    ck.check_launch(gpu_engine, fc.all_launches()[k][1], WORST)


@pytest.mark.parametrize("k", range(len(gc.vel_launches())), ids=[L["name"] for L in gc.vel_launches()])
def test_existing_form_through_the_new_entry_is_bitwise_the_old_entries(gpu_engine, k):
    ck.check_existing_form_untouched(gpu_engine, gc.vel_launches()[k])


def test_unclosed_filter_leaves_the_ends(gpu_engine):
    ck.check_filter_ends(gpu_engine)


def test_standing_start_to_standstill_over_two_points_is_inf(gpu_engine):
    ck.check_standing_two_points(gpu_engine)


def test_negative_speeds_count_as_zero(gpu_engine):
    ck.check_negative_speeds(gpu_engine)


def test_end_speed_null_nan_zero_and_high(gpu_engine):
    ck.check_v_end_forms(gpu_engine)


def test_start_speed_against_the_lateral_limit(gpu_engine):
    ck.check_start_against_the_lateral_limit(gpu_engine)


def test_timed_launch_returns_the_same_bits(gpu_engine):
    ck.check_timed(gpu_engine)


def test_nan_rules(gpu_engine):
    ck.check_nan_rules(gpu_engine)


def test_argument_errors(gpu_engine):
    ck.check_argument_errors(gpu_engine)


def test_report(gpu_engine, request):
    """Last in the file: the worst deviation per kind and quantity next to the guard it was held to, past pytest's capture into the log."""
    assert WORST.w, "no comparison has run"
    print_uncaptured(request.config, WORST.report("velocity profile forms on the GPU", what="deviation"))
