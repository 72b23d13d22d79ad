"""The regularised primal-dual Newton step on the MI355X: the bodies of tests/mtstep_checks.py (the ones tests/test_emu_mtstep.py runs on the
interpreter) against the longdouble reference under the rules of tests/mtstep_guard.py, the long chains N = 257 and N = 1025 as well, ending with
the report of the worst deviations."""
import pytest

import mtstep_cases as sc
import mtstep_checks as ck
from global_racetrajectory_optimization_amd import engine

pytestmark = pytest.mark.gpu
REPORT = {}


@pytest.mark.parametrize("key", sc.EMU_KEYS + sc.GPU_KEYS)
def test_case_against_the_reference(gpu_engine, key):
    REPORT[key] = ck.check_case(gpu_engine, key, (0, 1, 2) if key in sc.REFINE_KEYS else (2,))


@pytest.mark.parametrize("key", [k for k in sc.LOCAL_KEYS if k != "zero"])
def test_one_part_of_K_at_a_time(gpu_engine, key):
    REPORT[key] = ck.check_case(gpu_engine, key)


def test_zero_blocks_in_closed_form(gpu_engine):
    ck.check_zero_blocks(gpu_engine)


def test_right_hand_sides_around_the_tile_of_four(gpu_engine):
    ck.check_nvec(gpu_engine)


def test_company_order_and_width_do_not_change_a_bit(gpu_engine):
    ck.check_company(gpu_engine)


def test_prefilled_outputs_and_the_sizes_at_nmax(gpu_engine):
    ck.check_prefilled_and_sizes(gpu_engine)


def test_a_non_finite_input_stays_in_its_problem(gpu_engine):
    ck.check_nonfinite(gpu_engine)


def test_an_exact_zero_pivot_is_singular(gpu_engine):
    ck.check_singular(gpu_engine)


def test_every_refusal_alone(gpu_engine):
    ck.check_refusals(gpu_engine)


def test_bytes_against_the_workspace_the_handle_grew():
    ck.check_bytes(lambda: engine.Engine(0))


def test_chained_step_on_the_mincurv_flow(gpu_engine):
    REPORT["flow"] = ck.check_flow(gpu_engine)


def test_report():
    """The worst deviation of every quantity, in units of its guard (1.0 is the limit); the flow's equality residual before and after the step."""
    for name in sorted(REPORT):
        print("mintime step %-16s %s" % (name, "  ".join("%s %.3g" % kv for kv in sorted(REPORT[name].items()))))
    assert REPORT
