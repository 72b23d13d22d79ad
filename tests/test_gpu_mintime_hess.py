"""The Hessian of the minimum-time Lagrangian and H v on the MI355X: the bodies of tests/mintime_hess_checks.py (the ones
tests/test_emu_mintime_hess.py runs on the interpreter) against the longdouble restatement under the guards of tests/mintime_hess_guard.py, ending
with the report of the worst deviations."""
import pytest

import mintime_cases as mc
import mintime_hess_checks as ck

pytestmark = pytest.mark.gpu
REPORT = {}


@pytest.mark.parametrize("name", sorted(mc.LAUNCHES))
def test_launch_against_the_restatement(gpu_engine, name):
    REPORT[name] = ck.check_launch(gpu_engine, name)


def test_one_row_kind_at_a_time_and_the_objective_alone(gpu_engine):
    REPORT["row kinds"] = ck.check_localising(gpu_engine)


def test_company_order_and_width_do_not_change_a_bit(gpu_engine):
    ck.check_company(gpu_engine)


def test_nan_and_inf_stay_in_their_blocks(gpu_engine):
    ck.check_nan(gpu_engine)


def test_prefilled_outputs_and_the_sizes_at_nmax(gpu_engine):
    ck.check_prefilled_and_sizes(gpu_engine)


def test_every_refusal_alone(gpu_engine):
    ck.check_refusals(gpu_engine)


def test_unit_vectors_return_the_assembled_columns(gpu_engine):
    ck.check_unit_vectors(gpu_engine)


def test_several_vectors_against_the_dense_product(gpu_engine):
    REPORT["nvec"] = ck.check_nvec(gpu_engine)


def test_physically_meant_w_from_the_mincurv_flow(gpu_engine):
    REPORT["flow"] = ck.check_flow(gpu_engine)


def test_report():
    """The worst deviation of every quantity, in units of its guard (1.0 is the limit)."""
    for name in sorted(REPORT):
        print("mintime hess %-14s %s" % (name, "  ".join("%s %.3g" % kv for kv in sorted(REPORT[name].items()))))
    assert REPORT
