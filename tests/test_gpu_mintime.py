"""The minimum-time NLP's entries on the MI355X: the bodies of tests/mintime_checks.py (the ones tests/test_emu_mintime.py runs on the interpreter)
against the longdouble restatement under the guards of tests/mintime_guard.py, ending with the report of the worst deviations."""
import pytest

import mintime_cases as mc
import mintime_checks as ck
from conftest import load_golden

pytestmark = pytest.mark.gpu
REPORT = {}


def test_layout_and_collocation_constants(gpu_engine):
    ck.check_layout(gpu_engine)


@pytest.mark.parametrize("name", sorted(mc.LAUNCHES))
def test_bounds_exactly(gpu_engine, name):
    ck.check_bounds(gpu_engine, name)


@pytest.mark.parametrize("name", sorted(mc.LAUNCHES))
def test_launch_against_the_restatement(gpu_engine, name):
    REPORT[name] = ck.check_launch(gpu_engine, name)


def test_jacobian_coo_against_the_dense_jacobian(gpu_engine):
    REPORT["dense"] = ck.check_dense(gpu_engine)


def test_certificate_returns_the_residual_set_by_hand(gpu_engine):
    REPORT["certificate"] = ck.check_certificate(gpu_engine)


def test_company_order_and_width_do_not_change_a_bit(gpu_engine):
    ck.check_company(gpu_engine)


def test_nan_and_inf_stay_in_their_problem(gpu_engine):
    ck.check_nan(gpu_engine)


def test_prefilled_outputs_are_overwritten(gpu_engine):
    ck.check_prefilled(gpu_engine)


def test_physically_meant_w_from_the_mincurv_flow(gpu_engine):
    REPORT["flow"] = ck.check_flow(gpu_engine)


def test_every_refusal_alone(gpu_engine):
    ck.check_refusals(gpu_engine)


def test_export_files_byte_for_byte(gpu_engine, tmp_path):
    ck.check_export(gpu_engine, str(tmp_path))


def test_mincurv_flow_and_resident_friction_fit_feed_the_evaluation_on_berlin(gpu_engine):
    REPORT["berlin"] = ck.check_end_to_end(gpu_engine, load_golden("berlin_2018"))


def test_report():
    """The worst deviation of every quantity, in units of its guard (1.0 is the limit); Berlin's flow-built guess: lap times,
    infeasibility and undecided denominators, reported only."""
    for name in sorted(REPORT):
        print("mintime %-14s %s" % (name, "  ".join("%s %.3g" % kv for kv in sorted(REPORT[name].items()))))
    assert REPORT
