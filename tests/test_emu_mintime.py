"""The minimum-time NLP's kernels (csrc/mcq_mintime.inc behind the mcq_mintime_* entries) and their Python surface on the SIMT interpreter (tests/emu),
UNCHANGED sources: the launches of tests/mintime_cases.py against tests/mintime_ref.py under the rules of tests/mintime_guard.py.
tests/test_gpu_mintime.py runs the same bodies (tests/mintime_checks.py) on the MI355X, where the code object is what is tested -- the interpreter
has the host's sin, cos, atan and exp and no fused multiply-add; here the kernels' logic is: the lanes' shares, the quad's exchange, the blocks'
owners, the ordered sums, the tails."""
import pytest

import mintime_cases as mc
import mintime_checks as ck
from conftest import load_golden
from global_racetrajectory_optimization_amd import engine


@pytest.fixture(scope="module")
def emu(emu_lib):
    eng = engine.Engine(0, lib_path=emu_lib)
    assert "mcq_mintime_eval_device" in engine.EXPORTED_SYMBOLS and hasattr(eng.lib, "mcq_mintime_kkt_device")
    yield eng
    eng.close()


def test_layout_and_collocation_constants(emu):
    ck.check_layout(emu)


@pytest.mark.parametrize("name", sorted(mc.LAUNCHES))
def test_bounds_exactly(emu, name):
    ck.check_bounds(emu, name)


@pytest.mark.parametrize("name", sorted(mc.LAUNCHES))
def test_launch_against_the_restatement(emu, name):
    ck.check_launch(emu, name)


def test_jacobian_coo_against_the_dense_jacobian(emu):
    ck.check_dense(emu)


def test_certificate_returns_the_residual_set_by_hand(emu):
    ck.check_certificate(emu)


def test_company_order_and_width_do_not_change_a_bit(emu):
    ck.check_company(emu)


def test_nan_and_inf_stay_in_their_problem(emu):
    ck.check_nan(emu)


def test_prefilled_outputs_are_overwritten(emu):
    ck.check_prefilled(emu)


def test_physically_meant_w_from_the_mincurv_flow(emu):
    ck.check_flow(emu)


def test_every_refusal_alone(emu):
    ck.check_refusals(emu)


def test_export_files_byte_for_byte(emu, tmp_path):
    ck.check_export(emu, str(tmp_path))


def test_mincurv_flow_and_resident_friction_fit_feed_the_evaluation_on_berlin(emu):
    ck.check_end_to_end(emu, load_golden("berlin_2018"))
