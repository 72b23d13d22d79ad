"""The Hessian of the minimum-time Lagrangian and H v (mcq_mintime_hess_device, mcq_mintime_hessvec_device; csrc/mcq_mintime.inc) on the SIMT
interpreter (tests/emu), UNCHANGED sources: the bodies of tests/mintime_hess_checks.py against tests/mintime_hess_ref.py under the rules of
tests/mintime_hess_guard.py.  tests/test_gpu_mintime_hess.py runs the same bodies on the MI355X.  Here the kernels' logic is tested: the lanes'
pairs, the exchange through LDS, the entries' single writers, the k = 0 slots, the order of H v."""
import pytest

import mintime_cases as mc
import mintime_hess_checks as ck
from global_racetrajectory_optimization_amd import engine


@pytest.fixture(scope="module")
def emu(emu_lib):
    eng = engine.Engine(0, lib_path=emu_lib)
    assert "mcq_mintime_hess_device" in engine.EXPORTED_SYMBOLS and hasattr(eng.lib, "mcq_mintime_hessvec_device")
    yield eng
    eng.close()


@pytest.mark.parametrize("name", sorted(mc.LAUNCHES))
def test_launch_against_the_restatement(emu, name):
    ck.check_launch(emu, name)


def test_one_row_kind_at_a_time_and_the_objective_alone(emu):
    ck.check_localising(emu)


def test_company_order_and_width_do_not_change_a_bit(emu):
    ck.check_company(emu)


def test_nan_and_inf_stay_in_their_blocks(emu):
    ck.check_nan(emu)


def test_prefilled_outputs_and_the_sizes_at_nmax(emu):
    ck.check_prefilled_and_sizes(emu)


def test_every_refusal_alone(emu):
    ck.check_refusals(emu)


def test_unit_vectors_return_the_assembled_columns(emu):
    ck.check_unit_vectors(emu)


def test_several_vectors_against_the_dense_product(emu):
    ck.check_nvec(emu)


def test_physically_meant_w_from_the_mincurv_flow(emu):
    ck.check_flow(emu)
