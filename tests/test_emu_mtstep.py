"""The regularised primal-dual Newton step (mcq_mintime_step_device; csrc/mcq_mtstep.inc) on the SIMT interpreter (tests/emu), UNCHANGED sources:
the bodies of tests/mtstep_checks.py against tests/mtstep_ref.py under the rules of tests/mtstep_guard.py.  tests/test_gpu_mtstep.py runs the same
bodies on the MI355X, and the long chains.  Here the kernel's logic is tested: the fronts' assembly, the placeholders, the wrap and the border,
the pivots' signs, the waves' sweeps, the residual's rows."""
import pytest

import mtstep_cases as sc
import mtstep_checks as ck
from global_racetrajectory_optimization_amd import engine


@pytest.fixture(scope="module")
def emu(emu_lib):
    eng = engine.Engine(0, lib_path=emu_lib)
    assert "mcq_mintime_step_device" in engine.EXPORTED_SYMBOLS and hasattr(eng.lib, "mcq_mintime_step_bytes")
    yield eng
    eng.close()


@pytest.mark.parametrize("key", sc.EMU_KEYS)
def test_case_against_the_reference(emu, key):
    ck.check_case(emu, key, (0, 1, 2) if key in sc.REFINE_KEYS else (2,))


@pytest.mark.parametrize("key", [k for k in sc.LOCAL_KEYS if k != "zero"])
def test_one_part_of_K_at_a_time(emu, key):
    ck.check_case(emu, key)


def test_zero_blocks_in_closed_form(emu):
    ck.check_zero_blocks(emu)


def test_right_hand_sides_around_the_tile_of_four(emu):
    ck.check_nvec(emu)


def test_company_order_and_width_do_not_change_a_bit(emu):
    ck.check_company(emu)


def test_prefilled_outputs_and_the_sizes_at_nmax(emu):
    ck.check_prefilled_and_sizes(emu)


def test_a_non_finite_input_stays_in_its_problem(emu):
    ck.check_nonfinite(emu)


def test_an_exact_zero_pivot_is_singular(emu):
    ck.check_singular(emu)


def test_every_refusal_alone(emu):
    ck.check_refusals(emu)


def test_bytes_against_the_workspace_the_handle_grew(emu_lib):
    ck.check_bytes(lambda: engine.Engine(0, lib_path=emu_lib))


def test_chained_step_on_the_mincurv_flow(emu):
    ck.check_flow(emu)
