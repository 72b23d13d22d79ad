"""The device kernels around the QP on the MI355X -- mcq_relinearise_kernel, mcq_raceline_kernel, mcq_vel_profile_kernel (its three entries),
mcq_normals_crossing_kernel, the derive branch of assemble_problem (mcq_prep_device), mcq_widen_kernel / mcq_narrow_kernel / mcq_widen_rows_kernel --
at their structural edges (tests/glue_cases.py), against a plain longdouble reference (tests/glue_ref.py; oracle/vel_ref.py for the velocity
profiles), each quantity held to max(floor, 4 x spread) (tests/glue_guard.py).  The bodies are tests/glue_checks.py's, shared with the SIMT
interpreter's run (tests/test_emu_glue.py): agreement there says nothing about the gfx950 code object or the device's pow / sqrt / atan2 / hypot.
Point counts, statuses and crossing verdicts are exact; every launch is repeated in reversed order and must return the same bits.  Reads nothing
outside the repository."""
import pytest

import glue_cases as gc
import glue_checks as ck
from ring_guard import Worst, print_uncaptured

pytestmark = pytest.mark.gpu

WORST = Worst()


@pytest.mark.parametrize("family", tuple(gc.FAMILIES))
def test_raceline_kernel_against_the_reference(gpu_engine, family):
    for launch in gc.raceline_launches(family):
        ck.check_raceline_launch(gpu_engine, family, launch, WORST)


@pytest.mark.parametrize("family", tuple(gc.FAMILIES))
def test_relinearise_kernel_against_the_reference(gpu_engine, family):
    for launch in gc.relin_launches(family):
        ck.check_relin_launch(gpu_engine, family, launch, WORST)
    ck.check_relin_mask_and_arguments(gpu_engine, family)


@pytest.mark.parametrize("family", tuple(gc.FAMILIES))
def test_prep_against_the_reference(gpu_engine, family):
    ck.check_prep(gpu_engine, family, WORST)


@pytest.mark.parametrize("k", range(len(gc.vel_launches())), ids=[L["name"] for L in gc.vel_launches()])
def test_velocity_profiles_against_the_oracle(gpu_engine, k):
    ck.check_vel_launch(gpu_engine, gc.vel_launches()[k], WORST)


@pytest.mark.parametrize("family", tuple(gc.FAMILIES))
def test_raceline_into_velocity_profile(gpu_engine, family):
    ck.check_raceline_into_vel(gpu_engine, family, WORST)


def test_normals_crossing_against_the_reference(gpu_engine):
    ck.check_crossing(gpu_engine)


@pytest.mark.parametrize("batch,n", gc.F32_SHAPES)
def test_fp32_boundary(gpu_engine, batch, n):
    ck.check_f32(gpu_engine, batch, n, WORST)


def test_report(gpu_engine, request):
    """Last in the file: the worst deviation per family and quantity next to the guard it was held to, past pytest's capture into the log."""
    assert WORST.w, "no comparison has run"
    print_uncaptured(request.config, WORST.report("helper kernels on the GPU", what="deviation"))
