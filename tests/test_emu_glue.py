"""The device kernels around the QP -- mcq_relinearise_kernel, mcq_raceline_kernel, mcq_vel_profile_kernel, mcq_normals_crossing_kernel, the derive
branch of assemble_problem (mcq_prep_device) and the fp32 boundary kernels -- on the SIMT interpreter (tests/emu), UNCHANGED sources: every launch
of tests/glue_cases.py against the longdouble reference of tests/glue_ref.py / oracle/vel_ref.py under the guards of tests/glue_guard.py.
tests/test_gpu_glue.py runs the same bodies (tests/glue_checks.py) on the MI355X, where the code object and the device's pow / sqrt / atan2
are what is tested; here the kernels' logic is."""
import pytest

import glue_cases as gc
import glue_checks as ck
from global_racetrajectory_optimization_amd import engine
from ring_guard import Worst

WORST = Worst()


@pytest.fixture(scope="module")
def emu(emu_lib):
    eng = engine.Engine(0, lib_path=emu_lib)
    yield eng
    eng.close()


@pytest.mark.parametrize("family", tuple(gc.FAMILIES))
def test_raceline_kernel_against_the_reference(emu, family):
    for launch in gc.raceline_launches(family):
        ck.check_raceline_launch(emu, family, launch, WORST)


@pytest.mark.parametrize("family", tuple(gc.FAMILIES))
def test_relinearise_kernel_against_the_reference(emu, family):
    for launch in gc.relin_launches(family):
        ck.check_relin_launch(emu, family, launch, WORST)
    ck.check_relin_mask_and_arguments(emu, family)


@pytest.mark.parametrize("family", tuple(gc.FAMILIES))
def test_prep_against_the_reference(emu, family):
    ck.check_prep(emu, family, WORST)


@pytest.mark.parametrize("k", range(len(gc.vel_launches())), ids=[L["name"] for L in gc.vel_launches()])
def test_velocity_profiles_against_the_oracle(emu, k):
    ck.check_vel_launch(emu, gc.vel_launches()[k], WORST)


@pytest.mark.parametrize("family", tuple(gc.FAMILIES))
def test_raceline_into_velocity_profile(emu, family):
    ck.check_raceline_into_vel(emu, family, WORST)


def test_normals_crossing_against_the_reference(emu):
    ck.check_crossing(emu)


@pytest.mark.parametrize("batch,n", [s for s in gc.F32_SHAPES if s != (3, 777)])
def test_fp32_boundary(emu, batch, n):
    """Every comparison needs the SOLVER two or three times, and the interpreter takes seconds per solve of a long ring: the shapes up to 65
    waypoints run one variant of each comparison, (3, 333) and (1, 2049) the two that stand on the kernels' own edges (mcq_widen_kernel's tail
    through the scalings, mcq_widen_rows_kernel's slices of more than one row through increments that do not close), (3, 777) and the reversed
    track order run on the GPU only (tests/test_gpu_glue.py: every shape, every variant)."""
    ck.check_f32(emu, batch, n, WORST, variants=ck.F32_LIGHT if n <= 65 else ck.F32_ONE, reversed_too=False)


def test_report(emu):
    """The worst deviation per family and quantity next to its guard (what the interpreter achieves; the GPU file prints its own)."""
    print(WORST.report("helper kernels on the interpreter", what="deviation"))
