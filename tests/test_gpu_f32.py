"""The fp32 boundary at its edges on the MI355X: mcq_widen_rows_kernel, mcq_widen_kernel and mcq_narrow_kernel through mcq_f32_rows_device,
mcq_f32_widen_device and mcq_f32_narrow_device -- the launches the fp32 solve entries make -- on every case of tests/f32_cases.py against
tests/f32_ref.py: the rebuilt x, y of the increment layout within the guard derived from the kernel's roundings, everything else bit for bit, the
fp32 solve entries included (their alpha is float32 of mcq_solve_device's on the rows mcq_f32_rows_device wrote).  The bodies are
tests/f32_checks.py's, shared with the SIMT interpreter's run (tests/test_emu_f32.py): agreement there says nothing about the gfx950 code object,
the device's conversions (ties, overflow, subnormals) or the wave's shuffles.  No goldens; reads nothing outside the repository."""
import pytest

import f32_cases as fc
import f32_checks as ck
from global_racetrajectory_optimization_amd import engine
from ring_guard import Worst, print_uncaptured

pytestmark = pytest.mark.gpu

WORST = Worst()


@pytest.fixture(scope="module", autouse=True)
def the_entries_exist(gpu_engine):
    assert all(hasattr(gpu_engine.lib, nm) for nm in ("mcq_f32_rows_device", "mcq_f32_widen_device", "mcq_f32_narrow_device"))


@pytest.mark.parametrize("n", fc.REBUILD_N)
def test_rebuild_against_the_reference(gpu_engine, n):
    ck.check_rebuild(gpu_engine, n, WORST)


@pytest.mark.parametrize("batch,n", fc.SOLVES)
def test_solves_are_exact_on_what_was_rebuilt(gpu_engine, batch, n):
    ck.check_solve(gpu_engine, batch, n)


def test_narrow_track_in_the_middle(gpu_engine):
    assert ck.check_narrow_track(gpu_engine) == engine.STATUS_INFEASIBLE


def test_nan_increment_in_the_middle(gpu_engine):
    assert ck.check_nan_track(gpu_engine) == engine.STATUS_BAD_INPUT


@pytest.mark.parametrize("count", fc.COUNTS)
def test_narrow(gpu_engine, count):
    ck.check_narrow(gpu_engine, count)


@pytest.mark.parametrize("count", fc.COUNTS)
def test_widen(gpu_engine, count):
    ck.check_widen(gpu_engine, count)


def test_staging_reuse():
    ck.check_staging_reuse(lambda: engine.Engine(0))


def test_arguments(gpu_engine):
    ck.check_arguments(gpu_engine)


def test_report(gpu_engine, request):
    """Last in the file: the worst rebuild deviation per launch next to the guard it was held to, past pytest's capture into the log."""
    assert WORST.w, "no comparison has run"
    print_uncaptured(request.config, ck.report(WORST, "fp32 rows rebuilt on the GPU"))
