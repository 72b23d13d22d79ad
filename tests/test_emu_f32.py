"""The fp32 boundary at its edges on the SIMT interpreter (tests/emu), UNCHANGED sources: mcq_widen_rows_kernel, mcq_widen_kernel and mcq_narrow_kernel
through mcq_f32_rows_device, mcq_f32_widen_device and mcq_f32_narrow_device -- the launches the fp32 solve entries make -- on every case of
tests/f32_cases.py against tests/f32_ref.py.  tests/test_gpu_f32.py runs the same bodies (tests/f32_checks.py) on the MI355X, where the code object,
the device's conversions and the wave's shuffles are what is tested; here the kernels' logic and the host's launches are."""
import pytest

import f32_cases as fc
import f32_checks as ck
from global_racetrajectory_optimization_amd import engine
from ring_guard import Worst

WORST = Worst()


@pytest.fixture(scope="module")
def emu(emu_lib):
    eng = engine.Engine(0, lib_path=emu_lib)
    assert all(nm in engine.EXPORTED_SYMBOLS and hasattr(eng.lib, nm) for nm in ("mcq_f32_rows_device", "mcq_f32_widen_device", "mcq_f32_narrow_device"))
    yield eng
    eng.close()


@pytest.mark.parametrize("n", fc.REBUILD_N)
def test_rebuild_against_the_reference(emu, n):
    ck.check_rebuild(emu, n, WORST)


@pytest.mark.parametrize("batch,n", fc.SOLVES)
def test_solves_are_exact_on_what_was_rebuilt(emu, batch, n):
    ck.check_solve(emu, batch, n)


def test_narrow_track_in_the_middle(emu):
    assert ck.check_narrow_track(emu) == engine.STATUS_INFEASIBLE


def test_nan_increment_in_the_middle(emu):
    assert ck.check_nan_track(emu) == engine.STATUS_BAD_INPUT


@pytest.mark.parametrize("count", fc.COUNTS)
def test_narrow(emu, count):
    ck.check_narrow(emu, count)


@pytest.mark.parametrize("count", fc.COUNTS)
def test_widen(emu, count):
    ck.check_widen(emu, count)


def test_staging_reuse(emu_lib):
    ck.check_staging_reuse(lambda: engine.Engine(0, lib_path=emu_lib))


def test_arguments(emu):
    ck.check_arguments(emu)


def test_report(emu):
    """The worst rebuild deviation per launch next to its guard (what the interpreter achieves; the GPU file prints its own).  Under pytest-xdist
    the comparisons may have run in other processes: what this one saw."""
    if WORST.w:
        print(ck.report(WORST, "fp32 rows rebuilt on the interpreter"))
