"""The friction kernels (mcq_fmap_query_kernel, mcq_friction_grid_kernel behind mcq_fmap_query_device / mcq_friction_grid_device) and their Python
surface on the SIMT interpreter (tests/emu), UNCHANGED sources: the cases of tests/fric_cases.py against tests/fric_ref.py under the rules of
tests/fric_guard.py.  tests/test_gpu_fric.py runs the same bodies (tests/fric_checks.py) on the MI355X, where the code object is what is tested --
the interpreter build has no fused multiply-add and cannot see a contracted numpy.linspace; here the kernels' logic is."""
import pytest

import fric_cases as fc
import fric_checks as ck
import fric_guard as fg
from conftest import load_golden
from global_racetrajectory_optimization_amd import engine


@pytest.fixture(scope="module")
def emu(emu_lib):
    eng = engine.Engine(0, lib_path=emu_lib)
    assert "mcq_fmap_query_device" in engine.EXPORTED_SYMBOLS and hasattr(eng.lib, "mcq_friction_grid_device")
    yield eng
    eng.close()


@pytest.mark.parametrize("name", sorted(fc.maps()))
def test_map_against_the_brute_force(emu, name):
    ck.check_map(emu, name)


def test_exact_ties_take_the_lowest_index(emu):
    ck.check_exact_ties(emu)


def test_queries_that_are_not_finite(emu):
    ck.check_nonfinite(emu)


def test_map_arguments(emu):
    ck.check_map_arguments(emu)


@pytest.mark.parametrize("track", fg.TRACKS)
def test_recorded_queries(emu, track):
    ck.check_recorded_queries(emu, track)


@pytest.mark.parametrize("name", sorted(fc.grid_cases()))
def test_grid_against_the_reference(emu, name):
    ck.check_grid_case(emu, name)


def test_grid_overwrites_prefilled_outputs(emu):
    ck.check_grid_prefilled(emu)


def test_width_list_against_scalar_calls(emu):
    ck.check_width_list(emu)


def test_grid_arguments(emu):
    ck.check_grid_arguments(emu)


@pytest.mark.parametrize("track", fg.TRACKS)
def test_whole_track_against_the_recorded_reference(emu, track):
    ck.check_recorded_grid(emu, track)


def test_the_reference_names(emu, tmp_path):
    ck.check_dropin(emu, str(tmp_path))


def test_prep_solve_raceline_mu_profile_on_berlin(emu):
    ck.check_end_to_end(emu, load_golden("berlin_2018"))
