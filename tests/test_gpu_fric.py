"""The friction entries on the MI355X (mcq_fmap_query_device, mcq_friction_grid_device through the Engine and through friction.py) at their
structural edges (tests/fric_cases.py) against the plain reference (tests/fric_ref.py) under the rules of tests/fric_guard.py.  The bodies are
tests/fric_checks.py's, shared with the SIMT interpreter's run (tests/test_emu_fric.py): agreement there says nothing about the gfx950 code object.
Decided here only: numpy.linspace's bits at dn 0.1 and 0.3 (a fused multiply-add would change them; the interpreter build has none).  Reads
nothing outside the repository."""
import pytest

import fric_cases as fc
import fric_checks as ck
import fric_guard as fg
from conftest import load_golden
from ring_guard import print_uncaptured

pytestmark = pytest.mark.gpu

WORST = {}


@pytest.fixture(scope="module", autouse=True)
def the_entries_exist(gpu_engine):
    assert hasattr(gpu_engine.lib, "mcq_fmap_query_device") and hasattr(gpu_engine.lib, "mcq_friction_grid_device")


@pytest.mark.parametrize("name", sorted(fc.maps()))
def test_map_against_the_brute_force(gpu_engine, name):
    ck.check_map(gpu_engine, name)


def test_exact_ties_take_the_lowest_index(gpu_engine):
    ck.check_exact_ties(gpu_engine)


def test_queries_that_are_not_finite(gpu_engine):
    ck.check_nonfinite(gpu_engine)


def test_map_arguments(gpu_engine):
    ck.check_map_arguments(gpu_engine)


@pytest.mark.parametrize("track", fg.TRACKS)
def test_recorded_queries(gpu_engine, track):
    ck.check_recorded_queries(gpu_engine, track)


@pytest.mark.parametrize("name", sorted(fc.grid_cases()))
def test_grid_against_the_reference(gpu_engine, name):
    ck.check_grid_case(gpu_engine, name)


def test_grid_overwrites_prefilled_outputs(gpu_engine):
    ck.check_grid_prefilled(gpu_engine)


def test_width_list_against_scalar_calls(gpu_engine):
    ck.check_width_list(gpu_engine)


def test_grid_arguments(gpu_engine):
    ck.check_grid_arguments(gpu_engine)


@pytest.mark.parametrize("track", fg.TRACKS)
def test_whole_track_against_the_recorded_reference(gpu_engine, track):
    WORST[track] = ck.check_recorded_grid(gpu_engine, track)


def test_the_reference_names(gpu_engine, tmp_path):
    ck.check_dropin(gpu_engine, str(tmp_path))


def test_prep_solve_raceline_mu_profile_on_berlin(gpu_engine):
    ck.check_end_to_end(gpu_engine, load_golden("berlin_2018"))


def test_report(gpu_engine, request):
    """Last in the file: the lines' worst deviation next to the guard, past pytest's capture into the log."""
    assert WORST, "no whole track has run"
    print_uncaptured(request.config, "friction lines on the GPU (guard %.3e): %s" % (fg.w_guard(), "; ".join(
        "%s %.3e from the longdouble line, %.3e from numpy's polyfit" % (k, v[0], v[1]) for k, v in WORST.items())))
