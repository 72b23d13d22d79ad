"""The friction-map generation entries on the MI355X (mcq_points_in_path_device, mcq_friction_gen_device through the Engine and through
friction.py) at their structural edges (tests/fgen_cases.py) against matplotlib's recorded verdicts and the reference's recorded boundaries: equal,
no tolerance.  The bodies are tests/fgen_checks.py's, shared with the SIMT interpreter's run (tests/test_emu_fgen.py): agreement there says nothing
about the gfx950 code object.  Decided here only: that no product and sum of the contour, the boundaries or numpy.arange's grid was fused (the
interpreter build has no fused multiply-add), and the two large tracks whole.  Reads nothing outside the repository."""
import pytest

import fgen_cases as fc
import fgen_checks as ck
from conftest import load_golden
from ring_guard import print_uncaptured

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def the_entries_exist(gpu_engine):
    assert hasattr(gpu_engine.lib, "mcq_points_in_path_device") and hasattr(gpu_engine.lib, "mcq_friction_gen_device")


def test_paths_against_matplotlib(gpu_engine):
    ck.check_paths(gpu_engine)


def test_paths_of_up_to_three_vertices(gpu_engine):
    ck.check_tiny_paths(gpu_engine)


def test_point_counts(gpu_engine):
    ck.check_point_counts(gpu_engine)


def test_points_that_are_not_finite(gpu_engine):
    ck.check_nonfinite_points(gpu_engine)


def test_path_refusals(gpu_engine):
    ck.check_path_refusals(gpu_engine)


def test_path_layout(gpu_engine):
    ck.check_path_layout(gpu_engine)


def test_path_arguments(gpu_engine):
    ck.check_path_arguments(gpu_engine)


@pytest.mark.parametrize("name", sorted(fc.small_tracks()))
def test_small_and_open_tracks(gpu_engine, name):
    ck.check_small_track(gpu_engine, name)


@pytest.mark.parametrize("track", fc.TRACKS)
def test_whole_track_against_the_recorded_reference(gpu_engine, track):
    ck.check_whole_track(gpu_engine, track, widths=(2.0, 0.7) if track in fc.SMALL_TRACKS else (2.0,))


def test_refusals(gpu_engine):
    ck.check_refusals(gpu_engine)


def test_layout(gpu_engine):
    ck.check_layout(gpu_engine)


def test_gen_arguments(gpu_engine):
    ck.check_gen_arguments(gpu_engine)


def test_the_reference_names_and_files(gpu_engine, tmp_path):
    ck.check_dropin(gpu_engine, str(tmp_path), berlin=True)


def test_generated_map_under_the_berlin_raceline(gpu_engine, request):
    worst = ck.check_end_to_end(gpu_engine, load_golden("berlin_2018"))
    print_uncaptured(request.config, "friction map generation on the GPU: the Berlin raceline's farthest nearest cell %.3f m (cell 2.0 m)" % worst)
