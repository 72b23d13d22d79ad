"""The friction-map generation kernels (csrc/mcq_fgen.inc behind mcq_points_in_path_device / mcq_friction_gen_device) and their Python surface on
the SIMT interpreter (tests/emu), UNCHANGED sources: the cases of tests/fgen_cases.py against matplotlib's recorded verdicts and the reference's
recorded boundaries, equal.  tests/test_gpu_fgen.py runs the same bodies (tests/fgen_checks.py) on the MI355X, where the code object is what is
tested -- the interpreter build has no fused multiply-add and cannot see a contracted contour; here the kernels' logic is."""
import pytest

import fgen_cases as fc
import fgen_checks as ck
from global_racetrajectory_optimization_amd import engine


@pytest.fixture(scope="module")
def emu(emu_lib):
    eng = engine.Engine(0, lib_path=emu_lib)
    assert "mcq_friction_gen_device" in engine.EXPORTED_SYMBOLS and hasattr(eng.lib, "mcq_points_in_path_device")
    yield eng
    eng.close()


def test_paths_against_matplotlib(emu):
    ck.check_paths(emu)


def test_paths_of_up_to_three_vertices(emu):
    ck.check_tiny_paths(emu)


def test_point_counts(emu):
    ck.check_point_counts(emu)


def test_points_that_are_not_finite(emu):
    ck.check_nonfinite_points(emu)


def test_path_refusals(emu):
    ck.check_path_refusals(emu)


def test_path_layout(emu):
    ck.check_path_layout(emu)


def test_path_arguments(emu):
    ck.check_path_arguments(emu)


@pytest.mark.parametrize("name", sorted(fc.small_tracks()))
def test_small_and_open_tracks(emu, name):
    ck.check_small_track(emu, name)


@pytest.mark.parametrize("track", fc.SMALL_TRACKS)
def test_whole_track_against_the_recorded_reference(emu, track):
    ck.check_whole_track(emu, track, widths=(2.0, 0.7))


def test_refusals(emu):
    ck.check_refusals(emu)


def test_layout(emu):
    ck.check_layout(emu)


def test_gen_arguments(emu):
    ck.check_gen_arguments(emu)


def test_the_reference_names_and_files(emu, tmp_path):
    ck.check_dropin(emu, str(tmp_path))


def test_generated_map_under_the_berlin_raceline(emu):
    from conftest import load_golden
    ck.check_end_to_end(emu, load_golden("berlin_2018"))
