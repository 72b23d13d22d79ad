"""FITPACK's periodic smoothing fit on the MI355X (mcq_spline_fit_device through Engine.spline_fit_batch / prep_track_batch) at its structural
edges (tests/fit_cases.py), against scipy's recording and the longdouble restatement: knots, nk and ier exact, coefficients and fp held to
max(floor, 4 x spread) (tests/fit_guard.py).  The bodies are tests/fit_checks.py's, shared with the SIMT interpreter's run
(tests/test_emu_fit.py): agreement there says nothing about the gfx950 code object or the device's division and sqrt.  Reads the goldens;
imports no scipy; reads nothing outside the repository."""
import pytest

import fit_cases as fc
import fit_checks as ck
from conftest import load_golden
from ring_guard import Worst, print_uncaptured

pytestmark = pytest.mark.gpu

WORST = Worst()
DEV_C = {}


@pytest.fixture(scope="module", autouse=True)
def the_entry_exists(gpu_engine):
    assert hasattr(gpu_engine.lib, "mcq_spline_fit_device")


@pytest.mark.parametrize("name", fc.CASES)
def test_case_against_the_recording(gpu_engine, name):
    ck.check_case(gpu_engine, name, WORST)
    DEV_C[name] = WORST.w[name + ".c"][0]


@pytest.mark.parametrize("name", ("lobe_k3_s2", "rs256"))
def test_mi_at_and_beyond_mimax(gpu_engine, name):
    ck.check_mimax(gpu_engine, name)


def test_refusals_leave_the_other_tracks_alone(gpu_engine):
    ck.check_refusals(gpu_engine)


def test_arguments(gpu_engine):
    ck.check_arguments(gpu_engine)


def test_mixed_launch_alone_reversed_and_a_refused_track(gpu_engine):
    ck.check_batch(gpu_engine, WORST)


def test_nothing_stale_survives(gpu_engine):
    ck.check_stale(gpu_engine)


@pytest.mark.parametrize("name,key", (("rounded_rectangle", "rr_mincurv"), ("berlin_2018", "berlin_mincurv")))
def test_prep_track_with_the_device_fit_to_solve(gpu_engine, name, key):
    if name not in DEV_C:
        ck.check_case(gpu_engine, name, WORST)
        DEV_C[name] = WORST.w[name + ".c"][0]
    ck.check_end_to_end(gpu_engine, name, key, load_golden(name), load_golden("harness_runs"), WORST, DEV_C[name])


def test_report(gpu_engine, request):
    """Last in the file: the worst deviation per case and quantity next to the guard it was held to, past pytest's capture into the log."""
    assert WORST.w, "no comparison has run"
    print_uncaptured(request.config, WORST.report("periodic smoothing fit on the GPU", what="deviation"))
