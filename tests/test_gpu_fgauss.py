"""The Gaussian friction fit and the models' evaluation on the MI355X (mcq_friction_gauss_device, mcq_friction_model_device through the Engine and
through friction.py) at their structural edges (tests/fgauss_cases.py) and on the recorded whole tracks, against the longdouble restatement
(tests/fgauss_ref.py) under the rules of tests/fgauss_guard.py.  The bodies are tests/fgauss_checks.py's, shared with the SIMT interpreter's run
(tests/test_emu_fgauss.py): agreement there says nothing about the gfx950 code object -- its exp, its LDS exchange between the lanes of a wave, its
contraction-off arithmetic (center_dist and the linear model are compared bit for bit).  Reads nothing outside the repository."""
import pytest

import fgauss_cases as gc
import fgauss_checks as ck
import fgauss_guard as gg
from conftest import load_golden
from ring_guard import print_uncaptured

pytestmark = pytest.mark.gpu

WORST = {}


@pytest.fixture(scope="module", autouse=True)
def the_entries_exist(gpu_engine):
    assert hasattr(gpu_engine.lib, "mcq_friction_gauss_device") and hasattr(gpu_engine.lib, "mcq_friction_model_device")


@pytest.mark.parametrize("name", sorted(gc.launches()))
def test_hand_made_rows_against_the_restatement(gpu_engine, name):
    WORST["rows " + name] = "weights %.2f, fitted %.2f of their guards" % ck.check_launch(gpu_engine, name)


def test_explicit_rcond(gpu_engine):
    WORST["rcond"] = "weights %.2f, fitted %.2f of their guards" % ck.check_rcond(gpu_engine)


def test_arguments_and_the_lds_refusal(gpu_engine):
    ck.check_arguments(gpu_engine)


def test_model_evaluation(gpu_engine):
    WORST["evaluation"] = "%.2f of the fitted-value guard from the recorded predict, %.2f of the float64 bound from the longdouble evaluation" % \
        ck.check_model(gpu_engine)


def test_grid_batch_keeps_its_results_and_adds_the_fit(gpu_engine):
    ck.check_grid_surface(gpu_engine)


@pytest.mark.parametrize("n_gauss", gg.N_GAUSS)
@pytest.mark.parametrize("track", gg.TRACKS)
def test_whole_track_against_the_recorded_reference(gpu_engine, track, n_gauss):
    d = ck.check_whole_track(gpu_engine, track, n_gauss)
    WORST["%s n_gauss %d" % (track, n_gauss)] = ("weights %.3e (guard %.3e; %.3e from sklearn's), fitted %.3e (guard %.3e), %d sweeps, %d undecided"
                                                 % (d["w"], d["guard_w"], d["sklearn"], d["fitted"], d["guard_f"], d["sweeps"], d["undecided"]))


def test_the_reference_names(gpu_engine, tmp_path, monkeypatch):
    ck.check_dropin(gpu_engine, str(tmp_path), monkeypatch)


def test_grid_fit_evaluation_on_berlin(gpu_engine):
    d = ck.check_end_to_end(gpu_engine, load_golden("berlin_2018"))
    WORST["berlin end to end"] = "fitted %.3e (guard %.3e), evaluation %.2f of its bound" % (d["fitted"], d["guard_f"], d["eval"])


def test_report(gpu_engine, request):
    """Last in the file: the worst deviations next to their guards, past pytest's capture into the log."""
    assert any(k.startswith("berlin_2018") for k in WORST), "no whole track has run"
    print_uncaptured(request.config, "Gaussian friction fit on the GPU (longdouble restatement; floor %.3e): %s" % (
        gg.floor(), "; ".join("%s: %s" % kv for kv in WORST.items())))
