"""The Gaussian friction fit and the models' evaluation (mcq_friction_gauss_kernel, mcq_friction_model_kernel behind mcq_friction_gauss_device /
mcq_friction_model_device) and their Python surface on the SIMT interpreter (tests/emu), UNCHANGED sources: the rows of tests/fgauss_cases.py and
the recorded whole tracks against tests/fgauss_ref.py under the rules of tests/fgauss_guard.py.  tests/test_gpu_fgauss.py runs the same bodies
(tests/fgauss_checks.py) on the MI355X, where the code object is what is tested -- the interpreter has the host's exp and no fused multiply-add;
here the kernels' logic is: the lanes' shares, the exchange buffers, the pair order, the cut."""
import pytest

import fgauss_cases as gc
import fgauss_checks as ck
import fgauss_guard as gg
from conftest import load_golden
from global_racetrajectory_optimization_amd import engine


@pytest.fixture(scope="module")
def emu(emu_lib):
    eng = engine.Engine(0, lib_path=emu_lib)
    assert "mcq_friction_gauss_device" in engine.EXPORTED_SYMBOLS and hasattr(eng.lib, "mcq_friction_model_device")
    yield eng
    eng.close()


@pytest.mark.parametrize("name", sorted(gc.launches()))
def test_hand_made_rows_against_the_restatement(emu, name):
    ck.check_launch(emu, name)


def test_explicit_rcond(emu):
    ck.check_rcond(emu)


def test_arguments_and_the_lds_refusal(emu):
    ck.check_arguments(emu)


def test_model_evaluation(emu):
    ck.check_model(emu)


def test_grid_batch_keeps_its_results_and_adds_the_fit(emu):
    ck.check_grid_surface(emu)


@pytest.mark.parametrize("n_gauss", gg.N_GAUSS)
@pytest.mark.parametrize("track", gg.TRACKS)
def test_whole_track_against_the_recorded_reference(emu, track, n_gauss):
    ck.check_whole_track(emu, track, n_gauss)


def test_the_reference_names(emu, tmp_path, monkeypatch):
    ck.check_dropin(emu, str(tmp_path), monkeypatch)


def test_grid_fit_evaluation_on_berlin(emu):
    ck.check_end_to_end(emu, load_golden("berlin_2018"))
