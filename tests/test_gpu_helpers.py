"""The plumbing behind the helper entries on the MI355X: Engine.scope frees every pointer exactly once, a handle's grow-only scratch buffers
return a fresh handle's bits after they grew with a launch still queued, the row packer keeps its two modes apart.  The bodies are
tests/helper_checks.py's, shared with the SIMT interpreter's run (tests/test_emu_helpers.py, which also holds the header against the ABI table)."""
import pytest

import helper_checks as ck
from global_racetrajectory_optimization_amd import engine

pytestmark = pytest.mark.gpu


def test_every_pointer_is_freed_exactly_once(gpu_engine):
    ck.check_freed_once(gpu_engine)


@pytest.mark.parametrize("which", sorted(ck.STAGES))
def test_a_grown_scratch_returns_a_fresh_handles_bits(gpu_engine, which):
    ck.check_scratch_regrowth(lambda: engine.Engine(0), which)


def test_grown_ends_records_return_a_fresh_handles_bits(gpu_engine):
    ck.check_ends_regrowth(lambda: engine.Engine(0))


def test_the_packers_two_modes(gpu_engine):
    ck.check_packer_modes(gpu_engine)
