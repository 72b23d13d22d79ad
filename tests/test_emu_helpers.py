"""The plumbing behind the helper entries on the SIMT interpreter (tests/emu), UNCHANGED sources: Engine.scope frees every pointer exactly once, a
handle's grow-only scratch buffers return a fresh handle's bits after they grew, include/mcq.h and the ABI table of engine.py agree, the row
packer keeps its two modes apart.  The bodies are tests/helper_checks.py's, shared with tests/test_gpu_helpers.py."""
import pytest

import helper_checks as ck
from global_racetrajectory_optimization_amd import engine


@pytest.fixture(scope="module")
def emu(emu_lib):
    eng = engine.Engine(0, lib_path=emu_lib)
    yield eng
    eng.close()


def test_header_and_abi_table_agree():
    """Needs no library."""
    ck.check_abi_table()


def test_every_pointer_is_freed_exactly_once(emu):
    ck.check_freed_once(emu)


@pytest.mark.parametrize("which", sorted(ck.STAGES))
def test_a_grown_scratch_returns_a_fresh_handles_bits(emu_lib, which):
    ck.check_scratch_regrowth(lambda: engine.Engine(0, lib_path=emu_lib), which)


def test_grown_ends_records_return_a_fresh_handles_bits(emu_lib):
    ck.check_ends_regrowth(lambda: engine.Engine(0, lib_path=emu_lib))


def test_the_packers_two_modes(emu):
    ck.check_packer_modes(emu)
