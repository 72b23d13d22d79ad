"""The chain form of the raceline kernel on the MI355X (mcq_raceline_ends_kernel behind mcq_raceline_device_ends / Engine.raceline_batch(ends=...))
at its structural edges (tests/race_open_cases.py), against a plain longdouble reference (tests/race_open_ref.py), each quantity held to
max(floor, 4 x spread) (tests/race_open_guard.py).  The bodies are tests/race_open_checks.py's, shared with the SIMT interpreter's run
(tests/test_emu_race_open.py): agreement there says nothing about the gfx950 code object or the device's hypot / atan2 / sqrt.  Point counts and
statuses are exact; every launch is repeated in reversed order and must return the same bits; ring rows of a mixed launch are
mcq_raceline_device's bits.  Reads nothing outside the repository."""
import pytest

import race_open_cases as oc
import race_open_checks as ck
from conftest import load_golden
from ring_guard import Worst, print_uncaptured

pytestmark = pytest.mark.gpu

WORST = Worst()


@pytest.fixture(scope="module", autouse=True)
def the_entry_exists(gpu_engine):
    assert hasattr(gpu_engine.lib, "mcq_raceline_device_ends")


@pytest.mark.parametrize("family", tuple(oc.FAMILIES))
def test_open_raceline_against_the_reference(gpu_engine, family):
    for launch in oc.launches(family):
        ck.check_launch(gpu_engine, family, launch, WORST)


@pytest.mark.parametrize("family", tuple(oc.FAMILIES))
def test_rings_and_chains_in_one_launch(gpu_engine, family):
    ck.check_mixed(gpu_engine, family)


def test_arguments_and_status(gpu_engine):
    ck.check_arguments_and_status(gpu_engine, "peanut")


def test_chain_solve_into_open_raceline_into_unclosed_profile(gpu_engine):
    ck.check_end_to_end(gpu_engine, load_golden("open_handling_a"), WORST)


def test_report(gpu_engine, request):
    """Last in the file: the worst deviation per family and quantity next to the guard it was held to, past pytest's capture into the log."""
    assert WORST.w, "no comparison has run"
    print_uncaptured(request.config, WORST.report("open racelines on the GPU", what="deviation"))
