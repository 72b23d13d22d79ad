"""The Goldfarb-Idnani edges suite on the SIMT interpreter: the bodies of tests/gi_checks.py (shared with tests/test_gpu_gi_edges.py) on the cases
of tests/gi_cases.py the interpreter finishes in about a minute each (SPECS[...]["emu"]; measured: docs/NOTEBOOK.md, the Goldfarb-Idnani edges
section).  The unchanged kernel sources, step for step against the dense restatement's stored traces."""
import pytest

import gi_cases as gc
import gi_checks as ck
from global_racetrajectory_optimization_amd import engine
from ring_guard import Worst

WORST = Worst()
RESULTS = {}


@pytest.fixture(scope="module")
def emu(emu_lib):
    eng = engine.Engine(0, lib_path=emu_lib)
    yield eng
    eng.close()


@pytest.mark.parametrize("name", gc.EMU)
def test_case_step_for_step(emu, name):
    RESULTS[name] = ck.check_case(emu, name, WORST)


@pytest.mark.parametrize("name", tuple(gc.SLOT_EDGE))
def test_small_slot_edges_sit_where_they_claim(name):
    ck.check_slot_edge(name)


@pytest.mark.parametrize("name", tuple(n for n in ck.GROWN if n in gc.EMU))
def test_grown_route_against_full_slot_route(emu, name):
    ck.check_routes(emu, name, WORST, RESULTS.get(name))


def test_ragged_batch_is_bitwise_the_single_solves(emu):
    ck.check_ragged(emu, WORST)


def test_report():
    assert WORST.w, "no comparison has run"
    print(WORST.report("Goldfarb-Idnani edges on the interpreter"))
