"""The Goldfarb-Idnani path (csrc/mcq_gi.inc) on the MI355X, STEP FOR STEP at the edges of its own code (tests/gi_cases.py: the 64-column blocks
of gi_backsub, the tail of gi_dots, deletions at l = 0 / q - 1 / q = 1 / 65 -> 64, the shift beyond 1024 constraints, a working set of exactly n
rows, a small slot that ends at qcap - 1 / qcap / qcap + 1, gi_grow, the polish's curvature lists in the slot, a ragged batch), against the dense
restatement of tests/gi_ref.py as stored in tests/golden/gi_edges.npz: step counts, working sets, as_iters == 1, the polish not rejected, alpha
under the guard of tests/ring_guard.py's rule -- and the GROWN route against the route that starts in a full slot, bit for bit (the regression
for gi_grow: inlined, it returned wrong vertices on this device only, docs/NOTEBOOK.md R6.4).  The bodies are tests/gi_checks.py's, shared with the
SIMT interpreter's run (tests/test_emu_gi_edges.py).  Reads nothing outside the repository and no live oracle."""
import pytest

import gi_cases as gc
import gi_checks as ck
from ring_guard import Worst, print_uncaptured

pytestmark = pytest.mark.gpu

WORST = Worst()
RESULTS = {}
SMALL = tuple(n for n in gc.names() if n != gc.LARGE)


@pytest.mark.parametrize("name", SMALL)
def test_case_step_for_step(gpu_engine, name):
    RESULTS[name] = ck.check_case(gpu_engine, name, WORST)


def test_the_large_ring_step_for_step(gpu_engine):
    """The one large case: a constraint leaves from under more than 1024 others (the pass-by-pass shift of gi_delete), rows beyond 1024 (gi_sub)."""
    RESULTS[gc.LARGE] = ck.check_case(gpu_engine, gc.LARGE, WORST)


@pytest.mark.parametrize("name", tuple(gc.SLOT_EDGE))
def test_small_slot_edges_sit_where_they_claim(name):
    ck.check_slot_edge(name)


@pytest.mark.parametrize("name", ck.GROWN)
def test_grown_route_against_full_slot_route(gpu_engine, name):
    ck.check_routes(gpu_engine, name, WORST, RESULTS.get(name))


def test_the_comparison_of_routes_is_not_empty():
    assert set(gc.ALL_ACTIVE) <= set(ck.GROWN) and gc.LARGE in ck.GROWN


def test_ragged_batch_is_bitwise_the_single_solves(gpu_engine):
    ck.check_ragged(gpu_engine, WORST)


def test_report(gpu_engine, request):
    """Last in the file: the worst |d alpha| per family next to the guard it was held to, past pytest's capture into the log."""
    assert WORST.w, "no comparison has run"
    print_uncaptured(request.config, WORST.report("Goldfarb-Idnani edges on the GPU"))
