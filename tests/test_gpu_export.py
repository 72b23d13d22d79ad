"""The export kernels on the MI355X (mcq_export_device through Engine.export_device / Engine.export_batch) at their structural edges
(tests/export_cases.py), against a plain longdouble reference (tests/export_ref.py): s_ref, spline_lengths and spline_total held to
max(1e-9 m, 4 x spread), decided indices equal, copied columns bitwise (tests/export_guard.py).  The bodies are tests/export_checks.py's, shared
with the SIMT interpreter's run (tests/test_emu_export.py): agreement there says nothing about the gfx950 code object.  Every launch is repeated in
reversed order and must return the same bits; outputs are pre-filled and must be overwritten whole.  Reads nothing outside the repository."""
import pytest

import export_cases as xc
import export_checks as ck
from conftest import load_golden
from ring_guard import Worst, print_uncaptured

pytestmark = pytest.mark.gpu

WORST = Worst()


@pytest.fixture(scope="module", autouse=True)
def the_entry_exists(gpu_engine):
    assert hasattr(gpu_engine.lib, "mcq_export_device")


@pytest.mark.parametrize("name", ("sizes", "rowblock", "tiles", "chunks", "large", "variants"))
@pytest.mark.parametrize("family", xc.FAMILIES)
def test_tables_against_the_reference(gpu_engine, family, name):
    L = next(q for q in xc.launches(family) if q["name"] == "%s/%s" % (family, name))
    ck.check_launch(gpu_engine, L, WORST, alone=name in ("sizes", "variants"))


def test_hand_made_s_columns(gpu_engine):
    ck.check_handmade(gpu_engine)


def test_ties(gpu_engine):
    ck.check_ties(gpu_engine, WORST)


def test_refusals_leave_the_neighbours_alone(gpu_engine):
    ck.check_refusals(gpu_engine)


def test_arguments(gpu_engine):
    ck.check_arguments(gpu_engine)


def test_export_batch(gpu_engine):
    ck.check_export_batch(gpu_engine, WORST)


def test_solve_raceline_profile_trajectory_export_on_berlin(gpu_engine):
    ck.check_end_to_end(gpu_engine, load_golden("berlin_2018"), WORST)


def test_report(gpu_engine, request):
    """Last in the file: the worst deviation per family and quantity next to the guard it was held to, past pytest's capture into the log."""
    assert WORST.w, "no comparison has run"
    print_uncaptured(request.config, WORST.report("export tables on the GPU", what="deviation"))
