"""The minimum-time kernels against the TRACED reference (tests/golden/mintime/trace.npz: what the reference's own opt_mintime.py builds, recorded
by scripts/make_golden_mintime_trace.py) on the SIMT interpreter (tests/emu), UNCHANGED sources: the bodies of tests/mintime_trace_checks.py.
tests/test_gpu_mintime_trace.py runs the same bodies on the MI355X.  The fixture alone is read, never the reference tree: the engine's problem of
every case was made from the reference's nested `pars` by mintime.pars_from_ini and mintime.problem_from_track."""
import pytest

import mintime_trace_cases as tc
import mintime_trace_checks as tk
from global_racetrajectory_optimization_amd import engine

LAUNCHED, REPORT = {}, {}


def _merge(worst):
    for k, v in worst.items():
        REPORT[k] = max(REPORT.get(k, 0.0), v)


@pytest.fixture(scope="module")
def emu(emu_lib):
    eng = engine.Engine(0, lib_path=emu_lib)
    yield eng
    eng.close()


@pytest.mark.parametrize("lname,name", [(l, n) for l in sorted(tc.LAUNCHES) for n in tc.LAUNCHES[l][0]])
def test_case_against_the_traced_reference(emu, lname, name):
    """bounds exactly; values, the post-processed arrays, J v, grad J . v, u^T H v under their guards; the step's blocks bit for bit"""
    if lname not in LAUNCHED:
        LAUNCHED[lname] = tk.run_launch(emu, lname)
    _merge(tk.check_case(LAUNCHED[lname], name))


@pytest.mark.parametrize("name", tc.VALUES_ONLY)
def test_the_large_evaluation_against_the_traced_reference(emu, name):
    _merge({"N65 " + k: v for k, v in tk.check_values_only(emu, name).items()})


def test_every_small_case_is_in_a_launch():
    assert sorted(n for l in tc.LAUNCHES.values() for n in l[0]) == sorted(tc.SMALL)


def test_report():
    """The worst deviation of every quantity, in units of its guard (1.0 is the limit)."""
    for what in sorted(REPORT):
        print("mintime trace, interpreter against fixture  %-14s %.3g" % (what, REPORT[what]))
    assert REPORT
