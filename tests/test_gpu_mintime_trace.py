"""The minimum-time kernels against the TRACED reference on the MI355X: the bodies of tests/mintime_trace_checks.py (the ones
tests/test_emu_mintime_trace.py runs on the interpreter) against tests/golden/mintime/trace.npz -- what the reference's own opt_mintime.py builds
at each case's w, recorded on the CPU -- ending with the report of the worst deviations.  The fixture alone is read."""
import pytest

import mintime_trace_cases as tc
import mintime_trace_checks as tk

pytestmark = pytest.mark.gpu
LAUNCHED, REPORT = {}, {}


def _merge(worst):
    for k, v in worst.items():
        REPORT[k] = max(REPORT.get(k, 0.0), v)


@pytest.mark.parametrize("lname,name", [(l, n) for l in sorted(tc.LAUNCHES) for n in tc.LAUNCHES[l][0]])
def test_case_against_the_traced_reference(gpu_engine, lname, name):
    """bounds exactly; values, the post-processed arrays, J v, grad J . v, u^T H v under their guards; the step's blocks bit for bit"""
    if lname not in LAUNCHED:
        LAUNCHED[lname] = tk.run_launch(gpu_engine, lname)
    _merge(tk.check_case(LAUNCHED[lname], name))


@pytest.mark.parametrize("name", tc.VALUES_ONLY)
def test_the_large_evaluation_against_the_traced_reference(gpu_engine, name):
    _merge({"N65 " + k: v for k, v in tk.check_values_only(gpu_engine, name).items()})


def test_report():
    """The worst deviation of every quantity, in units of its guard (1.0 is the limit)."""
    for what in sorted(REPORT):
        print("mintime trace, kernels against fixture  %-14s %.3g" % (what, REPORT[what]))
    assert REPORT
