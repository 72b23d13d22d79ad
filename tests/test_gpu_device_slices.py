"""mcq_solve_device in two slices on the GPU (tests/device_slices_checks.py), slicing forced with $MCQ_DEVICE_SLICE_MIN=2: here the two
compute streams really run side by side, so what is checked is the ORDER the handle promises.  Every case pre-fills its outputs with a NaN
sentinel by upload, enqueues six calls back to back and downloads with no synchronisation of its own in between -- the download has to
join the streams --, then asserts that no sentinel is left and that the results are bitwise those of the one launch
($MCQ_DEVICE_ONE_LAUNCH=1) and of a problem-by-problem run.  (a) the same buffers and (b) two sets of outputs in turn take the overlapped
path; (c) output rows that cross those of the other slice, (d) scalings read from where an earlier call wrote alpha and (e) a helper entry
straight after take the join -- read from the entry's trace lines.

Shapes: batch 5 and 8 (slices of 3 + 2 and 4 + 4), n = 47 and 257 (a segment edge and `tid + 256 u < n` in play).  The references of a
shape are computed once and shared.  Separately: one sliced call against the dense oracle at ring_guard.FIXED."""
import numpy as np
import pytest

import device_slices_checks as dc
import ring_guard
from global_racetrajectory_optimization_amd import engine
from global_racetrajectory_optimization_amd.trajectory_planning_helpers import calc_splines as cs
from oracle import tph_ref

SHAPES = [(5, 47), (8, 47), (5, 257), (8, 257)]


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(0)
    yield e
    e.close()


@pytest.fixture()
def sliced(monkeypatch):
    monkeypatch.setenv("MCQ_DEVICE_SLICE_MIN", "2")
    monkeypatch.setenv("MCQ_DEVICE_SLICE_TRACE", "1")
    monkeypatch.delenv("MCQ_DEVICE_ONE_LAUNCH", raising=False)


_refs = {}


def refs(eng, monkeypatch, batch, n):
    """per shape, once: the batches a and b, each in one launch and problem by problem -- which must agree before anything is compared to them"""
    if (batch, n) not in _refs:
        a, b = dc.ovals(batch, n), dc.ovals(batch, n, first=batch)
        r = {"a": a, "b": b}
        with monkeypatch.context() as m:
            m.setenv("MCQ_DEVICE_ONE_LAUNCH", "1")
            for key, x in (("a", a), ("b", b)):
                inp, out = dc.Inputs(eng, *x), dc.Outputs(eng, batch, n)
                dc.solve(eng, inp, out)
                r["one_" + key] = out.get(eng)
                r["each_" + key] = dc.one_by_one(eng, *x)
                dc.same(r["one_" + key], r["each_" + key], "one launch against problem by problem (%s)" % key)
                assert (r["one_" + key][2] == 0).all()
        _refs[(batch, n)] = r
    return _refs[(batch, n)]


@pytest.mark.gpu
@pytest.mark.parametrize("batch,n", SHAPES)
def test_same_buffers(eng, sliced, monkeypatch, capfd, batch, n):
    r = refs(eng, monkeypatch, batch, n)
    capfd.readouterr()
    res = dc.case_same_buffers(eng, r["a"], r["b"])
    assert dc.paths(capfd.readouterr().err) == ["joined"] + ["overlapped"] * (dc.CALLS - 1)
    dc.no_sentinel(res, "same buffers")
    dc.same(res, r["one_b"], "same buffers against the one launch")
    dc.same(res, r["each_b"], "same buffers against problem by problem")


@pytest.mark.gpu
@pytest.mark.parametrize("batch,n", SHAPES)
def test_alternating_buffers(eng, sliced, monkeypatch, capfd, batch, n):
    r = refs(eng, monkeypatch, batch, n)
    capfd.readouterr()
    res = dc.case_alternating(eng, r["a"], r["b"])
    assert dc.paths(capfd.readouterr().err) == ["joined"] + ["overlapped"] * (dc.CALLS - 1)
    for k, key in enumerate("ab"):
        dc.no_sentinel(res[k], "alternating buffers, set %d" % k)
        dc.same(res[k], r["one_" + key], "alternating buffers, set %d against the one launch" % k)
        dc.same(res[k], r["each_" + key], "alternating buffers, set %d against problem by problem" % k)


@pytest.mark.gpu
@pytest.mark.parametrize("batch,n", SHAPES)
def test_outputs_shifted_by_two_rows(eng, sliced, monkeypatch, capfd, batch, n):
    r = refs(eng, monkeypatch, batch, n)
    capfd.readouterr()
    res = dc.case_shifted(eng, r["a"], r["b"])
    assert dc.paths(capfd.readouterr().err) == ["joined"] * dc.CALLS
    dc.no_sentinel(res, "shifted outputs")
    with monkeypatch.context() as m:
        m.setenv("MCQ_DEVICE_ONE_LAUNCH", "1")
        dc.same(res, dc.case_shifted(eng, r["a"], r["b"]), "shifted outputs against the one launch")
    dc.same(res, r["each_a"], "shifted outputs, rows 0 and 1, against problem by problem", rows=slice(0, 2))
    dc.same(tuple(x[2:] for x in res), r["each_b"], "shifted outputs, rows 2 .., against problem by problem")


@pytest.mark.gpu
@pytest.mark.parametrize("batch,n", SHAPES)
def test_scaling_read_from_an_earlier_alpha(eng, sliced, monkeypatch, capfd, batch, n):
    r = refs(eng, monkeypatch, batch, n)
    a, b = r["a"], r["b"]
    capfd.readouterr()
    res = dc.case_scaling_from_alpha(eng, a, b)
    assert dc.paths(capfd.readouterr().err) == ["joined"] * dc.CALLS
    for k in range(2):
        dc.no_sentinel(res[k], "scalings from alpha, set %d" % k)
    assert (res[0][2] == 0).all() and (res[1][2] == 0).all() and np.max(np.abs(res[0][0] - b[2])) < 2e-9
    with monkeypatch.context() as m:
        m.setenv("MCQ_DEVICE_ONE_LAUNCH", "1")
        one = dc.case_scaling_from_alpha(eng, a, b)
        each_pinned = dc.one_by_one(eng, dc.pinned_at(a[0], b[2]), a[1], a[2])
        each = dc.one_by_one(eng, b[0], b[1], each_pinned[0])
    for k, (o, e) in enumerate(zip(one, (each_pinned, each))):
        dc.same(res[k], o, "scalings from alpha, set %d against the one launch" % k)
        dc.same(res[k], e, "scalings from alpha, set %d against problem by problem" % k)


@pytest.mark.gpu
@pytest.mark.parametrize("batch,n", SHAPES)
def test_helper_entry_straight_after(eng, sliced, monkeypatch, capfd, batch, n):
    r = refs(eng, monkeypatch, batch, n)
    capfd.readouterr()
    res = dc.case_helper_after(eng, r["a"])
    assert dc.paths(capfd.readouterr().err) == ["joined"]
    dc.no_sentinel(res[0], "helper after")
    with monkeypatch.context() as m:
        m.setenv("MCQ_DEVICE_ONE_LAUNCH", "1")
        dc.same_raceline(res, dc.case_helper_after(eng, r["a"]), "raceline straight after the slices")
    dc.same(res[0], r["each_a"], "helper after, against problem by problem")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [47, 257])
def test_sliced_call_against_the_dense_oracle(eng, sliced, capfd, request, n):
    ref, nv, sc = dc.ovals(5, n)
    inp, out = dc.Inputs(eng, ref, nv, sc), dc.Outputs(eng, 5, n)
    capfd.readouterr()
    dc.solve(eng, inp, out)
    res = out.get(eng)
    assert dc.paths(capfd.readouterr().err) in (["joined"], ["overlapped"]) and (res[2] == 0).all()
    worst = 0.0
    for k in range(5):
        a_ref, _ = tph_ref.opt_min_curv(ref[k], nv[k], cs.build_les_matrix(n, sc[k]), dc.KAPPA_BOUND, dc.W_VEH)
        worst = max(worst, ring_guard.dmax(res[0][k], a_ref))
    ring_guard.print_uncaptured(request.config, "sliced call, n = %d: max |alpha - dense oracle| = %.2e m (bound %.0e m)" % (n, worst, ring_guard.FIXED))
    assert worst < ring_guard.FIXED
