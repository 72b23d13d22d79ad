"""The batched vector loops and the folded pass of ipm_box (MCQ_KKT_CORR_BATCH, MCQ_ENTRY_BATCH, MCQ_IPB_FOLD_P1:
tests/test_emu_entry_batch.py holds them to the earlier forms bit for bit on the interpreter) on the GPU, where the compiler decides what is in flight: one ragged launch of thirteen ovals at the
edges of the batching against live references, and the same launch in reversed order and problem by problem, bit for bit.

References: the dense oracle up to n = 273 (under 0.1 s each), CPU-B from n = 1040 (on these ovals it returns status 4 below that and
status 0 with 9-11 interior-point iterations and 1-2 rounds from 1040 on).  Bound: ring_guard.FIXED, 1e-8 m, the suite's rule for live
references.  On the interpreter the same comparison gives 6.7e-10 m (dense oracle, at n = 47) and 2.5e-13 m (CPU-B) at worst."""
import numpy as np
import pytest

import ring_guard
from global_racetrajectory_optimization_amd import synthetic
from global_racetrajectory_optimization_amd.trajectory_planning_helpers import calc_splines as cs
from oracle import banded_ref, tph_ref

SIZES = (47, 48, 255, 256, 272, 273, 1040, 1041, 1057, 2047, 2048, 2064, 2065)
DENSE_UP_TO = 273
KAPPA, W_VEH = 0.12, 3.4


def problems():
    out = []
    for n in SIZES:
        ref, nv, sc = synthetic.oval_batch(1, n=n, first=0)
        out.append(dict(reftrack=ref[0], normvec=nv[0], scaling=sc[0], kappa_bound=KAPPA, w_veh=W_VEH))
    return out


def references(probs):
    """alpha of the dense oracle (n <= 273) or CPU-B (n >= 1040) per problem, and which of the two it was"""
    out = []
    for p in probs:
        n = p["reftrack"].shape[0]
        if n <= DENSE_UP_TO:
            a, _ = tph_ref.opt_min_curv(p["reftrack"], p["normvec"], cs.build_les_matrix(n, p["scaling"]), KAPPA, W_VEH)
            out.append(("dense", a))
        else:
            a, _, st, _, _ = banded_ref.solve_batch(p["reftrack"][None], p["normvec"][None], p["scaling"][None], KAPPA, W_VEH)
            assert st[0] == 0, (n, st[0])
            out.append(("cpu_b", a[0]))
    return out


def compare(eng, show=print):
    """The whole check on `eng` (the GPU engine here; scripts may hand in an interpreter engine): returns the worst deviation per reference."""
    probs = problems()
    refs = references(probs)
    al, curv, st, _ = eng.solve_batch(probs)
    assert list(st) == [0] * len(probs), list(st)
    worst = {"dense": 0.0, "cpu_b": 0.0}
    for k, (kind, a_ref) in enumerate(refs):
        d = ring_guard.dmax(al[k], a_ref)
        show("n = %4d  %-5s  max |alpha - reference| = %.2e m" % (SIZES[k], kind, d))
        worst[kind] = max(worst[kind], d)
    show("worst: dense oracle %.2e m, CPU-B %.2e m (bound %.0e m)" % (worst["dense"], worst["cpu_b"], ring_guard.FIXED))
    assert worst["dense"] < ring_guard.FIXED and worst["cpu_b"] < ring_guard.FIXED, worst
    # the same problems in reversed order, then one per launch: nothing may depend on which workgroup runs next to which
    al_r, curv_r, st_r, _ = eng.solve_batch(probs[::-1])
    assert np.array_equal(st_r[::-1], st) and np.array_equal(curv_r[::-1], curv)
    for k in range(len(probs)):
        assert np.array_equal(al_r[len(probs) - 1 - k], al[k]), ("reversed", SIZES[k])
        al_1, curv_1, st_1, _ = eng.solve_batch([probs[k]])
        assert st_1[0] == st[k] and curv_1[0] == curv[k] and np.array_equal(al_1[0], al[k]), ("alone", SIZES[k])
    return worst


@pytest.mark.gpu
def test_thirteen_ovals_at_the_edges_of_the_batching(gpu_engine, request):
    compare(gpu_engine, show=lambda line: ring_guard.print_uncaptured(request.config, line))
