"""The route of the host-buffer entries (csrc/mcq_api.hip, slices_for / note_solve): what tests/test_emu_host_routes.py runs on the SIMT
interpreter and tests/test_gpu_host_routes.py on the GPU.  Rings of 16 waypoints in batches of four, $MCQ_HOST_SLICE_MIN=4: mcq_solve_host and
mcq_solve_batch WOULD take such a batch in two slices.

(a) A warm start that applies -- working sets carried over by mcq_relinearise_device for exactly this layout -- takes the one launch and is
    honoured, as in mcq_solve_device: the sequence returns, bit for bit, what it returns with $MCQ_HOST_ONE_LAUNCH=1.  (Before the routing rule
    was stated once, the sliced host entries dropped the warm start silently.)  That the comparison can tell: the same sequence without the
    warm start reports interior-point iterations, the warm one none.
(b) An open mcq_timing_begin / mcq_timing_end span counts one launch per call, sliced or not; mcq_last_timing after a sliced host call still
    refuses (no single pair of events spans the slices)."""
import numpy as np
import pytest

import device_slices_checks as dc
from global_racetrajectory_optimization_amd import engine

BATCH, N = 4, 16


def sliced_env(monkeypatch):
    monkeypatch.setenv("MCQ_HOST_SLICE_MIN", "4")
    for name in ("MCQ_HOST_ONE_LAUNCH", "MCQ_HOST_SLICES", "MCQ_DEVICE_SLICE_MIN", "MCQ_DEVICE_ONE_LAUNCH"):
        monkeypatch.delenv(name, raising=False)


def iters(info):
    """the iteration fields of the info records, whichever way the entry returned them (mcq_solve_host: McqInfo array; mcq_solve_batch: dicts)"""
    return [tuple(int(i[f] if isinstance(i, dict) else getattr(i, f)) for f in dc.ITER_FIELDS) for i in info]


class Carry:
    """The batch resident on the device, solved there once, and what mcq_relinearise_device needs to carry its working sets over (state2)"""

    def __init__(self, eng, a):
        self.eng, self.inp, self.out = eng, dc.Inputs(eng, *a), dc.Outputs(eng, BATCH, N)
        self.d_n, self.d_m, self.d_st = (eng.alloc(4 * BATCH) for _ in range(3))
        self.d_ro, self.d_no = eng.alloc(8 * BATCH * N * 4), eng.alloc(8 * BATCH * N * 2)
        eng.upload(self.d_n, np.full(BATCH, N, dtype=np.int32))

    def solve_on_device(self):
        dc.solve(self.eng, self.inp, self.out)      # (four problems: below mcq_solve_device's own threshold)

    def carry_over(self):
        self.eng.relinearise_device(BATCH, N, self.d_n, self.inp.ref, self.inp.nv, self.out.alpha, None, 1.0, 400.0, self.d_ro, self.d_no, self.d_m,
                                    self.d_st)


def sequence(eng, a, warm_start):
    """solve on the device, carry over, mcq_solve_host; carry over, mcq_solve_batch; then mcq_solve_host with nothing carried over"""
    ref, nv, sc = a
    probs = [dict(reftrack=ref[k], normvec=nv[k], scaling=sc[k], kappa_bound=dc.KAPPA_BOUND, w_veh=dc.W_VEH) for k in range(BATCH)]
    c = Carry(eng, a)
    c.solve_on_device()
    c.carry_over()
    al, cu, st, info = eng.solve_host(ref, nv, sc, dc.KAPPA_BOUND, dc.W_VEH, warm_start=warm_start)
    res = [(al.copy(), cu.copy(), st.copy(), iters(info))]
    c.carry_over()
    al, cu, st, info = eng.solve_batch(probs, warm_start=warm_start)
    res.append((np.stack(al), cu.copy(), st.copy(), iters(info)))
    al, cu, st, info = eng.solve_host(ref, nv, sc, dc.KAPPA_BOUND, dc.W_VEH, warm_start=warm_start)       # (the solves above have spent state2)
    res.append((al.copy(), cu.copy(), st.copy(), iters(info)))
    return res


def same(x, y, what):
    for k, name in enumerate(("alpha", "curv_error", "status")):
        assert np.array_equal(x[k], y[k]), "%s: %s differs" % (what, name)
    assert x[3] == y[3], "%s: info records differ: %r / %r" % (what, x[3], y[3])


WHAT = ("mcq_solve_host, warm", "mcq_solve_batch, warm", "mcq_solve_host, nothing carried over")


def check_warm_start_through_the_host_entries(eng, monkeypatch):
    a = dc.ovals(BATCH, N)
    sliced_env(monkeypatch)
    warm = sequence(eng, a, 1)
    cold = sequence(eng, a, -1)
    with monkeypatch.context() as m:
        m.setenv("MCQ_HOST_ONE_LAUNCH", "1")
        warm_one = sequence(eng, a, 1)
        cold_one = sequence(eng, a, -1)
    ipm = dc.ITER_FIELDS.index("ipm_iters")
    for k in range(3):
        assert (warm[k][2] == 0).all() and (cold[k][2] == 0).all(), WHAT[k]
        same(warm[k], warm_one[k], WHAT[k] + ", against the one launch")
        same(cold[k], cold_one[k], WHAT[k] + ", no warm start, against the one launch")
    for k in range(2):
        # the case can tell: a warm start that is honoured runs no interior-point iteration, the cold solve of the same batch does
        assert all(i[ipm] == 0 for i in warm[k][3]) and all(i[ipm] > 0 for i in cold[k][3]), (WHAT[k], warm[k][3], cold[k][3])
        assert warm[k][3] != cold[k][3]
        assert np.max(np.abs(warm[k][0] - cold[k][0])) < 2e-6      # (the same minimiser, each within the solver's 1e-6 m of it)
    # the third call found nothing carried over: sliced again, the cold solve
    same(warm[2], cold[2], WHAT[2])
    assert all(i[ipm] > 0 for i in warm[2][3])


def check_span_counts_calls(eng, monkeypatch):
    sliced_env(monkeypatch)
    ref, nv, sc = dc.ovals(BATCH, N)
    eng.timing_begin()
    eng.solve_host(ref, nv, sc, dc.KAPPA_BOUND, dc.W_VEH)                       # sliced
    eng.solve_host(ref, nv, sc, dc.KAPPA_BOUND, dc.W_VEH)                       # sliced
    eng.solve_host(ref[:2], nv[:2], sc[:2], dc.KAPPA_BOUND, dc.W_VEH)           # two problems: below the threshold
    ms, launches = eng.timing_end()
    assert launches == 3 and ms > 0.0
    assert eng.last_timing_ms()["solve"] > 0.0                                  # (the unsliced call: timed)
    eng.solve_host(ref, nv, sc, dc.KAPPA_BOUND, dc.W_VEH)
    with pytest.raises(engine.EngineError, match="no timed launch"):
        eng.last_timing_ms()
