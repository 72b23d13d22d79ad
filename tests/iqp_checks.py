"""The bodies of tests/test_emu_iqp.py (SIMT interpreter) and tests/test_gpu_iqp.py (MI355X): mcq_iqp_batch -- iqp_step_track, mcq_iqp_step_kernel,
mcq_iqp_rounds_kernel, the host's round loop, round cap and two-buffer download -- on the cases of tests/iqp_cases.py against tests/iqp_ref.py under
the guards of tests/iqp_guard.py.  Round counts, waypoint counts and statuses are compared exactly; alpha, ring rows, normals and curvature errors
within their guards; the routes of one call (fused launch or round by round, timed, callback, caller's buffers, a batch's order and neighbours,
the resident entry mcq_iqp_device on buffers of the test's own, a handle whose buffers grew in between) bit for bit.  Every function takes the engine; those that compare with the reference take a ring_guard.Worst that collects the worst deviation
per family and quantity next to its guard."""
import contextlib
import os

import numpy as np
import pytest

import iqp_cases as ic
import iqp_guard as ig
from global_racetrajectory_optimization_amd import engine
from global_racetrajectory_optimization_amd.trajectory_planning_helpers import iqp_handler as iq

OK, ITER_CAP = engine.STATUS_OK, engine.STATUS_ITER_CAP
TRACE = engine.IQP_TRACE


def _input(name):
    t = ic.track(ic.CASES[name]["track"])
    return dict(reftrack=t["reftrack"], normvectors=t["normvectors"], scaling=t["scaling"])


def run_case(eng, name, max_rounds=ic.MAX_ROUNDS, **kw):
    c = ic.CASES[name]
    kw.setdefault("curv_error_allowed", c["allowed"])
    return eng.iqp_batch([_input(name)], c["kappa_bound"], c["w_veh"], c["stepsize"], iters_min=c["iters_min"], max_rounds=max_rounds, **kw)


def check_track(what, out, k, ref_rounds, g, worst, family, status=OK):
    """Track k of an iqp_batch result against the reference's rounds (the last of them is the state to come back): counts and status exactly,
    the end state and every recorded round of the trace within the guards g."""
    R, last = len(ref_rounds), ref_rounds[-1]
    assert out["status"][k] == status and out["rounds"][k] == R and out["n"][k] == last["n"], \
        "%s: status %d rounds %d n %d, reference %d / %d / %d" % (what, out["status"][k], out["rounds"][k], out["n"][k], status, R, last["n"])
    dev = ig.round_dev(dict(alpha=out["alpha"][k], reftrack=out["reftrack"][k], normvec=out["normvectors"][k], curv_error_max=out["curv_err"][k]), last)
    tr = out["curv_trace"][k]
    dev[3] = max(dev[3], max(abs(tr[j] - ref_rounds[j]["curv_error_max"]) for j in range(min(R, TRACE))))
    print("%s: " % what + ", ".join("%s %.2e (guard %.0e)" % (q, d, g[q]) for q, d in zip(ig.Q, dev)))
    for q, d in zip(ig.Q, dev):
        worst.add("%s %s" % (family, q), d, g[q])
    for q, d in zip(ig.Q, dev):
        assert d < g[q], "%s: %s is %.3e from the reference, guard %.3e" % (what, q, d, g[q])
    assert not np.any(tr[min(R, TRACE):]), "%s: the trace holds rounds that did not run" % what
    # the returned ring plus alpha along the returned normals is the last pass's own raceline
    race = out["reftrack"][k][:, :2] + out["alpha"][k][:, None] * out["normvectors"][k]
    assert ig.dmax(race, last["reftrack"][:, :2] + last["alpha"][:, None] * last["normvec"]) < g["ring"] + g["alpha"] + 4.0 * g["normals"], what


def same_track(a, ka, b, kb, state=True):
    """Track ka of one result and kb of another: the same bits (state=False: status, rounds and waypoint count only -- a track that never had a
    solved pass has no alpha to speak of)."""
    if not (a["status"][ka] == b["status"][kb] and a["rounds"][ka] == b["rounds"][kb] and a["n"][ka] == b["n"][kb]):
        return False
    if not state:
        return True
    return all(np.array_equal(np.ascontiguousarray(a[q][ka]).view(np.uint64), np.ascontiguousarray(b[q][kb]).view(np.uint64))
               for q in ("alpha", "reftrack", "normvectors")) and a["curv_err"][ka].tobytes() == b["curv_err"][kb].tobytes() \
        and a["curv_trace"][ka].tobytes() == b["curv_trace"][kb].tobytes()


def check_case(eng, name, worst, family=None, **kw):
    out = run_case(eng, name, **kw)
    ref = ic.reference(name)
    assert len(ref) == ic.CASES[name]["rounds"]
    check_track(name + (" %r" % kw if kw else ""), out, 0, ref, ig.guards(name), worst, family or name.split("/")[0])
    assert out["stats"]["rounds"] == len(ref) and out["stats"]["qp_solves"] == len(ref)
    return out


def check_warm_and_cold(eng, name, worst):
    """Passes 2+ from the working set the glue mapped onto the new ring (the default) and from the interior point (warm_start = -1): both on the
    reference, the same round counts."""
    warm = check_case(eng, name, worst)
    cold = check_case(eng, name, worst, warm_start=-1)
    assert warm["rounds"][0] == cold["rounds"][0] and warm["n"][0] == cold["n"][0]


# ---- the round cap -------------------------------------------------------------------------------------------------------------------------------
def check_round_cap(eng, worst):
    """include/mcq.h: a track still iterating at max_rounds comes back with MCQ_ITER_CAP, rounds = max_rounds, the ring and normals of pass
    max_rounds and that pass's alpha AS THE QP RETURNED IT -- undamped also where max_rounds < iters_min (the damping belongs to the step into
    the next ring, which is not taken).  At and above the rounds the track needs the cap is not felt: the uncapped run's bits."""
    name, R = ic.CAP_CASE, ic.CAP_ROUNDS
    ref, g, c = ic.reference(name), ig.guards(name), ic.CASES[name]
    assert len(ref) == R and any(m < c["iters_min"] for m in ic.CAP_BELOW) and (R - 1) in ic.CAP_BELOW
    free = run_case(eng, name)
    check_track(name, free, 0, ref, g, worst, "cap")
    for m in ic.CAP_BELOW:
        out = run_case(eng, name, max_rounds=m)
        check_track("%s max_rounds=%d" % (name, m), out, 0, ref[:m], g, worst, "cap", status=ITER_CAP)
        assert out["stats"]["rounds"] == m and out["stats"]["qp_solves"] == m
        if m < c["iters_min"]:          # (what a damped alpha_out would be is far outside the guard: the case decides between the two readings)
            assert ig.dmax(ref[m - 1]["alpha"] * (m / c["iters_min"]), ref[m - 1]["alpha"]) > 1e3 * g["alpha"]
    for m in ic.CAP_FREE:
        assert same_track(run_case(eng, name, max_rounds=m), 0, free, 0), "max_rounds = %d changes a run of %d rounds" % (m, R)
    t = _input(name)
    for resident in (True, False):
        with pytest.raises(RuntimeError, match="iqp_handler: no convergence within %d rounds" % (R - 1)):
            iq.iqp_handler_batch([t], c["kappa_bound"], c["w_veh"], c["stepsize"], c["iters_min"], c["allowed"], engine=eng, max_rounds=R - 1,
                                 device_resident=resident)


def check_boundary_is_inclusive(eng, worst):
    """iqp_handler ends a track on curv_error_max <= allowed.  The reference's own value cannot serve as `allowed` here -- the engine's curvature
    error differs from it in its last bits -- so the engine is given ITS OWN round-3 value: it has to end in round 3, on the reference's
    round-3 state (that of ladder/3/3: the same track and damping)."""
    free = run_case(eng, ic.CAP_CASE)
    e3 = float(free["curv_trace"][0][2])
    assert free["rounds"][0] == ic.CAP_ROUNDS and e3 > ic.CASES[ic.CAP_CASE]["allowed"]
    out = run_case(eng, ic.CAP_CASE, curv_error_allowed=e3)
    check_track("allowed == the engine's own round-3 error", out, 0, ic.reference("ladder/3/3"), ig.guards("ladder/3/3"), worst, "cap")
    out = run_case(eng, ic.CAP_CASE, curv_error_allowed=float(np.nextafter(e3, 0.0)))
    assert out["rounds"][0] > 3


# ---- batches -------------------------------------------------------------------------------------------------------------------------------------
def _batch_call(eng, entries, **kw):
    return eng.iqp_batch([ic.batch_track(kind, trk) for kind, trk in entries], ic.KAPPA, ic.W_VEH, ic.BATCH_STEP, iters_min=ic.BATCH_ITERS_MIN,
                         curv_error_allowed=ic.BATCH_ALLOWED, max_rounds=ic.MAX_ROUNDS, nmax=ic.BATCH_NMAX, **kw)


def _has_state(kind):
    return kind in ("ok", "overflow")           # (the overflowing track keeps its first pass: a solved one)


def check_batch_against_reference(what, entries, out, worst, family):
    for k, (kind, trk) in enumerate(entries):
        if kind == "ok":
            check_track("%s[%d] %s" % (what, k, trk), out, k, ic.reference("batch/" + trk), ig.guards("batch/" + trk), worst, family)
        else:
            assert (out["status"][k], out["rounds"][k]) == ic.FAILS[kind], "%s[%d] %s: status %d, rounds %d" % (what, k, kind, out["status"][k], out["rounds"][k])
    ran = [int(out["rounds"][k]) for k, (kind, _) in enumerate(entries) if kind != "empty"]
    assert out["stats"]["qp_solves"] == sum(ran) and out["stats"]["rounds"] == max(ran), (out["stats"], ran)


def check_same_batch(what, entries, a, b, order=None):
    order = range(len(entries)) if order is None else order
    for k, j in enumerate(order):
        assert same_track(a, k, b, j, _has_state(entries[k][0])), "%s: track %d (%s %s) has other bits" % (what, k, *entries[k])


def check_mixed_batch(eng, worst):
    """Tracks that end in rounds 3, 4 and 5 (both ring buffers hold end states: the download that goes track by track) next to one narrower than
    the vehicle, an empty one, one with a non-finite row and one whose re-sampled ring outgrows nmax.  Returns the result (the routes compare
    with it)."""
    E = ic.MIXED
    assert 10 <= len(E) <= ic.MAX_BATCH
    out = _batch_call(eng, E)
    check_batch_against_reference("mixed", E, out, worst, "mixed")
    ends = {int(out["rounds"][k]) for k, (kind, _) in enumerate(E) if kind == "ok"}
    assert ends == {3, 4, 5}
    rev = _batch_call(eng, E[::-1])
    check_same_batch("mixed, reversed", E, out, rev, range(len(E) - 1, -1, -1))
    for k in range(len(E)):
        one = _batch_call(eng, [E[k]])
        assert same_track(out, k, one, 0, _has_state(E[k][0])), "mixed: track %d (%s %s) has other bits in a call of its own" % (k, *E[k])
    return out


def check_same_round_batch(eng, worst):
    """Every track ends in round 3: one ring buffer holds every end state, which goes out in two copies."""
    E = ic.SAME_ROUND
    out = _batch_call(eng, E)
    check_batch_against_reference("same_round", E, out, worst, "same_round")
    assert set(out["rounds"]) == {3}
    for k in range(len(E)):
        assert same_track(out, k, _batch_call(eng, [E[k]]), 0)


def _resident_call(eng, entries):
    """The batch through Engine.iqp_device on buffers of the test's own -- two ring sets padded to [batch][BATCH_NMAX][*], buf, rounds, trace --
    as an iqp_batch result: ring and normals of a track are the first n rows of set buf[k].  Also buf, and n_io as it came back."""
    tracks = [ic.batch_track(kind, trk) for kind, trk in entries]
    bsz, nmax = len(tracks), ic.BATCH_NMAX
    ns = np.array([t["reftrack"].shape[0] for t in tracks], dtype=np.int32)
    ref, nv, sc = np.zeros((bsz, nmax, 4)), np.zeros((bsz, nmax, 2)), np.ones((bsz, nmax))
    for k, t in enumerate(tracks):
        ref[k, :ns[k]], nv[k, :ns[k]] = t["reftrack"], t["normvectors"]
        if t["scaling"] is not None:
            sc[k, :ns[k]] = t["scaling"]
    with eng.scope() as dev:
        d_n, d_sc = dev.up(ns), dev.up(sc)
        d_sets = ((dev.up(ref), dev.up(nv)), (dev.out((bsz, nmax, 4)), dev.out((bsz, nmax, 2))))
        d_alpha, d_curv, d_status = dev.out((bsz, nmax)), dev.out(bsz), dev.out(bsz, np.int32)
        d_buf, d_rounds, d_trace = dev.out(bsz, np.int32), dev.out(bsz, np.int32), dev.out((bsz, TRACE))
        stats = eng.iqp_device(bsz, nmax, d_n, d_sets[0][0], d_sets[0][1], d_sets[1][0], d_sets[1][1], d_sc, ic.KAPPA, ic.W_VEH, ic.BATCH_STEP,
                               ic.BATCH_ITERS_MIN, ic.BATCH_ALLOWED, ic.MAX_ROUNDS, d_alpha, d_buf, d_curv, d_status, d_rounds, d_trace)
        n, buf, alpha = dev.get(d_n), dev.get(d_buf), dev.get(d_alpha)
        sets = [(dev.get(d_r), dev.get(d_v)) for d_r, d_v in d_sets]
        out = dict(n=n, buf=buf, curv_err=dev.get(d_curv), status=dev.get(d_status), rounds=dev.get(d_rounds), curv_trace=dev.get(d_trace), stats=stats)
    assert set(buf) <= {0, 1} and np.all((n >= 0) & (n <= nmax))
    out.update(alpha=[alpha[k, :n[k]] for k in range(bsz)], reftrack=[sets[buf[k]][0][k, :n[k]] for k in range(bsz)],
               normvectors=[sets[buf[k]][1][k, :n[k]] for k in range(bsz)])
    return out


def check_resident_entry(eng):
    """mcq_iqp_device on a caller's own buffers (everywhere else it runs inside mcq_iqp_batch, over the handle's): per track the bits of
    mcq_iqp_batch for the same entries -- status, rounds and n exactly (n is n_io as it came back), alpha, the ring and normals of set buf[k],
    curvature error and trace bit for bit (same_track's rule for tracks without state) -- and buf the set the track's last round read
    (mcq_iqp_batch hands no buf back; its rounds say which set that is).  Fused and round by round."""
    for what, E in (("same_round", ic.SAME_ROUND), ("mixed", ic.MIXED)):
        base = _batch_call(eng, E)
        for fused in ("1", "0"):
            with _env("MCQ_IQP_FUSED", fused):
                res = _resident_call(eng, E)
            check_same_batch("resident %s, MCQ_IQP_FUSED=%s" % (what, fused), E, res, base)
            assert np.array_equal(res["buf"], (base["rounds"] - 1) & 1), (what, fused, res["buf"], base["rounds"])
            assert res["stats"]["rounds"] == base["stats"]["rounds"] and res["stats"]["qp_solves"] == base["stats"]["qp_solves"]


def check_buffer_growth(eng_factory):
    """One handle through IQP calls of growing and shrinking batches with a regrowth of staging set 0 in between (a solve_batch of more
    problems than any call before it): every IQP result is bitwise that of a fresh handle that runs only that call, and the two mixed
    batches are bitwise each other's."""
    E = ic.MIXED
    probs = [dict(reftrack=t["reftrack"], normvec=t["normvectors"], scaling=t["scaling"], kappa_bound=ic.KAPPA, w_veh=ic.W_VEH)
             for t in (ic.batch_track(kind, trk) for kind, trk in ic.SAME_ROUND * 4)]
    assert len(probs) == 16 > len(E)
    used = eng_factory()
    try:
        cap1 = run_case(used, ic.CAP_CASE)
        mixed1 = _batch_call(used, E)
        assert np.all(used.solve_batch(probs)[2] == OK)
        mixed2 = _batch_call(used, E)
        cap2 = run_case(used, ic.CAP_CASE)
    finally:
        used.close()
    fresh = eng_factory()
    try:
        cap = run_case(fresh, ic.CAP_CASE)
    finally:
        fresh.close()
    fresh = eng_factory()
    try:
        mixed = _batch_call(fresh, E)
    finally:
        fresh.close()
    assert cap["rounds"][0] == ic.CAP_ROUNDS and {int(mixed["rounds"][k]) for k, (kind, _) in enumerate(E) if kind == "ok"} == {3, 4, 5}
    assert same_track(cap1, 0, cap, 0), "the first IQP call of a handle is not a fresh handle's"
    assert same_track(cap2, 0, cap, 0), "an IQP call after larger batches and a regrowth of the staging is not a fresh handle's"
    check_same_batch("mixed after a smaller IQP call", E, mixed1, mixed)
    check_same_batch("mixed after a regrowth of the staging", E, mixed2, mixed)
    check_same_batch("mixed, before and after the regrowth", E, mixed1, mixed2)


@contextlib.contextmanager
def _env(key, value):
    old = os.environ.get(key)
    os.environ[key] = value
    try:
        yield
    finally:
        if old is None:
            del os.environ[key]
        else:
            os.environ[key] = old


def check_routes(eng, base, worst):
    """The mixed batch through the other routes of the same call: the same bits.  With the callback: the (round, curv, live) sequence of the
    reference."""
    E = ic.MIXED
    with _env("MCQ_IQP_FUSED", "1"):
        check_same_batch("MCQ_IQP_FUSED=1", E, base, _batch_call(eng, E))
    with _env("MCQ_IQP_FUSED", "0"):
        check_same_batch("MCQ_IQP_FUSED=0", E, base, _batch_call(eng, E))
    timed = _batch_call(eng, E, timed=True)
    check_same_batch("timed", E, base, timed)
    assert len(timed["stats"]["solver_ms"]) == base["stats"]["rounds"] and timed["stats"]["qp_solves"] == base["stats"]["qp_solves"]
    seen = []
    eng.set_iqp_round_callback(lambda rnd, curv, live: seen.append((rnd, curv, live)))
    try:
        cb = _batch_call(eng, E)
    finally:
        eng.set_iqp_round_callback(None)
    check_same_batch("round callback", E, base, cb)
    assert [s[0] for s in seen] == list(range(1, base["stats"]["rounds"] + 1))
    for k, (kind, trk) in enumerate(E):
        R = int(base["rounds"][k])
        live = [int(s[2][k]) for s in seen]
        assert live == [1] * R + [0] * (len(seen) - R), "callback: live of track %d (%s) is %s, it ran %d rounds" % (k, kind, live, R)
        if kind == "ok":
            ref, g = ic.reference("batch/" + trk), ig.guards("batch/" + trk)
            for j in range(R):
                d = abs(float(seen[j][1][k]) - ref[j]["curv_error_max"])
                worst.add("callback curv", d, g["curv"])
                assert d < g["curv"], (k, j, d)
    nmax = ic.BATCH_NMAX
    bufs = dict(alpha=np.full((len(E), nmax), np.nan), reftrack=np.full((len(E), nmax, 4), np.nan), normvectors=np.full((len(E), nmax, 2), np.nan))
    ob = _batch_call(eng, E, out=bufs)
    check_same_batch("out= buffers", E, base, ob)
    assert all(np.shares_memory(ob[q][k], bufs[q]) for q in bufs for k in range(len(E)) if ob["n"][k] > 0)
    # the host-glue driver: the upstream chain written out, one launch per round -- a third route, within the guards of the reference
    healthy = [(k, trk) for k, (kind, trk) in enumerate(E) if kind == "ok"]
    st = {}
    res = iq.iqp_handler_batch([ic.batch_track("ok", trk) for _, trk in healthy], ic.KAPPA, ic.W_VEH, ic.BATCH_STEP, ic.BATCH_ITERS_MIN, ic.BATCH_ALLOWED,
                               engine=eng, max_rounds=ic.MAX_ROUNDS, stats=st, device_resident=False)
    assert st["rounds"] == max(base["rounds"][k] for k, _ in healthy) and st["qp_solves"] == sum(base["rounds"][k] for k, _ in healthy)
    for (k, trk), (al, ref_o, nv_o) in zip(healthy, res):
        last, g = ic.reference("batch/" + trk)[-1], ig.guards("batch/" + trk)
        assert al.shape == last["alpha"].shape, trk
        dev = ig.round_dev(dict(alpha=al, reftrack=ref_o, normvec=nv_o, curv_error_max=last["curv_error_max"]), last)
        for q, d in zip(ig.Q[:3], dev[:3]):
            worst.add("host_glue %s" % q, d, g[q])
            assert d < g[q], "host-glue driver, %s: %s is %.3e from the reference" % (trk, q, d)


# ---- the trace beyond its length -------------------------------------------------------------------------------------------------------------------
def check_long_trace(eng, worst):
    name = "trace/t12"
    R = ic.CASES[name]["rounds"]
    assert R > TRACE
    seen = []
    eng.set_iqp_round_callback(lambda rnd, curv, live: seen.append((rnd, float(curv[0]), int(live[0]))))
    try:
        cb = run_case(eng, name)
    finally:
        eng.set_iqp_round_callback(None)
    out = check_case(eng, name, worst)          # rounds_out, rounds 1 .. 16 of the trace, the end state of round R
    assert out["rounds"][0] == R and same_track(out, 0, cb, 0)
    ref, g = ic.reference(name), ig.guards(name)
    assert [s[0] for s in seen] == list(range(1, R + 1)) and all(s[2] == 1 for s in seen)
    assert max(abs(s[1] - r["curv_error_max"]) for s, r in zip(seen, ref)) < g["curv"]


# ---- handle history --------------------------------------------------------------------------------------------------------------------------------
def _same_solve(a, b):
    return all(np.array_equal(x.view(np.uint64), y.view(np.uint64)) for x, y in zip(a[0], b[0])) and a[1].tobytes() == b[1].tobytes() \
        and np.array_equal(a[2], b[2])


def check_handle_history(eng_factory):
    """(i) After an IQP call the working sets its last glue left belong to nobody: a plain solve_batch with warm_start = 1 on the same handle is
    that of a fresh handle.  (ii) An IQP call refused with MCQ_E_ARG leaves nothing behind: the next valid call is that of a fresh handle."""
    t = _input(ic.CAP_CASE)
    c = ic.CASES[ic.CAP_CASE]
    probs = [dict(reftrack=t["reftrack"], normvec=t["normvectors"], scaling=t["scaling"], kappa_bound=c["kappa_bound"], w_veh=c["w_veh"])]
    bad = (dict(iters_min=0), dict(max_rounds=0), dict(stepsize_interp=0.0))
    used = eng_factory()
    try:
        run_case(used, ic.CAP_CASE)
        after_iqp = used.solve_batch(probs, warm_start=1)
        for kw in bad:
            args = dict(stepsize_interp=c["stepsize"], iters_min=c["iters_min"], max_rounds=ic.MAX_ROUNDS, nmax=ic.BATCH_NMAX)      # (nmax: the wrapper divides by the stepsize to size it)
            args.update(kw)
            with pytest.raises(engine.EngineError, match=r"\(-1\)"):
                used.iqp_batch([t], c["kappa_bound"], c["w_veh"], curv_error_allowed=c["allowed"], **args)
        after_refusals = run_case(used, ic.CAP_CASE)
    finally:
        used.close()
    fresh = eng_factory()
    try:
        alone = fresh.solve_batch(probs, warm_start=1)
    finally:
        fresh.close()
    assert alone[2][0] == OK and _same_solve(after_iqp, alone), "solve_batch(warm_start=1) after an IQP call is not a fresh handle's"
    fresh = eng_factory()
    try:
        assert same_track(after_refusals, 0, run_case(fresh, ic.CAP_CASE), 0), "the IQP call after three refused ones is not a fresh handle's"
    finally:
        fresh.close()
