"""The bodies of the Newton-step tests, run by tests/test_emu_mtstep.py (the SIMT interpreter, unchanged sources) and tests/test_gpu_mtstep.py (the
MI355X).  Every comparison is against tests/mtstep_ref.py's longdouble reference under the rules of tests/mtstep_guard.py; company, NaN isolation
and pre-filled outputs bit for bit.  The bodies return their worst deviation / guard ratios."""
import ctypes
import os

import numpy as np

import mintime_cases as mc
import mtstep_cases as sc
import mtstep_guard as sg
import mtstep_ref as sr
from global_racetrajectory_optimization_amd import engine, mintime

LD = np.longdouble
OK, BAD, SINGULAR = engine.STATUS_OK, engine.STATUS_BAD_INPUT, engine.STATUS_SINGULAR


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def run(eng, inps, refine=2, nmax=None, fill=None, n_list=None):
    """mcq_mintime_step_device on a list of inputs (mtstep_cases.inputs dicts: the same options and nvec for all), padded to nmax.  fill: what the
    output buffers hold before the launch.  Returns dict(sol [B, nvec, nw + ng of nmax], res, inertia, status, nw, ng) and own(b, t) -> [nw_b + ng_b]."""
    B = len(inps)
    safe, energy, nvec = inps[0]["safe"], inps[0]["energy"], inps[0]["rhs"].shape[0]
    assert all(i["safe"] == safe and i["energy"] == energy and i["rhs"].shape[0] == nvec for i in inps)
    nmax = max(i["N"] for i in inps) if nmax is None else nmax
    opts = eng.mintime_opts(safe_traj=bool(safe), limit_energy=bool(energy))
    nw, ng = eng.mintime_sizes(nmax, opts)
    hb, jb = np.full((B, nmax, 33, 33), 7.0), np.full((B, nmax, 33, 33), 7.0)       # (past a problem's own blocks: never read)
    ge, dw, dg, rhs = np.full((B, nw), 7.0), np.full((B, nw), 7.0), np.full((B, ng), 7.0), np.full((B, nvec, nw + ng), 7.0)
    for b, i in enumerate(inps):
        hb[b, :i["N"]], jb[b, :i["N"]] = i["hblocks"], i["blocks"]
        if energy:
            ge[b, :i["nw"]] = i["grad_energy"]
        dw[b, :i["nw"]], dg[b, :i["ng"]] = i["dw"], i["dg"]
        rhs[b, :, :i["nw"]], rhs[b, :, nw:nw + i["ng"]] = i["rhs"][:, :i["nw"]], i["rhs"][:, i["nw"]:]
    Ns = np.array([i["N"] for i in inps] if n_list is None else n_list, dtype=np.int32)
    with eng.scope() as dev:
        z = dev.out(64)
        data = eng.mintime_data(B, nmax, dev.up(Ns), None, None, z, z, z)
        if fill is None:
            d_sol, d_res, d_in, d_st = dev.out((B, nvec, nw + ng)), dev.out((B, nvec)), dev.out((B, 3), np.int32), dev.out(B, np.int32)
        else:
            d_sol, d_res = dev.up(np.full((B, nvec, nw + ng), float(fill))), dev.up(np.full((B, nvec), float(fill)))
            d_in, d_st = dev.up(np.full((B, 3), int(fill), dtype=np.int32)), dev.up(np.full(B, int(fill), dtype=np.int32))
        eng.mintime_step_device(data, opts, dev.up(hb), dev.up(jb), dev.up(ge) if energy else None, dev.up(dw), dev.up(dg), dev.up(rhs), nvec, refine,
                                d_sol, d_res, d_in, d_st)
        out = dict(sol=dev.get(d_sol), res=dev.get(d_res), inertia=dev.get(d_in), status=dev.get(d_st), nw=nw, ng=ng)
    out["own"] = lambda b, t: np.concatenate((out["sol"][b, t, :inps[b]["nw"]], out["sol"][b, t, nw:nw + inps[b]["ng"]]))
    out["tail"] = lambda b: np.concatenate((out["sol"][b, :, inps[b]["nw"]:nw], out["sol"][b, :, nw + inps[b]["ng"]:]), axis=1)
    return out


def held(key, out, b, refine=2, nvec=2):
    """items 1 - 4 of mtstep_guard for problem b of a launch; returns the ratios"""
    ref = sg.reference(key, nvec)
    inp = ref["inp"]
    assert out["status"][b] == OK, "%s: status %d" % (key, out["status"][b])
    assert np.all(np.isnan(out["tail"](b))), "%s: entries past the problem's own nw / ng are not NaN" % key
    worst = {}
    g = sg.guard(key, refine, nvec)
    for t in range(inp["rhs"].shape[0]):
        x = out["own"](b, t)
        assert np.all(np.isfinite(x)), "%s: the solution is not finite" % key
        fwd = float(np.max(np.abs(x.astype(LD) - ref["x"][t]))) / float(np.max(np.abs(ref["x"][t])))
        worst["forward"] = max(worst.get("forward", 0.0), fwd / g)
        print("%s rhs %d refine %d: forward %.3e (guard %.3e)" % (key, t, refine, fwd, g))
        assert fwd <= g, "%s, refine %d: the solution is %.3g guards from the reference" % (key, refine, fwd / g)
        if refine >= 1:
            ratio, rmax, bmax = sg.backward_ratio(ref, x, inp["rhs"][t])
            print("%s rhs %d refine %d: backward %.3g of its bound, res_out %.3e against %.3e" % (key, t, refine, ratio, out["res"][b, t], rmax))
            if refine >= 2:
                worst["backward"] = max(worst.get("backward", 0.0), ratio)
                assert ratio <= 1.0, "%s: a row's residual is %.3g times its bound" % (key, ratio)
            dres = abs(float(out["res"][b, t]) - rmax)
            worst["res"] = max(worst.get("res", 0.0), dres / bmax)
            assert dres <= bmax, "%s: res_out %.3e, the longdouble residual %.3e" % (key, out["res"][b, t], rmax)
    assert ref["decided"], "%s: the reference's inertia is not decided" % key
    assert tuple(out["inertia"][b]) == ref["inertia"], "%s: inertia %s, the reference's %s" % (key, tuple(out["inertia"][b]), ref["inertia"])
    return worst


def check_case(eng, key, refines=(2,)):
    """one key alone under each refine count"""
    worst = {}
    for r in refines:
        w = held(key, run(eng, [sc.inputs(key)], refine=r), 0, r)
        for k, v in w.items():
            worst["%s r%d" % (k, r)] = v
    return worst


def check_zero_blocks(eng):
    """hblocks = blocks = 0: K is diagonal apart from the periodicity rows and the energy row -- an entry no row touches is rhs / dw (and
    -rhs / dg for a multiplier) to one rounding: the layout of dw, dg and rhs."""
    inp = sc.inputs("zero")
    out = run(eng, [inp])
    held("zero", out, 0)
    nw, N = inp["nw"], inp["N"]
    ge = inp["grad_energy"]
    for t in range(inp["rhs"].shape[0]):
        x = out["own"](0, t)
        free = np.setdiff1d(np.arange(5, 24 * N), np.flatnonzero(ge))            # (not X_0, not X_N, not in the energy row)
        assert free.size > 0
        assert np.allclose(x[free], inp["rhs"][t, free] / inp["dw"][free], rtol=4 * sg.EPS, atol=0)
        rows = nw + np.arange(inp["ng"] - 6)
        assert np.allclose(x[rows], -inp["rhs"][t, rows] / inp["dg"][:inp["ng"] - 6], rtol=4 * sg.EPS, atol=0)


def check_nvec(eng):
    """nvec = 1, 2, 3, 4, 5 (a sweep carries four right-hand sides, a wave each): a right-hand side's solution does not depend on how many others
    the launch holds or on its place among them, bit for bit; the five together within item 1's bound."""
    inp2, inp5 = sc.inputs("N3/a"), sc.inputs("N3/a", 5)
    assert _bits(inp2["rhs"], inp5["rhs"][:2])
    two, five = run(eng, [inp2]), run(eng, [inp5])
    held("N3/a", two, 0)
    assert _bits(two["sol"][0], five["sol"][0, :2]) and _bits(two["res"][0], five["res"][0, :2]) and _bits(two["inertia"], five["inertia"])
    ref = sg.reference("N3/a")
    for t in range(5):
        assert sg.backward_ratio(ref, five["own"](0, t), inp5["rhs"][t])[0] <= 1.0
    for nvec in (1, 2, 3, 4):
        first = 5 - nvec
        out = run(eng, [dict(inp5, rhs=inp5["rhs"][first:first + nvec])])
        assert _bits(out["sol"][0], five["sol"][0, first:first + nvec]) and _bits(out["res"][0], five["res"][0, first:first + nvec])
        assert _bits(out["inertia"], five["inertia"])


def check_company(eng):
    """The same problems alone / reversed / beside others / under a wider nmax: bit for bit."""
    keys = ["N2/a", "N3/b", "N7/a", "N8/c"]
    inps = [sc.inputs(k) for k in keys]
    base = run(eng, inps)
    rev = run(eng, inps[::-1])
    wide = run(eng, inps + [sc.inputs("N63/a")], nmax=70)
    B = len(keys)
    for b, key in enumerate(keys):
        held(key, base, b)
        alone = run(eng, [inps[b]])
        for other, i in ((rev, B - 1 - b), (wide, b), (alone, 0)):
            for t in range(2):
                assert _bits(base["own"](b, t), other["own"](i, t)), key
            assert _bits(base["res"][b], other["res"][i]) and _bits(base["inertia"][b], other["inertia"][i]) and base["status"][b] == other["status"][i]
    held("N63/a", wide, B)


def check_prefilled_and_sizes(eng):
    """Outputs that hold other numbers before the launch come back as from zeroed buffers; N == nmax; a device-side N of nmax + 1 and of 1: that
    problem BAD_INPUT, NaN, inertia -1, its neighbour untouched."""
    inps = [sc.inputs("N3/a"), sc.inputs("N7/a")]
    base = run(eng, inps, nmax=7)
    pre = run(eng, inps, nmax=7, fill=123)
    for k in ("sol", "res", "inertia", "status"):
        assert _bits(base[k], pre[k]), "output %s keeps what the buffer held" % k
    held("N7/a", base, 1)
    for n_bad in (8, 1):
        out = run(eng, inps, nmax=7, n_list=[3, n_bad], fill=5)
        assert out["status"][1] == BAD and np.all(np.isnan(out["sol"][1])) and np.all(np.isnan(out["res"][1])) and np.all(out["inertia"][1] == -1)
        assert _bits(out["sol"][0], base["sol"][0]) and _bits(out["res"][0], base["res"][0]) and _bits(out["inertia"][0], base["inertia"][0])


def check_nonfinite(eng):
    """A NaN in dw, in dg, in one block entry (of H, of J), an inf in rhs, each inside one problem of a batch: that problem BAD_INPUT, its solution
    and residual NaN, its inertia -1; the other problems keep their bits.  The same values PAST the problem's own extent change nothing."""
    keys = ["N3/a", "N7/a", "N2/a"]
    inps = [sc.inputs(k) for k in keys]
    base = run(eng, inps, nmax=8)

    def spoil(field, idx, value):
        bad = dict(inps[1])
        a = np.array(bad[field], copy=True)
        a[idx] = value
        bad[field] = a
        return bad
    for field, idx, value in (("dw", 24 * 4 + 7, np.nan), ("dg", 40, np.nan), ("hblocks", (3, 12, 30), np.nan), ("blocks", (6, 31, 2), np.nan),
                              ("blocks", (0, 28, 29), np.inf), ("rhs", (1, 100), np.inf)):
        out = run(eng, [inps[0], spoil(field, idx, value), inps[2]], nmax=8, fill=9)
        assert out["status"][1] == BAD and np.all(np.isnan(out["sol"][1])) and np.all(np.isnan(out["res"][1])) and np.all(out["inertia"][1] == -1), field
        for b in (0, 2):
            assert _bits(out["sol"][b], base["sol"][b]) and _bits(out["res"][b], base["res"][b]) and _bits(out["inertia"][b], base["inertia"][b])
            assert out["status"][b] == OK


def check_singular(eng):
    """An exact zero pivot by construction -- the zero-blocks case with one dw entry 0 on a variable no row touches -- is MCQ_SINGULAR with finite
    neighbours; the inertia counts the pivots before it and the one zero."""
    inp = sc.inputs("zero")
    bad = dict(inp)
    dw = inp["dw"].copy()
    at = 24 * 2 + 12                  # a collocation state of interval 2: pivot 12 of front 2
    dw[at] = 0.0
    bad["dw"] = dw
    base = run(eng, [inp, inp])
    out = run(eng, [inp, bad, inp], fill=3)
    assert list(out["status"]) == [OK, SINGULAR, OK]
    assert np.all(np.isnan(out["sol"][1])) and np.all(np.isnan(out["res"][1])) and out["inertia"][1, 2] == 1 and np.all(out["inertia"][1, :2] >= 0)
    assert out["inertia"][1, 0] + out["inertia"][1, 1] < inp["nw"] + inp["ng"]
    for b in (0, 2):
        assert _bits(out["sol"][b], base["sol"][0]) and _bits(out["inertia"][b], base["inertia"][0])


def check_refusals(eng):
    """Every refusal of the two entries alone."""
    with eng.scope() as dev:
        opts, z = eng.mintime_opts(), dev.out(1 << 16)
        en = eng.mintime_opts(limit_energy=True)
        good = eng.mintime_data(1, 3, None, None, None, z, z, z)
        ref = ctypes.byref
        S = lambda data, o, *a: eng.lib.mcq_mintime_step_device(eng.h, data, o, *a)
        args = [z, z, None, z, z, z, 1, 2, z, z, z, z]
        assert S(ref(good), ref(opts), *args) == 0
        eng.sync()
        for i in (0, 1, 3, 4, 5, 8, 9, 10, 11):
            a = list(args)
            a[i] = None
            assert S(ref(good), ref(opts), *a) == -1, "argument %d NULL" % i
        assert S(ref(good), ref(en), *args) == -1                                   # grad_energy NULL with limit_energy
        for nvec, refine in ((0, 2), (-1, 2), (1, -1)):
            a = list(args)
            a[6], a[7] = nvec, refine
            assert S(ref(good), ref(opts), *a) == -1
        for data, want in ((eng.mintime_data(0, 3, None, None, None, z, z, z), -1), (eng.mintime_data(1, 1, None, None, None, z, z, z), -1),
                           (eng.mintime_data(1, 3, None, None, None, z, z, None), -1), (eng.mintime_data(70000, 3, None, None, None, z, z, z), -3)):
            assert S(ref(data), ref(opts), *args) == want
        bad = eng.mintime_opts()
        bad.friction = 7
        assert S(ref(good), ref(bad), *args) == -1 and S(None, ref(opts), *args) == -1 and S(ref(good), None, *args) == -1
        assert eng.lib.mcq_mintime_step_device(None, ref(good), ref(opts), *args) == -1
        out = ctypes.c_size_t(0)
        Bt = eng.lib.mcq_mintime_step_bytes
        assert Bt(3, ref(opts), 1, ref(out)) == 0 and out.value > 0
        assert Bt(1, ref(opts), 1, ref(out)) == -1 and Bt(3, None, 1, ref(out)) == -1 and Bt(3, ref(opts), 0, ref(out)) == -1
        assert Bt(3, ref(opts), 1, None) == -1 and Bt(3, ref(bad), 1, ref(out)) == -1


def check_bytes(eng_factory):
    """mcq_mintime_step_bytes against the workspace a fresh handle grew: batch x bytes per problem, exactly; a smaller launch afterwards grows nothing"""
    eng = eng_factory()
    try:
        assert eng.mintime_step_workspace() == 0
        inps = [sc.inputs("N3/a"), sc.inputs("N7/a")]
        run(eng, inps, nmax=9)
        want = 2 * eng.mintime_step_bytes(9, 2)
        per = (9 * 94 * 57 + 37 * 37 + 2 * sum(eng.mintime_sizes(9, eng.mintime_opts()))) * 8
        assert eng.mintime_step_workspace() == want == 2 * per, (eng.mintime_step_workspace(), want, 2 * per)
        run(eng, inps[:1])
        assert eng.mintime_step_workspace() == want
    finally:
        eng.close()


def check_flow(eng):
    """The chained call Engine.mintime_step_batch on the physically meant w of rounded_rectangle (mintime_cases.flow_problem): the reference K is
    built from the blocks the call returns, the diagonals from mcq_mintime_bounds_device's bounds and a barrier of 1e-2, items 1 - 3 asserted, the
    spread measured on the spot.  Returns the ratios and the change of the nonlinear equality residual after the full step (reported, not asserted)."""
    z = np.load(os.path.join(mc.GOLDEN, "rounded_rectangle.npz"))
    prob, _ = mc.flow_problem(eng, z["reftrack"], mc.PARS, float(z["kappa_bound"]), float(z["w_veh"]))
    N = prob["h"].shape[0]
    nw, ng, per = sr.sizes(N, 0, 0)
    rng = np.random.default_rng(78)
    lam, sig = rng.uniform(-1, 1, ng), 1.0
    bnd = eng.mintime_bounds_batch([prob])
    lbw, ubw, lbg, ubg = bnd["lbw"][0, :nw], bnd["ubw"][0, :nw], bnd["lbg"][0, :ng], bnd["ubg"][0, :ng]
    mu, w = 1e-2, prob["w"]
    gap = lambda lo, hi, v: np.maximum(np.minimum(np.where(np.isfinite(lo), np.abs(v - lo), np.inf), np.where(np.isfinite(hi), np.abs(hi - v), np.inf)), 1e-3)
    ev = eng.mintime_eval_batch([prob])
    g = ev["g"][0, :ng]
    dw = np.where(np.isfinite(gap(lbw, ubw, w)), mu / gap(lbw, ubw, w) ** 2, 0.0) + 1e-4
    dg = np.where(lbg == ubg, 1e-8, np.where(np.isfinite(gap(lbg, ubg, g)), gap(lbg, ubg, g) ** 2 / mu, 1e8))
    rhs = np.concatenate((np.zeros(nw), -np.where(lbg == ubg, g - lbg, 0.0)))[None]
    out = eng.mintime_step_batch([prob], [lam], [dw], [dg], [rhs], sigma=[sig], refine=2)
    assert out["status"][0] == OK
    inp = dict(N=N, safe=0, energy=0, hblocks=out["hblocks"][0], blocks=out["blocks"][0], grad_energy=None, dw=dw, dg=dg, rhs=rhs, nw=nw, ng=ng)
    trip = sc.triplets_of(inp)
    ch = sr.Chain(trip, N, 0, 0)
    x_ref, omega = sr.refine(ch, sr.Factor(ch, True), rhs[0].astype(LD))
    assert omega <= 4 * sr.EPS_LD
    x_w, x_lam = mintime.step_of(out)
    x = np.concatenate((x_w, x_lam))
    ref = dict(chain=ch, nnz=ch.nnz_rows())
    ratio, rmax, bmax = sg.backward_ratio(ref, x, rhs[0])
    assert ratio <= 1.0, "a row's residual is %.3g times its bound" % ratio
    assert abs(float(out["res"][0, 0]) - rmax) <= bmax
    spread = 0.0
    inert = []
    for rev in (False, True):
        c64 = sr.Chain(trip, N, 0, 0, reverse=rev, dtype=np.float64)
        x64, _ = sr.refine(c64, sr.Factor(c64, False), rhs[0], steps=2)
        spread = max(spread, float(np.max(np.abs(x64.astype(LD) - x_ref))))
        inert.append(sr.inertia_of(sr.Factor(ch if not rev else sr.Chain(trip, N, 0, 0, reverse=True), False).pivots))
    scale = float(np.max(np.abs(x_ref)))
    bt = np.asarray(sg.beta(ref, x_ref, rhs[0]), dtype=np.float64)
    kinv = np.abs(np.linalg.inv(np.asarray(sr.dense(trip, ch.n), dtype=np.float64))) if N <= 65 else None
    floor = 2.0 * float(np.max(kinv @ bt)) if kinv is not None else 0.0
    fwd = float(np.max(np.abs(x.astype(LD) - x_ref)))
    guard = max(floor, 4 * spread)
    assert fwd <= guard, "the step is %.3g guards from the reference" % (fwd / guard)
    assert inert[0] == inert[1] == tuple(out["inertia"][0])
    after = dict(prob, w=w + x_w)
    g1 = eng.mintime_eval_batch([after])["g"][0, :ng]
    eq = lbg == ubg
    return dict(forward=fwd / guard, backward=ratio, eq_before=float(np.max(np.abs(g[eq]))), eq_after=float(np.max(np.abs(g1[eq]))), scale=scale)
