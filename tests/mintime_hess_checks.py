"""The bodies of the Hessian tests, run by tests/test_emu_mintime_hess.py (the SIMT interpreter, unchanged sources) and tests/test_gpu_mintime_hess.py
(the MI355X).  Every comparison is against the longdouble restatement (tests/mintime_hess_ref.py) under the guards of tests/mintime_hess_guard.py;
symmetry, company, NaN isolation and pre-filled outputs bit for bit.  The bodies return their worst deviation / guard ratios."""
import ctypes
import os

import numpy as np

import mintime_cases as mc
import mintime_hess_cases as hc
import mintime_hess_guard as hg
import mintime_hess_ref as hr
import mintime_ref as mr
from global_racetrajectory_optimization_amd import mintime

LD = np.longdouble


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _ratio(got, ref, guard):
    dev = float(np.max(np.abs(np.asarray(got).astype(LD) - ref))) if np.size(ref) else 0.0
    return dev / guard if np.isfinite(dev) else float("inf")


def _launch(name):
    option, names, nmax = mc.LAUNCHES[name]
    lam = [hc.multipliers(n)[0] for n in names]
    sg = [hc.multipliers(n)[1] for n in names]
    return mc.OPTIONS[option], names, [mc.cases()[n][1] for n in names], lam, sg, nmax


def _vectors(seed, nvec, nw):
    return np.random.default_rng(9000 + seed).uniform(-1.0, 1.0, (nvec, nw))


def check_launch(eng, name, nvec=2):
    """The blocks of a launch against the restatement, their tails NaN, every block symmetric bit for bit; H v of nvec seeded vectors per problem
    against the restatement's product, its tail NaN."""
    opts, names, probs, lam, sg, nmax = _launch(name)
    vs = [_vectors(i, nvec, p["w"].shape[0]) for i, p in enumerate(probs)]
    out = eng.mintime_hessvec_batch(probs, lam, vs, sigma=sg, nmax=nmax, **opts)
    worst = {}
    for b, cname in enumerate(names):
        N, blk, y = int(out["N"][b]), out["hblocks"][b], out["y"][b]
        nw = 5 + 24 * N
        ref = hg.restated(cname)
        assert np.all(np.isnan(blk[N:])) and np.all(np.isnan(y[:, nw:])), "%s: blocks or entries past the problem's own N are not NaN" % cname
        assert _bits(blk[:N], blk[:N].transpose(0, 2, 1)), "%s: a block is not symmetric bit for bit" % cname
        g = hg.guard(cname, ref)
        r = _ratio(blk[:N], ref, g)
        worst["hblocks"] = max(worst.get("hblocks", 0.0), r)
        assert r <= 1.0, "%s: the Hessian blocks are %.3g guards from the restatement" % (cname, r)
        ry = _ratio(y[:, :nw], hr.hessvec(ref, N, vs[b]), hg.guard_y(g, ref, vs[b]))
        worst["y"] = max(worst.get("y", 0.0), ry)
        assert ry <= 1.0, "%s: H v is %.3g guards from the restatement's product" % (cname, ry)
    return worst


def check_localising(eng):
    """"N5 all" with the multipliers of ONE row kind at a time and sigma = 0, and the objective alone: one launch of the same problem under each
    setting.  With the objective alone the controls' part is the regularisation's constant cyclic stencil in closed form."""
    kinds = hc.KINDS + ("objective",)
    option, prob = mc.cases()[hc.LOCAL_CASE]
    opts, N = mc.OPTIONS[option], prob["h"].shape[0]
    sets = [hc.localising(k) for k in kinds]
    out = eng.mintime_hess_batch([prob] * len(kinds), [s[0] for s in sets], sigma=[s[1] for s in sets], **opts)
    worst = {}
    for b, kind in enumerate(kinds):
        key = "%s@%s" % (hc.LOCAL_CASE, kind)
        ref = hg.restated(key)
        blk = out["hblocks"][b]
        assert np.any(ref != 0) and _bits(blk, blk.transpose(0, 2, 1))
        worst[kind] = _ratio(blk, ref, hg.guard(key, ref))
        assert worst[kind] <= 1.0, "row kind %s: the blocks are %.3g guards from the restatement" % (kind, worst[kind])
    A = mintime.hessian_coo(out["hblocks"][len(kinds) - 1], N).toarray()
    ctrl = np.concatenate([24 * k + 5 + np.arange(4) for k in range(N)])
    sten = hr.reg_stencil(prob["pars"], N)
    dev = float(np.max(np.abs(A[np.ix_(ctrl, ctrl)].astype(LD) - sten)))
    assert dev <= 16 * hg.EPS * hg.scale(sten), "the controls' part under the objective alone is %.3e from the closed-form stencil" % dev
    return worst


def check_company(eng):
    """The same problems alone / reversed / beside others / under a wider nmax: blocks and H v bit for bit."""
    opts, names, probs, lam, sg, nmax = _launch("wave edges")
    big, blam, bsg = mc.cases()["N256"][1], hc.multipliers("N256")[0], hc.multipliers("N256")[1]
    vs = [_vectors(i, 2, p["w"].shape[0]) for i, p in enumerate(probs)]
    vbig = _vectors(7, 2, big["w"].shape[0])

    def run(idx, nm, extra=False):
        ps, ls, ss, vv = [probs[i] for i in idx], [lam[i] for i in idx], [sg[i] for i in idx], [vs[i] for i in idx]
        if extra:
            ps, ls, ss, vv = ps + [big], ls + [blam], ss + [bsg], vv + [vbig]
        return eng.mintime_hessvec_batch(ps, ls, vv, sigma=ss, nmax=nm, **opts)
    B = len(probs)
    base, rev, wide = run(range(B), nmax), run(range(B - 1, -1, -1), nmax), run(range(B), None, True)
    for b in range(B):
        N = int(base["N"][b])
        nw = 5 + 24 * N
        alone = run([b], None)
        assert np.all(np.isfinite(base["hblocks"][b, :N])) and np.all(np.isfinite(base["y"][b, :, :nw]))
        for other, i in ((rev, B - 1 - b), (wide, b), (alone, 0)):
            assert _bits(base["hblocks"][b, :N], other["hblocks"][i, :N]), names[b]
            assert _bits(base["y"][b, :, :nw], other["y"][i, :, :nw]), names[b]


def check_nan(eng):
    """A NaN and an inf in one problem's w: the blocks that hold the entry are NaN entirely, every other block and problem keeps its bits.  A NaN in
    ONE multiplier: exactly its interval's block.  A NaN multiplier on a periodicity row, and where a disabled energy row would lie: nothing changes."""
    opts, names, probs, lam, sg, nmax = _launch("small plain")
    base = eng.mintime_hess_batch(probs, lam, sigma=sg, nmax=9, **opts)["hblocks"]

    def others_same(got, b, blocks):
        for i in range(len(probs)):
            N = probs[i]["h"].shape[0]
            for k in range(N):
                if i == b and k in blocks:
                    assert np.all(np.isnan(got[i, k])), "block %d of the spoilt problem is not NaN entirely" % k
                else:
                    assert _bits(got[i, k], base[i, k]), "block %d of problem %d changed" % (k, i)
    for bad_value in (np.nan, np.inf):
        bad = dict(probs[2])
        w = bad["w"].copy()
        w[24 * 3 + 5 + 1] = bad_value          # f_drive of interval 3 (N = 7): a slot of block 3, and of block 4 as U_k-1
        bad["w"] = w
        got = eng.mintime_hess_batch([probs[0], probs[1], bad, probs[3]], lam, sigma=sg, nmax=9, **opts)["hblocks"]
        others_same(got, 2, (3, 4))
    bad = dict(probs[2])
    w = bad["w"].copy()
    w[24 * 6 + 5] = np.nan                     # delta of the LAST interval: block 6, and block 0's slots 29 .. 32
    bad["w"] = w
    others_same(eng.mintime_hess_batch([probs[0], probs[1], bad, probs[3]], lam, sigma=sg, nmax=9, **opts)["hblocks"], 2, (6, 0))
    for k, r in ((0, 3), (4, 22), (5, 28), (6, 17)):      # a collocation row, a Kamm row, an actuator row, a continuity row
        l2 = [x.copy() for x in lam]
        l2[2][mr.row_of(7, k, r, 0)] = np.nan
        others_same(eng.mintime_hess_batch(probs, l2, sigma=sg, nmax=9, **opts)["hblocks"], 2, (k,))
    l2 = [x.copy() for x in lam]
    l2[2][mr.row_of(7, 7, 0, 0) + 2] = np.nan                                   # a periodicity row
    l2[1] = np.append(l2[1], np.nan)                                            # where N = 3's energy row would lie, were it enabled
    l2[3] = np.append(l2[3], [0.0, np.nan])                                     # past N = 8's own rows
    others_same(eng.mintime_hess_batch(probs, l2, sigma=sg, nmax=9, **opts)["hblocks"], -1, ())
    s2 = list(sg)
    s2[1] = np.nan                                                              # sigma: every block of its problem
    others_same(eng.mintime_hess_batch(probs, lam, sigma=s2, nmax=9, **opts)["hblocks"], 1, (0, 1, 2))
    # the energy row's multiplier where the row is enabled: every block of its problem; the periodicity rows beside it: nothing
    o5, n5, p5, l5, s5, nm5 = _launch("all")
    base5 = eng.mintime_hess_batch(p5, l5, sigma=s5, nmax=nm5, **o5)["hblocks"]
    l6 = [x.copy() for x in l5]
    l6[0][-1] = np.nan
    l6[1][-3] = np.nan
    got = eng.mintime_hess_batch(p5, l6, sigma=s5, nmax=nm5, **o5)["hblocks"]
    assert np.all(np.isnan(got[0, :3])) and _bits(got[1:], base5[1:])


def check_prefilled_and_sizes(eng):
    """Outputs that hold other numbers before the launch come back as from zeroed buffers, through the device entries; sigma NULL is 1; N == nmax;
    a device-side N of nmax + 1 and of 1: that problem NaN throughout, its neighbour untouched."""
    opts_kw, names, probs, lam, sg, nmax = _launch("all")
    vs = [_vectors(i, 3, p["w"].shape[0]) for i, p in enumerate(probs)]
    base = eng.mintime_hessvec_batch(probs, lam, vs, sigma=sg, nmax=nmax, **opts_kw)
    opts = eng.mintime_opts(**opts_kw)
    with eng.scope() as dev:
        data, Ns, nmax = eng._mintime_up(dev, probs, opts, nmax, True)
        B, (nw, ng) = len(Ns), eng.mintime_sizes(nmax, opts)
        lg, s = eng._mintime_lam(Ns, lam, sg, ng)
        vv = np.zeros((B, 3, nw))
        for b in range(B):
            vv[b, :, :vs[b].shape[1]] = vs[b]
        d_h, d_y = dev.up(np.full((B, nmax, 33, 33), 123.0)), dev.up(np.full((B, 3, nw), 123.0))
        eng.mintime_hess_device(data, opts, dev.up(lg), dev.up(s), d_h)
        eng.mintime_hessvec_device(data, opts, d_h, dev.up(vv), 3, d_y)
        assert _bits(dev.get(d_h), base["hblocks"]) and _bits(dev.get(d_y), base["y"]), "an output keeps what the buffer held"
    one = eng.mintime_hess_batch(probs[:1], lam[:1], sigma=[1.0], **opts_kw)["hblocks"]          # N == nmax = 3
    assert _bits(one, eng.mintime_hess_batch(probs[:1], lam[:1], **opts_kw)["hblocks"]) and np.all(np.isfinite(one))
    try:
        eng.mintime_hess_batch(probs[:1], lam[:1], nmax=2, **opts_kw)
    except ValueError:
        pass
    else:
        raise AssertionError("mintime_hess_batch took nmax + 1 intervals")
    p = mc.cases()["N3"][1]
    l3 = hc.multipliers("N3")[0]
    opts = eng.mintime_opts()
    ok = eng.mintime_hessvec_batch([p, p], [l3, l3], [vs[0][:, :77]] * 2, nmax=4)
    for n_bad in (5, 1):
        with eng.scope() as dev:
            data, Ns, nmax = eng._mintime_up(dev, [p, p], opts, 4, True)
            data.n_list = dev.up(np.array([3, n_bad], dtype=np.int32))
            nw, ng = eng.mintime_sizes(4, opts)
            lg, _ = eng._mintime_lam(Ns, [l3, l3], None, ng)
            vv = np.zeros((2, 3, nw))
            vv[:, :, :77] = vs[0][:, :77]
            d_h, d_y = dev.up(np.full((2, 4, 33, 33), 9.0)), dev.up(np.full((2, 3, nw), 9.0))
            eng.mintime_hess_device(data, opts, dev.up(lg), None, d_h)
            eng.mintime_hessvec_device(data, opts, d_h, dev.up(vv), 3, d_y)
            h, y = dev.get(d_h), dev.get(d_y)
            assert np.all(np.isnan(h[1])) and np.all(np.isnan(y[1])) and _bits(h[0], ok["hblocks"][0]) and _bits(y[0], ok["y"][0])


def check_refusals(eng):
    """Every refusal of the two entries alone."""
    with eng.scope() as dev:
        opts, z = eng.mintime_opts(), dev.out(4096)
        good = eng.mintime_data(1, 3, None, z, z, z, z, z, z)
        H = lambda data, o, *a: eng.lib.mcq_mintime_hess_device(eng.h, data, o, *a)
        V = lambda data, o, *a: eng.lib.mcq_mintime_hessvec_device(eng.h, data, o, *a)
        ref = ctypes.byref
        for data, what in ((eng.mintime_data(0, 3, None, z, z, z, z, z, z), "batch <= 0"), (eng.mintime_data(1, 1, None, z, z, z, z, z, z), "nmax < 2"),
                           (eng.mintime_data(1, 3, None, z, z, z, z, None, z), "pars NULL"), (eng.mintime_data(70000, 3, None, z, z, z, z, z, z), "too many")):
            want = -3 if what == "too many" else -1
            assert H(ref(data), ref(opts), z, None, z) == want, what
            assert V(ref(data), ref(opts), z, z, 1, z) == want, what
        for data, what in ((eng.mintime_data(1, 3, None, z, z, z, z, z, None), "w NULL"), (eng.mintime_data(1, 3, None, None, z, z, z, z, z), "h NULL"),
                           (eng.mintime_data(1, 3, None, z, None, z, z, z, z), "kappa_cl NULL")):
            assert H(ref(data), ref(opts), z, None, z) == -1, what
        assert H(ref(good), ref(opts), None, None, z) == -1 and H(ref(good), ref(opts), z, None, None) == -1           # lam_g, hblocks
        assert H(None, ref(opts), z, None, z) == -1 and H(ref(good), None, z, None, z) == -1
        assert eng.lib.mcq_mintime_hess_device(None, ref(good), ref(opts), z, None, z) == -1
        lin, gau = eng.mintime_opts(friction="linear"), eng.mintime_opts(friction="gauss", n_gauss=2)
        assert H(ref(good), ref(lin), z, None, z) == -1                                                                  # the model's weights missing
        assert H(ref(eng.mintime_data(1, 3, None, z, z, z, z, z, z, d_w_mue=z)), ref(gau), z, None, z) == -1             # center_dist missing
        bad = eng.mintime_opts()
        bad.friction = 7
        assert H(ref(good), ref(bad), z, None, z) == -1 and V(ref(good), ref(bad), z, z, 1, z) == -1
        assert V(ref(good), ref(opts), None, z, 1, z) == -1 and V(ref(good), ref(opts), z, None, 1, z) == -1 and V(ref(good), ref(opts), z, z, 1, None) == -1
        assert V(ref(good), ref(opts), z, z, 0, z) == -1 and V(ref(good), ref(opts), z, z, -2, z) == -1                   # nvec <= 0
        assert V(None, ref(opts), z, z, 1, z) == -1 and eng.lib.mcq_mintime_hessvec_device(None, ref(good), ref(opts), z, z, 1, z) == -1


def check_unit_vectors(eng):
    """H v with unit vectors returns the assembled columns exactly (an entry has at most two contributions, and products with 0 and 1 are exact):
    every column at N = 2, where each block holds one of the regularisation's two equal terms; the columns of U_N-1 and X_N, of U_0 and X_0 and of
    an interval inside at N = 257."""
    for cname, pick in (("N2", None), ("N257", lambda N: np.concatenate((np.arange(9), 24 * 128 + np.arange(24), 24 * (N - 1) + np.arange(5, 29))))):
        option, p = mc.cases()[cname]
        N, (lam, sg) = p["h"].shape[0], hc.multipliers(cname)
        nw = 5 + 24 * N
        cols = np.arange(nw) if pick is None else pick(N)
        v = np.zeros((cols.shape[0], nw))
        v[np.arange(cols.shape[0]), cols] = 1.0
        out = eng.mintime_hessvec_batch([p], [lam], [v], sigma=[sg])
        A = mintime.lagrangian_hessian(out, 0).tocsc()
        want = A[:, cols].toarray().T
        assert np.array_equal(out["y"][0], want), "%s: H e_i is not column i of the assembled Hessian" % cname
        low = mintime.lagrangian_hessian(out, 0, "lower").toarray()
        full = A.toarray()
        assert np.array_equal(low, np.tril(full)) and np.array_equal(full, full.T)


def check_nvec(eng):
    """nvec = 1, 2, 5 at N = 2 and N = 257 against the restatement's product; the entries of U_N-1 and X_N among them."""
    worst = 0.0
    for cname in ("N2", "N257"):
        option, p = mc.cases()[cname]
        N, (lam, sg) = p["h"].shape[0], hc.multipliers(cname)
        ref = hg.restated(cname)
        g = hg.guard(cname, ref)
        for nvec in (1, 2, 5):
            v = _vectors(40 + nvec, nvec, 5 + 24 * N)
            y = eng.mintime_hessvec_batch([p], [lam], [v], sigma=[sg])["y"][0]
            assert y.shape == (nvec, 5 + 24 * N)
            want = hr.hessvec(ref, N, v)
            gy = hg.guard_y(g, ref, v)
            tail = np.r_[24 * (N - 1) + 5:24 * N + 5]
            assert np.all(want[:, tail[:4]] != 0) and np.all(want[:, tail[19:23]] != 0)         # U_N-1; v, beta, omega_z, n of X_N (xi enters no path row)
            r = max(_ratio(y, want, gy), _ratio(y[:, tail], want[:, tail], gy))
            worst = max(worst, r)
            assert r <= 1.0, "%s, nvec %d: H v is %.3g guards from the restatement" % (cname, nvec, r)
    return dict(y=worst)


def check_flow(eng):
    """The physically meant w on rounded_rectangle (mintime_cases.flow_problem, the engine's own minimum-curvature flow) with seeded multipliers,
    end to end: blocks and H v against the restatement, the spread measured on the spot from the float64 restatement's two orders."""
    z = np.load(os.path.join(mc.GOLDEN, "rounded_rectangle.npz"))
    prob, _ = mc.flow_problem(eng, z["reftrack"], mc.PARS, float(z["kappa_bound"]), float(z["w_veh"]))
    N = prob["h"].shape[0]
    rng = np.random.default_rng(77)
    lam, sg = rng.uniform(-1, 1, N * 27 + 4 * (N - 1) + 5), float(rng.uniform(0.5, 1.5))
    ref = hr.blocks(prob, prob["w"], {}, lam, sg)
    spread = max(float(np.max(np.abs(hr.blocks(prob, prob["w"], {}, lam, sg, np.float64, o).astype(LD) - ref))) for o in (0, 1))
    g = max(hg.floor(ref), 4 * spread)
    v = _vectors(5, 2, 5 + 24 * N)
    out = eng.mintime_hessvec_batch([prob], [lam], [v], sigma=[sg])
    worst = dict(hblocks=_ratio(out["hblocks"][0], ref, g), y=_ratio(out["y"][0], hr.hessvec(ref, N, v), hg.guard_y(g, ref, v)))
    assert worst["hblocks"] <= 1.0 and worst["y"] <= 1.0, worst
    assert _bits(out["hblocks"][0], out["hblocks"][0].transpose(0, 2, 1))
    return worst
