"""The bodies of the mintime tests, run by tests/test_mintime_ref.py (CPU: what needs no engine), tests/test_emu_mintime.py (the SIMT interpreter,
unchanged sources) and tests/test_gpu_mintime.py (the MI355X).  Every comparison is against the longdouble restatement (tests/mintime_ref.py) under
the guards of tests/mintime_guard.py; bounds, layouts and statuses exactly.  The bodies return their worst deviation / guard ratios."""
import os

import numpy as np

import mintime_cases as mc
import mintime_guard as mg
import mintime_ref as mr
from global_racetrajectory_optimization_amd import engine, mintime

LD = np.longdouble


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _ratio(got, ref, guard):
    dev = float(np.max(np.abs(np.asarray(got).astype(LD) - ref))) if np.size(ref) else 0.0
    return dev / guard if np.isfinite(dev) else float("inf")


def _launch(name):
    option, names, nmax = mc.LAUNCHES[name]
    return mc.OPTIONS[option], names, [mc.cases()[n][1] for n in names], nmax


def check_layout(eng):
    """mcq_mintime_layout: sizes and offsets for every option set; the collocation constants against both constructions to rounding."""
    tau, C, D, B = mr.collocation(LD)
    t64, C64, D64, B64 = mr.collocation_poly1d()
    for oname, o in mc.OPTIONS.items():
        for N in (2, 3, 65):
            lay = eng.mintime_layout(N, **o)
            safe, en = int(bool(o.get("safe_traj"))), int(bool(o.get("limit_energy")))
            assert lay["nw"] == 5 + 24 * N and lay["ng"] == N * (27 + 2 * safe) + 4 * (N - 1) + 5 + en
            assert (lay["off_x"], lay["off_u"], lay["off_xc"], lay["stride_w"]) == (0, 5, 9, 24)
            assert lay["rows_first"] == 27 + 2 * safe and lay["rows_next"] == 31 + 2 * safe
            assert lay["row_periodic"] == mr.row_of(N, N, 0, safe) and lay["row_energy"] == (lay["row_periodic"] + 5 if en else -1)
            assert lay["row_periodic"] + 5 + en == lay["ng"]
            # k = 0 has no actuator rows, and the next group starts where the layout says
            assert mr.row_of(N, 0, 27, safe) == -1 and mr.row_of(N, 1, 0, safe) == lay["rows_first"]
            assert mr.row_of(N, 1, 27, safe) == lay["rows_first"] + lay["row_act"]
            assert (mr.row_of(N, 1, 31, safe) == lay["rows_first"] + lay["row_safe"]) if safe else lay["row_safe"] == -1
    lay = eng.mintime_layout(4)
    eps = np.finfo(np.float64).eps
    for got, ld, f64 in ((lay["tau"], tau, t64), (lay["C"], C, C64), (lay["D"], D, D64), (lay["B"], B, B64)):
        # the engine's: the longdouble construction rounded once; numpy.poly1d's float64 construction: to its monomial basis's rounding
        assert np.all(np.abs(got.astype(LD) - ld) <= eps * np.maximum(1.0, np.abs(ld).astype(np.float64)))
        assert np.all(np.abs(got - f64) <= mg.COLL_POLY1D_EPS * eps)


def check_bounds(eng, name):
    opts, names, probs, nmax = _launch(name)
    out = eng.mintime_bounds_batch(probs, nmax=nmax, **opts)
    for b, p in enumerate(probs):
        for key, ref in zip(("w0", "lbw", "ubw", "lbg", "ubg"), mr.bounds(p, opts)):
            assert _bits(out[key][b, :ref.shape[0]], ref), "%s of %s differs from the reference's construction" % (key, names[b])
            assert np.all(np.isnan(out[key][b, ref.shape[0]:]))


def check_launch(eng, name):
    """g, J, the sums and the f_sol outputs of a launch against the restatement; tails NaN; the Jacobian blocks, grad J and grad energy."""
    opts, names, probs, nmax = _launch(name)
    out = eng.mintime_eval_batch(probs, nmax=nmax, **opts)
    jac = eng.mintime_jac_batch(probs, nmax=nmax, **opts)
    worst = {}
    for b, (cname, p) in enumerate(zip(names, probs)):
        N = int(out["N"][b])
        ref = mg.restated(cname)
        assert out["status"][b] == 0, "%s: status %d" % (cname, out["status"][b])
        for q in mg.VALUES:
            got = out[q][b]
            if q in ("J", "lap_time", "energy"):
                live = np.asarray(got)
            elif q == "g":
                live, tail = got[:ref["g"].shape[0]], got[ref["g"].shape[0]:]
                assert np.all(np.isnan(tail)), "%s: rows beyond ng are not NaN" % cname
            elif q == "x_opt":
                live = got[:N + 1]
                assert np.all(np.isnan(got[N + 1:]))
            else:
                live = got[:N]
                assert np.all(np.isnan(got[N:])), "%s: %s beyond N is not NaN" % (cname, q)
            r = _ratio(live, ref[q], mg.guard(cname, q, ref[q]))
            worst[q] = max(worst.get(q, 0.0), r)
            assert r <= 1.0, "%s: %s is %.2f guards from the longdouble restatement" % (cname, q, r)
        rb = mg.restated_blocks(cname)
        blk = jac["blocks"][b]
        assert np.all(np.isnan(blk[N:])) and np.all(np.isnan(jac["grad_J"][b, 5 + 24 * N:])) and np.all(np.isnan(jac["grad_energy"][b, 5 + 24 * N:]))
        r = _ratio(blk[:N], rb["blocks"], mg.guard(cname, "blocks", rb["blocks"]))
        worst["blocks"] = max(worst.get("blocks", 0.0), r)
        assert r <= 1.0, "%s: the Jacobian blocks are %.2f guards from the dual-number restatement" % (cname, r)
        # inside an interval grad energy is d ec_k / d slot; grad J is d dt_k / d slot on the collocation states, the cyclic regularisation's
        # gradient on the controls (the wrap at N = 2, the neighbours across workgroup edges), and zero on the node states
        gE = jac["grad_energy"][b, :24 * N].reshape(N, 24)
        gJ = jac["grad_J"][b, :24 * N].reshape(N, 24)
        r = max(_ratio(gE, rb["dE"], mg.guard(cname, "dE", rb["dE"])), _ratio(gJ[:, 9:], rb["dJ"][:, 9:], mg.guard(cname, "dJ", rb["dJ"])))
        reg = mr.reg_gradient(p, p["w"])
        r = max(r, _ratio(gJ[:, 5:9], reg, mg.floor("grad_J", reg)))
        worst["grads"] = max(worst.get("grads", 0.0), r)
        assert r <= 1.0, "%s: grad energy / grad J are %.2f guards off" % (cname, r)
        assert not np.any(gJ[:, :5]) and not np.any(jac["grad_J"][b, 24 * N:24 * N + 5]) and not np.any(jac["grad_energy"][b, 24 * N:24 * N + 5])
    return worst


def check_dense(eng):
    """jacobian_coo against the dense longdouble Jacobian at N = 3 (every option on), and grad J / grad energy against the dense dual passes."""
    cname = "N3 all"
    option, p = mc.cases()[cname]
    opts = mc.OPTIONS[option]
    J, gJ, gE = mr.dense_derivatives(p, p["w"], opts)
    jac = eng.mintime_jac_batch([p], **opts)
    A = mintime.jacobian_coo(jac["blocks"][0], 3, safe_traj=True, grad_energy=jac["grad_energy"][0])
    assert A.shape == J.shape
    dense = A.toarray()
    tol = max(mg.FLOOR_EPS_DERIV * mg.EPS * mg.scale(J), 4 * mg.fixture()[cname + "/blocks"])
    # the sparsity agrees, except where an entry is zero analytically and of rounding size numerically: d (dn / ds) / dv of a collocation point --
    # sf * v does not depend on v, and the two terms cancel to 1e-18 in either arithmetic.  Only such rows (n of a collocation point against the
    # v of its own state) may differ in being zero, and only at rounding size
    for r, c in np.argwhere((dense != 0) != np.asarray(J != 0)):
        k, rr = (0, r) if r < 29 else (1 + (r - 29) // 33, (r - 29) % 33)
        assert rr < 15 and rr % 5 == 3 and c == 24 * k + 9 + 5 * (rr // 5), "an entry at (%d, %d) on one side only" % (r, c)
        assert abs(dense[r, c]) <= tol * 1e-3 and abs(float(J[r, c])) <= tol * 1e-3
    dev = float(np.max(np.abs(dense.astype(LD) - J)))
    assert dev <= tol, "jacobian_coo: %.3e from the dense Jacobian (guard %.3e)" % (dev, tol)
    for got, ref, what in ((jac["grad_J"][0], gJ, "grad J"), (jac["grad_energy"][0], gE, "grad energy")):
        t = max(mg.FLOOR_EPS_DERIV * mg.EPS * mg.scale(ref), 4 * mg.fixture()[cname + "/dJ"])
        d = float(np.max(np.abs(got.astype(LD) - ref)))
        assert d <= t, "%s: %.3e from the dense dual passes (guard %.3e)" % (what, d, t)
    return dict(dense=dev / tol)


def check_certificate(eng):
    """A constructed pair: with random lam_g, lam_x = -(grad J + J^T lam_g) + a residual set by hand on the regularisation's entries (the controls of
    interval 1); the entry must return that residual.  The complementarity and violation maxima against their definitions on the host."""
    cname = "N3 all"
    option, p = mc.cases()[cname]
    opts = mc.OPTIONS[option]
    rng = np.random.default_rng(5)
    J, gJ, _ = mr.dense_derivatives(p, p["w"], opts)
    ng, nw = J.shape
    lam_g = rng.uniform(-1, 1, ng)
    want = np.zeros(nw)
    want[24 + 5:24 + 9] = (3e-3, -2e-3, 1e-3, 0.0)
    lam_x = np.asarray(-(gJ + J.T @ lam_g.astype(LD)) + want, dtype=np.float64)
    out = eng.mintime_kkt_batch([p], [lam_g], [lam_x], **opts)
    scale = float(np.max(np.abs(J.T.astype(np.float64)) @ np.abs(lam_g)) + np.max(np.abs(lam_x)))
    tol = mg.FLOOR_EPS_DERIV * mg.EPS * max(1.0, scale) + 4 * mg.fixture()[cname + "/blocks"] * float(np.sum(np.abs(lam_g)))
    dev = float(np.max(np.abs(out["r"][0, :nw] - want)))
    assert dev <= tol, "the certificate's residual is %.3e from the one set by hand (tolerance %.3e)" % (dev, tol)
    assert abs(out["kkt"][0, 0] - 3e-3) <= tol
    ref = mg.restated(cname)
    w0, lbw, ubw, lbg, ubg = mr.bounds(p, opts)
    g, w = ref["g"].astype(np.float64), p["w"]
    viol = max(0.0, float(np.max(lbw - w)), float(np.max(w - ubw)), float(np.max(lbg - g)), float(np.max(g - ubg)))
    comp = 0.0
    for lam, x, lo, hi in ((lam_x, w, lbw, ubw), (lam_g, g, lbg, ubg)):
        up, dn = (lam > 0) & np.isfinite(hi), (lam < 0) & np.isfinite(lo)
        comp = max(comp, float(np.max(np.abs(lam[up] * (hi[up] - x[up])), initial=0.0)), float(np.max(np.abs(lam[dn] * (x[dn] - lo[dn])), initial=0.0)))
    gt = mg.guard(cname, "g", ref["g"])
    assert abs(out["kkt"][0, 1] - viol) <= gt and abs(out["kkt"][0, 2] - comp) <= 2 * gt * max(1.0, float(np.max(np.abs(lam_g))))
    cert = mintime.certificate(out, 0)
    assert set(cert) == {"stationarity", "violation", "complementarity", "status"} and cert["stationarity"] == out["kkt"][0, 0]
    return dict(residual=dev / tol)


def check_company(eng):
    """The same problems alone / reversed / beside others / in wider buffers: bitwise.  Pre-filled outputs are overwritten (check_launch)."""
    opts, names, probs, nmax = _launch("wave edges")
    lam = {id(p): (np.random.default_rng(11 + i).normal(size=mg.restated(names[i])["g"].shape[0]), np.random.default_rng(21 + i).normal(size=p["w"].shape[0]))
           for i, p in enumerate(probs)}
    big = mc.cases()["N256"][1]
    lam[id(big)] = (np.zeros(mg.restated("N256")["g"].shape[0]), np.zeros(big["w"].shape[0]))

    def both(ps, nm):
        kkt = eng.mintime_kkt_batch(ps, [lam[id(p)][0] for p in ps], [lam[id(p)][1] for p in ps], nmax=nm, **opts)
        e, j = eng.mintime_eval_batch(ps, nmax=nm, **opts), eng.mintime_jac_batch(ps, nmax=nm, **opts)
        j.update(r=kkt["r"], kkt=kkt["kkt"])
        return e, j
    base_e, base_j = both(probs, nmax)
    rev_e, rev_j = both(probs[::-1], nmax)
    wide_e, wide_j = both(probs + [big], None)
    B = len(probs)
    for b in range(B):
        N = int(base_e["N"][b])
        ng = mg.restated(names[b])["g"].shape[0]
        alone_e, alone_j = both([probs[b]], None)
        for oe, oj, i in ((rev_e, rev_j, B - 1 - b), (wide_e, wide_j, b), (alone_e, alone_j, 0)):
            for q in ("J", "lap_time", "energy"):
                assert _bits(base_e[q][b], oe[q][i]), (names[b], q)
            assert _bits(base_e["g"][b, :ng], oe["g"][i, :ng]) and _bits(base_e["tf_opt"][b, :N], oe["tf_opt"][i, :N])
            assert _bits(base_j["blocks"][b, :N], oj["blocks"][i, :N]) and _bits(base_j["grad_J"][b, :5 + 24 * N], oj["grad_J"][i, :5 + 24 * N])
            assert _bits(base_j["r"][b, :5 + 24 * N], oj["r"][i, :5 + 24 * N]) and _bits(base_j["kkt"][b], oj["kkt"][i]) and np.all(np.isfinite(oj["kkt"][i]))


def check_nan(eng):
    """A NaN and an inf w entry in one problem of a batch: NaN in that problem's affected rows and sums, the other problems' bits untouched."""
    opts, names, probs, nmax = _launch("small plain")
    base = eng.mintime_eval_batch(probs, **opts)
    base_j = eng.mintime_jac_batch(probs, **opts)
    for bad_value in (np.nan, np.inf):
        bad = dict(probs[2])
        w = bad["w"].copy()
        w[24 * 3 + 5 + 1] = bad_value          # f_drive of interval 3 (N = 7)
        bad["w"] = w
        out = eng.mintime_eval_batch([probs[0], probs[1], bad, probs[3]], **opts)
        jac = eng.mintime_jac_batch([probs[0], probs[1], bad, probs[3]], **opts)
        for q in base:
            for b in (0, 1, 3):
                assert _bits(base[q][b], out[q][b]), q
        for b in (0, 1, 3):
            assert _bits(base_j["blocks"][b], jac["blocks"][b])
        assert out["status"][2] == 4 and np.isnan(out["J"][2]) and np.isnan(out["lap_time"][2]) and np.isnan(out["energy"][2])
        r3 = mr.row_of(7, 3, 0, 0)
        assert np.all(np.isnan(out["g"][2, r3:r3 + 15])) and np.all(np.isnan(out["g"][2, r3 + 20:r3 + 27]))
        r4 = mr.row_of(7, 4, 27, 0)
        assert np.isnan(out["g"][2, r4 + 1])                      # the next interval's actuator row reads it as U_k-1
        r2 = mr.row_of(7, 2, 0, 0)
        assert _bits(out["g"][2, :r2 + 27], base["g"][2, :r2 + 27])       # intervals 0 .. 2 do not read it
        assert np.all(np.isnan(jac["blocks"][2, 3, :15, 5:9])) and _bits(jac["blocks"][2, :3], base_j["blocks"][2, :3])


def check_refusals(eng):
    """Every refusal alone: the layout's N < 2, the options, the sizes, NULL where required; the batch surface's N < 2 and N > nmax."""
    p = mc.cases()["N3"][1]
    for kw in (dict(N=1), dict(N=0), dict(N=3, friction=7), dict(N=3, friction="gauss", n_gauss=0), dict(N=3, friction="gauss", n_gauss=16)):
        try:
            eng.mintime_layout(**kw)
        except engine.EngineError as e:
            assert "(-1)" in str(e), str(e)
        else:
            raise AssertionError("mintime_layout took %r" % kw)
    for call in (lambda: eng.mintime_layout(3, pwr_behavior=True), lambda: eng.mintime_eval_batch([p], pwr_behavior=True)):
        try:
            call()
        except NotImplementedError:
            pass
        else:
            raise AssertionError("pwr_behavior was taken")
    o = engine.McqMintimeOpts(-1, 0, 0, 0, 1)
    d = engine.McqMintimeDims()
    import ctypes
    assert eng.lib.mcq_mintime_layout(3, ctypes.byref(o), ctypes.byref(d)) == -1            # the powertrain flag in C: MCQ_E_ARG
    one = dict(p)
    one.update(h=p["h"][:1], kappa_cl=p["kappa_cl"][:2], w_tr_right_cl=p["w_tr_right_cl"][:2], w_tr_left_cl=p["w_tr_left_cl"][:2], w=p["w"][:29])
    for probs, nmax in (([one], None), ([p], 2), ([p, one], 3)):           # N < 2; nmax + 1 intervals; one bad problem among good ones
        try:
            eng.mintime_eval_batch(probs, nmax=nmax)
        except ValueError:
            pass
        else:
            raise AssertionError("mintime_eval_batch took N outside 2 .. nmax")
    out = eng.mintime_eval_batch([p], nmax=3)                                # N == nmax
    assert out["status"][0] == 0
    with eng.scope() as dev:
        opts = eng.mintime_opts()
        z = dev.out(64)
        for data, what in ((eng.mintime_data(0, 3, None, z, z, z, z, z, z), "batch <= 0"), (eng.mintime_data(1, 1, None, z, z, z, z, z, z), "nmax < 2"),
                           (eng.mintime_data(1, 3, None, z, z, z, z, None, z), "pars NULL"), (eng.mintime_data(1, 3, None, z, z, z, z, z, None), "w NULL"),
                           (eng.mintime_data(70000, 3, None, z, z, z, z, z, z), "too many problems")):
            rc = eng.lib.mcq_mintime_eval_device(eng.h, ctypes.byref(data), ctypes.byref(opts), z, z, None, None, None, None, None, None, None, None, None, z)
            assert rc == (-3 if what == "too many problems" else -1), what
        lin = eng.mintime_opts(friction="linear")
        data = eng.mintime_data(1, 3, None, z, z, z, z, z, z)
        assert eng.lib.mcq_mintime_eval_device(eng.h, ctypes.byref(data), ctypes.byref(lin), z, z, None, None, None, None, None, None, None, None, None, z) == -1
        assert eng.lib.mcq_mintime_jac_device(eng.h, ctypes.byref(data), ctypes.byref(opts), None, z, None) == -1
        assert eng.lib.mcq_mintime_jac_device(eng.h, ctypes.byref(data), ctypes.byref(opts), z, None, None) == -1
        gau = eng.mintime_opts(friction="gauss", n_gauss=2)
        with_w = eng.mintime_data(1, 3, None, z, z, z, z, z, z, d_w_mue=z)            # the Gaussian model without center_dist
        assert eng.lib.mcq_mintime_eval_device(eng.h, ctypes.byref(with_w), ctypes.byref(gau), z, z, None, None, None, None, None, None, None, None, None, z) == -1
        for miss in range(5):                                                       # every output of the bounds entry alone
            args = [None if i == miss else z for i in range(5)]
            assert eng.lib.mcq_mintime_bounds_device(eng.h, ctypes.byref(data), ctypes.byref(opts), *args) == -1
        en = eng.mintime_opts(limit_energy=True)
        for miss in range(12):                                                      # every array of the certificate alone (grad_energy: with its row)
            args = [None if i == miss else z for i in range(12)]
            o = en if miss == 3 else opts
            assert eng.lib.mcq_mintime_kkt_device(eng.h, ctypes.byref(data), ctypes.byref(o), *args) == -1, miss
        args = [None if i == 3 else z for i in range(12)]
        assert eng.lib.mcq_mintime_kkt_device(eng.h, None, ctypes.byref(opts), *args) == -1 and eng.lib.mcq_mintime_bounds_device(None, ctypes.byref(data), ctypes.byref(opts), z, z, z, z, z) == -1
    # a device-side N outside 2 .. nmax: status MCQ_BAD_INPUT and NaN outputs, the neighbour untouched
    with eng.scope() as dev:
        opts = eng.mintime_opts()
        data, Ns, nmax = eng._mintime_up(dev, [p, p], opts, 4, True)
        data.n_list = dev.up(np.array([3, 5], dtype=np.int32))
        nw, ng = eng.mintime_sizes(4, opts)
        d_g, d_J, d_st = dev.up(np.full((2, ng), 9.0)), dev.up(np.full(2, 9.0)), dev.up(np.full(2, 9, dtype=np.int32))
        eng.mintime_eval_device(data, opts, d_g, d_J, d_st)
        g, J, st = dev.get(d_g), dev.get(d_J), dev.get(d_st)
        assert list(st) == [0, 4] and np.isfinite(J[0]) and np.isnan(J[1]) and np.all(np.isnan(g[1])) and np.all(np.isfinite(g[0, :mr.row_of(3, 3, 0, 0) + 5]))


def check_export(eng, tmp):
    """mintime.export_mintime_solution on arrays the engine produced reproduces the recorded files of the reference's own writer byte for byte."""
    z = np.load(os.path.join(mc.GOLDEN, "mintime", "export_n8.npz"))
    option, p = mc.cases()["N8"]
    out = eng.mintime_eval_batch([p])
    sol = mintime.extract_solution(out, 0)
    s = np.append(0.0, np.cumsum(p["h"]))
    lam_x, lam_g = z["lam_x0"], z["lam_g0"]
    mintime.export_mintime_solution(tmp, {"pwr_params_mintime": {"pwr_behavior": False}}, s, sol["t_opt"], sol["x_opt"], sol["u_opt"], sol["tf_opt"],
                                    sol["ax_opt"], sol["ay_opt"], sol["atot_opt"], p["w"], lam_x, lam_g)
    for f in mintime.EXPORT_FILES:
        got = open(os.path.join(tmp, f), "rb").read()
        assert got == z[f].tobytes(), "%s differs from the reference writer's bytes" % f


def check_prefilled(eng):
    """Outputs that hold other numbers before the launch come back as from zeroed buffers, bit for bit: through the device entries."""
    opts_kw, names, probs, nmax = _launch("all")
    base_e, base_j = eng.mintime_eval_batch(probs, nmax=nmax, **opts_kw), eng.mintime_jac_batch(probs, nmax=nmax, **opts_kw)
    base_b = eng.mintime_bounds_batch(probs, nmax=nmax, **opts_kw)
    opts = eng.mintime_opts(**opts_kw)
    with eng.scope() as dev:
        data, Ns, nmax = eng._mintime_up(dev, probs, opts, nmax, True)
        B, (nw, ng) = len(Ns), eng.mintime_sizes(nmax, opts)
        fill = lambda shape: dev.up(np.full(shape, 123.0))
        e = dict(g=fill((B, ng)), J=fill(B), lap_time=fill(B), energy=fill(B), x_opt=fill((B, nmax + 1, 5)), u_opt=fill((B, nmax, 4)),
                 tf_opt=fill((B, nmax, 12)), dt_opt=fill((B, nmax)), ax_opt=fill((B, nmax)), ay_opt=fill((B, nmax)), ec_opt=fill((B, nmax)))
        d_st = dev.up(np.full(B, 77, dtype=np.int32))
        eng.mintime_eval_device(data, opts, e["g"], e["J"], d_st, e["lap_time"], e["energy"], e["x_opt"], e["u_opt"], e["tf_opt"], e["dt_opt"],
                                e["ax_opt"], e["ay_opt"], e["ec_opt"])
        j = dict(blocks=fill((B, nmax, 33, 33)), grad_J=fill((B, nw)), grad_energy=fill((B, nw)))
        eng.mintime_jac_device(data, opts, j["blocks"], j["grad_J"], j["grad_energy"])
        bd = dict(w0=fill((B, nw)), lbw=fill((B, nw)), ubw=fill((B, nw)), lbg=fill((B, ng)), ubg=fill((B, ng)))
        eng.mintime_bounds_device(data, opts, bd["w0"], bd["lbw"], bd["ubw"], bd["lbg"], bd["ubg"])
        for base, got in ((base_e, e), (base_j, j), (base_b, bd)):
            for k, ptr in got.items():
                assert _bits(base[k], dev.get(ptr)), "%s keeps what the buffer held" % k
        assert not np.any(dev.get(d_st))


def _restated_live(prob, opts):
    """(longdouble restatement, {quantity: guard}) of a problem that is not in the case table: the spread measured here, from the float64
    restatement's two orders -- nothing of the code under test."""
    ld = mr.nlp(prob, prob["w"], opts)
    f64 = [mr.nlp(prob, prob["w"], opts, np.float64, o) for o in (0, 1)]
    guards = {}
    for q in mg.VALUES:
        spread = max(float(np.max(np.abs(np.asarray(f[q]).astype(LD) - ld[q]))) for f in f64)
        guards[q] = max(mg.floor(q, ld[q]), 4 * spread)
    return ld, guards


def undecided(prob, opts):
    """the denominators of a problem that come within a factor 4 of zero in the longdouble restatement (tests/test_mintime_ref.py states the rule)"""
    den = []
    mr.nlp(prob, prob["w"], opts, LD, 0, den)
    return sorted({what for what, values, minimum in den if not np.all(np.abs(values) >= minimum)})


def check_flow(eng):
    """The physically meant w on rounded_rectangle: prep -> solve -> raceline -> velocity profile on the engine give v, n = -alpha, xi from the
    headings, omega_z, delta, the forces (mintime_cases.flow_problem); the case is DECIDED; evaluation and Jacobian against the restatement."""
    z = np.load(os.path.join(mc.GOLDEN, "rounded_rectangle.npz"))
    prob, flow = mc.flow_problem(eng, z["reftrack"], mc.PARS, float(z["kappa_bound"]), float(z["w_veh"]))
    assert float(np.max(np.abs(flow["alpha"] - z["alpha"]))) < 1e-6 and undecided(prob, {}) == []
    ld, guards = _restated_live(prob, {})
    out = eng.mintime_eval_batch([prob, mc.cases()["N64"][1]], nmax=105)
    N = prob["h"].shape[0]
    assert out["status"][0] == 0
    worst = {}
    for q in mg.VALUES:
        got = out[q][0] if q in ("J", "lap_time", "energy", "g") else out[q][0][:N + (q == "x_opt")]
        worst[q] = _ratio(got, ld[q], guards[q])
        assert worst[q] <= 1.0, "%s is %.2f guards from the restatement" % (q, worst[q])
    rb = mr.blocks(prob, prob["w"], {})[0]
    spread = max(float(np.max(np.abs(mr.blocks(prob, prob["w"], {}, np.float64, o)[0].astype(LD) - rb))) for o in (0, 1))
    jac = eng.mintime_jac_batch([prob])
    worst["blocks"] = _ratio(jac["blocks"][0], rb, max(mg.floor("blocks", rb), 4 * spread))
    assert worst["blocks"] <= 1.0
    # the flow's profile and the NLP's quadrature time the same lap (a guess on a coarse line: a few percent)
    worst["lap_time_nlp"], worst["lap_time_profile"] = float(out["lap_time"][0]), flow["lap_time_profile"]
    return worst


def check_end_to_end(eng, golden):
    """Berlin, the whole chain on the engine: prep -> solve -> raceline -> velocity profile (mintime_cases.flow_problem builds w from them) ->
    friction grid -> Gaussian fit, RESIDENT -> mcq_mintime_eval_device reads the fit without a copy.  Asserted: agreement with the restatement, and
    finiteness.  Reported, not asserted: how close the guess comes to feasibility, and how many kinds of
    denominator it leaves undecided."""
    import fric_guard as fg
    g = fg.recorded("berlin_2018")
    ref, ng = golden["reftrack"], 5
    n = ref.shape[0]
    pars = dict(mc.PARS, width_opt=float(g["width"]), wheelbase_front=float(g["wb_f"]), wheelbase_rear=float(g["wb_r"]))
    prob, flow = mc.flow_problem(eng, ref, pars, float(golden["kappa_bound"]), float(golden["w_veh"]), stepsize=2.0)
    nv = flow["normvec"]
    opts = dict(friction="gauss", n_gauss=ng)
    with eng.friction_map(g["cells"], g["mue"]) as fmap, eng.scope() as dev:
        jmax = eng.friction_jmax([ref], [pars["width_opt"]], float(g["dn"]))
        rows = n + 1
        d_no, d_cnt, d_mu = dev.out((1, rows, jmax)), dev.out((1, rows), np.int32), dev.out((1, 4, rows, jmax))
        d_st, d_wg, d_cd = dev.out(1, np.int32), dev.out((1, 4, rows, 2 * ng + 2)), dev.out((1, rows))
        eng.friction_grid_device(fmap, 1, n, None, dev.up(ref), dev.up(nv), pars["width_opt"], None, pars["wheelbase_front"], pars["wheelbase_rear"],
                                 float(g["dn"]), jmax, d_no, d_cnt, d_mu, None, None, d_st)
        eng.friction_gauss_device(1, n, jmax, d_no, d_cnt, d_mu, d_st, ng, None, d_wg, d_cd)
        out = eng.mintime_eval_batch([prob], resident=(d_wg, d_cd), **opts)
        prob["w_mue"], prob["center_dist"] = dev.get(d_wg)[0], dev.get(d_cd)[0]
    assert out["status"][0] == 0 and np.all(np.isfinite(out["g"][0])) and np.isfinite(out["J"][0])
    ld, guards = _restated_live(prob, opts)
    dev_g = float(np.max(np.abs(out["g"][0].astype(LD) - ld["g"])))
    assert dev_g <= guards["g"], "g on Berlin is %.3e from the restatement (guard %.3e)" % (dev_g, guards["g"])
    assert abs(float(out["lap_time"][0]) - float(ld["lap_time"])) <= guards["lap_time"]
    w0, lbw, ubw, lbg, ubg = mr.bounds(prob, opts)
    gg = out["g"][0]
    return dict(g=dev_g / guards["g"], lap_time=float(out["lap_time"][0]), lap_time_profile=flow["lap_time_profile"], undecided=len(undecided(prob, opts)),
                infeasibility=float(np.max(np.maximum(lbg - gg, gg - ubg))))
