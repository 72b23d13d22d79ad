"""The traced reference NLP as the anchor (oracle/mintime_trace.py runs the reference's own text; tests/mintime_trace_cases.py the cases).

Three parts.  (1) Restated: what tests/mintime_ref.py and tests/mintime_hess_ref.py say about a problem, with the guards every comparison uses --
nothing of the code under test, nothing of the trace.  (2) live(): one case traced in float64 and longdouble, on duals and hyper-duals: the record
that scripts/make_golden_mintime_trace.py writes to tests/golden/mintime/trace.npz (needs the reference tree; tests/test_mintime_trace_ref.py holds
the restatement to it).  (3) The kernel bodies, run by tests/test_emu_mintime_trace.py (the SIMT interpreter) and tests/test_gpu_mintime_trace.py
(the MI355X): they read the FIXTURE only -- the problem, the traced results and the guards' recorded ingredients.

Guards.  Values: mintime_checks._restated_live's rule, max(512 eps x scale, 4 x spread of the float64 restatement's two orders) (mintime_guard).
J v: a row of the Jacobian times v is a sum of (entries in the row) products, each carrying the entry's error times |v|: (entries in the row) x
the entry guard x max |v|, the entry guard max(2048 eps x scale, 4 x spread) of mintime_guard's derivative rule; grad J . v and grad energy . v
alike over their own entries.  u^T H v: mintime_hess_guard's entry rule, max(8192 eps x scale, 4 x spread), summed over the entries the pair
touches: guard x sum over H_ij != 0 of |u_i| |v_j|.  The post-processed arrays: the guards of the values they are made of (t: N x dt's; atot:
ax's + ay's).  Bounds, row numbering and the step's blocks: exactly."""
import functools

import numpy as np

import mintime_checks as ck
import mintime_guard as mg
import mintime_hess_guard as hg
import mintime_hess_ref as hr
import mintime_ref as mr
import mintime_trace_cases as tc
from global_racetrajectory_optimization_amd import engine, mintime

LD = np.longdouble
EPS_LD = float(np.finfo(LD).eps)
BOUNDS = ("w0", "lbw", "ubw", "lbg", "ubg")
POST = ("s", "t", "x", "u", "tf", "ax", "ay", "atot", "alpha_opt", "v_opt")
PROBLEM = ("h", "s_opt", "kappa_cl", "w_tr_right_cl", "w_tr_left_cl", "w")
_bits = ck._bits


def coo_times(A, v):
    """A v in longdouble from a COO matrix's triplets"""
    out = np.zeros(A.shape[0], LD)
    np.add.at(out, A.row, A.data.astype(LD) * np.asarray(v, dtype=LD)[A.col])
    return out


def full_gradient(per_interval, N, controls=None):
    """[N, 24] interval entries (and [N, 4] on the controls) -> [5 + 24 N]"""
    out = np.zeros(5 + 24 * N, per_interval.dtype)
    out[:24 * N] = per_interval.reshape(-1)
    if controls is not None:
        for k in range(N):
            out[24 * k + 5:24 * k + 9] += controls[k]
    return out


class Restated:
    """The restatement's numbers and guards for one problem; every part computed once."""

    def __init__(self, prob, opts):
        self.prob, self.opts, self.N = prob, opts, int(np.asarray(prob["h"]).shape[0])
        self.safe, self.energy = bool(opts.get("safe_traj")), bool(opts.get("limit_energy"))
        self.nw = 5 + 24 * self.N
        self.row0, self.ng, self.slots = mintime.g_rows(self.N, self.safe, self.energy)

    @functools.cached_property
    def values(self):
        """(longdouble restatement, {quantity: guard})"""
        return ck._restated_live(self.prob, self.opts)

    @functools.cached_property
    def values_stored(self):
        """The restatement with C, D, B as the reference STORES them -- float64 arrays filled from its polynomial construction, whatever the
        precision of tau -- in longdouble, and the rule one precision up: max(512 eps_ld x scale, 4 x |order 1 - order 0|)."""
        tau, C, D, B = mr.collocation(LD)
        coll = (tau,) + tuple(c.astype(np.float64).astype(LD) for c in (C, D, B))
        construct = mr.collocation
        mr.collocation = lambda dtype=LD: coll          # mintime_ref.nlp asks its module for the constants: these, for the two calls below
        try:
            a, b = [mr.nlp(self.prob, self.prob["w"], self.opts, LD, o) for o in (0, 1)]
        finally:
            mr.collocation = construct
        return a, {q: max(mg.FLOOR_EPS * EPS_LD * mg.scale(a[q]), 4 * float(np.max(np.abs(np.asarray(b[q]) - a[q])))) for q in mg.VALUES}

    @functools.cached_property
    def jac(self):
        """dict(A: jacobian_coo of the restated blocks, gJ, gE [nw] longdouble, guard: {blocks, gJ, dE} entry guards, row_nnz [ng], gJ_nnz, gE_nnz)"""
        p, o, N = self.prob, self.opts, self.N
        ld = mr.blocks(p, p["w"], o)
        f64 = [mr.blocks(p, p["w"], o, np.float64, order) for order in (0, 1)]
        reg = mr.reg_gradient(p, p["w"])
        spread = [max(float(np.max(np.abs(f[i].astype(LD) - ld[i]))) for f in f64) for i in range(3)]
        guard = dict(blocks=max(mg.floor("blocks", ld[0]), 4 * spread[0]), dE=max(mg.floor("dE", ld[2]), 4 * spread[2]),
                     gJ=max(mg.floor("dJ", ld[1]), 4 * spread[1], mg.floor("grad_J", reg)))
        gJ, gE = full_gradient(ld[1], N, reg), full_gradient(ld[2], N)
        A = mintime.jacobian_coo(ld[0].astype(np.float64), N, self.safe, gE.astype(np.float64) if self.energy else None)
        return dict(A=A, gJ=gJ, gE=gE, guard=guard, row_nnz=np.bincount(A.row, minlength=self.ng), gJ_nnz=int(np.count_nonzero(gJ)),
                    gE_nnz=int(np.count_nonzero(gE)))

    @functools.lru_cache(maxsize=None)
    def hess(self, lam_key, sigma):
        """(dense hess L [nw, nw] in longdouble, entry guard) for the multipliers given as bytes and one sigma"""
        p, o = self.prob, self.opts
        lam = np.frombuffer(lam_key)
        ld = hr.blocks(p, p["w"], o, lam, sigma)
        spread = max(float(np.max(np.abs(hr.blocks(p, p["w"], o, lam, sigma, np.float64, order).astype(LD) - ld))) for order in (0, 1))
        return hr.dense(ld, self.N), max(hg.floor(ld), 4 * spread)

    def row_guards(self, jac_guard, row_nnz, gE_nnz, vmax):
        """the guard of every row of J v [ng]: the energy row's entries carry grad energy's guard"""
        g = np.asarray(row_nnz, dtype=np.float64) * jac_guard["blocks"] * vmax
        if self.energy:
            g[-1] = gE_nnz * jac_guard["dE"] * vmax
        return g

    def post(self, values, guards):
        """mintime.extract_solution of the restatement's outputs, in the names of the reference's export call, with the guards"""
        out = {q: np.asarray(values[q])[None] for q in mg.VALUES}
        out["N"] = np.array([self.N])
        sol = mintime.extract_solution(out, 0)
        ref = dict(s=np.asarray(self.prob["s_opt"]), t=sol["t_opt"], x=sol["x_opt"], u=sol["u_opt"], tf=sol["tf_opt"], ax=sol["ax_opt"], ay=sol["ay_opt"],
                   atot=sol["atot_opt"], alpha_opt=sol["alpha_opt"], v_opt=sol["v_opt"])
        g = dict(s=0.0, t=self.N * guards["dt_opt"], x=guards["x_opt"], u=guards["u_opt"], tf=guards["tf_opt"], ax=guards["ax_opt"], ay=guards["ay_opt"],
                 atot=guards["ax_opt"] + guards["ay_opt"], alpha_opt=guards["x_opt"], v_opt=guards["x_opt"])
        return ref, g


def pair_weights(H, U, V):
    """sum over H_ij != 0 of |u_i| |v_j| for every pair [P]"""
    nz = np.asarray(H != 0, dtype=np.float64)
    return np.array([float(np.abs(u) @ nz @ np.abs(v)) for u, v in zip(U, V)])


# ---- (2) the live trace -----------------------------------------------------------------------------------------------------------------
def _dual_ops():
    from oracle import casadi_trace as ct
    return ct.Ops(LD, mr.sin, mr.cos, mr.atan, mr.exp, mr.val)


def _hyper_ops():
    from oracle import casadi_trace as ct
    return ct.Ops(LD, hr.sin, hr.cos, hr.atan, hr.exp, hr.val)


@functools.lru_cache(maxsize=None)
def live(name):
    """One case traced: dict(f64, ld: the numbers of the two runs; bounds: of the float64 run's nlpsol call; fix: what the fixture holds for
    the case, float64 rounded once from longdouble; restated: the Restated of the case's problem; trace: the longdouble Trace)."""
    from oracle import mintime_trace as mt
    s = tc.setup(name)
    prob, opts = tc.problem(name)
    rs = Restated(prob, opts)
    runs = {t: mt.run(s, t) for t in (np.float64, LD)}
    num = {t: r.numbers(s["w"]) for t, r in runs.items()}
    tr, ld = runs[LD], num[LD]
    f64 = lambda a: np.asarray(a, dtype=np.float64)
    fix = {k: f64(prob[k]) for k in PROBLEM}
    fix["pars"] = np.array([prob["pars"][k] for k in engine.MINTIME_PARS])
    fix["opts"] = np.array([{None: -1, "linear": 0, "gauss": 1}[opts["friction"]], opts["n_gauss"], opts["safe_traj"], opts["limit_energy"]], dtype=np.int64)
    if prob["w_mue"] is not None:
        fix["w_mue"] = f64(prob["w_mue"])
    if prob["center_dist"] is not None:
        fix["center_dist"] = f64(prob["center_dist"])
    fix.update({q: f64(ld[q]) for q in mg.VALUES})
    out = dict(f64=num[np.float64], ld=ld, bounds=runs[np.float64].bounds(), fix=fix, restated=rs, trace=tr, export={t: r.export for t, r in runs.items()},
               returned={t: r.returned for t, r in runs.items()})
    if name in tc.VALUES_ONLY:
        return out
    fix.update(zip(BOUNDS, out["bounds"]))
    ex, ret = tr.export, tr.returned
    fix.update({"post_" + k: f64(ex[k]) for k in POST[:8]})
    fix.update(post_alpha_opt=f64(ret[0]), post_v_opt=f64(ret[1]))
    # first derivatives along three directions: one pass on duals each
    V = tc.directions(name)
    w = s["w"]
    Jv, gJv = np.zeros((3, tr.ng), LD), np.zeros(3, LD)
    for i, v in enumerate(V):
        J, g = tr.nlp(_dual_ops(), [mr.Dual(LD(a), LD(b)) for a, b in zip(w, v)])
        gJv[i], Jv[i] = mr.tan(J), [mr.tan(x) for x in g]
    fix.update(V=V, Jv=f64(Jv), gJv=f64(gJv))
    # second derivatives along pairs: one pass on hyper-duals each gives J's and every row's mixed part; L is linear in (sigma, lam)
    lam, sigmas = tc.multipliers(name)
    PU, PV, labels = tc.pairs(name, ld["ax_opt"])
    uHv = np.zeros((len(sigmas), len(PU)), LD)
    for i, (u, v) in enumerate(zip(PU, PV)):
        J, g = tr.nlp(_hyper_ops(), [hr.H2(LD(a), LD(b), LD(c)) for a, b, c in zip(w, u, v)])
        mixed = lambda x: x.ab if isinstance(x, hr.H2) else LD(0)
        rows = np.array([mixed(x) for x in g], dtype=LD)
        for j, sg in enumerate(sigmas):
            uHv[j, i] = LD(sg) * mixed(J) + np.sum(lam.astype(LD) * rows)
    fix.update(lam=lam, sigmas=np.array(sigmas), PU=PU, PV=PV, labels=np.array(labels), uHv=f64(uHv))
    # the guards' ingredients, from the restatement alone
    jac = rs.jac
    hs = [rs.hess(lam.tobytes(), sg) for sg in sigmas]
    fix.update(jac_guard=np.array([jac["guard"][k] for k in ("blocks", "gJ", "dE")]), row_nnz=jac["row_nnz"].astype(np.int64),
               grad_nnz=np.array([jac["gJ_nnz"], jac["gE_nnz"]], dtype=np.int64), hess_guard=np.array([h[1] for h in hs]),
               pair_weight=np.array([pair_weights(h[0], PU, PV) for h in hs]))
    return out


# ---- (3) the kernels against the fixture ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fixture():
    z = np.load(tc.FIXTURE)
    return {k: z[k] for k in z.files}


def recorded(name):
    """{key: array} of one case of the fixture"""
    pre = name + "/"
    return {k[len(pre):]: v for k, v in fixture().items() if k.startswith(pre)}


@functools.lru_cache(maxsize=None)
def fixture_problem(name):
    """(problem, option keywords, Restated) of a case, from the fixture alone.  Cached: shared, not to be changed."""
    r = recorded(name)
    prob = {k: r[k] for k in PROBLEM}
    prob.update(pars=dict(zip(engine.MINTIME_PARS, (float(x) for x in r["pars"]))), w_mue=r.get("w_mue"), center_dist=r.get("center_dist"))
    fr, ng, safe, energy = (int(x) for x in r["opts"])
    opts = dict(friction={-1: None, 0: "linear", 1: "gauss"}[fr], n_gauss=ng, safe_traj=bool(safe), limit_energy=bool(energy))
    return prob, opts, Restated(prob, opts)


def run_launch(eng, lname):
    """One launch of each entry for the cases of one option set, ragged under a wider nmax: bounds, evaluation, Jacobian, Hessian (once per sigma)
    and the Newton step (at the first sigma; its diagonals make K quasi-definite enough to factor -- only its blocks are compared)."""
    names, nmax = tc.LAUNCHES[lname]
    probs = [fixture_problem(n)[0] for n in names]
    opts = fixture_problem(names[0])[1]
    assert all(fixture_problem(n)[1] == opts for n in names)
    recs = [recorded(n) for n in names]
    lam, sigmas = [r["lam"] for r in recs], recs[0]["sigmas"]
    out = dict(names=names, bounds=eng.mintime_bounds_batch(probs, nmax=nmax, **opts), ev=eng.mintime_eval_batch(probs, nmax=nmax, **opts),
               jac=eng.mintime_jac_batch(probs, nmax=nmax, **opts),
               hess=[eng.mintime_hess_batch(probs, lam, sigma=[float(sg)] * len(probs), nmax=nmax, **opts) for sg in sigmas])
    rng = np.random.default_rng(818100 + sorted(tc.LAUNCHES).index(lname))
    dw = [np.full(p["w"].shape[0], 1e3) for p in probs]
    dg = [np.full(l.shape[0], 1e-6) for l in lam]
    rhs = [rng.uniform(-1, 1, (1, p["w"].shape[0] + l.shape[0])) for p, l in zip(probs, lam)]
    out["step"] = eng.mintime_step_batch(probs, lam, dw, dg, rhs, sigma=[float(sigmas[0])] * len(probs), nmax=nmax, **opts)
    return out


def check_case(out, name):
    """Problem `name` of a launch's results against the fixture.  Returns {quantity: worst deviation / guard}."""
    b = out["names"].index(name)
    rec = recorded(name)
    prob, opts, rs = fixture_problem(name)
    N, nw, ng = rs.N, rs.nw, rs.ng
    worst = {}

    def hold(what, got, ref, guard):
        dev = np.abs(np.asarray(got).astype(LD) - np.asarray(ref).astype(LD))
        assert np.all(np.isfinite(np.asarray(got, dtype=np.float64))), "%s: %s is not finite" % (name, what)
        r = float(np.max(dev / guard)) if dev.size else 0.0
        print("%s: %-12s %.3e of its guard" % (name, what, r))
        worst[what] = max(worst.get(what, 0.0), r)
        assert r <= 1.0, "%s: %s is %.3g guards from the traced reference" % (name, what, r)
    # bounds, exactly; NaN past the problem's own sizes
    for key in BOUNDS:
        got = out["bounds"][key][b]
        n = rec[key].shape[0]
        assert n == (nw if key in BOUNDS[:3] else ng)
        assert _bits(got[:n], rec[key]), "%s: %s differs from the bounds the reference handed to its solver" % (name, key)
        assert np.all(np.isnan(got[n:]))
    # values
    ev = out["ev"]
    assert ev["status"][b] == 0 and int(ev["N"][b]) == N
    guards = rs.values[1]
    cut = dict(g=ng, x_opt=N + 1)
    for q in mg.VALUES:
        got = ev[q][b]
        if q not in ("J", "lap_time", "energy"):
            n = cut.get(q, N)
            assert np.all(np.isnan(got[n:])), "%s: %s past the problem's own size is not NaN" % (name, q)
            got = got[:n]
        hold(q, got, rec[q], guards[q])
    # the post-processed arrays, through mintime.extract_solution
    sol = mintime.extract_solution(ev, b)
    _, pg = rs.post(rec, guards)
    for k, key in (("t", "t_opt"), ("x", "x_opt"), ("u", "u_opt"), ("tf", "tf_opt"), ("ax", "ax_opt"), ("ay", "ay_opt"), ("atot", "atot_opt"),
                   ("alpha_opt", "alpha_opt"), ("v_opt", "v_opt")):
        hold("post " + k, sol[key], rec["post_" + k], pg[k])
    assert _bits(np.asarray(prob["s_opt"]), rec["post_s"])
    # J v, grad J . v, grad energy . v from the kernel's blocks
    jac = out["jac"]
    jg = dict(zip(("blocks", "gJ", "dE"), rec["jac_guard"]))
    A = mintime.jacobian_coo(jac["blocks"][b], N, rs.safe, jac["grad_energy"][b] if rs.energy else None)
    assert A.shape == (ng, nw)
    for i, v in enumerate(rec["V"]):
        vmax = float(np.max(np.abs(v)))
        hold("J v", coo_times(A, v), rec["Jv"][i], rs.row_guards(jg, rec["row_nnz"], int(rec["grad_nnz"][1]), vmax))
        hold("grad J . v", np.sum(jac["grad_J"][b, :nw].astype(LD) * v), rec["gJv"][i], int(rec["grad_nnz"][0]) * jg["gJ"] * vmax)
    # u^T H v from the kernel's Hessian blocks
    for j, hs in enumerate(out["hess"]):
        H = mintime.hessian_coo(hs["hblocks"][b], N).tocoo()
        for i, (u, v) in enumerate(zip(rec["PU"], rec["PV"])):
            got = np.sum(np.asarray(u, dtype=LD) * coo_times(H, v))
            hold("u H v", got, rec["uHv"][j, i], rec["hess_guard"][j] * rec["pair_weight"][j, i])
    # the step's blocks are the separate launches' blocks
    st = out["step"]
    assert st["status"][b] in (engine.STATUS_OK, engine.STATUS_SINGULAR)
    assert _bits(st["blocks"][b, :N], jac["blocks"][b, :N]), "%s: the step's Jacobian blocks differ from the Jacobian launch's" % name
    assert _bits(st["hblocks"][b, :N], out["hess"][0]["hblocks"][b, :N]), "%s: the step's Hessian blocks differ from the Hessian launch's" % name
    assert _bits(st["grad_energy"][b, :nw], jac["grad_energy"][b, :nw])
    return worst


def check_values_only(eng, name):
    """The N = 65 evaluation against the fixture (beside the N = 8 case of the same options, under a wider nmax)."""
    other = "N8 all"
    probs = [fixture_problem(n)[0] for n in (name, other)]
    prob, opts, rs = fixture_problem(name)
    ev = eng.mintime_eval_batch(probs, nmax=rs.N + 2, **opts)
    rec, guards = recorded(name), rs.values[1]
    assert ev["status"][0] == 0
    worst = {}
    for q in mg.VALUES:
        got = ev[q][0]
        if q not in ("J", "lap_time", "energy"):
            n = dict(g=rs.ng, x_opt=rs.N + 1).get(q, rs.N)
            assert np.all(np.isnan(got[n:]))
            got = got[:n]
        worst[q] = ck._ratio(got, rec[q].astype(LD), guards[q])
        print("%s: %-12s %.3e of its guard" % (name, q, worst[q]))
        assert worst[q] <= 1.0, "%s: %s is %.3g guards from the traced reference" % (name, q, worst[q])
    return worst
