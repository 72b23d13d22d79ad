"""A plain numpy restatement of what the mcq_mintime_* entries compute (include/mcq.h "the minimum-time optimal-control problem"): the reference's
NLP [REF opt_mintime_traj/src/opt_mintime.py:143-861] as functions of a decision vector w -- g, J, the f_sol outputs, the bounds -- written from
the maths, interval by interval with numpy arrays over the intervals, in longdouble (the reference of every comparison) and in float64 in TWO
operation orders (order 0: sums from left to right as the reference writes them; order 1: from right to left), whose distance from longdouble is the
measured spread of tests/mintime_guard.py.  The derivatives are forward-mode dual numbers in longdouble (Dual below), seeded either per column slot
of the interval blocks (33 passes, every interval at once) or per entry of w (nw passes: the dense Jacobian of small cases).  Nothing here shares
structure with csrc/mcq_mintime.inc: no lanes, no blocks' owners, no tree sums (sums run in index order)."""
import numpy as np

LD = np.longdouble
XS = (50.0, 0.5, 1.0, 5.0, 1.0)
US = (0.5, 7500.0, 20000.0, 5000.0)
PARS = ("mass", "dragcoeff", "g", "v_max",
        "wheelbase_front", "wheelbase_rear", "track_width_front", "track_width_rear", "cog_z", "I_z", "liftcoeff_front", "liftcoeff_rear",
        "k_brake_front", "k_drive_front", "k_roll", "t_delta", "t_drive", "t_brake", "power_max", "f_drive_max", "f_brake_max", "delta_max",
        "c_roll", "f_z0", "B_front", "C_front", "eps_front", "E_front", "B_rear", "C_rear", "eps_rear", "E_rear",
        "width_opt", "mue", "penalty_F", "penalty_delta", "energy_limit", "ax_pos_safe", "ax_neg_safe", "ay_safe")


class Dual:
    """value + one tangent, arrays of one dtype"""
    __array_priority__ = 100
    __array_ufunc__ = None

    def __init__(self, v, d=None):
        self.v = np.asarray(v)
        self.d = np.zeros_like(self.v) if d is None else np.asarray(d)

    @staticmethod
    def lift(x):
        return x if isinstance(x, Dual) else Dual(x)

    def __add__(self, o):
        o = Dual.lift(o)
        return Dual(self.v + o.v, self.d + o.d)
    __radd__ = __add__

    def __sub__(self, o):
        o = Dual.lift(o)
        return Dual(self.v - o.v, self.d - o.d)

    def __rsub__(self, o):
        return Dual.lift(o) - self

    def __mul__(self, o):
        o = Dual.lift(o)
        return Dual(self.v * o.v, self.d * o.v + self.v * o.d)
    __rmul__ = __mul__

    def __truediv__(self, o):
        o = Dual.lift(o)
        return Dual(self.v / o.v, (self.d * o.v - self.v * o.d) / (o.v * o.v))

    def __rtruediv__(self, o):
        return Dual.lift(o) / self

    def __neg__(self):
        return Dual(-self.v, -self.d)


def val(x):
    return x.v if isinstance(x, Dual) else x


def tan(x):
    return x.d if isinstance(x, Dual) else np.zeros_like(x)


def _f(fn, dfn):
    def g(x):
        if isinstance(x, Dual):
            return Dual(fn(x.v), dfn(x.v) * x.d)
        return fn(x)
    return g


sin = _f(np.sin, np.cos)
cos = _f(np.cos, lambda v: -np.sin(v))
atan = _f(np.arctan, lambda v: 1 / (1 + v * v))
exp = _f(np.exp, np.exp)
pos = _f(lambda v: np.maximum(v, 0), lambda v: (v > 0).astype(v.dtype))
neg = _f(lambda v: np.minimum(v, 0), lambda v: (v < 0).astype(v.dtype))


def S(order, *terms):
    """the sum of the terms, from the left (order 0) or from the right (order 1)"""
    t = list(terms) if order == 0 else list(terms)[::-1]
    acc = t[0]
    for x in t[1:]:
        acc = acc + x
    return acc


def collocation(dtype=LD):
    """tau, C, D, B as the reference describes them: Lagrange polynomials through tau in the monomial basis (numpy.poly1d's arithmetic: polymul,
    polyder, polyint, polyval), here in `dtype`"""
    s15 = np.sqrt(dtype(15)) / dtype(10)
    tau = np.array([dtype(0), dtype(0.5) - s15, dtype(0.5), dtype(0.5) + s15], dtype=dtype)
    C, D, B = np.zeros((4, 4), dtype), np.zeros(4, dtype), np.zeros(4, dtype)
    for j in range(4):
        p = np.array([1], dtype=dtype)
        for r in range(4):
            if r != j:
                p = np.polymul(p, np.array([1, -tau[r]], dtype=dtype) / (tau[j] - tau[r]))
        D[j] = np.polyval(p, dtype(1))
        pd = np.polyder(p)
        for r in range(4):
            C[j, r] = np.polyval(pd, tau[r])
        B[j] = np.polyval(np.polyint(p), dtype(1))
    return tau, C, D, B


def collocation_poly1d():
    """The same constants through numpy.poly1d in float64 (the class the reference builds them with), from the roots: the Lagrange polynomial of
    point j is the monic polynomial through the other three points over its own value at tau_j."""
    s15 = np.sqrt(15) / 10
    tau = np.array([0.0, 0.5 - s15, 0.5, 0.5 + s15])
    C, D, B = np.zeros((4, 4)), np.zeros(4), np.zeros(4)
    for j in range(4):
        monic = np.poly1d(np.delete(tau, j), True)
        lj = monic / monic(tau[j])
        D[j], B[j], C[j] = lj(1.0), lj.integ()(1.0), lj.deriv()(tau)
    return tau, C, D, B


def reg_gradient(prob, w):
    """d J / d U of the two cyclic regularisation terms alone, [N, 4] in longdouble: one dual pass per (interval, control)."""
    P, arr, _ = cast(prob, LD)
    N = arr["h"].shape[0]
    _, U, _ = split_w(np.asarray(w).astype(LD), N)
    out = np.zeros((N, 4), LD)
    for k in range(N):
        for c in range(3):
            Ud = [Dual(a) for a in U]
            Ud[c].d[k] = 1
            dp, fp = Ud[0] * US[0], Ud[1] * US[1] / 10000.0 + Ud[2] * US[2] / 10000.0
            tot = None
            for p_, pen in ((fp, P["penalty_F"]), (dp, P["penalty_delta"])):
                e = p_ - Dual(np.roll(p_.v, -1), np.roll(p_.d, -1))
                t = pen * (e * e)
                tot = t if tot is None else tot + t
            out[k, c] = np.sum(tot.d)
    return out


def model(x, u, kappa, P, order=0, denoms=None):
    """The double-track model at scaled states x [5] and controls u [4] (arrays over the evaluation points, or Duals): dx / x_s, sf, the tire forces
    fx, fy, fz (fl, fr, rl, rr), ax, ay.  denoms: a list that receives (name, values) of every denominator."""
    v, beta, omega, n, xi = (x[i] * XS[i] for i in range(5))
    delta, f_drive, f_brake, gamma_y = (u[i] * US[i] for i in range(4))
    mass, g, wb = P["mass"], P["g"], P["wheelbase_front"] + P["wheelbase_rear"]
    f_xdrag = P["dragcoeff"] * (v * v)
    f_xroll_f = 0.5 * P["c_roll"] * mass * g * P["wheelbase_rear"] / wb
    f_xroll_r = 0.5 * P["c_roll"] * mass * g * P["wheelbase_front"] / wb
    f_xroll = P["c_roll"] * mass * g
    f_zstat = (0.5 * mass * g * P["wheelbase_rear"] / wb, 0.5 * mass * g * P["wheelbase_front"] / wb)
    f_zlift = (0.5 * P["liftcoeff_front"] * (v * v), 0.5 * P["liftcoeff_rear"] * (v * v))
    f_long = S(order, f_drive, f_brake, -f_xdrag, -f_xroll)
    cz = 0.5 * P["cog_z"] / wb
    fz = [S(order, f_zstat[0], f_zlift[0], S(order, -cz * f_long, -P["k_roll"] * gamma_y)),
          S(order, f_zstat[0], f_zlift[0], S(order, -cz * f_long, P["k_roll"] * gamma_y)),
          S(order, f_zstat[1], f_zlift[1], S(order, cz * f_long, -(1.0 - P["k_roll"]) * gamma_y)),
          S(order, f_zstat[1], f_zlift[1], S(order, cz * f_long, (1.0 - P["k_roll"]) * gamma_y))]
    vs, vc = v * sin(beta), v * cos(beta)
    num_f, num_r = S(order, vs, P["wheelbase_front"] * omega), S(order, -vs, P["wheelbase_rear"] * omega)
    twf, twr = 0.5 * P["track_width_front"] * omega, 0.5 * P["track_width_rear"] * omega
    den = [vc - twf, vc + twf, vc - twr, vc + twr]
    alpha = [delta - atan(num_f / den[0]), delta - atan(num_f / den[1]), atan(num_r / den[2]), atan(num_r / den[3])]
    fy = []
    for q in range(4):
        ax_ = "front" if q < 2 else "rear"
        ba = P["B_" + ax_] * alpha[q]
        fy.append(P["mue"] * fz[q] * (1 + P["eps_" + ax_] * fz[q] / P["f_z0"]) * sin(P["C_" + ax_] * atan(ba - P["E_" + ax_] * (ba - atan(ba)))))
    fxf1 = S(order, 0.5 * f_drive * P["k_drive_front"], 0.5 * f_brake * P["k_brake_front"], -f_xroll_f)
    fxr1 = S(order, 0.5 * f_drive * (1 - P["k_drive_front"]), 0.5 * f_brake * (1 - P["k_brake_front"]), -f_xroll_r)
    fx = [fxf1, fxf1, fxr1, fxr1]
    sd, cd = sin(delta), cos(delta)
    fxf, fxr, fyf, fyr = fx[0] + fx[1], fx[2] + fx[3], fy[0] + fy[1], fy[2] + fy[3]
    ax = S(order, fxr, fxf * cd, -(fyf * sd), -(P["dragcoeff"] * (v * v))) / mass
    ay = S(order, fxf * sd, fy[2], fy[3], fyf * cd) / mass
    csum = cos(xi + beta)
    sf = (1.0 - n * kappa) / (v * csum)
    sb, cb, sdb, cdb = sin(beta), cos(beta), sin(delta - beta), cos(delta - beta)
    dv = (sf / mass) * S(order, fxr * cb, fxf * cdb, fyr * sb, -(fyf * sdb), -(f_xdrag * cb))
    dbeta = sf * S(order, -omega, S(order, -(fxr * sb), fxf * sdb, fyr * cb, fyf * cdb, f_xdrag * sb) / (mass * v))
    domega = (sf / P["I_z"]) * S(order, (fx[3] - fx[2]) * P["track_width_rear"] / 2, -(fyr * P["wheelbase_rear"]),
                                 S(order, (fx[1] - fx[0]) * cd, (fy[0] - fy[1]) * sd) * P["track_width_front"] / 2,
                                 S(order, fyf * cd, fxf * sd) * P["track_width_front"])
    dn = sf * v * sin(xi + beta)
    dxi = sf * omega - kappa
    if denoms is not None:
        for a in den:
            denoms.append(("v cos(beta) -+ 0.5 tw omega_z", val(a), np.abs(val(v)) / 4))
        denoms.append(("v", val(v), 4.0))            # four times the NLP's own lower bound of 1 m/s
        denoms.append(("cos(xi + beta)", val(csum), 0.25))
        for q in range(4):
            denoms.append(("mue f_z", val(P["mue"] * fz[q]), abs(P["mue"]) * f_zstat[q // 2] / 4))
    dx = [dv / XS[0], dbeta / XS[1], domega / XS[2], dn / XS[3], dxi / XS[4]]
    return dict(dx=dx, sf=sf, fx=fx, fy=fy, fz=fz, ax=ax, ay=ay)


def f_zstat_of(P, q):
    return 0.5 * P["mass"] * P["g"] * (P["wheelbase_rear"] if q < 2 else P["wheelbase_front"]) / (P["wheelbase_front"] + P["wheelbase_rear"])


def friction(fr, row_n, P, opts, q):
    """mue of wheel q at the rows k + 1 and lateral positions row_n [m]"""
    if opts.get("friction") is None:
        return P["mue"]
    wq = fr["w_mue"][q]           # [N, P]: rows 1 .. N
    if opts["friction"] == "linear":
        return wq[:, 0] * row_n + wq[:, 1]
    ng, cd = opts["n_gauss"], fr["center_dist"]
    sigma = 2.0 * cd
    acc = None
    for i in range(2 * ng + 1):
        dq = row_n - (i - ng) * cd
        t = wq[:, i] * exp(-(dq * dq) / (2.0 * (sigma * sigma)))
        acc = t if acc is None else acc + t
    return acc + wq[:, 2 * ng + 1]


def interval_rows(Xk, Uk, Xc, Xk1, Ukm1, hk, hkm1, kap, fr, P, opts, coll, order=0, denoms=None):
    """The 33 row slots of every interval (lists over the slots of arrays over k) and the interval outputs, with the five variable groups of an
    interval as independent inputs: Xk, Xk1, Xc[0..2] lists of 5, Uk, Ukm1 lists of 4 (arrays over k, or Duals)."""
    tau, C, D, B = coll
    ka, kb = kap[:-1], kap[1:]
    rows, q = [], []
    for j in (1, 2, 3):
        m = model(Xc[j - 1], Uk, ka + tau[j] * (kb - ka), P, order, denoms)
        for i in range(5):
            xp = S(order, C[0, j] * Xk[i], C[1, j] * Xc[0][i], C[2, j] * Xc[1][i], C[3, j] * Xc[2][i])
            rows.append(hk * m["dx"][i] - xp)
        q.append(B[j] * m["sf"] * hk)
    dt = S(order, q[0], q[1], q[2])
    ec = Xk[0] * XS[0] * Uk[1] * US[1] * dt
    for i in range(5):
        rows.append(S(order, D[0] * Xk[i], D[1] * Xc[0][i], D[2] * Xc[1][i], D[3] * Xc[2][i]) - Xk1[i])
    m = model(Xk1, Uk, ka, P, order, denoms)
    rows.append(Xk1[0] * Uk[1])
    n1 = Xk1[3] * XS[3]
    for w in range(4):
        den = friction(fr, n1, P, opts, w) * m["fz"][w]
        if denoms is not None:
            denoms.append(("mue f_z (Kamm)", val(den), abs(P["mue"]) * f_zstat_of(P, w) / 4))
        a, c = m["fx"][w] / den, m["fy"][w] / den
        rows.append(a * a + c * c)
    delta = Uk[0] * US[0]
    rows.append(S(order, (m["fy"][0] + m["fy"][1]) * cos(delta), m["fy"][2], m["fy"][3], (m["fx"][0] + m["fx"][1]) * sin(delta)) * P["cog_z"]
                / ((P["track_width_front"] + P["track_width_rear"]) / 2) - Uk[3] * US[3])
    rows.append(Uk[1] * Uk[2])
    sigma = (1 - ka * Xk1[3] * XS[3]) / (Xk1[0] * XS[0])
    if denoms is not None:
        denoms.append(("h sigma", val(hkm1 * sigma)[1:], (val(hkm1) / (4 * np.abs(val(Xk1[0] * XS[0]))))[1:]))
    for i in range(4):
        rows.append((Uk[i] - Ukm1[i]) / (hkm1 * sigma))
    ap, an, al = pos(m["ax"]) / P["ax_pos_safe"], neg(m["ax"]) / P["ax_neg_safe"], m["ay"] / P["ay_safe"]
    rows.append(ap * ap + al * al)
    rows.append(an * an + al * al)
    tf = []
    for w in range(4):
        tf += [m["fx"][w], m["fy"][w], m["fz"][w]]
    return rows, dict(dt=dt, ec=ec, tf=tf, ax=m["ax"], ay=m["ay"])


def split_w(w, N):
    """w [5 + 24 N] (an array or a Dual) -> X [N + 1] rows of 5, U [N] rows of 4, Xc [N][3] rows of 5, as lists of arrays over k"""
    def col(off, count, n):
        idx = off + 24 * np.arange(n)
        return [Dual(w.v[idx + i], w.d[idx + i]) if isinstance(w, Dual) else w[idx + i] for i in range(count)]
    return col(0, 5, N + 1), col(5, 4, N), [col(9 + 5 * j, 5, N) for j in range(3)]


def cast(prob, dtype):
    P = {k: dtype(prob["pars"][k]) for k in PARS}
    arr = {k: np.asarray(prob[k], dtype=np.float64).astype(dtype) for k in ("h", "kappa_cl", "w_tr_right_cl", "w_tr_left_cl")}
    fr = None
    if prob.get("w_mue") is not None:
        fr = dict(w_mue=np.asarray(prob["w_mue"], dtype=np.float64).astype(dtype)[:, 1:, :])
        if prob.get("center_dist") is not None:
            fr["center_dist"] = np.asarray(prob["center_dist"], dtype=np.float64).astype(dtype)[1:]
    return P, arr, fr


def take(x, sl):
    return [Dual(a.v[sl], a.d[sl]) if isinstance(a, Dual) else a[sl] for a in x]


def roll1(x):
    return [Dual(np.roll(a.v, 1), np.roll(a.d, 1)) if isinstance(a, Dual) else np.roll(a, 1) for a in x]


def nlp(prob, w, opts, dtype=LD, order=0, denoms=None):
    """Everything the evaluation entry returns for one problem, from w (an array, cast to dtype, or a Dual of that dtype)."""
    P, arr, fr = cast(prob, dtype)
    N = arr["h"].shape[0]
    coll = collocation(LD)
    coll = tuple(c.astype(dtype) for c in coll)
    if not isinstance(w, Dual):
        w = np.asarray(w).astype(dtype)
    X, U, Xc = split_w(w, N)
    rows, out = interval_rows(take(X, slice(0, N)), U, Xc, take(X, slice(1, N + 1)), roll1(U), arr["h"], np.roll(arr["h"], 1), arr["kappa_cl"],
                              fr, P, opts, coll, order, denoms)
    safe, energy = bool(opts.get("safe_traj")), bool(opts.get("limit_energy"))
    pieces_v, pieces_d = [], []
    dual = isinstance(w, Dual)
    for k in range(N):
        use = list(range(27)) + (list(range(27, 31)) if k > 0 else []) + ([31, 32] if safe else [])
        for r in use:
            pieces_v.append(val(rows[r])[k])
            if dual:
                pieces_d.append(tan(rows[r])[k])
    for i in range(5):
        per = X[i]
        pieces_v.append(val(per)[0] - val(per)[N])
        if dual:
            pieces_d.append(tan(per)[0] - tan(per)[N])
    dt, ec = out["dt"], out["ec"]

    def total(a):
        v, d = val(a), tan(a) if dual else None
        idx = range(N) if order == 0 else range(N - 1, -1, -1)
        sv = v[0] * 0
        sd = sv
        for k in idx:
            sv = sv + v[k]
            if dual:
                sd = sd + d[k]
        return (sv, sd)
    lap, en = total(dt), total(ec)
    if energy:
        pieces_v.append(en[0] / 3600000.0)
        if dual:
            pieces_d.append(en[1] / 3600000.0)
    dp = U[0] * US[0]
    fp = U[1] * US[1] / 10000.0 + U[2] * US[2] / 10000.0

    def cyc(p):
        nxt = Dual(np.roll(p.v, -1), np.roll(p.d, -1)) if dual else np.roll(p, -1)
        e = p - nxt
        return total(e * e)
    jd, jf = cyc(dp), cyc(fp)
    J = lap[0] + P["penalty_F"] * jf[0] + P["penalty_delta"] * jd[0]
    res = dict(g=np.array(pieces_v, dtype=dtype), J=J, lap_time=lap[0], energy=en[0] / 3600000.0,
               x_opt=np.stack([val(X[i]) * XS[i] for i in range(5)], axis=1), u_opt=np.stack([val(U[i]) * US[i] for i in range(4)], axis=1),
               tf_opt=np.stack([val(t) for t in out["tf"]], axis=1), dt_opt=val(dt), ec_opt=val(ec), ax_opt=val(out["ax"]), ay_opt=val(out["ay"]))
    if dual:
        res.update(g_d=np.array(pieces_d, dtype=dtype), J_d=lap[1] + P["penalty_F"] * jf[1] + P["penalty_delta"] * jd[1], energy_d=en[1] / 3600000.0)
    return res


def dense_derivatives(prob, w, opts):
    """The dense Jacobian [ng, nw], grad J and grad energy [nw] in longdouble: one dual pass per entry of w (small N only)."""
    w = np.asarray(w).astype(LD)
    nw = w.shape[0]
    cols, gJ, gE = [], np.zeros(nw, LD), np.zeros(nw, LD)
    for i in range(nw):
        d = np.zeros(nw, LD)
        d[i] = 1
        r = nlp(prob, Dual(w, d), opts)
        cols.append(r["g_d"])
        gJ[i], gE[i] = r["J_d"], r["energy_d"]
    return np.stack(cols, axis=1), gJ, gE


def blocks(prob, w, opts, dtype=LD, order=0):
    """The interval blocks [N, 33, 33] in longdouble (absent slots zero), and the entries of grad J / grad energy that live inside an interval:
    dJ [N, 24] = d dt_k / d slot (the quadrature's share: grad J without the regularisation), dE [N, 24] = d ec_k / d slot / 3.6e6.  One dual pass
    per column slot, every interval at once."""
    P, arr, fr = cast(prob, dtype)
    N = arr["h"].shape[0]
    coll = tuple(c.astype(dtype) for c in collocation(LD))
    w = np.asarray(w).astype(dtype)
    X, U, Xc = split_w(w, N)
    LD_ = dtype
    groups = [take(X, slice(0, N)), U, Xc[0], Xc[1], Xc[2], take(X, slice(1, N + 1)), roll1(U)]
    sizes = [5, 4, 5, 5, 5, 5, 4]
    out = np.zeros((N, 33, 33), LD_)
    dJ, dE = np.zeros((N, 24), LD_), np.zeros((N, 24), LD_)
    safe = bool(opts.get("safe_traj"))
    c = 0
    for gi, sz in enumerate(sizes):
        for i in range(sz):
            seeded = [[Dual(a, np.ones_like(a) if (g2 == gi and i2 == i) else None) for i2, a in enumerate(grp)] for g2, grp in enumerate(groups)]
            rows, o = interval_rows(seeded[0], seeded[1], seeded[2:5], seeded[5], seeded[6], arr["h"], np.roll(arr["h"], 1), arr["kappa_cl"], fr, P,
                                    opts, coll, order)
            for r in range(33):
                out[:, r, c] = rows[r].d
            if c < 24:
                dJ[:, c], dE[:, c] = o["dt"].d, o["ec"].d / 3600000.0
            c += 1
    out[0, 27:31, :] = 0
    if not safe:
        out[:, 31:33, :] = 0
    return out, dJ, dE


def bounds(prob, opts, dtype=np.float64):
    """w0, lbw, ubw, lbg, ubg as the reference builds them (float64 statements, left to right)"""
    P = prob["pars"]
    N = np.asarray(prob["h"]).shape[0]
    wr, wl = np.asarray(prob["w_tr_right_cl"], dtype=np.float64), np.asarray(prob["w_tr_left_cl"], dtype=np.float64)
    inf = np.inf
    delta_min, delta_max = -P["delta_max"] / 0.5, P["delta_max"] / 0.5
    f_drive_max, f_brake_min = P["f_drive_max"] / 7500.0, -P["f_brake_max"] / 20000.0
    v_guess = 20.0 / 50

    def xb(k):
        n_min, n_max = (-wr[k] + P["width_opt"] / 2.0) / 5.0, (wl[k] - P["width_opt"] / 2.0) / 5.0
        return ([1.0 / 50, -0.5 * np.pi / 0.5, -0.5 * np.pi / 1, n_min, -0.5 * np.pi / 1.0],
                [P["v_max"] / 50, 0.5 * np.pi / 0.5, 0.5 * np.pi / 1, n_max, 0.5 * np.pi / 1.0])
    lo, hi = xb(0)
    w0, lbw, ubw, lbg, ubg = [v_guess, 0, 0, 0, 0], list(lo), list(hi), [], []
    for k in range(N):
        lbw += [delta_min, 0.0, f_brake_min, -inf]
        ubw += [delta_max, f_drive_max, 0.0, inf]
        w0 += [0.0] * 4
        for j in range(3):
            lbw += [-inf] * 5
            ubw += [inf] * 5
            w0 += [v_guess, 0, 0, 0, 0]
        lo, hi = xb(k + 1)
        lbw += lo
        ubw += hi
        w0 += [v_guess, 0, 0, 0, 0]
        lbg += [0.0] * 20 + [-inf] + [0.0] * 4 + [0.0] + [-20000.0 / (7500.0 * 20000.0)]
        ubg += [0.0] * 20 + [P["power_max"] / (7500.0 * 50)] + [1.0] * 4 + [0.0] + [0.0]
        if k > 0:
            lbg += [delta_min / P["t_delta"], -inf, f_brake_min / P["t_brake"], -inf]
            ubg += [delta_max / P["t_delta"], f_drive_max / P["t_drive"], inf, inf]
        if opts.get("safe_traj"):
            lbg += [0.0] * 2
            ubg += [1.0] * 2
    lbg += [0.0] * 5
    ubg += [0.0] * 5
    if opts.get("limit_energy"):
        lbg += [0]
        ubg += [P["energy_limit"]]
    return tuple(np.array(a, dtype=dtype) for a in (w0, lbw, ubw, lbg, ubg))


def row_of(N, k, r, safe):
    """the index in g of row slot r of interval k, or -1 where the slot is absent"""
    start = k * (27 + 2 * safe) + 4 * max(k - 1, 0)
    if r < 27:
        return start + r
    if r < 31:
        return start + r if k > 0 else -1
    return (start + 27 + (4 if k > 0 else 0) + (r - 31)) if safe else -1
