"""A plain second-order restatement of what mcq_mintime_hess_device and mcq_mintime_hessvec_device compute (include/mcq.h "Hessian blocks"): the
Hessian of the Lagrangian sigma J + lam_g . g of the reference's minimum-time NLP [REF opt_mintime_traj/src/opt_mintime.py:143-861], written from
the maths with a hyper-dual scalar of its own (H2 below: value, two tangents, the mixed term; tests/mintime_ref.py's Dual does not nest) -- in
longdouble (the reference of every comparison) and in float64 in the two operation orders of mintime_ref.S, whose distance from longdouble is the
measured spread of tests/mintime_hess_guard.py.

The Lagrangian splits by interval: phi_k is a function of the interval's 33 slots [X_k, U_k, Xc_k,0..2, X_k+1, U_k-1 (cyclic: U_N-1 at k = 0)], and
phi_k itself is a sum of PARTS that read few slots each: the three collocation points (their rows, and their share of the interval's time under
sigma and under the energy row's multiplier with the START state's speed and the drive force), the path point (its rows at X_k+1 with U_k, the
actuator rows with U_k-1), the regularisation's term between U_k-1 and U_k, and the linear rows (collocation's polynomial part, continuity), which
have a gradient and no Hessian.  Arrays run over the intervals; the blocks take one pass per pair of slots inside a part; there are no lanes and no
owners.  mintime_ref supplies constants, collocation, cast and the cross-checks of tests/test_mintime_hess_ref.py."""
import numpy as np

import mintime_ref as mr

LD = np.longdouble
XS, US = mr.XS, mr.US
# the slots of an interval block, by group
SLOT_X, SLOT_U, SLOT_XC, SLOT_X1, SLOT_UP = 0, 5, 9, 24, 29
PARTS = ("c0", "c1", "c2", "path", "reg")
PART_SLOTS = {"c0": [0] + list(range(5, 14)), "c1": [0] + list(range(5, 9)) + list(range(14, 19)), "c2": [0] + list(range(5, 9)) + list(range(19, 24)),
              "path": list(range(5, 9)) + list(range(24, 33)), "reg": list(range(5, 9)) + list(range(29, 33))}
ROW_KINDS = {"collocation": list(range(0, 15)), "power": [20], "kamm_fl": [21], "kamm_fr": [22], "kamm_rl": [23], "kamm_rr": [24], "roll": [25],
             "pedal": [26], "actuator": [27, 28, 29, 30], "safe_pos": [31], "safe_neg": [32]}


class H2:
    """value, tangents along two directions, mixed second derivative: arrays of one dtype"""
    __array_priority__ = 100
    __array_ufunc__ = None

    def __init__(self, v, a=None, b=None, ab=None):
        self.v = np.asarray(v)
        z = np.zeros_like(self.v)
        self.a = z if a is None else np.asarray(a)
        self.b = z if b is None else np.asarray(b)
        self.ab = z if ab is None else np.asarray(ab)

    @staticmethod
    def lift(x):
        return x if isinstance(x, H2) else H2(x)

    def __add__(self, o):
        o = H2.lift(o)
        return H2(self.v + o.v, self.a + o.a, self.b + o.b, self.ab + o.ab)
    __radd__ = __add__

    def __sub__(self, o):
        o = H2.lift(o)
        return H2(self.v - o.v, self.a - o.a, self.b - o.b, self.ab - o.ab)

    def __rsub__(self, o):
        return H2.lift(o) - self

    def __neg__(self):
        return H2(-self.v, -self.a, -self.b, -self.ab)

    def __mul__(self, o):
        o = H2.lift(o)
        return H2(self.v * o.v, self.a * o.v + self.v * o.a, self.b * o.v + self.v * o.b,
                  self.ab * o.v + self.a * o.b + self.b * o.a + self.v * o.ab)
    __rmul__ = __mul__

    def __truediv__(self, o):
        """q = x / y from x = q y differentiated: x' = q' y + q y', x'' = q'' y + q'_a y'_b + q'_b y'_a + q y''"""
        o = H2.lift(o)
        q = self.v / o.v
        qa, qb = (self.a - q * o.a) / o.v, (self.b - q * o.b) / o.v
        return H2(q, qa, qb, (self.ab - qa * o.b - qb * o.a - q * o.ab) / o.v)

    def __rtruediv__(self, o):
        return H2.lift(o) / self


def chain(x, f, f1, f2):
    """f(x) from f, f', f'' at the value"""
    return H2(f, f1 * x.a, f1 * x.b, f1 * x.ab + f2 * (x.a * x.b))


def _fn(f, f1, f2):
    def g(x):
        if isinstance(x, H2):
            return chain(x, f(x.v), f1(x.v), f2(x.v))
        return f(x)
    return g


sin = _fn(np.sin, np.cos, lambda v: -np.sin(v))
cos = _fn(np.cos, lambda v: -np.sin(v), lambda v: -np.cos(v))
atan = _fn(np.arctan, lambda v: 1 / (1 + v * v), lambda v: -2 * v / ((1 + v * v) * (1 + v * v)))
exp = _fn(np.exp, np.exp, np.exp)
# max(x, 0) and min(x, 0): the branch taken (zero derivatives on the other)
pos = _fn(lambda v: np.maximum(v, 0), lambda v: (v > 0).astype(v.dtype), lambda v: np.zeros_like(v))
neg = _fn(lambda v: np.minimum(v, 0), lambda v: (v < 0).astype(v.dtype), lambda v: np.zeros_like(v))
S = mr.S


def val(x):
    return x.v if isinstance(x, H2) else x


def vehicle(x, u, kappa, P, order):
    """The double-track model [REF :284-441] at scaled states x [5] and controls u [4]: the five derivatives over their scalings, the time-distance
    factor sf, the tire forces of fl, fr, rl, rr and the accelerations."""
    v, beta, omega, n, xi = x[0] * XS[0], x[1] * XS[1], x[2] * XS[2], x[3] * XS[3], x[4] * XS[4]
    delta, f_drive, f_brake, gamma_y = u[0] * US[0], u[1] * US[1], u[2] * US[2], u[3] * US[3]
    m, g, lf, lr = P["mass"], P["g"], P["wheelbase_front"], P["wheelbase_rear"]
    wb = lf + lr
    twf, twr = P["track_width_front"], P["track_width_rear"]
    vv = v * v
    drag = P["dragcoeff"] * vv
    roll_f, roll_r, roll = 0.5 * P["c_roll"] * m * g * lr / wb, 0.5 * P["c_roll"] * m * g * lf / wb, P["c_roll"] * m * g
    stat = (0.5 * m * g * lr / wb, 0.5 * m * g * lf / wb)
    lift = (0.5 * P["liftcoeff_front"] * vv, 0.5 * P["liftcoeff_rear"] * vv)
    f_long = S(order, f_drive, f_brake, -drag, -roll)
    cz, kr = 0.5 * P["cog_z"] / wb, P["k_roll"]
    fz = [S(order, stat[0], lift[0], S(order, -cz * f_long, -kr * gamma_y)), S(order, stat[0], lift[0], S(order, -cz * f_long, kr * gamma_y)),
          S(order, stat[1], lift[1], S(order, cz * f_long, -(1.0 - kr) * gamma_y)), S(order, stat[1], lift[1], S(order, cz * f_long, (1.0 - kr) * gamma_y))]
    vs, vc = v * sin(beta), v * cos(beta)
    nf, nr = S(order, vs, lf * omega), S(order, -vs, lr * omega)
    hf, hr = 0.5 * twf * omega, 0.5 * twr * omega
    alpha = [delta - atan(nf / (vc - hf)), delta - atan(nf / (vc + hf)), atan(nr / (vc - hr)), atan(nr / (vc + hr))]
    fy = []
    for q in range(4):
        e = "front" if q < 2 else "rear"
        ba = P["B_" + e] * alpha[q]
        fy.append(P["mue"] * fz[q] * (1 + P["eps_" + e] * fz[q] / P["f_z0"]) * sin(P["C_" + e] * atan(ba - P["E_" + e] * (ba - atan(ba)))))
    fx_f = S(order, 0.5 * f_drive * P["k_drive_front"], 0.5 * f_brake * P["k_brake_front"], -roll_f)
    fx_r = S(order, 0.5 * f_drive * (1 - P["k_drive_front"]), 0.5 * f_brake * (1 - P["k_brake_front"]), -roll_r)
    fx = [fx_f, fx_f, fx_r, fx_r]
    sd, cd = sin(delta), cos(delta)
    fxf, fxr, fyf, fyr = fx[0] + fx[1], fx[2] + fx[3], fy[0] + fy[1], fy[2] + fy[3]
    ax = S(order, fxr, fxf * cd, -(fyf * sd), -(P["dragcoeff"] * vv)) / m
    ay = S(order, fxf * sd, fy[2], fy[3], fyf * cd) / m
    sf = (1.0 - n * kappa) / (v * cos(xi + beta))
    sb, cb, sdb, cdb = sin(beta), cos(beta), sin(delta - beta), cos(delta - beta)
    dv = (sf / m) * S(order, fxr * cb, fxf * cdb, fyr * sb, -(fyf * sdb), -(drag * cb))
    dbeta = sf * S(order, -omega, S(order, -(fxr * sb), fxf * sdb, fyr * cb, fyf * cdb, drag * sb) / (m * v))
    domega = (sf / P["I_z"]) * S(order, (fx[3] - fx[2]) * twr / 2, -(fyr * lr), S(order, (fx[1] - fx[0]) * cd, (fy[0] - fy[1]) * sd) * twf / 2,
                                 S(order, fyf * cd, fxf * sd) * twf)
    dn = sf * v * sin(xi + beta)
    dxi = sf * omega - kappa
    return dict(dx=[dv / XS[0], dbeta / XS[1], domega / XS[2], dn / XS[3], dxi / XS[4]], sf=sf, fx=fx, fy=fy, fz=fz, ax=ax, ay=ay)


def mue_of(fr, n, P, opts, q):
    """the friction coefficient of wheel q at the rows k + 1 and lateral positions n [m] (:717-747)"""
    if opts.get("friction") is None:
        return P["mue"]
    wq = fr["w_mue"][q]
    if opts["friction"] == "linear":
        return wq[:, 0] * n + wq[:, 1]
    ng, cd = opts["n_gauss"], fr["center_dist"]
    sigma = 2.0 * cd
    acc = None
    for i in range(2 * ng + 1):
        dq = n - (i - ng) * cd
        t = wq[:, i] * exp(-(dq * dq) / (2.0 * (sigma * sigma)))
        acc = t if acc is None else acc + t
    return acc + wq[:, 2 * ng + 1]


class Env:
    """one problem's constants in a dtype, its multipliers laid out per (row slot, interval) with zeros where a row is absent, sigma, the energy
    row's multiplier (zero where the row is disabled)"""

    def __init__(self, prob, opts, lam_g, sigma, dtype, order):
        self.P, arr, self.fr = mr.cast(prob, dtype)
        self.opts, self.order, self.dtype = opts, order, dtype
        self.h, self.kap = arr["h"], arr["kappa_cl"]
        N = self.N = self.h.shape[0]
        self.hp = np.roll(self.h, 1)
        self.coll = tuple(c.astype(dtype) for c in mr.collocation(LD))
        self.safe, self.energy = bool(opts.get("safe_traj")), bool(opts.get("limit_energy"))
        lam_g = np.asarray(lam_g, dtype=np.float64).astype(dtype)
        self.lam = np.zeros((33, N), dtype)
        for k in range(N):
            for r in range(33):
                i = mr.row_of(N, k, r, int(self.safe))
                if i >= 0:
                    self.lam[r, k] = lam_g[i]
        self.sigma = dtype(sigma)
        self.lam_e = lam_g[mr.row_of(N, N, 0, int(self.safe)) + 5] if self.energy else dtype(0)


def part(env, name, G):
    """One part of phi_k for every interval: G = [X_k (5), U_k (4), Xc_k,0 (5), Xc_k,1, Xc_k,2, X_k+1 (5), U_k-1 (4)], lists of arrays or H2."""
    Xk, Uk, Xc, Xk1, Up = G[0], G[1], G[2:5], G[5], G[6]
    P, lam, o, h = env.P, env.lam, env.order, env.h
    tau, C, D, B = env.coll
    ka, kb = env.kap[:-1], env.kap[1:]
    if name in ("c0", "c1", "c2"):
        j = int(name[1]) + 1
        m = vehicle(Xc[j - 1], Uk, ka + tau[j] * (kb - ka), P, o)
        q = B[j] * m["sf"] * h
        rows = S(o, *[lam[5 * (j - 1) + i] * (h * m["dx"][i]) for i in range(5)])
        return S(o, rows, env.sigma * q, env.lam_e * (Xk[0] * XS[0] * Uk[1] * US[1] * q) / 3600000.0)
    if name == "lin":
        terms = []
        for j in (1, 2, 3):
            for i in range(5):
                terms.append(-(lam[5 * (j - 1) + i] * S(o, C[0, j] * Xk[i], C[1, j] * Xc[0][i], C[2, j] * Xc[1][i], C[3, j] * Xc[2][i])))
        for i in range(5):
            terms.append(lam[15 + i] * (S(o, D[0] * Xk[i], D[1] * Xc[0][i], D[2] * Xc[1][i], D[3] * Xc[2][i]) - Xk1[i]))
        return S(o, *terms)
    if name == "path":
        m = vehicle(Xk1, Uk, ka, P, o)
        terms = [lam[20] * (Xk1[0] * Uk[1])]
        n1 = Xk1[3] * XS[3]
        for q in range(4):
            den = mue_of(env.fr, n1, P, env.opts, q) * m["fz"][q]
            a, c = m["fx"][q] / den, m["fy"][q] / den
            terms.append(lam[21 + q] * (a * a + c * c))
        delta = Uk[0] * US[0]
        terms.append(lam[25] * (S(o, (m["fy"][0] + m["fy"][1]) * cos(delta), m["fy"][2], m["fy"][3], (m["fx"][0] + m["fx"][1]) * sin(delta)) * P["cog_z"]
                                / ((P["track_width_front"] + P["track_width_rear"]) / 2) - Uk[3] * US[3]))
        terms.append(lam[26] * (Uk[1] * Uk[2]))
        sig = (1 - ka * Xk1[3] * XS[3]) / (Xk1[0] * XS[0])
        for i in range(4):
            terms.append(lam[27 + i] * ((Uk[i] - Up[i]) / (env.hp * sig)))      # (the multipliers of interval 0's absent rows are zeros)
        if env.safe:
            ap, an, al = pos(m["ax"]) / P["ax_pos_safe"], neg(m["ax"]) / P["ax_neg_safe"], m["ay"] / P["ay_safe"]
            terms += [lam[31] * (ap * ap + al * al), lam[32] * (an * an + al * al)]
        return S(o, *terms)
    if name == "reg":
        dd = Up[0] * US[0] - Uk[0] * US[0]
        df = (Up[1] * US[1] / 10000.0 + Up[2] * US[2] / 10000.0) - (Uk[1] * US[1] / 10000.0 + Uk[2] * US[2] / 10000.0)
        return env.sigma * S(o, P["penalty_delta"] * (dd * dd), P["penalty_F"] * (df * df))
    raise KeyError(name)


def groups_of(w, N):
    """the seven variable groups of every interval from w [5 + 24 N]: lists of arrays over k; U_k-1 cyclic"""
    X, U, Xc = mr.split_w(w, N)
    return [[a[:N] for a in X], U, Xc[0], Xc[1], Xc[2], [a[1:N + 1] for a in X], [np.roll(a, 1) for a in U]]


def seeded(groups, sa, sb):
    """the groups as H2 with unit tangents a on slot sa and b on slot sb (None: none)"""
    out, s = [], 0
    for grp in groups:
        g2 = []
        for x in grp:
            one = np.ones_like(x)
            g2.append(H2(x, one if s == sa else None, one if s == sb else None))
            s += 1
        out.append(g2)
    return out


def blocks(prob, w, opts, lam_g, sigma=1.0, dtype=LD, order=0, parts=PARTS):
    """The Hessian blocks [N, 33, 33] of one problem: for every part, one hyper-dual pass per unordered pair of the slots it reads."""
    env = Env(prob, opts, lam_g, sigma, dtype, order)
    grp = groups_of(np.asarray(w, dtype=np.float64).astype(dtype), env.N)
    out = np.zeros((env.N, 33, 33), dtype)
    for name in parts:
        slots = PART_SLOTS[name]
        for ia, sa in enumerate(slots):
            for sb in slots[ia:]:
                d2 = part(env, name, seeded(grp, sa, sb)).ab
                out[:, sa, sb] += d2
                if sb != sa:
                    out[:, sb, sa] += d2
    return out


def gradient(prob, w, opts, lam_g, sigma=1.0, dtype=LD, order=0, parts=PARTS + ("lin",)):
    """d phi_k / d slot [N, 33]: the first-order parts of the same passes"""
    env = Env(prob, opts, lam_g, sigma, dtype, order)
    grp = groups_of(np.asarray(w, dtype=np.float64).astype(dtype), env.N)
    out = np.zeros((env.N, 33), dtype)
    for s in range(33):
        for name in parts:
            if name == "lin" or s in PART_SLOTS[name]:
                out[:, s] += np.broadcast_to(H2.lift(part(env, name, seeded(grp, s, None))).a, (env.N,))
    return out


def slot_entries(N, k):
    """the entry of w behind each of the 33 slots of block k: at k = 0 slots 29 .. 32 are U_N-1"""
    km = k - 1 if k > 0 else N - 1
    return [24 * k + s for s in range(29)] + [24 * km + 5 + c for c in range(4)]


def dense(blk, N):
    """hess L [nw, nw] from the blocks: entry by entry, overlaps added"""
    nw = 5 + 24 * N
    H = np.zeros((nw, nw), blk.dtype)
    for k in range(N):
        e = slot_entries(N, k)
        for r in range(33):
            for c in range(33):
                H[e[r], e[c]] += blk[k, r, c]
    return H


def reg_stencil(P, N, sigma=1.0):
    """The regularisation's Hessian on the controls in closed form, [4 N, 4 N] over (interval, control): sigma times the sum over the cyclic pairs
    (k - 1, k) of 2 c c^T [[1, -1], [-1, 1]] with c = d p / d U -- 0.5 for delta under penalty_delta, (0.75, 2) for the forces under penalty_F."""
    cd = np.array([US[0], 0, 0, 0], dtype=LD)
    cf = np.array([0, LD(US[1]) / 10000, LD(US[2]) / 10000, 0], dtype=LD)
    Q = 2 * (LD(P["penalty_delta"]) * np.outer(cd, cd) + LD(P["penalty_F"]) * np.outer(cf, cf)) * LD(sigma)
    H = np.zeros((4 * N, 4 * N), LD)
    for k in range(N):
        a, b = 4 * ((k - 1) % N), 4 * k
        H[a:a + 4, a:a + 4] += Q
        H[b:b + 4, b:b + 4] += Q
        H[a:a + 4, b:b + 4] -= Q
        H[b:b + 4, a:a + 4] -= Q
    return H


def hessvec(blk, N, v):
    """H v [nvec, nw] in the blocks' dtype: block by block, y[entries of block k] += block k times v[entries of block k]"""
    v = np.atleast_2d(np.asarray(v)).astype(blk.dtype)
    y = np.zeros_like(v)
    for k in range(N):
        e = slot_entries(N, k)
        y[:, e] += v[:, e] @ blk[k].T
    return y


def min_abs_ax(prob, w, opts):
    """the smallest |ax| of the path points [m/s^2] in longdouble, with the signs present: the safe rows' branch is decided by it"""
    P, arr, _ = mr.cast(prob, LD)
    N = arr["h"].shape[0]
    grp = groups_of(np.asarray(w, dtype=np.float64).astype(LD), N)
    ax = vehicle(grp[5], grp[1], arr["kappa_cl"][:-1], P, 0)["ax"]
    return float(np.min(np.abs(ax))), bool(np.any(ax > 0)), bool(np.any(ax < 0))
