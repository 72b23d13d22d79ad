"""Hand-made cases for the mcq_mintime_* entries (include/mcq.h): the smallest shapes at which the kernels of csrc/mcq_mintime.inc can go wrong.

Interval counts: N = 2 (one actuator row; the regularisation wraps between two intervals), 3, 7 / 8 (256 lanes hold 7.1 intervals of the Jacobian's
36 lanes: the first interval that straddles two workgroups), 63 / 64 / 65 (64 intervals of the evaluation's 4 lanes fill a workgroup), 255 / 256 /
257 (its fourth workgroup edge, and the 256 partial sums of the ordered sum all used / one used twice), 1025.  Options: each alone and all together
at N = 5; friction none, linear, gauss at n_gauss 1 and 5.  w: seeded random values inside RANGES (below), and physically meant w's built from the
engine's own minimum-curvature flow on rounded_rectangle and Berlin (flow_problem).  Every case is DECIDED (tests/test_mintime_ref.py asserts it): each denominator of the model stays at least a factor 4
from zero -- RANGES keep |gamma_y| and braking moderate so that no wheel load approaches zero."""
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# the vehicle of the cases (hand-made: a 1.2 t racing car), varied per problem by vary()
PARS = dict(mass=1180.0, dragcoeff=0.8, g=9.81, v_max=72.0,
            wheelbase_front=1.55, wheelbase_rear=1.45, track_width_front=1.62, track_width_rear=1.58, cog_z=0.4, I_z=1250.0, liftcoeff_front=0.5,
            liftcoeff_rear=0.7, k_brake_front=0.6, k_drive_front=0.1, k_roll=0.55, t_delta=0.2, t_drive=0.05, t_brake=0.06, power_max=240000.0,
            f_drive_max=7100.0, f_brake_max=19000.0, delta_max=0.36,
            c_roll=0.012, f_z0=3100.0, B_front=9.5, C_front=2.4, eps_front=-0.1, E_front=0.9, B_rear=10.5, C_rear=2.6, eps_rear=-0.12, E_rear=1.0,
            width_opt=3.2, mue=1.05, penalty_F=0.012, penalty_delta=9.0, energy_limit=1.9, ax_pos_safe=9.0, ax_neg_safe=11.0, ay_safe=10.0)

# scaled decision variables: v 20 .. 50 m/s, beta +- 0.025 rad, omega_z +- 0.2 rad/s, n +- 1.5 m, xi +- 0.05 rad, delta +- 0.05 rad,
# f_drive 0 .. 3750 N, f_brake -4000 .. 0 N, gamma_y +- 1500 N
RANGES = dict(x=((0.4, 1.0), (-0.05, 0.05), (-0.2, 0.2), (-0.3, 0.3), (-0.05, 0.05)), u=((-0.1, 0.1), (0.0, 0.5), (-0.2, 0.0), (-0.3, 0.3)))

OPTIONS = {"plain": dict(), "safe": dict(safe_traj=True), "energy": dict(limit_energy=True), "linear": dict(friction="linear"),
           "gauss1": dict(friction="gauss", n_gauss=1), "gauss5": dict(friction="gauss", n_gauss=5),
           "all": dict(friction="gauss", n_gauss=5, safe_traj=True, limit_energy=True)}
SIZES = (2, 3, 7, 8, 63, 64, 65, 255, 256, 257, 1025)


def vary(seed):
    rng = np.random.default_rng(1000 + seed)
    p = dict(PARS)
    for k in ("mass", "dragcoeff", "mue", "liftcoeff_rear", "cog_z", "penalty_delta", "width_opt"):
        p[k] = float(p[k] * (1.0 + 0.1 * rng.uniform(-1, 1)))
    return p


def random_w(rng, N):
    w = np.zeros(5 + 24 * N)

    def xs():
        return [rng.uniform(*r) for r in RANGES["x"]]
    w[:5] = xs()
    for k in range(N):
        o = 24 * k
        w[o + 5:o + 9] = [rng.uniform(*r) for r in RANGES["u"]]
        for j in range(3):
            w[o + 9 + 5 * j:o + 14 + 5 * j] = xs()
        w[o + 24:o + 29] = xs()
    return w


def friction_weights(rng, N, opts):
    """weights in the friction entries' layout for one track: [4, N + 1, P], center_dist [N + 1]; mue between 0.8 and 1.2"""
    if opts.get("friction") is None:
        return None, None
    if opts["friction"] == "linear":
        w = np.stack([np.stack([rng.uniform(-0.02, 0.02, N + 1), rng.uniform(0.9, 1.1, N + 1)], axis=1) for _ in range(4)])
        return w, None
    ng = opts["n_gauss"]
    w = np.concatenate([rng.uniform(-0.03, 0.03, (4, N + 1, 2 * ng + 1)), rng.uniform(0.95, 1.05, (4, N + 1, 1))], axis=2)
    return w, rng.uniform(0.2, 0.4, N + 1)


@functools.lru_cache(maxsize=None)
def problem(N, option="plain", seed=0):
    """One problem: seeded random track data, parameters and w.  Cached: shared among the tests, not to be changed."""
    opts = OPTIONS[option]
    rng = np.random.default_rng(7919 * N + 31 * seed + sorted(OPTIONS).index(option))
    kap = 0.02 * np.sin(np.linspace(0.0, 2 * np.pi, N, endpoint=False) * max(1, N // 40) + rng.uniform(0, 6)) + rng.uniform(-0.003, 0.003, N)
    wr, wl = rng.uniform(3.5, 6.0, N), rng.uniform(3.5, 6.0, N)
    wm, cd = friction_weights(rng, N, opts)
    return dict(h=rng.uniform(2.5, 3.5, N), kappa_cl=np.append(kap, kap[0]), w_tr_right_cl=np.append(wr, wr[0]), w_tr_left_cl=np.append(wl, wl[0]),
                pars=vary(seed + N), w=random_w(rng, N), w_mue=wm, center_dist=cd)


# the vehicle of the flow below: a flat 7 m/s2 diagram and machine limit (moderate: |gamma_y| and braking stay far from unloading a wheel)
FLOW_V = np.arange(0.0, 72.1, 4.0)
FLOW_GGV = np.column_stack((FLOW_V, np.full(FLOW_V.size, 7.0), np.full(FLOW_V.size, 7.0)))
FLOW_AXM = np.column_stack((FLOW_V, np.interp(FLOW_V, [0.0, 20.0, 72.0], [5.3, 5.3, 1.2])))
FLOW_V_MAX = 50.0


def _nearest_station(points, stations):
    return np.array([int(np.argmin(np.sum((stations - p) ** 2, axis=1))) for p in points])


def flow_problem(eng, reftrack, pars, kappa_bound, w_veh, stepsize=1.0):
    """A physically meant problem and w from the minimum-curvature flow ON THE ENGINE: prep (normals, scalings) -> solve (alpha) -> raceline (and the
    reference line itself as the raceline of alpha = 0: its curvature and arc length) -> velocity profile.  At every waypoint of the reference
    line, from the nearest raceline station: v from the profile, n = -alpha, xi = raceline heading - reference heading, omega_z = v kappa,
    delta = wheelbase * kappa, the drive / brake force from the profile's ax and the drag, gamma_y from v^2 kappa.  The collocation states
    interpolate the nodes.  Test input only (a guess, not a solution).  Returns (problem, dict of the flow's own numbers)."""
    ref = np.asarray(reftrack, dtype=np.float64)
    n = ref.shape[0]
    nvs, scs = eng.prep_batch([ref])
    nv = nvs[0]
    al, _, st, _ = eng.solve_batch([dict(reftrack=ref, normvec=nv, scaling=scs[0], kappa_bound=kappa_bound, w_veh=w_veh)])
    assert st[0] == 0
    alpha = al[0]
    race = eng.raceline_batch([ref, ref], [nv, nv], [alpha, np.zeros(n)], stepsize)
    assert not np.any(race["status"])
    m, m0 = int(race["m"][0]), int(race["m"][1])
    vx, lap = eng.vel_profile_batch(race["kappa"][:1, :m], race["el_lengths"][:1, :m], FLOW_GGV[None], FLOW_AXM[None], [pars["dragcoeff"]], [pars["mass"]],
                                    [FLOW_V_MAX])
    vx, el, kr, psi = vx[0], race["el_lengths"][0, :m], race["kappa"][0, :m], race["psi"][0, :m]
    ax = (np.roll(vx, -1) ** 2 - vx ** 2) / (2.0 * el)
    j = _nearest_station(ref[:, :2] + alpha[:, None] * nv, race["xy"][0, :m])
    j0 = _nearest_station(ref[:, :2], race["xy"][1, :m0])
    s0 = np.append(0.0, np.cumsum(race["el_lengths"][1, :m0]))
    s_opt = np.append(s0[j0], s0[m0])
    assert j0[0] == 0 and np.all(np.diff(s_opt) > 0)
    dpsi = psi[j] - race["psi"][1, :m0][j0]
    xi = np.arctan2(np.sin(dpsi), np.cos(dpsi))
    v, kap = vx[j], kr[j]
    force = pars["mass"] * ax[j] + pars["dragcoeff"] * v * v
    gamma = pars["mass"] * v * v * kap * pars["cog_z"] / ((pars["track_width_front"] + pars["track_width_rear"]) / 2)
    X = np.stack([v / 50.0, np.zeros(n), v * kap, -alpha / 5.0, xi], axis=1)
    U = np.stack([(pars["wheelbase_front"] + pars["wheelbase_rear"]) * kap / 0.5, np.maximum(force, 0) / 7500.0, np.minimum(force, 0) / 20000.0,
                  gamma / 5000.0], axis=1)
    Xcl = np.vstack((X, X[:1]))
    w = np.zeros(5 + 24 * n)
    w[:5] = X[0]
    for k in range(n):
        o = 24 * k
        w[o + 5:o + 9] = U[k]
        for jj, tau in enumerate((0.5 - np.sqrt(15) / 10, 0.5, 0.5 + np.sqrt(15) / 10)):
            w[o + 9 + 5 * jj:o + 14 + 5 * jj] = Xcl[k] + tau * (Xcl[k + 1] - Xcl[k])
        w[o + 24:o + 29] = Xcl[k + 1]
    k0 = race["kappa"][1, :m0][j0]
    prob = dict(h=np.diff(s_opt), s_opt=s_opt, kappa_cl=np.append(k0, k0[0]), w_tr_right_cl=np.append(ref[:, 2], ref[0, 2]),
                w_tr_left_cl=np.append(ref[:, 3], ref[0, 3]), pars=dict(pars), w=w, w_mue=None, center_dist=None)
    return prob, dict(normvec=nv, alpha=alpha, lap_time_profile=float(lap[0]), stations=m)


@functools.lru_cache(maxsize=None)
def cases():
    """{name: (option, problem)}: every size with the plain options, every option at N = 5, N = 3 and N = 65 with everything.  (The physically
    meant w is flow_problem: it needs an engine, so it is a body of tests/mintime_checks.py with its spread measured on the spot.)"""
    out = {"N%d" % N: ("plain", problem(N)) for N in SIZES}
    out.update({"N5 %s" % o: (o, problem(5, o)) for o in OPTIONS if o != "plain"})
    out["N3 all"] = ("all", problem(3, "all"))
    out["N65 all"] = ("all", problem(65, "all"))
    return out


# launches: (option, case names, nmax or None): ragged under a wider nmax, per-problem parameters that differ (vary() by size)
LAUNCHES = {"small plain": ("plain", ("N2", "N3", "N7", "N8"), None),
            "wave edges": ("plain", ("N63", "N64", "N65"), 70),
            "block edges": ("plain", ("N255", "N256", "N257"), None),
            "N1025": ("plain", ("N1025", "N2"), None),
            "all": ("all", ("N3 all", "N5 all", "N65 all"), 66)}
LAUNCHES.update({o: (o, ("N5 %s" % o,), 6) for o in OPTIONS if o not in ("plain", "all")})
