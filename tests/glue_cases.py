"""The case tables of tests/test_emu_glue.py (SIMT interpreter) and tests/test_gpu_glue.py (MI355X): deterministic, seeded, built from
nothing but numpy and tests/glue_ref.py.  A LAUNCH is what one engine call sees (the entry points take one stepsize / horizon / option set
per call), a CASE one row of it; the reference says for every row what has to come back, statuses included.

Rings.  Three families of smooth closed curves, every family at every waypoint count of SIZES, sampled at a fixed nominal spacing so that a
family's rings share their stepsizes:  trefoil (non-convex, around the origin, 1.5 m), peanut (non-convex, 1.0 m), stadium (two straights --
curvature zero along them -- and two half circles, centred at (1000, -2000) m, 10 m: the spacing that keeps the curvature of a ring THERE
determined to the 1e-11 1/m floor, tests/glue_guard.py).  Widths 2.6 .. 3.4 m; alpha: two harmonics of about 12 and 30 waypoints'
wavelength, 0.6 m at most -- smooth, like a QP result -- and normals of the distance-scaled spline (glue_ref.prep in float64)."""
import functools
import math

import numpy as np

import glue_ref

LD = np.longdouble
SIZES = (3, 4, 5, 7, 47, 48, 49, 71, 72, 73, 95, 96, 97, 98, 143, 144, 145, 255, 256, 257, 511, 512, 513, 2047, 2048, 2049, 2600,
         4095, 4096, 4097)
FAMILIES = {"trefoil": 1.5, "peanut": 1.0, "stadium": 10.0}        # nominal waypoint spacing, m
INTEGER_GAP = 1e-6          # total / stepsize of every row of a launch stays this far from every integer (longdouble reference)
MARGIN_MIN = 1e-9           # crossing cases: every pair's margin (glue_ref.normals_crossing)
BAD_INPUT = 4               # MCQ_BAD_INPUT


def _seed(*key):
    s = "/".join(str(k) for k in key)
    return np.random.default_rng([sum((i + 1) * ord(c) for i, c in enumerate(s)), len(s)])


def _curve(family, n):
    h = FAMILIES[family]
    if family == "stadium":
        per = n * h
        ls = (0.3 if n >= 8 else 0.08) * per        # (a thin triangle would put cusps into the spline through 3 .. 7 waypoints)
        r = (per - 2.0 * ls) / (2.0 * math.pi)
        s = (np.arange(n) + 0.37) * h            # arclength of the waypoints (the 0.37 keeps them off the straight / arc junctions)
        xy = np.zeros((n, 2))
        for k, sk in enumerate(s):
            if sk < ls:
                xy[k] = (sk - ls / 2.0, -r)
            elif sk < ls + math.pi * r:
                a = (sk - ls) / r
                xy[k] = (ls / 2.0 + r * math.sin(a), -r * math.cos(a))
            elif sk < 2.0 * ls + math.pi * r:
                xy[k] = (ls / 2.0 - (sk - ls - math.pi * r), r)
            else:
                a = (sk - 2.0 * ls - math.pi * r) / r
                xy[k] = (-ls / 2.0 - r * math.sin(a), r * math.cos(a))
        return xy + np.array([1000.0, -2000.0])
    th = 2.0 * math.pi * (np.arange(n) + 0.21) / n
    k, a = (3, 0.35) if family == "trefoil" else (2, 0.45)         # a (k^2 - 1) > 1: not convex
    shape = 1.0 + a * np.cos(k * th)
    # radius from the curve's own length at unit size (fine polygon), so that the mean spacing is the nominal one
    tf = np.linspace(0.0, 2.0 * math.pi, 20001)
    rf = 1.0 + a * np.cos(k * tf)
    unit = float(np.sum(np.hypot(np.diff(rf * np.cos(tf)), np.diff(rf * np.sin(tf)))))
    R = n * h / unit
    return R * np.column_stack((shape * np.cos(th), shape * np.sin(th)))


@functools.lru_cache(maxsize=None)
def ring(family, n):
    """(reftrack [n, 4], normvec [n, 2], alpha [n]) of one ring."""
    xy = _curve(family, n)
    rng = _seed("ring", family, n)
    i = np.arange(n)
    ph = rng.uniform(0.0, 2.0 * math.pi, 4)
    k1, k2 = max(1, round(n / 12.0)), max(1, round(n / 30.0))
    if n < 8:
        k1 = k2 = 1
    alpha = 0.4 * np.sin(2.0 * math.pi * k1 * i / n + ph[0]) + 0.2 * np.sin(2.0 * math.pi * k2 * i / n + ph[1])
    wr = 3.0 + 0.4 * np.sin(2.0 * math.pi * k2 * i / n + ph[2])
    wl = 3.0 + 0.4 * np.cos(2.0 * math.pi * k2 * i / n + ph[3])
    nv, _ = glue_ref.prep(xy, np.float64)
    ref = np.column_stack((xy, wr, wl))
    for a in (ref, nv, alpha):
        a.setflags(write=False)
    return ref, nv, alpha


@functools.lru_cache(maxsize=None)
def ring_total(family, n, alpha_scale=1.0):
    """Raceline length of a ring in the longdouble reference."""
    ref, nv, al = ring(family, n)
    return glue_ref.front(ref, nv, al, LD, alpha_scale=alpha_scale)["total"]


def _settle(family, sizes, stepsize, alpha_scale=1.0):
    """The stepsize, multiplied by 1.001 until total / stepsize of every ring of the launch is INTEGER_GAP away from every integer."""
    for _ in range(50):
        r = [ring_total(family, n, alpha_scale) / LD(stepsize) for n in sizes]
        if all(abs(x - np.rint(x)) >= INTEGER_GAP for x in r):
            return float(stepsize)
        stepsize = float(stepsize) * 1.001
    raise RuntimeError("no stepsize found")


def _count(family, n, stepsize, alpha_scale=1.0):
    return int(math.ceil(ring_total(family, n, alpha_scale) / LD(stepsize)))


SMALL = tuple(n for n in SIZES if n <= 513)


@functools.lru_cache(maxsize=None)
def raceline_launches(family):
    """[(name, sizes, stepsize, mmax)]: mcq_raceline_device over the rings `sizes` of the family.  Generous launches at 1.37 / 0.61 times the
    spacing and at the reference's 2.0 / 3.0 m (mmax = the largest count: that ring sits at m == mmax); launches aimed at one ring K:
    m == mmax, m == mmax + 1 (MCQ_BAD_INPUT), m == 3, m == 2 and m == 1 (MCQ_BAD_INPUT), the other rings of the launch get what they get."""
    h = FAMILIES[family]
    out = []
    for tag, s in (("1.37h", 1.37 * h), ("0.61h", 0.61 * h), ("2.0", 2.0), ("3.0", 3.0)):
        s = _settle(family, SIZES, s)
        out.append((tag, SIZES, s, max(2, max(_count(family, n, s) for n in SIZES))))
    for K, sizes in ((97, SMALL), (2049, SIZES)):
        s = _settle(family, sizes, float(ring_total(family, K)) / (0.71 * K - 0.5))
        mK = _count(family, K, s)
        out.append(("m==mmax@%d" % K, sizes, s, mK))
        s1 = _settle(family, sizes, float(ring_total(family, K)) / (mK + 0.5))
        assert _count(family, K, s1) == mK + 1
        out.append(("m==mmax+1@%d" % K, sizes, s1, mK))
    for K in (3, 96, 4097):
        sizes = SMALL if K <= 513 else SIZES
        for m in (3, 2, 1):
            s = _settle(family, sizes, float(ring_total(family, K)) / (m - 0.5))
            assert _count(family, K, s) == m
            out.append(("m==%d@%d" % (m, K), sizes, s, max(2, max(_count(family, n, s) for n in sizes))))
    return out


@functools.lru_cache(maxsize=None)
def relin_launches(family):
    """[(name, sizes, alpha_scale, stepsize, nmax)]: mcq_relinearise_device.  nmax is the stride of inputs AND outputs, so the 0.61 h launch
    overflows for the long rings by itself (MCQ_BAD_INPUT, n_out == n); aimed launches put ring K at m == nmax, nmax + 1, 3 and 2."""
    h = FAMILIES[family]
    out = []
    for tag, s, sc in (("1.37h", 1.37 * h, 1.0), ("0.61h", 0.61 * h, 1.0 / 3.0), ("2.0", 2.0, 1.0), ("3.0", 3.0, 1.0 / 3.0)):
        out.append((tag, SIZES, sc, _settle(family, SIZES, s, sc), max(SIZES)))
    for K, sizes, nmax, sc in ((513, SMALL, 600, 1.0), (4095, SIZES, 4097, 1.0 / 3.0)):
        for m in (nmax, nmax + 1):
            s = _settle(family, sizes, float(ring_total(family, K, sc)) / (m - 0.5), sc)
            assert _count(family, K, s, sc) == m
            out.append(("m==%d@%d" % (m, K), sizes, sc, s, nmax))
    for K in (3, 98):
        for m in (3, 2):
            s = _settle(family, SMALL, float(ring_total(family, K)) / (m - 0.5))
            assert _count(family, K, s) == m
            out.append(("m==%d@%d" % (m, K), SMALL, 1.0, s, max(SMALL)))
    return out


# ---- velocity profiles ---------------------------------------------------------------------------------------------------------------------
VEL_N = (2, 3, 5, 17, 63, 64, 65, 130, 257, 400, 2048)
VEL_EXP = (1.0, 1.5, 2.0)
VEL_SEEDS = {"b1000": 1, "n257": 1}              # launch -> seed (default 0): tuned until tests/test_glue_ref.py's caps hold on the reference alone


def _profile(kind, n, rng):
    i = np.arange(n)
    if kind == "smooth":
        k = 0.012 + 0.02 * np.sin(2.0 * math.pi * i / max(n, 8) * 2 + rng.uniform(0, 6)) ** 2 + 0.01 * np.cos(2.0 * math.pi * i / max(n, 8) * 5)
    elif kind == "random":
        k = rng.uniform(0.002, 0.06, n)
    elif kind == "zeros":                    # exact zeros: infinite radius, the lateral limit runs its 100 rounds
        k = 0.03 * np.sin(2.0 * math.pi * i / max(n, 8) * 1.5 + rng.uniform(0, 6))
        k[rng.uniform(size=n) < 0.3] = 0.0
        k[0] = 0.0
    else:                                    # sign changes
        k = 0.04 * np.sin(2.0 * math.pi * i / max(n, 8) * 3 + rng.uniform(0, 6)) + rng.uniform(-0.004, 0.004, n)
    return k


KINDS = ("smooth", "random", "zeros", "signs")


def _vehicle(rng, rows, on_grid):
    """(ggv [rows, 3], ax_max_machines [6, 2], drag, mass, v_max): a random speed-dependent diagram."""
    vtop = 72.0
    if rows == 1:
        v = np.array([vtop])
    else:
        v = np.linspace(0.0, vtop, rows)
    ax = rng.uniform(8.0, 14.0) + rng.uniform(-0.05, 0.05) * v + rng.uniform(-0.5, 0.5, rows)
    ay = rng.uniform(8.0, 14.0) + rng.uniform(-0.06, 0.1) * v + rng.uniform(-0.5, 0.5, rows)
    ggv = np.column_stack((v, ax, ay))
    vm = np.linspace(0.0, vtop, 7)
    axm = np.column_stack((vm, np.interp(vm, [0.0, 20.0, 72.0], [rng.uniform(4.0, 7.0), rng.uniform(3.5, 5.5), rng.uniform(0.8, 2.0)])))
    if on_grid:                             # exactly on a grid point of the diagram (19 rows: 4 m/s apart)
        vmax = float(v[int(rng.integers(8, 17))]) if rows == 19 else vtop
    else:
        vmax = float(rng.uniform(28.0, 66.0))
    return ggv, axm, float(rng.uniform(0.5, 0.9)), float(rng.uniform(800.0, 1300.0)), vmax


def _vel_launch(name, ns, nmax, batch, rows, e, mu, fw, tracks_per_n=4, seed_extra=0, wild=False):
    """One launch: `tracks_per_n` profiles per entry of ns (kinds cycling; el uniform / non-uniform alternating) in rows of nmax, `batch`
    variants mapped onto them many-to-one in shuffled order.  wild: radii of 20 .. 2000 m in long swings and element lengths of 0.5 .. 500 m, independent
    from point to point -- a sweep that has run past v_max on a long element stays switched off until the next acceleration phase STARTS, however
    the profile rises in between (the gating on prev_rising; gentle profiles never show it)."""
    rng = _seed("vel", name, VEL_SEEDS.get(name, 0), seed_extra)
    nt = []
    for n in ns:
        nt += [n] * tracks_per_n
    T = len(nt)
    kappa = np.zeros((T, nmax))
    el = np.ones((T, nmax))
    muv = np.ones((T, nmax)) if mu else None
    for t, n in enumerate(nt):
        if n < 2 or n > nmax:
            continue
        kappa[t, :n] = _profile(KINDS[t % 4], n, rng) * (1.0, 0.25, 0.05)[(t + t // 4) % 3]     # tight .. fast: the last ones run into v_max
        el[t, :n] = 2.0 if (t // 4 + t) % 2 == 0 else 2.0 * (1.0 + 0.3 * np.sin(0.7 * np.arange(n) + t))
        if wild:
            kappa[t, :n] = 10.0 ** (-2.3 + np.sin(2.0 * math.pi * np.arange(n) / n * (1 + t % 3) + rng.uniform(0, 6)) + rng.uniform(-0.05, 0.05, n)) \
                * rng.choice([-1.0, 1.0], n)
            el[t, :n] = 10.0 ** rng.uniform(-0.3, 2.7, n)
        if mu:
            muv[t, :n] = 0.9 + 0.2 * np.cos(2.0 * math.pi * np.arange(n) / n * 3.0 + t)
    track_of = np.concatenate([rng.permutation(T) for _ in range(batch // T + 1)])[:batch].astype(np.int32)
    veh = [_vehicle(rng, rows, on_grid=(k % 3 == 0)) for k in range(batch)]
    uniform = len(set(nt)) == 1 and nt[0] == nmax
    return dict(name=name, kappa=kappa, el=el, mu=muv, n_of_track=None if uniform else np.array(nt, dtype=np.int32), track_of=track_of,
                ggv=np.stack([v[0] for v in veh]), axm=np.stack([v[1] for v in veh]), drag=np.array([v[2] for v in veh]),
                mass=np.array([v[3] for v in veh]), vmax=np.array([v[4] for v in veh]), exp=e, filt_window=fw)


@functools.lru_cache(maxsize=None)
def vel_launches():
    out = []
    batches = (1, 63, 64, 65, 129, 12, 12, 8, 8, 6, 4)
    for k, n in enumerate(VEL_N):                        # uniform rows: every profile length, the batches around the 64-thread block
        rows, e = (1, 2, 19)[k % 3], VEL_EXP[(k + k // 3) % 3]          # every pairing of the two over the eleven launches but one:
        if rows == 1 and e == 2.0:
            # EXCLUDED on purpose: with one ggv row the lateral limit does not depend on the speed, a sweep that starts at an apex evaluates
            # sqrt(1 - (ay_used / ay_max)^2) exactly AT the limit, and the radicand is +-1e-16 by construction -- 1.7e-7 m/s^2 or 0, 2e-8 m/s
            # on the next point, in the oracle itself (docs/NOTEBOOK.md).  The reference has no answer to the 1e-9 floor there; two rows
            # (a diagram linear in the speed) keep exponent 2 away from that point.
            rows = 2
        out.append(_vel_launch("n%d" % n, (n,), n, batches[k], rows, e, mu=(k % 2 == 1), fw=None, tracks_per_n=4 if n < 2048 else 2))
    out.append(_vel_launch("b1000", (17,), 17, 1000, 19, 1.5, mu=False, fw=None))
    for n in (3, 5, 17, 63, 65, 257):                    # filt_window == n
        out.append(_vel_launch("fw==n%d" % n, (n,), n, 6, 19, VEL_EXP[n % 3], mu=(n % 2 == 1), fw=n))
    # ragged rows together with mu and filt_window: the _opts entry with all three
    out.append(_vel_launch("ragged_fw1", (2, 3, 5, 17, 63, 64, 65, 130), 130, 65, 19, 1.5, mu=True, fw=1))
    out.append(_vel_launch("ragged_fw3", (3, 5, 17, 63, 64, 65, 130), 130, 63, 2, 1.0, mu=True, fw=3))
    out.append(_vel_launch("ragged_fw7", (17, 63, 64, 65, 130), 130, 40, 19, 1.5, mu=True, fw=7))
    out.append(_vel_launch("ragged_plain", (2, 3, 5, 17, 63, 64, 65), 65, 64, 1, 1.5, mu=False, fw=None))
    out.append(_vel_launch("gates", (40,), 40, 64, 19, 1.0, mu=False, fw=None, tracks_per_n=8, wild=True))
    out.append(_vel_launch("gates_mu", (23, 40), 40, 48, 2, 1.5, mu=True, fw=None, tracks_per_n=4, wild=True))
    # rows of 1 and of more than nmax entries: the documented NaN lap time and NaN row
    out.append(_vel_launch("nan_rows", (1, 5, 64, 66, 17), 65, 40, 19, 1.0, mu=True, fw=1, tracks_per_n=2))
    return out


def vel_case_count():
    return sum(L["ggv"].shape[0] for L in vel_launches())


# ---- normals crossing ----------------------------------------------------------------------------------------------------------------------
CROSS_N = (11, 12, 255, 256, 257, 600)


def _circle_track(n, radius, width, seed):
    rng = _seed("cross", n, seed)
    th = 2.0 * math.pi * (np.arange(n) + 0.13) / n
    r = radius * (1.0 + 0.1 * np.cos(2 * th + rng.uniform(0, 6)))
    xy = np.column_stack((r * np.cos(th), r * np.sin(th)))
    nv, _ = glue_ref.prep(xy, np.float64)
    return np.column_stack((xy, np.full(n, width) * rng.uniform(0.9, 1.1, n), np.full(n, width) * rng.uniform(0.9, 1.1, n))), nv


def _rot(v, a):
    c, s = math.cos(a), math.sin(a)
    return np.array([c * v[0] - s * v[1], s * v[0] + c * v[1]])


def _wrap_only(n):
    """A crossing between waypoint n - 2 and waypoint 1 and nowhere else: their normals are turned towards each other, everybody else's
    segment is too short to reach them."""
    trk, nv = _circle_track(n, 0.2 * n, 0.05, 7)
    trk, nv = trk.copy(), nv.copy()
    a, b = n - 2, 1
    mid = 0.5 * (trk[a, :2] + trk[b, :2])
    inward = -mid / np.linalg.norm(mid)
    apex = mid + 1.2 * np.linalg.norm(trk[b, :2] - trk[a, :2]) * inward
    for k in (a, b):
        d = apex - trk[k, :2]
        nv[k] = -d / np.linalg.norm(d)              # the normal points right (outwards here): the apex lies on the w_left side
        trk[k, 2] = 0.0
        trk[k, 3] = 1.5 * np.linalg.norm(d)
    return trk, nv


def _parallel(n, angle):
    """Two neighbours whose normals enclose `angle` (around the 1e-8 collinearity skip), the second waypoint sitting ON the first one's normal:
    not skipped, the pair is a hit at l0 = 0.5, l1 = 0."""
    trk, nv = _circle_track(n, 0.2 * n, 0.05, 11)
    trk, nv = trk.copy(), nv.copy()
    k = n // 3
    trk[k, 2:] = 1.0
    trk[k + 1, 2:] = 1.0
    trk[k + 1, :2] = trk[k, :2] + 0.5 * nv[k]
    nv[k + 1] = _rot(nv[k], angle)
    return trk, nv


def _exact(n, ulp_down):
    """Exact arithmetic on the inclusive bound: waypoints on a grid 128 m apart, axis-parallel normals, widths 0.25 -- no pair comes near --
    except waypoints 4 and 5: p4 + l0 (1, 0) = p5 + l1 (0, 1) at l0 = 2, l1 = 1 with w_right(4) = 2 exactly (a hit), or one ulp less (none)."""
    trk = np.zeros((n, 4))
    nv = np.zeros((n, 2))
    for k in range(n):
        trk[k] = (1024.0 + 128.0 * k, 1024.0, 0.25, 0.25)
        nv[k] = (1.0, 0.0) if k % 2 == 0 else (0.0, 1.0)
    trk[5, :2] = trk[4, :2] + np.array([2.0, -1.0])
    trk[4, 2] = np.nextafter(2.0, 0.0) if ulp_down else 2.0
    trk[5, 2] = 1.5
    return trk, nv


@functools.lru_cache(maxsize=None)
def crossing_cases():
    """[(name, track, normvec, exact)]; exact: decided ON a bound (margin 0 by construction), every other case has margins above MARGIN_MIN
    at every horizon of crossing_horizons() -- a case that has not is rebuilt from the next seed here, never dropped at test time."""
    out = []
    for n in CROSS_N:
        for tag, width in (("narrow", 0.02 * n), ("wide", 0.35 * n)):
            for seed in range(20):
                trk, nv = _circle_track(n, 0.2 * n, width, seed)
                if all(glue_ref.normals_crossing(trk, nv, hz, LD)[1] > MARGIN_MIN for hz in crossing_horizons() if hz < n):
                    break
            else:
                raise RuntimeError("no seed gives a decided case")
            out.append(("%s%d" % (tag, n), trk, nv, False))
    for n in (255, 256, 600):
        out.append(("wrap_only%d" % n, *_wrap_only(n), False))
    for n in (11, 255):
        out.append(("parallel2e-8_%d" % n, *_parallel(n, 2e-8), False))
        out.append(("parallel5e-9_%d" % n, *_parallel(n, 5e-9), False))
    for n in (11, 256):
        out.append(("on_bound%d" % n, *_exact(n, False), True))
        out.append(("ulp_inside%d" % n, *_exact(n, True), True))
    return out


def crossing_horizons():
    return tuple(sorted({1, 10} | {n - 1 for n in CROSS_N} | set(CROSS_N)))


# ---- fp32 boundary -------------------------------------------------------------------------------------------------------------------------
F32_SHAPES = ((1, 3), (3, 333), (5, 63), (7, 64), (2, 65), (3, 777), (1, 2049))      # batch x n = 3, 3, 3, 0, 2, 3, 1 modulo 4
F32_KAPPA_BOUND, F32_W_VEH = 1.0, 2.0


@functools.lru_cache(maxsize=None)
def f32_tracks(batch, n):
    """fp64 rows [batch, n, 4] of `batch` different rings of n waypoints (the families in turn, shifted per track)."""
    fams = tuple(FAMILIES)
    rows = []
    for k in range(batch):
        ref = np.array(ring(fams[k % 3], n)[0])
        ref[:, :2] += np.array([37.0 * k, -53.0 * k])
        ref[:, 2:] += 0.01 * k
        rows.append(ref)
    return np.stack(rows)
