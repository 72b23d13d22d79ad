"""What the device kernels around the QP are held to: guard = max(floor, 4 x spread) per case and quantity -- the rule of tests/ring_guard.py and
tests/open_ref.py.

floor: the project's existing assertion for the quantity (tests/test_gpu_parity.py, tests/test_emu_kernels.py); nobody picked a number here.
spread: how far the REFERENCE's answer is determined.
  geometry (raceline, re-linearisation, prep): the larger of (i) the float64 run of tests/glue_ref.py against its longdouble run and (ii) the
    longdouble run's movement under SPREAD_DRAWS draws of a relative SPREAD_REL perturbation of its inputs (rows, normals, alpha);
  velocity profiles: oracle/vel_ref.py's movement under the same draws on kappa, el_lengths and mu (a sweep decides with `<` on computed
    speeds: a handful of cases flip a decision under an ulp -- the guard has to know which).
Spreads are written by scripts/make_golden_glue_spread.py into tests/golden/glue_spread.npz (one array per launch); the expected VALUES are
computed live.  A guard widens only through a recomputed spread there; tests/test_glue_ref.py recomputes entries and asserts the caps."""
import functools
import os

import numpy as np

import glue_cases as gc
import glue_ref
from ring_guard import SPREAD_DRAWS, SPREAD_REL, draw_rng

LD = np.longdouble
PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "glue_spread.npz")
FLOOR = dict(xy=1e-9, psi=1e-10, kappa=1e-11, el=1e-9, prep_normals=1e-10, prep_scalings=1e-12, relin_rows=1e-9, relin_normals=1e-9,
             vx=1e-9, lap=1e-9)
RACE_Q = ("xy", "psi", "kappa", "el")
RELIN_Q = ("relin_rows", "relin_normals")
PREP_Q = ("prep_normals", "prep_scalings")
VEL_Q = ("vx", "lap")


def guard(quantity, spread):
    return max(FLOOR[quantity], 4.0 * float(spread))


def dmax(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a.astype(LD) - b.astype(LD)))) if a.size else 0.0


def dpsi(a, b):
    """Largest heading difference modulo 2 pi."""
    d = np.abs(np.asarray(a).astype(LD) - np.asarray(b).astype(LD))
    two_pi = 2 * glue_ref.pi_of(LD)
    d = np.minimum(d, np.abs(two_pi - d))
    return float(np.max(d)) if d.size else 0.0


# ---- the runs of the reference on one ring: 0 = longdouble (THE reference), 1 = float64, 2 .. = longdouble on perturbed inputs -----------------
N_RUNS = 2 + SPREAD_DRAWS


def _perturb(a, rng):
    a = np.asarray(a, dtype=LD)
    return a * (LD(1) + LD(SPREAD_REL) * rng.standard_normal(a.shape).astype(LD))


@functools.lru_cache(maxsize=None)
def ring_run(family, n, run):
    """(dtype, ref, nv, alpha) of one run."""
    ref, nv, al = gc.ring(family, n)
    if run == 0:
        return LD, ref, nv, al
    if run == 1:
        return np.float64, ref, nv, al
    rng = draw_rng("glue/" + family, "ring", n, run - 2)
    return LD, _perturb(ref, rng), _perturb(nv, rng), _perturb(al, rng)


@functools.lru_cache(maxsize=256)
def front(family, n, alpha_scale, run):
    dt, ref, nv, al = ring_run(family, n, run)
    return glue_ref.front(ref, nv, al, dt, alpha_scale=alpha_scale)


def raceline_ref(family, n, stepsize):
    """The longdouble reference of one row of a raceline launch."""
    return glue_ref.stations(front(family, n, 1.0, 0), stepsize)


def relin_ref(family, n, alpha_scale, stepsize):
    return glue_ref.resample(front(family, n, alpha_scale, 0), stepsize)


@functools.lru_cache(maxsize=None)
def prep_ref(family, n):
    return glue_ref.prep(gc.ring(family, n)[0][:, :2], LD)


def _race_dev(a, b):
    return [dmax(a["xy"], b["xy"]), dpsi(a["psi"], b["psi"]), dmax(a["kappa"], b["kappa"]), dmax(a["el_lengths"], b["el_lengths"])]


def compute_raceline_spread(family, launch):
    """[rows, 4] (RACE_Q) of one launch of gc.raceline_launches(family); rows without stations (m < 2) hold zeros."""
    _, sizes, stepsize, _ = launch
    out = np.zeros((len(sizes), 4))
    for k, n in enumerate(sizes):
        r0 = raceline_ref(family, n, stepsize)
        if r0["m"] < 2:
            continue
        for run in range(1, N_RUNS):
            r = glue_ref.stations(front(family, n, 1.0, run), stepsize)
            assert r["m"] == r0["m"]
            out[k] = np.maximum(out[k], _race_dev(r, r0))
    return out


def compute_relin_spread(family, launch):
    """[rows, 2] (RELIN_Q) of one launch of gc.relin_launches(family)."""
    _, sizes, alpha_scale, stepsize, _ = launch
    out = np.zeros((len(sizes), 2))
    for k, n in enumerate(sizes):
        r0 = relin_ref(family, n, alpha_scale, stepsize)
        if r0["m"] < 3:
            continue
        for run in range(1, N_RUNS):
            r = glue_ref.resample(front(family, n, alpha_scale, run), stepsize)
            assert r["m"] == r0["m"]
            out[k] = np.maximum(out[k], [dmax(r["rows"], r0["rows"]), dmax(r["normals"], r0["normals"])])
    return out


def compute_prep_spread(family):
    """[len(SIZES), 2] (PREP_Q)."""
    out = np.zeros((len(gc.SIZES), 2))
    for k, n in enumerate(gc.SIZES):
        nv0, s0 = prep_ref(family, n)
        xy = gc.ring(family, n)[0][:, :2]
        runs = [glue_ref.prep(xy, np.float64)]
        runs += [glue_ref.prep(_perturb(xy, draw_rng("glue/" + family, "prep", n, d)), LD) for d in range(SPREAD_DRAWS)]
        for nv, s in runs:
            out[k] = np.maximum(out[k], [dmax(nv, nv0), dmax(s, s0)])
    return out


# ---- velocity profiles -----------------------------------------------------------------------------------------------------------------------
def vel_row(L, v):
    """(track row, valid entries) of variant v of a launch."""
    t = int(L["track_of"][v])
    return t, (L["kappa"].shape[1] if L["n_of_track"] is None else int(L["n_of_track"][t]))


def vel_ref_case(L, v, rng=None):
    """(vx [n], lap time) of variant v by oracle/vel_ref.py, or None where the kernel documents NaN (n < 2, n > nmax); rng: one draw of the
    relative perturbation of kappa, el_lengths and mu."""
    from oracle import vel_ref
    t, n = vel_row(L, v)
    if n < 2 or n > L["kappa"].shape[1]:
        return None
    kap, el = L["kappa"][t, :n], L["el"][t, :n]
    mu = None if L["mu"] is None else L["mu"][t, :n]
    if rng is not None:
        kap = kap * (1.0 + SPREAD_REL * rng.standard_normal(n))
        el = el * (1.0 + SPREAD_REL * rng.standard_normal(n))
        mu = None if mu is None else mu * (1.0 + SPREAD_REL * rng.standard_normal(n))
    fw = L["filt_window"]
    vx = vel_ref.calc_vel_profile(ax_max_machines=L["axm"][v], kappa=kap, el_lengths=el, closed=True, drag_coeff=float(L["drag"][v]),
                                  m_veh=float(L["mass"][v]), ggv=L["ggv"][v], v_max=float(L["vmax"][v]), dyn_model_exp=L["exp"], mu=mu,
                                  filt_window=fw if fw is not None and fw > 1 else None)
    return vx, vel_ref.lap_time_stable(vx, el)


def compute_vel_spread(L, only=None):
    """[batch, 2] (VEL_Q) of one launch; only: the variants to compute (the others stay zero)."""
    bsz = L["ggv"].shape[0]
    out = np.zeros((bsz, 2))
    for v in (range(bsz) if only is None else only):
        r0 = vel_ref_case(L, v)
        if r0 is None:
            continue
        for d in range(SPREAD_DRAWS):
            r = vel_ref_case(L, v, draw_rng("glue/vel/" + L["name"], "vx", v, d))
            out[v] = np.maximum(out[v], [dmax(r[0], r0[0]), abs(r[1] - r0[1])])
    return out


# ---- the stored spreads ----------------------------------------------------------------------------------------------------------------------
def entries():
    """{key: function that recomputes the array} of everything glue_spread.npz must hold."""
    out = {}
    for f in gc.FAMILIES:
        for L in gc.raceline_launches(f):
            out["raceline/%s/%s" % (f, L[0])] = functools.partial(compute_raceline_spread, f, L)
        for L in gc.relin_launches(f):
            out["relin/%s/%s" % (f, L[0])] = functools.partial(compute_relin_spread, f, L)
        out["prep/%s" % f] = functools.partial(compute_prep_spread, f)
    for L in gc.vel_launches():
        out["vel/%s" % L["name"]] = functools.partial(compute_vel_spread, L)
    return out


_Z = None


def spread(key):
    global _Z
    if _Z is None:
        z = np.load(PATH)
        _Z = {k: z[k] for k in z.files}
    return _Z[key]
