"""What the new forms of the velocity profile kernel are held to: the rule and the numbers of tests/glue_guard.py, nothing new --
guard = max(floor, 4 x spread) with glue_guard.FLOOR (vx 1e-9 m/s, lap 1e-9 s), spread = oracle/vel_ref.py's movement under SPREAD_DRAWS draws
of a relative SPREAD_REL (tests/ring_guard.py) on kappa, el_lengths, mu and loc_gg.  Spreads are written by
scripts/make_golden_vel_forms_spread.py into tests/golden/vel_forms/vel_forms_spread.npz (one [batch, 2] array per kind and launch that is compared; a
folder of its own: every .npz directly under tests/golden/ is a ring fixture to tests/test_ring_guard.py and must have an entry in ring_spread.npz); the expected VALUES are computed live.  tests/test_vel_forms_ref.py recomputes entries and asserts the caps."""
import functools
import os

import numpy as np

import glue_guard as gg
import vel_forms_cases as fc
from ring_guard import SPREAD_DRAWS, SPREAD_REL, draw_rng

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vel_forms", "vel_forms_spread.npz")
FLOOR, VEL_Q, guard, dmax = gg.FLOOR, gg.VEL_Q, gg.guard, gg.dmax


def lap_time_open(vx, el):
    """Time over the n - 1 elements of an unclosed profile by the stable sum 2 l / (v_a + v_b) (oracle/vel_ref.lap_time_stable is the closed one);
    +inf where the profile stands at both ends of an element."""
    with np.errstate(divide="ignore"):
        return float(np.sum(2.0 * el / (vx[:-1] + vx[1:])))


def ref_case(F, v, rng=None):
    """(vx [n], time) of variant v of a forms launch by oracle/vel_ref.py, or None where the kernel documents NaN (n < 2, n > nmax); rng: one
    draw of the relative perturbation of kappa, el_lengths, mu and loc_gg."""
    from oracle import vel_ref
    t, n = fc.row(F, v)
    if n < 2 or n > F["kappa"].shape[1]:
        return None
    closed = F["closed"]
    kap, el = F["kappa"][t, :n], F["el"][t, :n if closed else n - 1]
    mu = None if F["mu"] is None else F["mu"][t, :n]
    lg = None if F["loc_gg"] is None else F["loc_gg"][t, :n]
    if rng is not None:
        kap = kap * (1.0 + SPREAD_REL * rng.standard_normal(n))
        el = el * (1.0 + SPREAD_REL * rng.standard_normal(el.size))
        mu = None if mu is None else mu * (1.0 + SPREAD_REL * rng.standard_normal(n))
        lg = None if lg is None else lg * (1.0 + SPREAD_REL * rng.standard_normal((n, 2)))
    fw = F["filt_window"]
    ve = None if closed or F["v_end"] is None or np.isnan(F["v_end"][v]) else float(F["v_end"][v])
    vx = vel_ref.calc_vel_profile(ax_max_machines=F["axm"][v], kappa=kap, el_lengths=el, closed=closed, drag_coeff=float(F["drag"][v]),
                                  m_veh=float(F["mass"][v]), ggv=None if lg is not None else F["ggv"][v], loc_gg=lg, v_max=float(F["vmax"][v]),
                                  dyn_model_exp=F["exp"], mu=mu, v_start=None if closed else float(F["v_start"][v]), v_end=ve,
                                  filt_window=fw if fw is not None and fw > 1 else None)
    return vx, (vel_ref.lap_time_stable(vx, el) if closed else lap_time_open(vx, el))


def _dlap(a, b):
    return 0.0 if a == b else abs(a - b)            # (+inf on both sides: no movement)


def compute_spread(F, only=None):
    """[batch, 2] (VEL_Q) of one forms launch; only: the variants to compute (the others stay zero).  Launches that are not compared with the
    oracle (fc: parity False) have no spread."""
    bsz = F["ggv"].shape[0]
    out = np.zeros((bsz, 2))
    if not F["parity"]:
        return out
    for v in (range(bsz) if only is None else only):
        r0 = ref_case(F, v)
        if r0 is None:
            continue
        for d in range(SPREAD_DRAWS):
            r = ref_case(F, v, draw_rng("velforms/%s/%s" % (F["kind"], F["name"]), "vx", v, d))
            out[v] = np.maximum(out[v], [dmax(r[0], r0[0]), _dlap(r[1], r0[1])])
    return out


def key(F):
    return "%s/%s" % (F["kind"], F["name"])


def entries():
    """{key: function that recomputes the array} of everything vel_forms_spread.npz must hold."""
    return {key(F): functools.partial(compute_spread, F) for _, F in fc.all_launches() if F["parity"]}


_Z = None


def spread(k):
    global _Z
    if _Z is None:
        z = np.load(PATH)
        _Z = {q: z[q] for q in z.files}
    return _Z[k]
