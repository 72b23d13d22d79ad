"""What the chain form of the raceline kernel is held to: guard = max(floor, 4 x spread) per row and quantity with tests/glue_guard.py's floors
(xy 1e-9 m, psi 1e-10 rad, kappa 1e-11 1/m, el 1e-9 m) -- nobody picked a number here.

spread: how far the REFERENCE's answer is determined -- the larger of (i) the float64 run of tests/race_open_ref.py against its longdouble run and
(ii) the longdouble run's movement under SPREAD_DRAWS draws of a relative SPREAD_REL perturbation (tests/ring_guard.py) of its inputs: rows,
normals, alpha and the two headings.  Spreads are written by scripts/make_golden_race_open_spread.py into
tests/golden/race_open/race_open_spread.npz (one [rows, 4] array per family and launch; a folder of its own: every .npz directly under
tests/golden/ is a ring fixture to tests/test_ring_guard.py); the expected VALUES are computed live.  tests/test_race_open_ref.py recomputes
entries."""
import functools
import os

import numpy as np

import glue_guard as gg
import race_open_cases as oc
import race_open_ref as ror
from ring_guard import SPREAD_DRAWS, SPREAD_REL, draw_rng

LD = np.longdouble
PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "race_open", "race_open_spread.npz")
FLOOR, RACE_Q, guard, dmax, dpsi = gg.FLOOR, gg.RACE_Q, gg.guard, gg.dmax, gg.dpsi
N_RUNS = 2 + SPREAD_DRAWS       # 0 = longdouble (THE reference), 1 = float64, 2 .. = longdouble on perturbed inputs


def _perturb(a, rng):
    a = np.asarray(a, dtype=LD)
    return a * (LD(1) + LD(SPREAD_REL) * rng.standard_normal(a.shape).astype(LD))


@functools.lru_cache(maxsize=256)
def front(family, n, run):
    ref, nv, al, psi_s, psi_e = oc.arc(family, n)
    if run == 0:
        return ror.front(ref, nv, al, psi_s, psi_e, LD)
    if run == 1:
        return ror.front(ref, nv, al, psi_s, psi_e, np.float64)
    rng = draw_rng("race_open/" + family, "arc", n, run - 2)
    ref, nv, al = _perturb(ref, rng), _perturb(nv, rng), _perturb(al, rng)
    psi = _perturb(np.array([psi_s, psi_e]), rng)
    return ror.front(ref, nv, al, psi[0], psi[1], LD)


def reference(family, n, stepsize):
    """The longdouble reference of one row of a launch."""
    return ror.stations(front(family, n, 0), stepsize)


def deviations(a, b):
    """RACE_Q of two results of the same m: xy, psi (modulo 2 pi), kappa, the m - 1 element lengths."""
    m = b["m"]
    return [dmax(a["xy"], b["xy"]), dpsi(a["psi"], b["psi"]), dmax(a["kappa"], b["kappa"]), dmax(a["el_lengths"][:m - 1], b["el_lengths"][:m - 1])]


def compute_spread(family, launch):
    """[rows, 4] (RACE_Q) of one launch of oc.launches(family)."""
    _, sizes, stepsize, _ = launch
    out = np.zeros((len(sizes), 4))
    for k, n in enumerate(sizes):
        r0 = reference(family, n, stepsize)
        for run in range(1, N_RUNS):
            r = ror.stations(front(family, n, run), stepsize)
            assert r["m"] == r0["m"]
            out[k] = np.maximum(out[k], deviations(r, r0))
    return out


def key(family, launch):
    return "%s/%s" % (family, launch[0])


def entries():
    """{key: function that recomputes the array} of everything race_open_spread.npz must hold."""
    return {key(f, L): functools.partial(compute_spread, f, L) for f in oc.FAMILIES for L in oc.launches(f)}


_Z = None


def spread(k):
    global _Z
    if _Z is None:
        z = np.load(PATH)
        _Z = {q: z[q] for q in z.files}
    return _Z[k]
