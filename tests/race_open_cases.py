"""The case table of tests/test_emu_race_open.py (SIMT interpreter) and tests/test_gpu_race_open.py (MI355X): open chains for
mcq_raceline_device_ends, deterministic, built from tests/glue_cases.py's rings and tests/race_open_ref.py.

Arcs.  The first n waypoints of a longer ring (RING_OF(n) waypoints) of each family of glue_cases.FAMILIES, with that ring's normals, widths
and smooth alpha.  psi_s / psi_e: the heading of the first / last chord of the arc's raceline plus PSI_OFFSET -- a few hundredths of a radian, so
that the heading rows do something.

Sizes.  The smallest chains (2 .. 5); both sides of the closed-form kernel's switch on the mirrored ring of 2n - 2 points (2n - 2 = 96: n = 49;
50, 51 and 97 beyond); the 256-thread stride; the 2048-segment chunk of the running sum (n - 1 = 2047, 2048, 2049); a long row.

A LAUNCH is what one engine call sees: (name, sizes, stepsize, mmax).  Generous launches at 1.37 / 0.61 times the spacing and at 2.0 / 3.0 m
(mmax = the largest count: that arc sits at m == mmax); aimed launches put arc K at m == mmax, at m == mmax + 1 (MCQ_BAD_INPUT, m_out = m), at
m == 3 and at m == 2 (stepsize above the arc's length: exactly the two end points), the other arcs of the launch get what they get.
total / stepsize of every row stays INTEGER_GAP away from every integer in the longdouble reference (tests/test_race_open_ref.py asserts it)."""
import functools
import math

import numpy as np

import glue_cases as gc
import race_open_ref as ror

LD = np.longdouble
SIZES = (2, 3, 4, 5, 49, 50, 51, 97, 255, 256, 257, 2048, 2049, 2050, 4097)
SMALL = tuple(n for n in SIZES if n <= 257)
FAMILIES = gc.FAMILIES
INTEGER_GAP = gc.INTEGER_GAP
PSI_OFFSET = (0.03, -0.02)          # rad, on psi_s / psi_e


def RING_OF(n):
    """Waypoints of the ring an arc of n waypoints is cut from."""
    return max(96, (3 * n) // 2 + 5)


@functools.lru_cache(maxsize=None)
def arc(family, n):
    """(reftrack [n, 4], normvec [n, 2], alpha [n], psi_s, psi_e) of one arc."""
    ref, nv, al = gc.ring(family, RING_OF(n))
    ref, nv, al = ref[:n].copy(), nv[:n].copy(), al[:n].copy()
    P = ref[:, :2] + al[:, None] * nv
    first, last = P[1] - P[0], P[n - 1] - P[n - 2]
    psi_s = math.atan2(first[1], first[0]) - math.pi / 2.0 + PSI_OFFSET[0]
    psi_e = math.atan2(last[1], last[0]) - math.pi / 2.0 + PSI_OFFSET[1]
    for a in (ref, nv, al):
        a.setflags(write=False)
    return ref, nv, al, psi_s, psi_e


def ends_of(family, sizes):
    return [dict(psi_s=arc(family, n)[3], psi_e=arc(family, n)[4]) for n in sizes]


@functools.lru_cache(maxsize=None)
def arc_total(family, n):
    """Raceline length of an arc in the longdouble reference."""
    return ror.front(*arc(family, n), LD)["total"]


def _settle(family, sizes, stepsize):
    """The stepsize, multiplied by 1.001 until total / stepsize of every arc of the launch is INTEGER_GAP away from every integer."""
    for _ in range(50):
        r = [arc_total(family, n) / LD(stepsize) for n in sizes]
        if all(abs(x - np.rint(x)) >= INTEGER_GAP for x in r):
            return float(stepsize)
        stepsize = float(stepsize) * 1.001
    raise RuntimeError("no stepsize found")


def _count(family, n, stepsize):
    return int(math.ceil(arc_total(family, n) / LD(stepsize))) + 1


@functools.lru_cache(maxsize=None)
def launches(family):
    """[(name, sizes, stepsize, mmax)]."""
    h = FAMILIES[family]
    out = []
    for tag, s in (("1.37h", 1.37 * h), ("0.61h", 0.61 * h), ("2.0", 2.0), ("3.0", 3.0)):
        s = _settle(family, SIZES, s)
        out.append((tag, SIZES, s, max(_count(family, n, s) for n in SIZES)))
    for K, sizes in ((97, SMALL), (2049, SIZES)):
        s = _settle(family, sizes, float(arc_total(family, K)) / (0.71 * K - 0.5))
        mK = _count(family, K, s)
        out.append(("m==mmax@%d" % K, sizes, s, mK))
        s1 = _settle(family, sizes, float(arc_total(family, K)) / (mK - 0.5))
        assert _count(family, K, s1) == mK + 1
        out.append(("m==mmax+1@%d" % K, sizes, s1, mK))
    for K in (2, 51, 4097):
        sizes = SMALL if K <= 257 else SIZES
        for m in (3, 2):
            s = _settle(family, sizes, float(arc_total(family, K)) / (m - 1.5))
            assert _count(family, K, s) == m
            out.append(("m==%d@%d" % (m, K), sizes, s, max(_count(family, n, s) for n in sizes)))
    return out


def aimed(name):
    """(wanted m relative to the launch, K) of an aimed launch's name, or None."""
    if "@" not in name:
        return None
    what, K = name.split("@")
    return what, int(K)


# ---- the mixed launch: ring, chain, ring, chain, ... of different sizes ------------------------------------------------------------------
MIXED = (("ring", 97), ("chain", 50), ("ring", 3), ("chain", 2), ("ring", 513), ("chain", 257), ("ring", 48), ("chain", 2049), ("ring", 2049),
         ("chain", 5))
