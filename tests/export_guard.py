"""What mcq_export_device is held to.

s_ref, spline_lengths and spline_total: guard = max(1e-9 m, 4 x spread), the project's rule (tests/glue_guard.py).  spread: how far the REFERENCE's
answer is determined -- the largest deviation of tests/export_ref.front_variants (float64 restatements in other evaluation and summation orders)
from the longdouble run, per ring, written by scripts/make_golden_export_spread.py into tests/golden/export/export_spread.npz (one [3] array per
ring: s_ref, lengths, total), on the CPU from the restatement alone.  The same guard holds race_cl[-1, 0] against numpy.sum of the lengths.

Indices: a waypoint is DECIDED when the reference's margin (tests/export_ref.lookup) exceeds twice the guard of s_ref; there idx is the reference's
and columns 8 .. 11 are its station's bits.  At an undecided waypoint either candidate (the stations either side of s_ref) is accepted, and the row
must be the bitwise copy of THAT candidate's station.  At most UNDECIDED_CAP of a case's waypoints may be undecided (tests/test_export_ref.py
asserts it on the reference alone), except in the ties case, where the hand-made tables hold the rule instead."""
import os

import numpy as np

import export_cases as xc
import export_ref as xr
import glue_cases as gc
import glue_guard as gg

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "export", "export_spread.npz")
FLOOR = gg.FLOOR["el"]          # 1e-9 m
dmax = gg.dmax


def rings():
    """{key: (ref, nv, alpha)} of every ring the cases use."""
    out = {}
    for f in xc.FAMILIES:
        for L in xc.launches(f):
            for t in L["tracks"]:
                out["%s/%d" % (f, t[0].shape[0])] = t
    out["%s/%d" % xc.HAND_RING] = gc.ring(*xc.HAND_RING)
    out["ties"] = xc.ties()[0]
    return out


def compute_spread(track):
    """[3]: s_ref, lengths, total -- front_variants against the longdouble front."""
    r0 = xr.front(*track)
    out = np.zeros(3)
    for v in xr.front_variants(*track):
        out = np.maximum(out, [dmax(v["s_ref"], r0["s_ref"]), dmax(v["lengths"], r0["lengths"]), dmax(v["total"], r0["total"])])
    return out


_Z = None


def spread(key):
    global _Z
    if _Z is None:
        z = np.load(PATH)
        _Z = {q: z[q] for q in z.files}
    return _Z[key]


def guards(key=None, live=None):
    """(s_ref, lengths, total) guards of a ring; live: a spread computed on the spot (the end-to-end case, whose ring no file can know)."""
    s = spread(key) if live is None else live
    return tuple(max(FLOOR, 4.0 * float(x)) for x in s)


def undecided(margin, g_s):
    return np.asarray(margin) <= 2.0 * g_s
