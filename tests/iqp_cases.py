"""The case table of the IQP edges suite (tests/test_iqp_ref.py on the CPU, tests/test_emu_iqp.py on the SIMT interpreter, tests/test_gpu_iqp.py on the
MI355X): what mcq_iqp_batch is run on and held to tests/iqp_ref.py for.  Deterministic: rings from synthetic.oval_centreline / widths with small
perimeters (normals and the spline matrix from the dense oracle, the engine's scalings read out of that matrix) plus the two small goldens; at most
MAX_N waypoints per ring, MAX_BATCH tracks per call, MAX_ROUNDS rounds -- the smallest shapes that reach every branch of the loop.

A CASE is one track with one parameter set; `rounds` is what the reference needs (asserted by tests/test_iqp_ref.py, as is that every case is DECIDED:
in every round the reference's curv_error_max is at least ROUND_GAP x allowed away from allowed and length / stepsize at least INTEGER_GAP -- the
rule of tests/test_glue_ref.py::test_point_counts_are_decided -- from every integer, on both routes).  A case that is not decided gets other
parameters here; none is skipped at run time."""
import functools
import os

import numpy as np

import iqp_ref
from glue_cases import INTEGER_GAP          # the margin of tests/test_glue_ref.py::test_point_counts_are_decided, reused
from global_racetrajectory_optimization_amd import synthetic
from oracle import tph_ref

MAX_N, MAX_BATCH, MAX_ROUNDS = 300, 16, 20
ROUND_GAP = 1e-3
W_VEH, KAPPA = 2.0, 0.4
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# name: (waypoints, spacing m, widths seed, (amp1, k1, amp2, k2) of the centreline's two harmonics, axis ratio of the oval)
_H = (1.5, 3, 0.5, 5)
TRACKS = {
    "o60": (60, 3.0, 0, _H, 2.0), "o75": (75, 3.0, 2, (0.5, 3, 0.2, 5), 2.0), "o90": (90, 3.0, 3, (2.0, 4, 0.7, 7), 2.0),
    "o105": (105, 3.0, 4, (4.0, 3, 1.0, 6), 2.0), "c100": (100, 3.0, 20, (0.3, 3, 0.1, 5), 1.0), "c110": (110, 3.0, 21, (0.5, 2, 0.1, 5), 1.2),
    "c120": (120, 3.0, 22, (0.5, 3, 0.2, 4), 1.3), "c90": (90, 3.0, 23, (0.2, 3, 0.1, 5), 1.0),
    "coarse100": (100, 4.0, 15, (1.0, 3, 0.3, 5), 2.0),         # re-sampled at 3 m it needs 134 waypoints: the ring that outgrows nmax = 128
    "s46": (46, 3.0, 46, _H, 2.0), "s50": (50, 3.0, 50, _H, 2.0), "s92": (92, 3.0, 92, _H, 2.0), "s100": (100, 3.0, 100, _H, 2.0),
    "s250": (250, 2.0, 250, _H, 2.0), "s262": (262, 2.0, 262, _H, 2.0), "s16": (16, 6.0, 16, _H, 2.0), "s24": (24, 6.0, 24, _H, 2.0),
    "k296": (296, 1.0, 7, _H, 2.0),
    "t12": (12, 8.0, 5, (0.3, 2, 0.0, 3), 2.0),
}
GOLDENS = {"golden/rounded_rectangle": "rounded_rectangle", "golden/handling_track": "handling_track"}


@functools.lru_cache(maxsize=None)
def track(name):
    """dict(reftrack [n, 4], normvectors [n, 2], A [4n, 4n], scaling [n]) -- read-only."""
    if name in GOLDENS:
        z = np.load(os.path.join(GOLDEN_DIR, GOLDENS[name] + ".npz"))
        ref, nv = np.array(z["reftrack"]), np.array(z["normvec"])
        A = tph_ref.calc_splines(np.vstack((ref[:, :2], ref[0, :2])))[2]
    else:
        n, spacing, b, amp, ratio = TRACKS[name]
        xy = synthetic.oval_centreline(n, perimeter=n * spacing, ratio=ratio, amp1=amp[0], k1=amp[1], amp2=amp[2], k2=amp[3])
        _, _, A, nv = tph_ref.calc_splines(np.vstack((xy, xy[0])))
        ref = np.column_stack((xy, synthetic.widths(n, b, base=4.0, amp=1.0)))
    out = dict(reftrack=ref, normvectors=nv, A=A, scaling=iqp_ref.scalings_of(A))
    for v in out.values():
        v.setflags(write=False)
    return out


def _case(trk, stepsize, iters_min, allowed, rounds, kappa_bound=KAPPA, w_veh=W_VEH):
    return dict(track=trk, stepsize=stepsize, iters_min=iters_min, allowed=allowed, rounds=rounds, kappa_bound=kappa_bound, w_veh=w_veh)


CASES = {}
# ---- damping and termination ladder: iters_min in {1, 2, 3, 5}, ending in round iters_min / one to three rounds later
for _im, _al, _r in ((1, 0.06, 1), (1, 0.008, 3), (2, 0.02, 2), (2, 0.0035, 3), (3, 0.01, 3), (3, 0.002, 6), (5, 0.005, 5), (5, 0.001, 7)):
    CASES["ladder/%d/%d" % (_im, _r)] = _case("o60", 3.0, _im, _al, _r)
CASES["golden/rounded_rectangle"] = _case("golden/rounded_rectangle", 3.0, 3, 0.01, 3, 0.12, 3.4)
CASES["golden/handling_track"] = _case("golden/handling_track", 3.0, 3, 0.01, 4, KAPPA, 3.4)      # (at 0.12 a curvature row is active: 198 waypoints, no CPU-B)
# ---- round cap: a track that needs CAP_ROUNDS rounds, capped below, at and above (and below iters_min)
CASES["cap/o60"] = _case("o60", 3.0, 3, 0.0026, 5)
CAP_CASE, CAP_ROUNDS = "cap/o60", 5
CAP_BELOW = (CAP_ROUNDS - 1, 2, 1)          # max_rounds = R - 1 and < iters_min
CAP_FREE = (CAP_ROUNDS, CAP_ROUNDS + 1)
# ---- switch crossings between passes: the ring grows / shrinks past 48, 96, 256 and 20 waypoints after the first pass (s24 again after the third)
SWITCHES = {"switch/48/up": ("s46", 2.7, 0.006, 4, (46, 52)), "switch/48/down": ("s50", 3.3, 0.006, 4, (50, 46)),
            "switch/96/up": ("s92", 2.75, 0.002, 4, (92, 101)), "switch/96/down": ("s100", 3.25, 0.002, 4, (100, 93)),
            "switch/256/up": ("s250", 1.9, 0.001, 4, (250, 264)), "switch/256/down": ("s262", 2.1, 0.001, 4, (262, 250)),
            "switch/20/up": ("s16", 4.5, 0.015, 4, (16, 22)), "switch/20/down": ("s24", 8.0, 0.008, 5, (24, 19))}
for _name, (_t, _step, _al, _r, _) in SWITCHES.items():
    CASES[_name] = _case(_t, _step, 3, _al, _r)
# ---- curvature rows active inside the loop (rings of at least banded_ref.MIN_N waypoints: the second route needs CPU-B there)
CASES["kappa/k296"] = _case("k296", 1.0, 3, 0.0026, 4, kappa_bound=0.04)
# ---- the trace beyond its 16 entries
CASES["trace/t12"] = _case("t12", 8.0, 18, 0.01, 18)
# ---- the healthy tracks of the batches: one stepsize, iters_min and allowed per call
BATCH_STEP, BATCH_ITERS_MIN, BATCH_ALLOWED, BATCH_NMAX = 3.0, 3, 0.0026, 128
_BATCH_ROUNDS = {"c100": 3, "c110": 3, "c120": 3, "c90": 3, "o75": 4, "o90": 4, "o105": 4, "o60": 5}
for _t, _r in _BATCH_ROUNDS.items():
    CASES["batch/" + _t] = _case(_t, BATCH_STEP, BATCH_ITERS_MIN, BATCH_ALLOWED, _r)
# the mixed batch: (kind, track); kinds other than "ok" name what mcq.h states for a track that fails
MIXED = (("ok", "c100"), ("narrow", "o75"), ("ok", "o75"), ("ok", "o60"), ("empty", None), ("ok", "c120"), ("overflow", "coarse100"), ("ok", "o105"),
         ("nan", "o90"), ("ok", "c110"), ("ok", "o90"))
SAME_ROUND = (("ok", "c100"), ("ok", "c110"), ("ok", "c120"), ("ok", "c90"))        # every track ends in round 3: the two-copy download
# status, rounds of the failing kinds (include/mcq.h: MCQ_INFEASIBLE, MCQ_BAD_INPUT, MCQ_RING_OVERFLOW)
FAILS = {"narrow": (1, 1), "empty": (4, 1), "nan": (4, 1), "overflow": (7, 1)}


def batch_track(kind, trk):
    """The engine's input of one entry of a batch."""
    if kind == "empty":
        return dict(reftrack=np.zeros((0, 4)), normvectors=np.zeros((0, 2)), scaling=None)
    t = track(trk)
    ref = np.array(t["reftrack"])
    if kind == "narrow":
        ref[:, 2:] = 0.4 * W_VEH                      # narrower than the vehicle at every waypoint
    if kind == "nan":
        ref[ref.shape[0] // 3, 1] = np.nan
    return dict(reftrack=ref, normvectors=t["normvectors"], scaling=t["scaling"])


@functools.lru_cache(maxsize=None)
def reference(name, route="gi"):
    """The rounds of a case by tests/iqp_ref.py, computed once, read-only."""
    c = CASES[name]
    t = track(c["track"])
    return tuple(iqp_ref.run(t["reftrack"], t["normvectors"], t["A"], c["kappa_bound"], c["w_veh"], c["stepsize"], c["iters_min"], c["allowed"],
                             max_rounds=MAX_ROUNDS, route=route))
