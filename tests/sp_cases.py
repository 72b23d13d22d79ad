"""The case tables of the shortest-path suite (tests/test_sp_ref.py, tests/test_emu_sp.py, tests/test_gpu_sp.py): deterministic, seeded, numpy only.

A CASE is one ring (rows, normals, w_veh, solver options); a LAUNCH a ragged batch of cases through Engine.solve_batch, with the `bad` rows
between good ones.  The sizes sit on the switches of the scalar tridiagonal route (csrc/mcq_tri.inc: sp_chain_solve) and of the solver kernel,
read from the sources below: MCQ_NT threads own m = ceil(n / MCQ_NT) rows each, the last of them the separator; rings above TRI_MAXN run on
workspace vectors; rings above IPB_E * MCQ_NT take ipm() instead of ipm_box()."""
import functools
import math
import os
import re

import numpy as np

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "global_racetrajectory_optimization_amd", "csrc")


def _define(fname, name):
    with open(os.path.join(_CSRC, fname)) as fh:
        m = re.search(r"^#define\s+%s\s+(\d+)\b" % name, fh.read(), re.M)
    return int(m.group(1))


MCQ_NT = _define("mcq_kernels.hip", "MCQ_NT")
TRI_MAXN = _define("mcq_kernels.h", "MCQ_TRI_MAXN")
IPM_BOX_MAXN = _define("mcq_kernels.hip", "IPB_E") * MCQ_NT
# the sizes below are written for these values; if the sources move, the sizes move with them
assert (MCQ_NT, TRI_MAXN, IPM_BOX_MAXN) == (256, 2048, 2048), "the switches moved: move LADDER / EDGE_SIZES with them"

W_VEH = 2.0
LADDER = (3, 4, 5, 6, 8, 64, 255, 256, 257, 258, 511, 512, 513, 514, 768, 769, 1025, 2047, 2048, 2049, 2053, 2305, 4097)
EDGE_SIZES = (257, 514, 2048, 2053)          # single-row last block on both routes, the last LDS ring, two- and eight/nine-row blocks
CORNER_PATTERNS = ("row0", "last", "both", "second", "separators", "all", "all_but_one")
ALL_FREE = (3, 64, 256, 257, 300, 777)
LAST_RESORT_LADDER = (64, 257, 514, 2048, 2053)
CLIPPED_WIDTH = 0.9                          # below w_veh / 2: the box is clipped to +-0.001 m
FREE_WIDTH = 200.0
# a case that misses a condition of tests/test_sp_ref.py (spread, margin, or the dense oracle cannot make its comparison) gets another seed here,
# never a looser number
#   corner/257/row0: the DENSE oracle of tests/test_sp_ref.py leaves its own active rows 1.1e-12 m off their bounds on the first seed's ring and
#   ends 2.3e-12 m from the certified reference (ten times its distance anywhere else): the 1e-12 m comparison cannot be made there.
SEEDS = {"corner/257/row0": [257, 0, 1]}


# the families that solve problems of ladder and corner again under other solver options.  last_resort: one active-set round, so that a problem
# the first round does not settle goes on in the solver kernel's 8 n + 200 round continuation.  last_resort_cold: one interior-point iteration
# as well -- ipm_box / ipm run out of their budget, no working set is identified, and the continuation is the ONLY phase that can settle the
# problem, from an empty working set, on every case (a dozen rounds and more; with max_as_iter = 1 alone it is entered at one size and needs
# a single round there).
# unrefined: refine_steps = 0, the final working set's solve as the elimination leaves it.  The two default refinement rounds repair a solve
# that is slightly wrong (a cyclic reduction that stops one level early comes back within 1e-9 m through them on every ring of the table but
# the one of three waypoints), so the elimination is held to the floor WITHOUT them where a backward-stable one must reach it: its residual is
# about 3 eps |H| |x| <= 3 x 1.1e-16 x 8 |x|, the error that divided by the smallest eigenvalue of the free block -- about 2 (2 pi / n)^2 on a ring
# without a pinned row, far larger between pinned rows.  all_free/300 (|x| <= 25 m): 7.5e-11 m.  all_free/777 (65 m): 1.3e-9 m, above the floor --
# left out by this bound, not by a measurement.
OPTIONS = {"last_resort": dict(max_as_iter=1), "last_resort_cold": dict(max_as_iter=1, max_ipm_iter=1), "unrefined": dict(refine_steps=0)}
UNREFINED_FREE_NMAX = 300


def block_rows(n):
    return (n + MCQ_NT - 1) // MCQ_NT


def ring(n, seed):
    """(reftrack [n, 4], normvec [n, 2]): a wavy ring, unit right-pointing normals of the central differences, widths U(1.5, 5)."""
    rng = np.random.default_rng(seed)
    a, b, c = rng.uniform(0.0, 6.0, 3)
    th = np.linspace(0.0, 2.0 * math.pi, n, endpoint=False)
    R = max(40.0, 3.0 * n / (2.0 * math.pi))
    r = R * (1.0 + 0.15 * np.sin(3 * th + a) + 0.08 * np.cos(5 * th + b) + (0.02 * np.sin(17 * th + c) if n > 60 else 0.0))
    p = np.column_stack((r * np.cos(th), r * np.sin(th)))
    t = np.roll(p, -1, axis=0) - np.roll(p, 1, axis=0)
    nv = np.column_stack((t[:, 1], -t[:, 0])) / np.hypot(t[:, 0], t[:, 1])[:, None]
    w = rng.uniform(1.5, 5.0, (n, 2))
    return np.ascontiguousarray(np.column_stack((p, w))), np.ascontiguousarray(nv)


def corner_rows(n, pattern):
    i = np.arange(n)
    m = block_rows(n)
    return {"row0": i == 0, "last": i == n - 1, "both": (i == 0) | (i == n - 1), "second": i % 2 == 0, "separators": i % m == m - 1,
            "all": i >= 0, "all_but_one": i != n // 3}[pattern]


def names(family):
    if family == "ladder":
        return ["ladder/%d" % n for n in LADDER]
    if family == "corner":
        return ["corner/%d/%s" % (n, p) for n in EDGE_SIZES for p in CORNER_PATTERNS]
    if family == "all_free":
        return ["all_free/%d" % n for n in ALL_FREE]
    if family == "nonunit":
        return ["nonunit/%d" % n for n in EDGE_SIZES]
    if family == "unrefined":
        return (["unrefined/all_free/%d" % n for n in ALL_FREE if n <= UNREFINED_FREE_NMAX] + ["unrefined/ladder/%d" % n for n in EDGE_SIZES]
                + ["unrefined/corner/%d/separators" % n for n in EDGE_SIZES])
    if family in OPTIONS:
        return ["%s/ladder/%d" % (family, n) for n in LAST_RESORT_LADDER] + ["%s/corner/%d/second" % (family, n) for n in EDGE_SIZES]
    raise KeyError(family)


BASE_FAMILIES = ("ladder", "corner", "all_free", "nonunit")
FAMILIES = BASE_FAMILIES + tuple(OPTIONS)


def _split(name):
    family = name.split("/")[0]
    return (family, name[len(family) + 1:]) if family in OPTIONS else (None, name)


def base_name(name):
    """The case whose problem (and reference, and spread) `name` shares."""
    return _split(name)[1]


def options(name):
    return dict(OPTIONS.get(_split(name)[0], {}))


def size(name):
    name = base_name(name)
    return HOST_N if name.startswith("host/") else int(name.split("/")[1])


def default_seed(name):
    return [sum((i + 1) * ord(ch) for i, ch in enumerate(name)), len(name)]


def _seed_of(name):
    return SEEDS.get(name, default_seed(name))


@functools.lru_cache(maxsize=None)
def case(name):
    """(reftrack, normvec, w_veh) of a case; read-only arrays."""
    name = base_name(name)
    parts = name.split("/")
    family = parts[0]
    if family in ("w_veh", "f32", "host"):
        return _derived(parts)
    n = int(parts[1])
    ref, nv = ring(n, _seed_of(name))
    if family == "corner":
        ref[corner_rows(n, parts[2]), 2:4] = CLIPPED_WIDTH
    elif family == "all_free":
        ref[:, 2:4] = FREE_WIDTH
    elif family == "nonunit":
        nv *= np.random.default_rng(_seed_of(name) + [7]).uniform(0.5, 2.0, n)[:, None]
    ref.setflags(write=False)
    nv.setflags(write=False)
    return ref, nv, W_VEH


def problem(name):
    ref, nv, w_veh = case(name)
    return dict(reftrack=ref, normvec=nv, scaling=None, kappa_bound=1.0, w_veh=w_veh)


def all_names():
    return [n for f in BASE_FAMILIES for n in names(f)]


# ---- inputs derived from the cases for the entry-point, host-batch and fp32 bodies (tests/sp_checks.py): cases of their own, with spreads of their
#      own in the stored table, so that their guard is max(floor, 4 x spread) like everybody's ------------------------------------------------------
W_VEH_SWEEP = (W_VEH, 6.0, 2.5, 9.0, W_VEH)      # per-problem widths of the mcq_solve_device_ragged_params body: 6 and 9 m clip most rows
HOST_BATCH, HOST_N = 520, 24                     # above MCQ_HOST_SLICE_MIN (512)


def uniform_names(n):
    return ["ladder/%d" % n, "corner/%d/row0" % n, "corner/%d/both" % n, "corner/%d/separators" % n, "nonunit/%d" % n]


def _derived(parts):
    if parts[0] == "host":                       # host/<k>: ring k of the 520 x 24 batch
        ref, nv = ring(HOST_N, [HOST_N, int(parts[1])])
        w_veh = W_VEH
    else:
        n, k = int(parts[1]), int(parts[2])
        ref, nv, w_veh = case(uniform_names(n)[k])
        if parts[0] == "w_veh":                  # w_veh/<n>/<k>: problem k of uniform_names(n) under W_VEH_SWEEP[k]
            w_veh = W_VEH_SWEEP[k]
        else:                                    # f32/<n>/<k>: the same problem with rows and normals rounded to float
            ref, nv = ref.astype(np.float32).astype(np.float64), nv.astype(np.float32).astype(np.float64)
    ref, nv = ref.copy(), nv.copy()
    ref.setflags(write=False)
    nv.setflags(write=False)
    return ref, nv, w_veh


def derived_names():
    return (["%s/%d/%d" % (f, n, k) for f in ("w_veh", "f32") for n in (257, 2053) for k in range(len(W_VEH_SWEEP))]
            + ["host/%d" % k for k in range(HOST_BATCH)])


def spread_names():
    """Every entry of the stored spread table."""
    return all_names() + derived_names()


# ---- the rows a launch must refuse ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def bad(kind):
    if kind == "n2":
        ref, nv = ring(3, [2, 2])
        ref, nv = ref[:2].copy(), nv[:2].copy()
    elif kind == "nan_normal":
        ref, nv = ring(64, [64, 2])
        nv[5, 1] = np.nan
    elif kind == "inf_width":
        ref, nv = ring(257, [257, 2])
        ref[7, 2] = np.inf
    else:
        raise KeyError(kind)
    return dict(reftrack=ref, normvec=nv, scaling=None, kappa_bound=1.0, w_veh=W_VEH)


BAD = ("n2", "nan_normal", "inf_width")
MAX_LAUNCH = 48


def _interleave(good, bads=BAD):
    """The bad rows between good ones: after the 2nd, the middle and the last-but-one good row."""
    out = list(good)
    for pos, kind in zip((len(good) - 1, len(good) // 2, 2), bads[::-1]):
        out.insert(pos, "bad/" + kind)
    return out


def launches(nmax=None):
    """{launch name: (list of case names and 'bad/<kind>' entries, options)}.  Every launch holds rings on both sides of TRI_MAXN and one of
    at most six waypoints; nmax drops the longer rings (the interpreter's run)."""
    corner = {n: ["corner/%d/%s" % (n, p) for p in CORNER_PATTERNS] for n in EDGE_SIZES}
    L = {
        "ladder": (_interleave(names("ladder")), {}),
        "corner_a": (_interleave(corner[257] + names("all_free") + corner[2053]), {}),
        "corner_b": (_interleave(["ladder/4"] + corner[514] + names("nonunit") + corner[2048]), {}),
        "last_resort": (_interleave(["last_resort/ladder/6"] + names("last_resort")), OPTIONS["last_resort"]),
        "last_resort_cold": (_interleave(["last_resort_cold/ladder/6"] + names("last_resort_cold")), OPTIONS["last_resort_cold"]),
        "unrefined": (_interleave(names("unrefined")), OPTIONS["unrefined"]),
    }
    if nmax is not None:
        L = {k: ([n for n in v[0] if n.startswith("bad/") or size(n) <= nmax], v[1]) for k, v in L.items()}
    return L


def launch_problems(rows):
    return [bad(n[4:]) if n.startswith("bad/") else problem(n) for n in rows]
