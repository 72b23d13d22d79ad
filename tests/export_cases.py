"""Cases for the export kernels (mcq_export_s_kernel, mcq_export_rows_kernel behind mcq_export_device): the smallest shapes at which they can go wrong.

Rings are tests/glue_cases.ring(family, n) (families peanut and trefoil, as tests/traj_check_cases.py).  A trajectory here is just an array: its s
column is j * total / m for the m stations (total: the float64 restatement's raceline length), the other six columns are seeded noise -- the entry
copies them, it computes nothing from them -- so a wrong row shows as wrong bits.  The kernels' constants: ROWS = 1024 table rows per workgroup (four per thread,
256 apart), TILE = 1024 stations per LDS tile, relin_front's running-sum chunk of 2048.

launches(family):
  sizes    n = 3, 4, 255, 256, 257 (nmax = 257: n == nmax and n < nmax) with m = 2, 3, 255, 1023, 1500 (mmax = 1500: m == mmax and m < mmax);
           the last row's stepsize is so fine that its waypoints look into more than one tile
  rowblock n = 1022, 1023, 1024, 1025 (tables of ROWS - 1 .. ROWS + 2 rows) with m = 300, 255, 1023, 2500
  tiles    n = 143, 144, 145 with m = TILE, TILE + 1, 2 TILE + 1
  chunks   n = 2047, 2048, 2049 with m = 300 (several waypoints share a station), 2047, 3071 (the 1024 waypoints of a row block look into
           more than one tile)
  large    n = 4097, m = 700
  variants three tracks (n = 96, 257, 48; m = 255, 300, 46), seven variants through track_of in shuffled order (one track shared by three rows of
           other vx / ax), ragged m_of_track.  (m = 46, not 47: the families are symmetric, s_ref_24 of the ring of 48 is half the length up to
           rounding, and with 47 stations that is a station midpoint: an undecided waypoint, 2 % of the case.)
HANDMADE: s columns written by hand around the s_ref a track really has (handmade(s_ref)), with the expected idx written out.
ties(): a regular polygon whose s_ref fall on station midpoints up to rounding (waypoint spacing : stepsize = 3 : 2)."""
import functools
import math

import numpy as np

import export_ref as xr
import glue_cases as gc

LD = np.longdouble
FAMILIES = ("peanut", "trefoil")
ROWS, TILE = 1024, 1024         # MCQ_EX_ROWS, MCQ_EX_TILE
OK, BAD_INPUT = 0, 4
UNDECIDED_CAP = 0.01


@functools.lru_cache(maxsize=None)
def total64(family, n):
    ref, nv, al = gc.ring(family, n)
    return float(xr.front(ref, nv, al, np.float64)["total"])


def make_traj(total, m, *seed):
    """(m, 7): s_j = j total / m; columns 1 .. 6 seeded noise."""
    rng = gc._seed("export", *seed)
    t = rng.standard_normal((m, 7))
    t[:, 0] = np.arange(m) * (total / m)
    return t


def _launch(name, family, rows, track_of=None):
    """rows: [(n, m)], one track each; track_of: variants (default: one per track)."""
    track_of = np.arange(len(rows), dtype=np.int32) if track_of is None else np.asarray(track_of, dtype=np.int32)
    tracks = [gc.ring(family, n) for n, _ in rows]
    trajs = [make_traj(total64(family, rows[t][0]), rows[t][1], family, name, v) for v, t in enumerate(track_of)]
    # variants of one track share its s column bit for bit (make_traj's is a function of the track alone)
    return dict(name="%s/%s" % (family, name), family=family, tracks=tracks, ms=np.array([m for _, m in rows], dtype=np.int32), track_of=track_of,
                trajs=trajs)


@functools.lru_cache(maxsize=None)
def launches(family):
    rng = gc._seed("export", family, "order")
    return (
        _launch("sizes", family, [(3, 2), (4, 3), (255, 255), (256, TILE - 1), (257, 1500)]),
        _launch("rowblock", family, [(ROWS - 2, 300), (ROWS - 1, 255), (ROWS, TILE - 1), (ROWS + 1, 2500)]),
        _launch("tiles", family, [(143, TILE), (144, TILE + 1), (145, 2 * TILE + 1)]),
        _launch("chunks", family, [(2047, 300), (2048, 2047), (2049, 3071)]),
        _launch("large", family, [(4097, 700)]),
        _launch("variants", family, [(96, 255), (257, 300), (48, 46)], track_of=rng.permutation([0, 0, 0, 1, 1, 2, 2])),
    )


def pack(L, order=None):
    """The padded arrays of a launch as mcq_export_device takes them; order: a permutation of the VARIANTS."""
    order = np.arange(len(L["track_of"])) if order is None else np.asarray(order)
    ns = np.array([t[0].shape[0] for t in L["tracks"]], dtype=np.int32)
    nmax, mmax = int(ns.max()), int(L["ms"].max())
    T = len(ns)
    ref, nv, al = np.zeros((T, nmax, 4)), np.zeros((T, nmax, 2)), np.zeros((T, nmax))
    for k, (r, v, a) in enumerate(L["tracks"]):
        ref[k, :ns[k]], nv[k, :ns[k]], al[k, :ns[k]] = r, v, a
    tj = np.full((len(order), mmax, 7), np.nan)
    for k, v in enumerate(order):
        t = L["trajs"][v]
        tj[k, :t.shape[0]] = t
    return dict(ns=ns, ms=L["ms"].copy(), ref=ref, nv=nv, al=al, track_of=L["track_of"][order].copy(), traj=tj, nmax=nmax, mmax=mmax)


@functools.lru_cache(maxsize=None)
def reference(family, name, v):
    """tests/export_ref.table of variant v of a launch in longdouble, computed once and shared."""
    L = next(q for q in launches(family) if q["name"] == "%s/%s" % (family, name))
    ref, nv, al = L["tracks"][L["track_of"][v]]
    return xr.table(ref, nv, al, L["trajs"][v])


# ---- hand-made s columns --------------------------------------------------------------------------------------------------------------------------
HAND_RING = ("peanut", 7)
HAND_D = 2.0 ** -6


def handmade(q):
    """[(name, s column, expected idx [7])] around the s_ref q[0 .. 6] of HAND_RING (q[0] = 0 < q[1] < ...; spacings ~1 m).  Every index is
    decided exactly: by a distance of 0, by a tie (equal distances: the lower index), or by being outside the stations."""
    d = HAND_D
    for a in (q[1], q[3]):
        assert (a + d) - a == d and a - (a - d) == d, "the midpoints are not exact at this s_ref"
    return [
        ("duplicates", [q[0], q[1], q[1], q[2], q[2], q[2], q[3], q[4], q[5], q[6], q[6]], [0, 1, 3, 6, 7, 8, 9]),
        ("midpoints", [q[1] - d, q[1] + d, q[2], q[3] - d, q[3] + d, q[3] + d], [0, 0, 2, 3, 4, 4, 4]),
        ("outside", [q[2], q[3]], [0, 0, 0, 1, 1, 1, 1]),
        # the rounding plateau [0, 1e-17, 2e-17, 1] queried at 0.5, scaled to the track: |s_j - q1| rounds to q1 for the first three stations
        # and IS q1 for the fourth
        ("plateau", [0.0, 1e-17, 2e-17, 2.0 * q[1]], [0, 0, 3, 3, 3, 3, 3]),
    ]


def hand_traj(col, name):
    t = gc._seed("export", "hand", name).standard_normal((len(col), 7))
    t[:, 0] = col
    return t


# ---- ties -----------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ties(n=48):
    """A regular n-gon (alpha 0): every spline length is the same up to rounding, and with m = 3 n / 2 stations every second s_ref sits on the
    midpoint of two stations up to rounding.  (track, traj)."""
    th = 2.0 * math.pi * np.arange(n) / n
    R = n * 1.5 / (2.0 * math.pi)
    xy = R * np.column_stack((np.cos(th), np.sin(th)))
    ref = np.column_stack((xy, np.full(n, 3.0), np.full(n, 3.0)))
    nv = np.column_stack((np.cos(th), np.sin(th)))
    al = np.zeros(n)
    total = float(xr.front(ref, nv, al, np.float64)["total"])
    return (ref, nv, al), make_traj(total, 3 * n // 2, "ties", n)
