"""The cases of the friction entries: the smallest shapes at which the index, the search and the grids can go wrong.  Everything is seeded and
small; coordinates stay below 1e3 m (the acceptance of an index, tests/fric_guard.py, rests on that)."""
import functools
import math

import numpy as np

import fric_ref as fr

WB_F, WB_R = 1.6, 1.4       # [REF params/racecar.ini: vehicle_params_mintime]


def _mue(c):
    return 0.5 + 0.001 * np.arange(c)        # a value of its own per cell: mue_out names the cell


def _lattice(nx, ny, h=1.0, x0=0.0, y0=0.0):
    return np.array([[x0 + h * i, y0 + h * j] for i in range(nx) for j in range(ny)])


@functools.lru_cache(maxsize=None)
def maps():
    """{name: (cells [c, 2], mue [c], bin_side or None)}."""
    rng = np.random.default_rng(20261019)
    lat = _lattice(4, 4)
    ring = np.array([p for p in lat if not (1 <= p[0] <= 2 and 1 <= p[1] <= 2)])
    out = {
        "one": (np.array([[3.0, -2.0]]), None),
        "two": (np.array([[0.0, 0.0], [4.0, 2.0]]), None),
        "line3": (np.array([[0.0, 1.0], [2.0, 1.0], [5.0, 1.0]]), None),            # one bin along y
        "lattice": (lat, None),
        "ring": (ring, 1.0),                                                        # empty bins between a query in the middle and its answer
        "dup": (np.vstack((lat, lat[::3], lat[5:6])), None),                        # duplicated cells: the plain case of a tie
        "edges": (_lattice(5, 5), 1.0),                                             # every cell on a bin edge, four on the box's corners
        # bins of side 1 from (0, 0): the query (2.5, 2.5) scans bins 1 .. 3; cell 3 inside that block and cell 0 in bin 4, exactly ON the block's
        # side, are both exactly 1.5 away -- only the strict `<` of the stopping rule goes on to the ring that holds the lower index
        "strict": (np.array([[4.0, 2.5], [0.0, 0.0], [6.0, 6.0], [1.0, 2.5]]), 1.0),
        "onebin": (rng.uniform(0.0, 100.0, (257, 2)), 1.0e6),
        "sparse": (rng.uniform(0.0, 100.0, (40, 2)), 0.5),                          # 40 000 bins for 40 cells
    }
    for c in (255, 256, 257):
        out["c%d" % c] = (rng.uniform(-50.0, 50.0, (c, 2)), None)
    res = {k: (v[0], _mue(v[0].shape[0]), v[1]) for k, v in out.items()}
    mu = _mue(16)
    mu[5] = np.nan
    res["nanmue"] = (lat, mu, None)
    return res


COUNTS = (0, 1, 63, 64, 65, 255, 256, 257)


def queries(name):
    """Finite queries of a map: on cells, on exact midpoints of two and of four cells, 1 km outside the box on each side and diagonally, and seeded
    ones in and around the box."""
    cells = maps()[name][0]
    rng = np.random.default_rng(sum(map(ord, name)))
    lo, hi = cells.min(axis=0), cells.max(axis=0)
    mid, far = 0.5 * (lo + hi), 1000.0
    q = [cells[i] for i in range(min(cells.shape[0], 6))]
    q += [0.5 * (cells[i] + cells[(i + 1) % cells.shape[0]]) for i in range(min(cells.shape[0], 6))]
    if cells.shape[0] >= 4:
        q += [0.25 * (cells[0] + cells[1] + cells[-2] + cells[-1]), mid]
    q += [np.array([lo[0] - far, mid[1]]), np.array([hi[0] + far, mid[1]]), np.array([mid[0], lo[1] - far]), np.array([mid[0], hi[1] + far])]
    q += [np.array([lo[0] - far, lo[1] - far]), np.array([hi[0] + far, hi[1] + far]), np.array([lo[0] - far, hi[1] + far]),
          np.array([hi[0] + far, lo[1] - far])]
    span = np.maximum(hi - lo, 1.0)
    q += list(rng.uniform(lo - 0.3 * span, hi + 0.3 * span, (257 - len(q), 2)))
    return np.array(q)


# exact cases: dyadic coordinates, every product exact -> the index must be the lowest of the tied ones
def exact_ties():
    """[(map name, query, the tied cells' lowest index)]."""
    lat = maps()["lattice"][0]

    def at(x, y):
        return int(np.nonzero((lat[:, 0] == x) & (lat[:, 1] == y))[0][0])
    return [("lattice", (0.5, 0.5), min(at(0, 0), at(0, 1), at(1, 0), at(1, 1))), ("lattice", (2.5, 1.5), min(at(2, 1), at(2, 2), at(3, 1), at(3, 2))),
            ("lattice", (0.5, 0.0), min(at(0, 0), at(1, 0))), ("lattice", (3.0, 2.5), min(at(3, 2), at(3, 3))),
            ("ring", (1.5, 1.5), 1), ("dup", (0.0, 0.0), 0), ("dup", (0.0, 3.0), 3), ("dup", (1.0, 1.0), 5), ("dup", (0.25, 3.0), 3),
            ("edges", (2.0, 2.0), 12), ("edges", (1.5, 1.5), 6), ("edges", (4.0, 4.5), 24), ("two", (2.0, 1.0), 0), ("strict", (2.5, 2.5), 0),
            ("lattice", (-1000.0, 1.5), 1), ("lattice", (1.5, 1003.0), 7)]


# ---- grids -------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def grid_map():
    """A 0.5 m lattice of 45 x 45 cells over [-6, 16] x [-11, 11] with friction in hundredths."""
    cells = _lattice(45, 45, 0.5, -6.0, -11.0)
    mue = np.round(1.0 + 0.1 * np.sin(0.7 * cells[:, 0]) + 0.1 * np.cos(0.5 * cells[:, 1]), 2)
    return cells, mue


def ring_track(widths, radius=5.0, centre=(5.0, 0.0)):
    """n waypoints on a circle with outward normals; widths: [(w_right, w_left)] * n."""
    n = len(widths)
    th = 2.0 * math.pi * np.arange(n) / n + 0.3
    nv = np.column_stack((np.cos(th), np.sin(th)))
    return np.column_stack((np.asarray(centre) + radius * nv, np.asarray(widths, dtype=np.float64))), nv


def _w(count_r, count_l, width, dn, frac=0.5):
    """Widths whose quotient lies `frac` above the wanted integers."""
    return (0.5 * width + 0.5 + (count_r + frac) * dn, 0.5 * width + 0.5 + (count_l + frac) * dn)


@functools.lru_cache(maxsize=None)
def grid_cases():
    """{name: dict(tracks [(reftrack, normvec)], width (scalar or list), dn, jmax or None)}."""
    W = 3.4
    small = [(-1, -1), (-1, 0), (0, 0), (0, 1)]        # (num_right, num_left): counts -1, 0, 1, 2
    out = {}
    for n in (1, 2, 3):
        out["n%d" % n] = dict(tracks=[ring_track([_w(2 + k, 3, W, 0.25) for k in range(n)])], width=W, dn=0.25, jmax=None)
    out["counts"] = dict(tracks=[ring_track([_w(a, b, W, 0.25) for a, b in small] + [_w(3, 4, W, 0.25)])], width=W, dn=0.25, jmax=None)
    out["floor"] = dict(tracks=[ring_track([(5.0, 5.0), (5.0, 4.0), (4.0, 5.0)])], width=W, dn=0.1, jmax=None)            # 27, not 28
    out["floor_exact"] = dict(tracks=[ring_track([(4.5, 4.5), (4.5, 3.25), (2.0, 4.5)])], width=3.0, dn=0.25, jmax=None)  # 2.5 / 0.25 = 10
    out["fma01"] = dict(tracks=[ring_track([_w(7, 9, W, 0.1)] * 3)], width=W, dn=0.1, jmax=None)
    out["fma03"] = dict(tracks=[ring_track([_w(3, 5, W, 0.3)] * 3)], width=W, dn=0.3, jmax=None)
    out["jmax_eq"] = dict(tracks=[ring_track([_w(3, 4, W, 0.25), _w(1, 2, W, 0.25)])], width=W, dn=0.25, jmax=8)
    out["jmax_over"] = dict(tracks=[ring_track([_w(3, 4, W, 0.25), _w(1, 2, W, 0.25)]), ring_track([_w(1, 2, W, 0.25)] * 2)], width=W, dn=0.25, jmax=7)
    ragged = [ring_track([_w(2 + (k % 3), 1 + (k % 4), W, 0.25) for k in range(n)], radius=3.0 + n % 3) for n in (5, 1, 9, 3)]
    out["ragged"] = dict(tracks=ragged, width=W, dn=0.25, jmax=None)
    out["widths"] = dict(tracks=ragged, width=[3.4, 2.0, 3.0, 1.2], dn=0.25, jmax=None)
    bad = ring_track([_w(2, 2, W, 0.25)] * 4)
    bad[0][2, 1] = np.nan
    out["nan_track"] = dict(tracks=[ragged[0], bad, ragged[2]], width=W, dn=0.25, jmax=None)
    out["outside"] = dict(tracks=[ring_track([(12.0, 3.0), (3.0, 14.0), (9.0, 9.0)], radius=9.0)], width=W, dn=0.25, jmax=None)
    out["wide"] = dict(tracks=[ring_track([_w(40, 41, W, 0.1), _w(8, 8, W, 0.1)])], width=W, dn=0.1, jmax=None)           # 82 positions: six per lane
    return out


def widths_of(case):
    k = len(case["tracks"])
    return [float(case["width"])] * k if np.ndim(case["width"]) == 0 else [float(w) for w in case["width"]]


def check_case_table():
    """The cases are what their names say (asserted by tests/test_fric_ref.py)."""
    g = grid_cases()
    cnt = lambda name, t=0: [r["cnt"] for r in fr.grid(*g[name]["tracks"][t], widths_of(g[name])[t], WB_F, WB_R, g[name]["dn"])]    # noqa: E731
    assert cnt("counts") == [-1, 0, 1, 2, 8, -1]
    assert cnt("floor")[0] == 27 + 27 + 1 and (5.0 - 1.7 - 0.5) / 0.1 == 27.999999999999996
    assert cnt("floor_exact")[0] == 21 and (4.5 - 1.5 - 0.5) / 0.25 == 10.0
    assert cnt("fma01") == [17] * 4 and fr.counts(*g["fma01"]["tracks"][0][0][0, 2:], 3.4, 0.1) == (7, 9)
    assert cnt("fma03") == [9] * 4 and fr.counts(*g["fma03"]["tracks"][0][0][0, 2:], 3.4, 0.3) == (3, 5)
    assert max(cnt("jmax_eq")) == 8 == g["jmax_eq"]["jmax"] and max(cnt("jmax_over")) == g["jmax_over"]["jmax"] + 1
    assert max(cnt("wide")) == 82
    cells = grid_map()[0]
    xy = np.vstack([r["xy"].reshape(-1, 2) for r in fr.grid(*g["outside"]["tracks"][0], 3.4, WB_F, WB_R, 0.25)])
    assert np.any(xy < cells.min(axis=0)) or np.any(xy > cells.max(axis=0)), "no position of 'outside' leaves the map's box"
