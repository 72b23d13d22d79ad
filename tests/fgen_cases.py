"""The case table of the friction-map generation tests (tests/fgen_checks.py; scripts/make_golden_friction_gen.py records matplotlib's verdicts on
the same table): hand-made polygons at the contour's structural edges, point sets at the kernels' block edges, tracks and cell widths."""
import math

import numpy as np

from conftest import load_golden

RADII = (0.0, 0.5, -0.5, 2.0, -2.0, 6.0, -6.0)
TILE = 512                  # MCQ_FGEN_TILE: contour vertices per LDS tile of the crossing kernels
WIDTHS = (2.0, 2.5, 0.7, 0.3, 0.1)
TRACKS = ("rounded_rectangle", "handling_track", "modena_2019", "berlin_2018")
SMALL_TRACKS = TRACKS[:2]
INSIDE = {"rounded_rectangle": "left", "handling_track": "left", "modena_2019": "right", "berlin_2018": "left"}     # the side that gives cells
SMALL_INSIDE = "left"       # the hand-made lines run counter-clockwise


def _ring(k, r_of, cx=4.0, cy=4.0):
    return np.array([(cx + r_of(i) * math.cos(2.0 * math.pi * i / k), cy + r_of(i) * math.sin(2.0 * math.pi * i / k)) for i in range(k)])


def polygons():
    """name -> vertices [v, 2].  The eleven hand-made ones, then rings of 255 / 256 / 257 vertices: `circle` (one contour point per join) and
    `star` (spikes and notches beyond both miter limits at radius +-6: two per join, 2 * 256 = one LDS tile exactly)."""
    p = {
        "triangle": [(0, 0), (8, 0), (3, 7)],
        "square_ccw": [(0, 0), (8, 0), (8, 8), (0, 8)],
        "square_cw": [(0, 0), (0, 8), (8, 8), (8, 0)],
        "collinear": [(0, 0), (2, 0), (4, 0), (8, 0), (8, 4), (8, 8), (3, 8), (0, 8), (0, 5)],
        "spike": [(0, 0), (8, 0), (8, 8), (4.25, 8), (4, 15), (3.75, 8), (0, 8)],            # outward, beyond the miter limit
        "notch": [(0, 0), (8, 0), (8, 8), (4.25, 8), (4, 1), (3.75, 8), (0, 8)],             # inward
        "reversal": [(0, 0), (8, 0), (8, 8), (4, 8), (4, 12), (4, 8), (0, 8)],               # a 180 degree turn: the offset lines are parallel
        "duplicates": [(0, 0), (0, 0), (8, 0), (8, 0), (8, 0), (8, 8), (0, 8), (0, 8), (0, 0), (0, 0)],       # runs, and last == first
        "short_edges": [(0, 0), (4, 0), (4.25, 0.25), (4.5, 0), (8, 0), (8, 8), (7.75, 8.25), (7.5, 8), (0, 8)],   # edges shorter than the offset
        "bowtie": [(0, 0), (8, 8), (8, 0), (0, 8)],
        "two": [(0, 0), (8, 8)],
    }
    p = {k: np.array(v, dtype=np.float64) for k, v in p.items()}
    for k in (255, 256, 257):
        p["circle%d" % k] = _ring(k, lambda i: 10.0)
        p["star%d" % k] = _ring(k, lambda i: 11.0 if i % 2 else 3.0)
    return p


def tiny_paths():
    """Paths of 0, 1, 2 and 3 vertices."""
    tri = polygons()["triangle"]
    return [tri[:k] for k in (0, 1, 2, 3)]


def path_cases():
    """[(name, radius)] in a fixed order: the rows of the recorded verdicts."""
    return [(n, r) for n in polygons() for r in RADII]


def base_points():
    """A 0.25 lattice over [-8, 16]^2 -- points exactly on edges and vertices of the integer polygons -- and 1500 random points."""
    g = np.arange(-8.0, 16.0 + 0.125, 0.25)
    lat = np.column_stack((np.repeat(g, g.shape[0]), np.tile(g, g.shape[0])))
    return np.vstack((lat, np.random.default_rng(20261019).uniform(-9.0, 17.0, (1500, 2))))


def corner_points(contour_of):
    """Points on contour corners: of every case's contour (contour_of(vertices, radius) -> [c, 2]) the first 12 and last 4 vertices, and those
    either side of the LDS tile's edge."""
    out = []
    polys = polygons()
    for name, r in path_cases():
        c = contour_of(polys[name], r)
        out += [c[:12], c[-4:], c[TILE - 4:TILE + 4]]
    return np.unique(np.vstack(out), axis=0)


COUNTS = (0, 1, 63, 64, 65, 255, 256, 257)         # point counts around a wave and a workgroup

NONFINITE = {3: (np.nan, 1.0), 17: (1.0, np.nan), 33: (np.inf, 4.0), 34: (4.0, -np.inf), 63: (np.nan, np.nan), 64: (-np.inf, np.inf)}


def raw_tracks():
    """name -> reftrack [n, 4] as the reference's track files hold them (recorded in tests/golden/friction_gen/reference.npz)."""
    z = load_golden("friction_gen/reference")
    return {t: z["%s/reftrack" % t] for t in TRACKS}


def oval(n, rx=40.0, ry=25.0, wr=3.0, wl=2.5):
    """A closed line of n waypoints on an ellipse (the last a step short of the first)."""
    t = np.linspace(0.0, 2.0 * math.pi * (1.0 - 1.0 / n), n)
    return np.column_stack((rx * np.cos(t), ry * np.sin(t), np.full(n, wr), np.full(n, wl)))


def small_tracks():
    """name -> (reftrack, cellwidth): n = 3, the closed / open threshold from both sides, an open arc of the handling track, ovals at the cell
    widths 2.5, 0.3 and 0.1 -- (start + step) - start is not step there, and the axes' length quotients land on an integer (181.0, 201.0, 313.0),
    just above one (33.00000000000001) and just below one (640.9999999999999)."""
    ht = raw_tracks()["handling_track"]
    tri = np.array([(0.0, 0.0, 2.0, 2.0), (6.0, 0.5, 2.0, 1.5), (2.5, 5.0, 1.5, 2.0)])
    under, over = oval(40), oval(40)
    under[-1, :2] = under[0, :2] + (0.0, -9.999)
    over[-1, :2] = over[0, :2] + (0.0, -10.001)
    return {"n3": (tri, 0.7), "gap_under": (under, 2.0), "gap_over": (over, 2.0), "open_arc": (ht[40:160].copy(), 2.0),
            "oval_2p5": (oval(61), 2.5), "oval_0p3": (oval(61, 9.0, 6.0, 1.5, 1.0), 0.3), "oval_0p1": (oval(37, 3.0, 2.0, 0.6, 0.5), 0.1),
            "oval_below": (oval(37, 25.0, 2.0, 0.6, 0.5), 0.1)}       # (x1 + 0.1 - x0) / 0.1 = 640.9999999999999: just below an integer


def refused_tracks():
    """name -> (reftrack, status bit): a NaN waypoint, a waypoint with a zero gradient (its neighbours coincide), fewer than 3 rows."""
    import fgen_ref as fr
    nan = oval(30)
    nan[11, 1] = np.nan
    inf_w = oval(30)
    inf_w[5, 2] = np.inf
    zero = oval(30)
    zero[13, :2] = zero[11, :2]
    return {"nan": (nan, fr.ST_NONFINITE), "inf_width": (inf_w, fr.ST_NONFINITE), "zero_gradient": (zero, fr.ST_NONFINITE),
            "two_rows": (oval(30)[:2], fr.ST_FEW)}


def grid_refused():
    """(reftrack, cellwidth): a 3 km x 2 km oval at a 5 cm cell, 60 442 x 40 242 points, more than 2^31 - 1 -- MCQ_FGEN_GRID; none of them is
    tested or stored.  (The grid's margin of 5 m and more keeps every track above 200 x 200 points at this width: small tracks beside it stay small.)"""
    return oval(30, 1500.0, 1000.0), 0.05
