"""What the friction entries are held to.

An INDEX (accept_indices): no finite query is left out; the returned cell's longdouble distance is within INDEX_TOL = 1e-9 m (the project's metre
floor; coordinates stay below 1e3 m, where a double's rounding is about 1e-13 m) of the minimum over all cells (tests/fric_ref.nearest); where the
gap to the runner-up exceeds INDEX_TOL that leaves one admissible index, which must then also be cKDTree's recorded one where there is a recording.
mue_out is mue[idx_out], bits unchanged.  dist_out: max(1e-9 m, 4 x spread), the project's rule (tests/glue_guard.py), the spread being how far
float64 determines the distance (numpy.hypot in float64 against longdouble).

w_mue: max(floor, 4 x spread) with both numbers from the fixture (scripts/make_golden_friction.py): floor = the largest difference between the
longdouble line and numpy's own polyfit over the whole case table -- the engine need not be nearer the exact answer than the routine every user
has -- and spread = the largest difference between the longdouble line and the float64 closed form summed forwards and backwards."""
import functools
import os

import numpy as np

import fric_ref as fr

LD = np.longdouble
PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "friction", "reference.npz")
INDEX_TOL = 1e-9
DIST_FLOOR = 1e-9
TRACKS = ("rounded_rectangle", "berlin_2018")


@functools.lru_cache(maxsize=None)
def fixture():
    z = np.load(PATH)
    return {k: z[k] for k in z.files}


def w_guard():
    f = fixture()
    return max(float(f["w_floor"]), 4.0 * float(f["w_spread"]))


@functools.lru_cache(maxsize=None)
def recorded(track):
    """The fixture's entries of one track, the map expanded: cells [c, 2] in metres, mue [c]; mue4 [4, rows, jmax] (NaN behind a row's count)."""
    f = fixture()
    g = {k.split("/", 1)[1]: v for k, v in f.items() if k.startswith(track + "/")}
    g["cells"], g["mue"] = g["cells_hm"] / 2.0, g["mue_c"] / 100.0
    g["mue4"] = np.where(g["mue_c4"] == 255, np.nan, g["mue_c4"] / 100.0)
    g["decided"] = np.unpackbits(g["decided"])[:g["mue_c4"].size].reshape(g["mue_c4"].shape).astype(bool)
    g["width"], g["wb_f"], g["wb_r"], g["dn"] = (float(v) for v in f["params"])
    return g


@functools.lru_cache(maxsize=None)
def recorded_nearest(track):
    """tests/fric_ref.nearest on the track's recorded queries: computed once, shared."""
    g = recorded(track)
    return fr.nearest(g["cells"], g["q"])


def accept_indices(cells, mue, q, idx, mue_out=None, dist_out=None, ref=None, ckd=None, label=""):
    """Holds idx (and mue_out, dist_out) of the queries q to the rule above; ref: fric_ref.nearest(cells, q) where the caller has it already.
    Returns the number of queries with one admissible index."""
    q = np.asarray(q, dtype=np.float64).reshape(-1, 2)
    idx = np.asarray(idx).reshape(-1)
    r_idx, r_dist, r_gap = ref if ref is not None else fr.nearest(cells, q)
    fin = np.all(np.isfinite(q), axis=1)
    assert np.all(idx[~fin] == -1), "%s: a query that is not finite has an index" % label
    assert np.all((idx[fin] >= 0) & (idx[fin] < len(cells))), "%s: a finite query was left out" % label
    d = fr.dists_to(cells, q[fin], idx[fin])
    over = d - r_dist[fin]
    assert np.all(over <= INDEX_TOL), "%s: a returned cell is %.3e m farther than the nearest" % (label, float(over.max()))
    single = fin & (r_gap > INDEX_TOL)
    assert np.array_equal(idx[single], r_idx[single]), "%s: the one admissible index was not returned" % label
    if ckd is not None:
        assert np.array_equal(idx[single], np.asarray(ckd)[single]), "%s: differs from cKDTree's recorded index" % label
    if mue_out is not None:
        want = np.where(idx >= 0, np.asarray(mue)[np.maximum(idx, 0)], np.nan)
        assert np.asarray(mue_out).reshape(-1).tobytes() == want.tobytes(), "%s: mue_out is not mue[idx_out]" % label
    if dist_out is not None:
        dist_out = np.asarray(dist_out).reshape(-1)
        assert np.all(np.isnan(dist_out[~fin]))
        c = np.asarray(cells)[idx[fin]]
        spread = np.abs(np.hypot(c[:, 0] - q[fin, 0], c[:, 1] - q[fin, 1]).astype(LD) - d)
        dev = np.abs(dist_out[fin].astype(LD) - d)
        assert np.all(dev <= np.maximum(DIST_FLOOR, 4.0 * spread)), "%s: dist_out off by %.3e m" % (label, float(dev.max()))
    return int(single.sum())
