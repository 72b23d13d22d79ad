"""Friction maps behind the reference's names [REF opt_mintime_traj/src/friction_map_interface.py, extract_friction_coeffs.py,
approx_friction_map.py]: the same argument names, return shapes and error behaviour, on the engine's device entries (include/mcq.h "friction
maps": mcq_fmap_create, mcq_fmap_query_device, mcq_friction_grid_device).

  load_friction_map(tpamap_path, tpadata_path)          the two files as (cells [c, 2], mue [c]); a cell without data is NaN
  FrictionMapInterface(tpamap_path, tpadata_path)       .get_friction_singlepos(positions) -> [k, 1]
  extract_friction_coeffs(...)                          -> n, mue_fl, mue_fr, mue_rl, mue_rr: lists with one entry per row of the closed track
  approx_friction_map(...)                              -> w_mue_fl, w_mue_fr, w_mue_rl, w_mue_rr, center_dist for var_friction == "linear"
  approx_friction_map_gauss(...)                        the same five for var_friction == "gauss": [rows, 2 n_gauss + 2] each, center_dist [rows, 1]
  eval_friction_model(q, w_mue_fl, ..., center_dist)    either model at lateral positions (mcq_friction_model_device)
  check_isclosed_refline(refline), calc_trackboundaries(reftrack)       [REF frictionmap/src/reftrack_functions.py], the latter on the device
  gen_friction_map(reftrack, cellwidth_m, initial_mue, inside_trackbound)   -> (cells, mue): the reference's main_gen_frictionmap.py
                                                        (mcq_friction_gen_device), cell for cell matplotlib's contains_points verdicts
  write_friction_map(cells, mue, tpamap_path, tpadata_path)             the two files that script writes, byte for byte

Differences from the reference, all stated in include/mcq.h: among cells at exactly the same distance the lowest index is taken (scipy's cKDTree
documents no rule); a row of exactly one lateral position has a NaN line where numpy.polyfit returns a minimum-norm answer with a RankWarning.
var_friction == "gauss" (an sklearn pipeline of Gaussian features and a LinearRegression) is approx_friction_map_gauss: the minimum-norm solution
under sklearn's cut-off from a one-sided Jacobi decomposition on the device (mcq_friction_gauss_device) -- equal to sklearn's to the problem's
conditioning, not bit for bit.  approx_friction_map itself raises NotImplementedError for "gauss" unless MCQ_GAUSS_DEVICE=1 is set in the
environment (read at every call, like MCQ_PREP_DEVICE and MCQ_FIT_DEVICE); then it calls approx_friction_map_gauss.  plot_debug is ignored.
Every function takes an `engine` keyword (default: engine.default_engine())."""
import json
import math
import os

import numpy as np

from . import engine as _engine


def load_friction_map(tpamap_path, tpadata_path):
    """(cells [c, 2], mue [c]): the map file as numpy.loadtxt reads it (comments '#', delimiter ';'), the data file's keys as ints, each value a
    list of one number (ValueError otherwise); a cell the data file does not name has mue NaN."""
    cells = np.loadtxt(tpamap_path, comments='#', delimiter=';').reshape(-1, 2)
    with open(tpadata_path, 'r') as fh:
        data = json.load(fh)
    mue = np.full(cells.shape[0], np.nan)
    for k, v in data.items():
        i = int(k)
        if not isinstance(v, list) or len(v) != 1 or isinstance(v[0], (list, dict, str, bool)) or v[0] is None:
            raise ValueError("tpadata entry %r: expected a list of one number, got %r" % (k, v))
        if not 0 <= i < cells.shape[0]:
            raise ValueError("tpadata entry %r names no cell of the map (%d cells)" % (k, cells.shape[0]))
        mue[i] = float(v[0])
    return cells, mue


class FrictionMapInterface:
    """The reference's class on a device-resident map."""

    def __init__(self, tpamap_path, tpadata_path, engine=None):
        self.engine = engine or _engine.default_engine()
        self.fmap = self.engine.friction_map(*load_friction_map(tpamap_path, tpadata_path))

    def close(self):
        self.fmap.close()

    def get_friction_singlepos(self, positions):
        """[[mue_0], [mue_1], ...] for positions [[x_0, y_0], ...]; numpy.asarray([]) for an empty input; KeyError (the cell's index) where the
        nearest cell has no data, as the reference's dict lookup raises."""
        positions = np.asarray(positions, dtype=np.float64)
        if positions.size == 0:
            return np.asarray([])
        mue, idx = self.engine.friction_query_batch(self.fmap, positions.reshape(-1, 2), want_idx=True)
        _raise_missing(mue, idx)
        return mue.reshape(-1, 1)


def _raise_missing(mue, idx):
    miss = np.isnan(mue) & (idx >= 0)
    if np.any(miss):
        raise KeyError(int(idx[miss][0]))


def _grid(reftrack, normvectors, tpamap_path, tpadata_path, pars, dn, fit, engine, n_gauss=5):
    eng = engine or _engine.default_engine()
    reftrack, normvectors = np.asarray(reftrack, dtype=np.float64), np.asarray(normvectors, dtype=np.float64)
    width = pars["optim_opts"]["width_opt"]
    wb_f = pars["vehicle_params_mintime"]["wheelbase_front"]
    wb_r = pars["vehicle_params_mintime"]["wheelbase_rear"]
    cells, mue = load_friction_map(tpamap_path, tpadata_path)
    with eng.friction_map(cells, mue) as fmap:
        g = eng.friction_grid_batch(fmap, [reftrack], [normvectors], float(width), wb_f, wb_r, float(dn), fit=fit, want_idx=True, n_gauss=n_gauss)
    if g["status"][0] != 0:
        raise ValueError("friction grid: the track was refused (a row that is not finite?)")
    rows = int(g["rows"][0])
    cnt = g["cnt"][0, :rows]
    if np.any(cnt < 0):     # numpy.linspace's own words
        raise ValueError("Number of samples, %d, must be non-negative." % int(cnt[cnt < 0][0]))
    for w in range(4):
        for i in range(rows):
            _raise_missing(g["mue"][0, w, i, :cnt[i]], g["idx"][0, w, i, :cnt[i]])
    return g, rows, cnt


def extract_friction_coeffs(reftrack, normvectors, tpamap_path, tpadata_path, pars, dn, print_debug=False, plot_debug=False, engine=None):
    """n, mue_fl, mue_fr, mue_rl, mue_rr: lists of len(reftrack) + 1 entries; n[i] is [cnt_i], mue_x[i] is [cnt_i, 1] (numpy.asarray([]) for an
    empty row, as the reference's interface returns for an empty input)."""
    g, rows, cnt = _grid(reftrack, normvectors, tpamap_path, tpadata_path, pars, dn, False, engine)
    n = [g["n"][0, i, :cnt[i]].copy() for i in range(rows)]
    mue = [[g["mue"][0, w, i, :cnt[i]].reshape(-1, 1).copy() if cnt[i] else np.asarray([]) for i in range(rows)] for w in range(4)]
    return n, mue[0], mue[1], mue[2], mue[3]


def approx_friction_map(reftrack, normvectors, tpamap_path, tpadata_path, pars, dn, n_gauss=0, print_debug=False, plot_debug=False, engine=None):
    """w_mue_fl, w_mue_fr, w_mue_rl, w_mue_rr [rows, 2] (slope, intercept per row: numpy.polyfit's order) and center_dist [rows, 1] (zeros) for
    pars["optim_opts"]["var_friction"] == "linear"."""
    method = pars["optim_opts"]["var_friction"]
    if method == "gauss":
        if os.environ.get("MCQ_GAUSS_DEVICE") == "1":
            return approx_friction_map_gauss(reftrack, normvectors, tpamap_path, tpadata_path, pars, dn, n_gauss, print_debug, plot_debug, engine=engine)
        raise NotImplementedError("var_friction 'gauss' (regression with Gaussian basis functions) runs on the device with MCQ_GAUSS_DEVICE=1 in "
                                  "the environment, or through approx_friction_map_gauss")
    if method != "linear":
        raise ValueError('Unknown method for friction map approximation!')
    g, rows, cnt = _grid(reftrack, normvectors, tpamap_path, tpadata_path, pars, dn, True, engine)
    if np.any(cnt == 0):    # numpy.polyfit's own words
        raise TypeError("expected non-empty vector for x")
    w = [g["w_mue"][0, k, :rows].copy() for k in range(4)]
    return w[0], w[1], w[2], w[3], np.zeros((rows, 1))


def approx_friction_map_gauss(reftrack, normvectors, tpamap_path, tpadata_path, pars, dn, n_gauss, print_debug=False, plot_debug=False, engine=None):
    """w_mue_fl, w_mue_fr, w_mue_rl, w_mue_rr [rows, 2 n_gauss + 2] (the weights of the 2 n_gauss + 1 Gaussian bumps, then the intercept) and
    center_dist [rows, 1]: the reference's var_friction == "gauss" (mcq_friction_gauss_device).  ValueError where the reference fails: n_gauss
    outside 1 .. 15, a row of fewer than two lateral positions (its features are NaN and sklearn raises), a row that did not settle."""
    n_gauss = int(n_gauss)
    if not 1 <= n_gauss <= 15:
        raise ValueError("approx_friction_map_gauss: n_gauss must be 1 .. 15, got %d" % n_gauss)
    g, rows, cnt = _grid(reftrack, normvectors, tpamap_path, tpadata_path, pars, dn, "gauss", engine, n_gauss)
    if np.any(cnt <= 1):
        i = int(np.flatnonzero(cnt <= 1)[0])
        raise ValueError("approx_friction_map_gauss: row %d has %d lateral position(s); the Gaussian basis needs two" % (i, int(cnt[i])))
    if np.any(g["rank"][0, :rows] < 0):
        raise ValueError("approx_friction_map_gauss: row %d did not settle" % int(np.flatnonzero(g["rank"][0, :rows] < 0)[0]))
    w = [g["w_gauss"][0, k, :rows].copy() for k in range(4)]
    return w[0], w[1], w[2], w[3], g["center_dist"][0, :rows].reshape(-1, 1).copy()


def eval_friction_model(q, w_mue_fl, w_mue_fr, w_mue_rl, w_mue_rr, center_dist=None, mintime=True, n=None, engine=None):
    """mue_fl, mue_fr, mue_rl, mue_rr [rows, k] at the lateral positions q [rows, k] (or [rows]: one per row) of either model's weights
    [rows, P]: P == 2 the lines (slope * q + intercept), else the Gaussian model with center_dist [rows, 1].  mintime=True places the bumps as
    the reference's consumer does (numpy.linspace(-n_gauss, n_gauss, N) * center_dist, sigma = 2 center_dist [REF opt_mintime.py:733-747]);
    mintime=False as the fit did, which takes n: extract_friction_coeffs' list of positions.  The two agree only for rows symmetric about 0."""
    eng = engine or _engine.default_engine()
    w = np.stack([np.asarray(a, dtype=np.float64) for a in (w_mue_fl, w_mue_fr, w_mue_rl, w_mue_rr)])[None]        # [1, 4, rows, P]
    rows = w.shape[2]
    q = np.asarray(q, dtype=np.float64)
    flat = q.ndim == 1
    q = q.reshape(rows, -1)[None]
    kw = {}
    if w.shape[3] != 2:
        if center_dist is None:
            raise ValueError("eval_friction_model: the Gaussian model takes center_dist")
        kw = dict(center_dist=np.asarray(center_dist, dtype=np.float64).reshape(1, rows), centres=_engine.FRIC_CENTRES_MINTIME)
        if not mintime:
            if n is None or len(n) != rows:
                raise ValueError("eval_friction_model: mintime=False takes the rows' positions n")
            cnt = np.array([len(r) for r in n], dtype=np.int32)
            n_pad = np.full((rows, max(int(cnt.max()), 1)), np.nan)
            for i, r in enumerate(n):
                n_pad[i, :cnt[i]] = r
            kw.update(centres=_engine.FRIC_CENTRES_FIT, n=n_pad[None], cnt=cnt[None])
    out = eng.friction_model_batch(q, w, **kw)[0]
    return tuple(out[k, :, 0].copy() if flat else out[k].copy() for k in range(4))


# ---- generating a map [REF main_gen_frictionmap.py, frictionmap/src/reftrack_functions.py] ---------------------------------------------------------
def check_isclosed_refline(refline):
    """True where the last point of the reference line [n, 2] lies within 10 m of the first: the track is a circuit."""
    refline = np.asarray(refline, dtype=np.float64)
    return math.sqrt((refline[-1, 0] - refline[0, 0]) ** 2 + (refline[-1, 1] - refline[0, 1]) ** 2) <= 10.0


def _gen(reftrack, cellwidth_m, inside_trackbound, engine):
    eng = engine or _engine.default_engine()
    reftrack = np.asarray(reftrack, dtype=np.float64)
    if reftrack.ndim != 2 or reftrack.shape[1] < 4:
        raise ValueError("reftrack must be [n, 4]: x_m, y_m, trackwidth_right_m, trackwidth_left_m")
    if inside_trackbound not in ("right", "left"):
        raise ValueError("inside_trackbound must be 'right' or 'left'")
    g = eng.friction_gen_batch([reftrack], float(cellwidth_m), inside_trackbound)
    st = int(g["status"][0])
    if st & _engine.FGEN_FEW:
        raise ValueError("the reference track needs at least 3 waypoints")
    if st & _engine.FGEN_NONFINITE:
        raise ValueError("the reference track, or a boundary derived from it, is not finite (a NaN, or a waypoint whose neighbours coincide)")
    if st & _engine.FGEN_GRID:
        raise ValueError("the grid has more than 2^31 - 1 points at this cell width")
    return g


def calc_trackboundaries(reftrack, engine=None):
    """(track_boundary_right, track_boundary_left), [n, 2] each, of reftrack [n, 4] = x_m, y_m, trackwidth_right_m, trackwidth_left_m: the
    reference's bits, from the boundaries-only form of mcq_friction_gen_device (Engine.track_boundaries_batch: no grid, no cells).  As in the
    reference, a waypoint whose neighbours coincide (a zero gradient) has NaN rows and nothing is raised (a NaN's sign bit is the device's).  Differences: a NaN or infinite entry
    anywhere makes EVERY row NaN (numpy keeps the rows the entry does not reach), and fewer than 3 waypoints is a ValueError."""
    eng = engine or _engine.default_engine()
    reftrack = np.asarray(reftrack, dtype=np.float64)
    if reftrack.ndim != 2 or reftrack.shape[1] < 4:
        raise ValueError("reftrack must be [n, 4]: x_m, y_m, trackwidth_right_m, trackwidth_left_m")
    right, left, status = eng.track_boundaries_batch([reftrack])
    if int(status[0]) & _engine.FGEN_FEW:
        raise ValueError("the reference track needs at least 3 waypoints")
    return right[0], left[0]


def gen_friction_map(reftrack, cellwidth_m, initial_mue, inside_trackbound="right", engine=None):
    """(cells [c, 2], mue [c]) of the reference's script: the points of its grid that lie on the track or within 1.1 cell widths of it, in its
    order, each with initial_mue.  inside_trackbound ('right' / 'left') matters for circuits only -- with the wrong one the map is EMPTY, as
    the reference's is (the offset's side follows the boundary's orientation).  ValueError for a track the entry refuses."""
    if not float(cellwidth_m) > 0.0 or not math.isfinite(float(cellwidth_m)):
        raise ValueError("cellwidth_m must be positive")
    cells = _gen(reftrack, cellwidth_m, inside_trackbound, engine)["cells"][0]
    return cells, np.full(cells.shape[0], float(initial_mue))


def write_friction_map(cells, mue, tpamap_path, tpadata_path):
    """The reference's two files, byte for byte: '*_tpamap.csv' (numpy.savetxt, '%0.4f', ';', header 'x_m;y_m') and '*_tpadata.json'
    ({"i": [mue_i], ...} with the separators (',', ': ')).  The reference writes the JSON's keys in the order of its cKDTree's index array, a
    by-product of the tree's build; the same tree is built here for the same order (the content does not depend on it).  load_friction_map
    reads the files back."""
    from scipy.spatial import cKDTree
    cells, mue = np.asarray(cells, dtype=np.float64).reshape(-1, 2), np.asarray(mue, dtype=np.float64).reshape(-1)
    if mue.shape[0] != cells.shape[0]:
        raise ValueError("write_friction_map: cells must be [c, 2] and mue [c]")
    with open(tpamap_path, 'wb') as fh:
        np.savetxt(fh, cells, fmt='%0.4f', delimiter=';', header='x_m;y_m')
    order = cKDTree(cells).indices.tolist() if cells.shape[0] else []
    with open(tpadata_path, 'w') as fh:
        json.dump({str(i): [float(mue[i])] for i in order}, fh, separators=(',', ': '))
