"""Friction maps behind the reference's names [REF opt_mintime_traj/src/friction_map_interface.py, extract_friction_coeffs.py,
approx_friction_map.py]: the same argument names, return shapes and error behaviour, on the engine's device entries (include/mcq.h "friction
maps": mcq_fmap_create, mcq_fmap_query_device, mcq_friction_grid_device).

  load_friction_map(tpamap_path, tpadata_path)          the two files as (cells [c, 2], mue [c]); a cell without data is NaN
  FrictionMapInterface(tpamap_path, tpadata_path)       .get_friction_singlepos(positions) -> [k, 1]
  extract_friction_coeffs(...)                          -> n, mue_fl, mue_fr, mue_rl, mue_rr: lists with one entry per row of the closed track
  approx_friction_map(...)                              -> w_mue_fl, w_mue_fr, w_mue_rl, w_mue_rr, center_dist for var_friction == "linear"
  approx_friction_map_gauss(...)                        the same five for var_friction == "gauss": [rows, 2 n_gauss + 2] each, center_dist [rows, 1]
  eval_friction_model(q, w_mue_fl, ..., center_dist)    either model at lateral positions (mcq_friction_model_device)

Differences from the reference, all stated in include/mcq.h: among cells at exactly the same distance the lowest index is taken (scipy's cKDTree
documents no rule); a row of exactly one lateral position has a NaN line where numpy.polyfit returns a minimum-norm answer with a RankWarning.
var_friction == "gauss" (an sklearn pipeline of Gaussian features and a LinearRegression) is approx_friction_map_gauss: the minimum-norm solution
under sklearn's cut-off from a one-sided Jacobi decomposition on the device (mcq_friction_gauss_device) -- equal to sklearn's to the problem's
conditioning, not bit for bit.  approx_friction_map itself raises NotImplementedError for "gauss" unless MCQ_GAUSS_DEVICE=1 is set in the
environment (read at every call, like MCQ_PREP_DEVICE and MCQ_FIT_DEVICE); then it calls approx_friction_map_gauss.  plot_debug is ignored.
Every function takes an `engine` keyword (default: engine.default_engine())."""
import json
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
