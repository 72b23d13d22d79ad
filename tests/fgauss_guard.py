"""What the Gaussian friction fit (mcq_friction_gauss_device) is held to.

The reference is the longdouble restatement (tests/fgauss_ref.py).  guard = max(floor, 4 x spread), the project's rule (tests/fric_guard.py,
tests/glue_guard.py): floor = the w_floor of tests/fric_guard.py's fixture; spread = the largest deviation from the longdouble restatement of
three things -- sklearn's recording, the float64 restatement, the float64 restatement with its sums reversed -- written into
tests/golden/friction_gauss/reference.npz by scripts/make_golden_friction_gauss.py.  A CASE is a hand-made row, or a whole track at one n_gauss
(the largest spread over its rows).  The guard is applied twice: to the weights, and to the fitted values features . weights + intercept formed
on the host in longdouble from the weights under test -- the tight check, because the weights carry the problem's conditioning (sigma_min /
sigma_max is about 6e-7 at n_gauss = 5) and the fitted values do not.  center_dist and the rank are compared exactly.

A row is DECIDED when every singular value lies outside a factor 4 either side of the cut, by sklearn's recorded values AND by the float64
restatement's; rank and weights are compared on decided rows only (an undecided row has two defensible answers).  tests/test_fgauss_ref.py
asserts which rows are undecided: none of the whole tracks', and of the hand-made rows the one named in LAPACK_FLOOR."""
import functools
import os

import numpy as np

import fgauss_cases as gc
import fgauss_ref as gr
import fric_guard as fg

LD = np.longdouble
PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "friction_gauss", "reference.npz")
TRACKS = fg.TRACKS
N_GAUSS = (1, 5)
# The one hand-made row sklearn's own values leave undecided: N = 31 with cnt = 31 has rank 30 (centring removes one), and LAPACK's gelsd reports
# the vanished singular value as 0.52 of the cut (at more than 25 columns its divide-and-conquer solver raises tiny values to a floor) -- for
# every choice of positions tried.  The float64 restatement decides the row (its zero lies 3.4 decades below the cut).
LAPACK_FLOOR = {("n15", "cnt 31 A smooth")}


@functools.lru_cache(maxsize=None)
def fixture():
    z = np.load(PATH)
    return {k: z[k] for k in z.files}


def floor():
    return float(fg.fixture()["w_floor"])


def guard(spread):
    return max(floor(), 4.0 * float(spread))


@functools.lru_cache(maxsize=None)
def track_rows(track):
    """(ns, mues) of a recorded track's rows: the grids of tests/golden/friction/reference.npz."""
    g = fg.recorded(track)
    cnt = g["cnt"]
    return [g["n"][i, :cnt[i]] for i in range(len(cnt))], [g["mue4"][:, i, :cnt[i]] for i in range(len(cnt))]


@functools.lru_cache(maxsize=None)
def track_restated(track, n_gauss, dtype_name="longdouble"):
    """The restatement of a whole track: computed once, shared, not to be changed."""
    ns, mues = track_rows(track)
    return gr.fit_rows(ns, mues, n_gauss, dtype=LD if dtype_name == "longdouble" else np.float64)


@functools.lru_cache(maxsize=None)
def launch_restated(name, dtype_name="longdouble"):
    L = gc.launches()[name]
    rows = gc.fitted_rows(L)
    return gr.fit_rows([r["n"] for _, _, r in rows], [r["mue"] for _, _, r in rows], L["n_gauss"],
                       dtype=LD if dtype_name == "longdouble" else np.float64)


def _decided(sing_rec, sing_f64, cnts, N):
    out = []
    for s, f, c in zip(sing_rec, sing_f64, cnts):
        out.append(gr.decided(s[:min(c, N)], c, N) and gr.decided(f, c, N))
    return np.array(out)


@functools.lru_cache(maxsize=None)
def track_decided(track, n_gauss):
    f, N = fixture(), 2 * n_gauss + 1
    ns, _ = track_rows(track)
    return _decided(f["%s/g%d/sing" % (track, n_gauss)], track_restated(track, n_gauss, "float64")["sing"], [len(n) for n in ns], N)


@functools.lru_cache(maxsize=None)
def launch_decided(name):
    L = gc.launches()[name]
    return _decided(fixture()[name + "/sing"], launch_restated(name, "float64")["sing"], [r["cnt"] for _, _, r in gc.fitted_rows(L)],
                    2 * L["n_gauss"] + 1)


def track_guards(track, n_gauss):
    """(weights, fitted values): one pair for the whole track."""
    f = fixture()
    pre = "%s/g%d/" % (track, n_gauss)
    return guard(f[pre + "spread_w"].max()), guard(f[pre + "spread_f"].max())


def launch_guards(name):
    """(weights [k], fitted values [k]) over fgauss_cases.fitted_rows: a pair per row."""
    f = fixture()
    return np.array([guard(s) for s in f[name + "/spread_w"]]), np.array([guard(s) for s in f[name + "/spread_f"]])


def eval_tol(q, w, centres, width, n_gauss):
    """How far float64 determines sum_k f_k w_k + b at q [k] for weights w [4, N + 1]: the sum of N + 1 rounded products takes (N + 2) eps of
    sum |f_k w_k| + |b|; a feature exp(-0.5 a^2) carries the rounding of a (2 eps relative: a difference and a quotient) times a^2, the product's
    and the exponential's own (4 eps together).  Used only where a float64 evaluation is compared with the longdouble evaluation of the SAME
    weights, for which the issue sets no bound; the comparison with the recorded predict is held to the fitted-value guard alone.  Per position: (N + 6 + 2 max a^2) eps (sum_k |f_k w_k| + |b|) -> [4, k] float64."""
    q, w = np.asarray(q, dtype=np.float64), np.abs(np.asarray(w, dtype=np.float64))
    a = (q[:, None] - np.asarray(centres)[None, :]) / width
    f = np.exp(-0.5 * a * a)
    mag = w[:, None, :-1] * f[None, :, :]
    N = 2 * n_gauss + 1
    return (N + 6 + 2.0 * (a * a).max(axis=1))[None, :] * gr.EPS64 * (mag.sum(axis=2) + w[:, -1:])
