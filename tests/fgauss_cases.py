"""The hand-made rows of the Gaussian friction fit's tests: the smallest shapes at which mcq_friction_gauss_device can go wrong.  A LAUNCH is one call:
one n_gauss, a few tracks of rows; a row is its positions n [cnt] and the four wheels' friction [4, cnt].  The rows go to the entry as the arrays
mcq_friction_grid_device would have left (arrays()), so every count and every value is the table's own.

Positions: pos(cnt, kind).  'A' is numpy.linspace(-3.1, 3.4, cnt).  Equidistant positions are symmetric about the row's middle, and so are the
centres: the features split into an even and an odd part and a row of N + 1 positions has rank N - 1, not N, with a computed zero wherever rounding
leaves it.  'B' and 'C' move the inner positions off the lattice (by a fixed sine, no random numbers), which gives the step to full rank at
cnt = N + 1 with margin; tests/test_fgauss_ref.py asserts the margins this table relies on."""
import functools

import numpy as np

import fgauss_ref as gr

OK, BAD = 0, 4
RANGES = {"A": (-3.1, 3.4, 0.0, 0.0), "B": (-3.1, 3.4, 0.3, 0.4), "C": (-2.25, 4.0, 0.2, 1.1)}


def pos(cnt, kind="A"):
    lo, hi, amp, ph = RANGES[kind]
    if cnt == 1:
        return np.array([0.25])
    n = np.linspace(lo, hi, cnt)
    if amp and cnt > 2:
        n = n + ((hi - lo) / (cnt - 1)) * amp * np.sin(2.3 * np.arange(cnt) + ph)
        n[0], n[-1] = lo, hi
    return n


def mue_of(n, kind="smooth"):
    """[4, cnt] in hundredths, as a friction map's values are: a smooth variation with a step, differing by wheel."""
    n = np.asarray(n)
    if kind == "const":
        return np.ones((4, len(n)))
    m = np.stack([np.round(1.0 + 0.15 * np.sin(1.7 * n + 0.6 * k) + 0.04 * (n > 0.3 - 0.2 * k), 2) for k in range(4)])
    if kind == "step":
        m = np.stack([np.where(n > 0.1 * k, 1.15, 0.85) for k in range(4)])
    if kind == "outlier":
        m = np.ones((4, len(n)))
        m[:, len(n) // 3] = 0.6
    if kind == "nan1":
        m[2, len(n) // 2] = np.nan
    return m


def row(cnt, kind="A", mue="smooth", n=None):
    if cnt <= 0:
        return dict(cnt=cnt, n=np.zeros(0), mue=np.zeros((4, 0)), label="cnt %d" % cnt)
    n = pos(cnt, kind) if n is None else np.asarray(n, dtype=np.float64)
    return dict(cnt=cnt, n=n, mue=mue_of(n, mue), label="cnt %d %s %s" % (cnt, kind, mue))


def _shapes(N):
    """cnt = 2, 3, N - 1, N, N + 1, N + 2: the rank is min(cnt - 1, N) (off the lattice at N + 1), the step to full rank lies at N + 1."""
    out = []
    for c in sorted({2, 3, N - 1, N, N + 1, N + 2}):
        out.append(row(c, "C" if (N, c) == (3, 3) else ("B" if c == N + 1 else "A")))
    return out


REFUSED = "refused"         # a track the grid call refused: status MCQ_BAD_INPUT, counts that exceed jmax (what cnt_out reports then)


@functools.lru_cache(maxsize=None)
def launches():
    dn = 0.25
    edges = [row(1), row(0), row(-1)]
    return {
        "n1": dict(n_gauss=1, tracks=[_shapes(3) + edges + [row(9, mue="const"), row(9, mue="nan1")], REFUSED,
                                      [row(63), row(64), row(65), row(12, mue="step"), row(12, mue="outlier")]]),
        "n5": dict(n_gauss=5, tracks=[_shapes(11) + [row(24, n=np.linspace(-dn * 7, dn * 16, 24)), row(21, n=np.linspace(-dn * 10, dn * 10, 21)),
                                                     row(30, mue="const"), row(30, mue="nan1")], REFUSED,
                                      [row(63), row(64), row(65), row(40, mue="step"), row(40, mue="outlier")] + edges, [row(17, "B")]]),
        "n15": dict(n_gauss=15, tracks=[_shapes(31) + [row(27)], [row(64), row(65), row(1), row(0)]]),
    }


SYMMETRIC = ("n5", 0, 7)        # launch, track, row: positions symmetric about 0 (num_right == num_left)
ASYMMETRIC = ("n5", 0, 6)       # num_right != num_left (7 and 16 steps)
RCOND_ROW = ("n5", 2, 3)        # the row of the explicit-rcond case (40 positions, full rank under sklearn's cut)


def arrays(launch, order=None):
    """The launch as mcq_friction_grid_device's outputs: n [T, rows, jmax], cnt [T, rows], mue [T, 4, rows, jmax], status [T]; a refused track
    has status MCQ_BAD_INPUT and counts of 1000.  order: a permutation of the tracks.  rows = the longest track's (at least 2)."""
    tracks = launch["tracks"] if order is None else [launch["tracks"][t] for t in order]
    rows = max(2, max(len(t) for t in tracks if t is not REFUSED))
    jmax = max(r["cnt"] for t in tracks if t is not REFUSED for r in t)
    T = len(tracks)
    n = np.full((T, rows, jmax), np.nan)
    cnt = np.zeros((T, rows), dtype=np.int32)
    mue = np.full((T, 4, rows, jmax), np.nan)
    status = np.zeros(T, dtype=np.int32)
    for t, tr in enumerate(tracks):
        if tr is REFUSED:
            status[t], cnt[t] = BAD, 1000
            continue
        for i, r in enumerate(tr):
            c = max(r["cnt"], 0)
            cnt[t, i] = r["cnt"]
            n[t, i, :c], mue[t, :, i, :c] = r["n"], r["mue"]
    return n, cnt, mue, status


def fitted_rows(launch):
    """(track, row, row dict) of every row that has a fit: cnt >= 2."""
    return [(t, i, r) for t, tr in enumerate(launch["tracks"]) if tr is not REFUSED for i, r in enumerate(tr) if r["cnt"] >= 2]


@functools.lru_cache(maxsize=None)
def rcond_case():
    """The explicit rcond: between the two smallest singular values of RCOND_ROW (the float64 restatement's), at their geometric mean -- it removes
    exactly one more than sklearn's cut does.  Returns (row dict, n_gauss, rcond, ratio of the two values: the margin either side is its root)."""
    name, t, i = RCOND_ROW
    L = launches()[name]
    r = L["tracks"][t][i]
    s = gr.fit_rows([r["n"]], [mue_of(r["n"])], L["n_gauss"])["sing"][0]
    return r, L["n_gauss"], float(np.sqrt(s[-1] * s[-2]) / s[0]), float(s[-2] / s[-1])


def eval_positions(r):
    """Positions on, between and outside a row's sampled range."""
    n = r["n"]
    return np.concatenate((n[:3], 0.5 * (n[:-1] + n[1:])[:4], [n[0] - 0.7, n[-1] + 1.3, 0.0], n[-2:]))
