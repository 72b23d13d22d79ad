"""A plain restatement of the Gaussian-basis friction fit (mcq_friction_gauss_device) and of the models' evaluation (mcq_friction_model_device),
independent of their kernels: numpy only, in float64 or in longdouble, a batch of rows at a time.

The problem is the reference's [REF opt_mintime_traj/src/approx_friction_map.py:102-127, GaussianFeatures] behind sklearn 1.7's dense
LinearRegression: centres numpy.linspace(n[0], n[-1], N) and width 2 (c[1] - c[0]) in FLOAT64 (they are part of the problem's statement), features
exp(-0.5 ((n_j - c_k) / width)^2), column means removed, the minimum-norm least-squares solution with every singular value <= rcond * sigma_max
counted as zero (rcond None: max(cnt, N) * float64's epsilon), intercept mean(mue) - mean(features) . weights.

The singular values come from a plain one-sided Jacobi sweep of this file's own (no LAPACK): rotations from the right until every pair of
columns is orthogonal to the working precision or has a column below the cut; x = V S^+ U^T b.  reverse=True takes every sum over the samples in
the opposite order (tests/fgauss_guard.py: one of the three spreads)."""
import numpy as np

LD = np.longdouble
EPS64 = float(np.finfo(np.float64).eps)
SWEEPS = 60


def centres(n0, n1, N):
    """numpy.linspace(n0, n1, N) and the width, float64."""
    c = np.linspace(np.float64(n0), np.float64(n1), N)
    return c, 2.0 * (c[1] - c[0])


def design(n, N, dtype=np.float64):
    """The features [cnt, N] of one row's positions n [cnt] in dtype (centres and width are float64's)."""
    n = np.asarray(n, dtype=np.float64)
    c, width = centres(n[0], n[-1], N)
    arg = (n.astype(dtype)[:, None] - c.astype(dtype)[None, :]) / dtype(width)
    return np.exp(dtype(-0.5) * (arg * arg))


def center_dist(n, n_gauss):
    return (n[-1] - n[0]) / (2 * n_gauss)


def _ssum(a, reverse):
    """The sum over axis 1 (the samples), forwards or backwards, one term after another."""
    s = np.zeros(a.shape[:1] + a.shape[2:], dtype=a.dtype)
    for j in (range(a.shape[1] - 1, -1, -1) if reverse else range(a.shape[1])):
        s = s + a[:, j]
    return s


def fit_rows(ns, mues, n_gauss, rcond=None, dtype=np.float64, reverse=False):
    """ns: a list of position arrays [cnt_r] (cnt_r >= 2); mues: a list of [4, cnt_r].  Returns a dict of arrays over the rows: w [R, 4, N + 1]
    (weights, intercept), rank [R], sing [R, N] (descending), fitted [list of [4, cnt_r]], sweeps (of the batch), rc [R] the cut's factor."""
    N = 2 * n_gauss + 1
    R, J = len(ns), max(len(n) for n in ns)
    cnt = np.array([len(n) for n in ns])
    F = np.zeros((R, J, N), dtype=dtype)
    B = np.zeros((R, J, 4), dtype=dtype)
    live = np.zeros((R, J), dtype=bool)
    for r, (n, m) in enumerate(zip(ns, mues)):
        F[r, :cnt[r]] = design(n, N, dtype)
        B[r, :cnt[r]] = np.asarray(m, dtype=np.float64).T.astype(dtype)
        live[r, :cnt[r]] = True
    cn = cnt.astype(dtype)
    fmean = _ssum(F, reverse) / cn[:, None]
    bmean = _ssum(B, reverse) / cn[:, None]
    A = np.where(live[:, :, None], F - fmean[:, None, :], dtype(0))
    Bc = np.where(live[:, :, None], B - bmean[:, None, :], dtype(0))
    V = np.broadcast_to(np.eye(N, dtype=dtype), (R, N, N)).copy()          # V[r, i, k]: entry i of column k
    rc = np.array([max(c, N) * EPS64 if rcond is None else rcond for c in cnt], dtype=dtype)
    tol = dtype(np.finfo(dtype).eps) * np.sqrt(cn)
    smax2 = np.zeros(R, dtype=dtype)
    sweeps = 0
    while True:
        sweeps += 1
        assert sweeps <= SWEEPS, "the restatement's Jacobi sweeps do not settle"
        any_rot = False
        for p in range(N - 1):
            for q in range(p + 1, N):
                ap, aq = A[:, :, p], A[:, :, q]
                al, be, ga = _ssum(ap * ap, reverse), _ssum(aq * aq, reverse), _ssum(ap * aq, reverse)
                smax2 = np.maximum(smax2, np.maximum(al, be))
                cut2 = rc * rc * smax2 * dtype(2.0 ** -40)          # (FREEZE: 2^-20 of the cut, squared)
                rot = (al > cut2) & (be > cut2) & (np.abs(ga) > tol * np.sqrt(al * be))
                if not rot.any():
                    continue
                any_rot = True
                g = np.where(rot, ga, dtype(1))
                zeta = (be - al) / (dtype(2) * g)
                t = np.where(zeta < 0, dtype(-1), dtype(1)) / (np.abs(zeta) + np.sqrt(dtype(1) + zeta * zeta))
                cs = dtype(1) / np.sqrt(dtype(1) + t * t)
                sn = cs * t
                cs, sn = np.where(rot, cs, dtype(1)), np.where(rot, sn, dtype(0))
                A[:, :, p], A[:, :, q] = cs[:, None] * ap - sn[:, None] * aq, sn[:, None] * ap + cs[:, None] * aq
                vp, vq = V[:, :, p].copy(), V[:, :, q].copy()
                V[:, :, p], V[:, :, q] = cs[:, None] * vp - sn[:, None] * vq, sn[:, None] * vp + cs[:, None] * vq
        if not any_rot:
            break
    s2 = _ssum(A * A, reverse)                          # [R, N]
    sig = np.sqrt(s2)
    thr = rc * sig.max(axis=1)
    keep = sig > thr[:, None]
    g = np.stack([_ssum(A * Bc[:, :, w:w + 1], reverse) for w in range(4)], axis=1)        # [R, 4, N]
    with np.errstate(divide="ignore", invalid="ignore"):
        z = np.where(keep[:, None, :], g / s2[:, None, :], dtype(0) * g)
    x = np.zeros((R, 4, N), dtype=dtype)
    for k in range(N):
        x = x + V[:, None, :, k] * z[:, :, k:k + 1]
    dot = np.zeros((R, 4), dtype=dtype)
    for i in range(N):
        dot = dot + fmean[:, None, i] * x[:, :, i]
    w = np.concatenate((x, (bmean - dot)[:, :, None]), axis=2)
    fitted = [fitted_values(ns[r], w[r], dtype) for r in range(R)]
    return dict(w=w, rank=keep.sum(axis=1), sing=-np.sort(-sig, axis=1), fitted=fitted, sweeps=sweeps, rc=rc)


def fitted_values(n, w, dtype=LD):
    """features . weights + intercept at the row's own positions, [4, cnt], in dtype from weights w [4, N + 1] of any dtype."""
    w = np.asarray(w).astype(dtype)
    F = design(n, w.shape[1] - 1, dtype)
    out = np.zeros((w.shape[0], len(n)), dtype=dtype)
    for k in range(w.shape[1] - 1):
        out = out + F[None, :, k] * w[:, k:k + 1]
    return out + w[:, -1:]


def decided(sing, cnt, N, rcond=None, margin=4.0):
    """Every singular value of the row lies outside a factor `margin` either side of the cut rcond * sigma_max."""
    sing = np.asarray(sing, dtype=np.float64)
    rc = max(cnt, N) * EPS64 if rcond is None else rcond
    cut = rc * sing.max()
    return bool(np.all((sing > margin * cut) | (sing < cut / margin)))


def gap_decades(sing, cnt, N, rcond=None):
    """The least distance of a singular value from the cut, in decades."""
    sing = np.asarray(sing, dtype=np.float64)
    rc = max(cnt, N) * EPS64 if rcond is None else rcond
    cut = rc * sing.max()
    with np.errstate(divide="ignore"):
        return float(np.min(np.abs(np.log10(np.maximum(sing, 1e-300) / cut))))


# ---- evaluation --------------------------------------------------------------------------------------------------------------------------------
def model_linear(q, w):
    """slope * q + intercept in two roundings: q [qcnt], w [4, 2] -> [4, qcnt] float64."""
    q, w = np.asarray(q, dtype=np.float64), np.asarray(w, dtype=np.float64)
    return w[:, :1] * q[None, :] + w[:, 1:]


def model_gauss(q, w, cd, n_gauss, n0=None, n1=None, mintime=False, dtype=LD):
    """The Gaussian model at q [qcnt] from w [4, N + 1]: the fit's centres (n0, n1 given: linspace(n0, n1, N), width 2 (c[1] - c[0])) or the
    consumer's (numpy.linspace(-n_gauss, n_gauss, N) * cd, sigma = 2 cd) -> [4, qcnt] in dtype."""
    N = 2 * n_gauss + 1
    q, w = np.asarray(q, dtype=np.float64).astype(dtype), np.asarray(w, dtype=np.float64).astype(dtype)
    if mintime:
        sigma = 2.0 * np.float64(cd)
        c = np.linspace(-n_gauss, n_gauss, N) * np.float64(cd)
        d = q[:, None] - c.astype(dtype)[None, :]
        F = np.exp(-(d * d) / dtype(2.0 * (sigma * sigma)))
    else:
        c, width = centres(n0, n1, N)
        arg = (q[:, None] - c.astype(dtype)[None, :]) / dtype(width)
        F = np.exp(dtype(-0.5) * (arg * arg))
    out = np.zeros((w.shape[0], len(q)), dtype=dtype)
    for k in range(N):
        out = out + F[None, :, k] * w[:, k:k + 1]
    return out + w[:, -1:]
