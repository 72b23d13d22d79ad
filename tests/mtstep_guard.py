"""What mcq_mintime_step_device is held to.  The reference is tests/mtstep_ref.py's self-certified longdouble solution of the longdouble-assembled K.

1. Backward error, independent of conditioning: per row i  |rhs - K x|_i <= (nnz_i + 2) eps (|K| |x| + |rhs|)_i  in longdouble, nnz_i the non-zeros
   of row i of the assembled K.  The kernel's last correction solves K dx = r with r the float64 residual: what is left is that residual's own
   rounding -- nnz_i products and sums, each within eps of a partial sum bounded by (|K| |x| + |rhs|)_i: the count's factor 1 -- plus the rounding
   of x + dx (half an eps of |K| |x|) and of the subtraction from rhs: the 2.
2. Forward error: |x - x_ref| <= max(floor, 4 x spread) max |x_ref|.
   spread: the largest deviation from the reference, relative to max |x_ref|, of the float64 restatement of the static-order LDL^T (mtstep_ref.Factor
   with pivoting off on the float64-rounded K) with `refine` float64 refinements, in two stage orders, forward and reversed; per key and refine in
   tests/golden/mintime/mtstep_spread.npz, written by scripts/make_golden_mtstep_spread.py.  Measured on the CPU, never against the code under test.
   floor: a solution whose rows meet item 1's bound beta_i differs from the exact one by K^-1 r with |r| <= beta, so
       |x - x_exact| <= |K^-1| beta   componentwise (Skeel),
   relative to max |x_ref|.  N <= 65: |K^-1| from the inverse of the float64-rounded K, which at these condition numbers (up to 1e14) is itself
   accurate to a few per cent of its large entries: times 2.  Above: |K^-1| beta is not formed; the reference's own solves of four seeded sign
   patterns s, max |K^-1 (s o beta)|, bound it from below, and |K^-1| beta <= sqrt(n) times a typical such product for entries of mixed sign: the
   maximum over the four, times 4 sqrt(nnz_max), is taken.  With refine < 2 item 1 is not promised; the floor stays and the spread of that refine
   count decides.
3. inertia_out equals the reference's where the case is DECIDED: the static-order LDL^T in longdouble agrees in its two stage orders, and its
   smallest |pivot| lies a factor 4 above the rounding level of its own elimination, growth x eps_longdouble x max |K|.
4. res_out equals the longdouble residual's max-norm within max_i beta_i (item 1's count bounds the float64 evaluation of one row as well)."""
import functools
import os

import numpy as np

import mtstep_cases as sc
import mtstep_ref as sr

LD = np.longdouble
EPS = sr.EPS
PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mintime", "mtstep_spread.npz")


@functools.lru_cache(maxsize=None)
def reference(key, nvec=2):
    """dict(chain, x [nvec, n], omega, inertia, decided, nnz) of a key: the pivoted bordered elimination refined to longdouble rounding, the
    static LDL^T's pivot signs in two orders.  Cached: shared, not to be changed."""
    inp = sc.inputs(key, nvec)
    trip = sc.triplets_of(inp)
    ch = sr.Chain(trip, inp["N"], inp["safe"], inp["energy"])
    fac = sr.Factor(ch, True)
    x, omega = sr.refine(ch, fac, to_chain(inp, inp["rhs"]))
    kmax = float(max(max(np.max(np.abs(d)) for d in ch.D), np.max(np.abs(ch.T))))
    inert, small = [], []
    for rev in (False, True):
        c2 = ch if not rev else sr.Chain(trip, inp["N"], inp["safe"], inp["energy"], reverse=True)
        f2 = sr.Factor(c2, False)
        inert.append(sr.inertia_of(f2.pivots))
        small.append(float(np.min(np.abs(np.concatenate(f2.pivots)))) / (max(f2.growth, 1.0) * sr.EPS_LD * kmax))
    return dict(chain=ch, x=x, omega=omega, inertia=inert[0], decided=inert[0] == inert[1] and min(small) >= 4.0,
                margin=min(small), inertias=inert, nnz=ch.nnz_rows(), inp=inp, factor=fac)


def to_chain(inp, v):
    """a vector in the kernel's own-extent layout [nw + ng] -> the chain's numbering (the same: (w, lam_g)) in longdouble"""
    return np.asarray(v, dtype=np.float64).astype(LD)


def beta(ref, x, rhs):
    """item 1's bound per row, in longdouble, for a solution x and right-hand side rhs [n]"""
    ch = ref["chain"]
    return (ref["nnz"] + 2.0) * EPS * (ch.matvec(np.asarray(x, dtype=LD), absolute=True) + np.abs(np.asarray(rhs, dtype=LD)))


def backward_ratio(ref, x, rhs):
    """(max_i |rhs - K x|_i / beta_i, the residual's max-norm, max beta) in longdouble"""
    ch = ref["chain"]
    x, rhs = np.asarray(x, dtype=np.float64).astype(LD), np.asarray(rhs, dtype=np.float64).astype(LD)
    r = np.abs(rhs - ch.matvec(x))
    bt = beta(ref, x, rhs)
    ratio = float(np.max(np.where(bt > 0, r / np.where(bt > 0, bt, 1), np.where(r > 0, np.inf, 0))))
    return ratio, float(np.max(r)), float(np.max(bt))


@functools.lru_cache(maxsize=None)
def floor(key, nvec=2):
    """item 2's floor, relative to max |x_ref|, the largest over the key's right-hand sides"""
    ref = reference(key, nvec)
    inp, ch = ref["inp"], ref["chain"]
    kinv = None
    if inp["N"] <= 65:
        A = np.asarray(sr.dense(sc.triplets_of(inp), ch.n), dtype=np.float64)
        kinv = np.abs(np.linalg.inv(A))
    bt = np.asarray(beta(ref, ref["x"], inp["rhs"]), dtype=np.float64)                   # [nvec, n]
    scale = np.max(np.abs(np.asarray(ref["x"], dtype=np.float64)), axis=1)
    if kinv is not None:
        return float(np.max(2.0 * np.max(bt @ kinv.T, axis=1) / scale))
    signs = np.random.default_rng(31).choice((-1.0, 1.0), (4,) + bt.shape)
    est = np.abs(np.asarray(ref["factor"].solve((signs * bt).reshape(-1, bt.shape[1]).astype(LD)), dtype=np.float64)).reshape(signs.shape)
    return float(np.max(4.0 * np.sqrt(float(np.max(ref["nnz"]))) * np.max(est, axis=(0, 2)) / scale))


def measure(key, refine, nvec=2):
    """the spread of a key at a refine count: float64 static-order LDL^T + `refine` float64 refinements, two stage orders, against the reference"""
    ref = reference(key, nvec)
    inp = ref["inp"]
    trip = sc.triplets_of(inp)
    worst = 0.0
    for rev in (False, True):
        ch = sr.Chain(trip, inp["N"], inp["safe"], inp["energy"], reverse=rev, dtype=np.float64)
        fac = sr.Factor(ch, False)
        x, _ = sr.refine(ch, fac, np.asarray(inp["rhs"], dtype=np.float64), steps=refine)
        scale = np.max(np.abs(ref["x"]), axis=1)
        worst = max(worst, float(np.max(np.max(np.abs(x.astype(LD) - ref["x"]), axis=1) / scale)))
    return worst


@functools.lru_cache(maxsize=None)
def fixture():
    z = np.load(PATH)
    return {k: float(z[k]) for k in z.files}


def guard(key, refine=2, nvec=2):
    return max(floor(key, nvec), 4.0 * fixture()["%s/r%d" % (key, refine)])
