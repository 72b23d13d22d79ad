"""The reference of mcq_mintime_step_device (include/mcq.h): the regularised primal-dual matrix

    K = [[H + diag(dw), J^T], [J, -diag(dg)]]

assembled in longdouble from the SAME float64 arrays the entry is given, by the statements of mintime.hessian_coo and mintime.jacobian_coo
(triplets(): the overlaps of neighbouring Hessian blocks and dw are added in longdouble, nothing is rounded), and eliminations that are not the
kernel's code:

  Factor(chain, True) + refine   a bordered block-tridiagonal LU with ROW PIVOTING inside each diagonal block, longdouble, refined in longdouble
                  until its own componentwise residual is at longdouble rounding (it certifies itself, as sp_ref.py does); held to
                  dense_pivoted at N <= 8
  dense_pivoted   Gaussian elimination with partial pivoting on the dense matrix, longdouble
  Factor(chain, False)   the same frontal code with pivoting off -- a static-order LDL^T: its pivot signs in two stage orders (forward,
                  reversed) are the inertia (numpy.linalg.eigvalsh beside them at N <= 8); in float64 with float64 refinements it is the
                  restatement whose two orders measure the spread (tests/mtstep_guard.py)

The partition: group k = [U_k-1, X_k (k > 0), Xc_k, the path rows of interval k - 1 (k > 0), the collocation and continuity rows of interval k];
border = [X_N, path rows of interval N - 1, X_0, U_N-1, periodicity rows, energy row].  Block k of H and J couples groups k and k + 1 and the
border only, so the groups form a block-tridiagonal chain in either direction."""
import numpy as np

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
EPS_LD = float(np.finfo(LD).eps)


def sizes(N, safe, energy):
    nw = 5 + 24 * N
    per = N * (27 + 2 * safe) + 4 * (N - 1)
    return nw, per + 5 + energy, per


def row_of(N, k, r, safe):
    start = k * (27 + 2 * safe) + 4 * max(k - 1, 0)
    if r < 27:
        return start + r
    if r < 31:
        return start + r if k > 0 else -1
    return (start + 27 + (4 if k > 0 else 0) + (r - 31)) if safe else -1


def triplets(hblocks, blocks, N, dw, dg, safe=False, grad_energy=None):
    """(rows, cols, values) of K in the (w, lam_g) numbering, float64 values, duplicates NOT added: every statement of hessian_coo (all 33 x 33
    entries of a block at hessian_slots), of jacobian_coo (present row slots, 29 or 33 columns, the periodicity rows, the energy row) and the two
    diagonals; J's entries twice (J and J^T)."""
    safe = int(bool(safe))
    nw, ng, per = sizes(N, safe, grad_energy is not None)
    R, C, V = [], [], []
    for k in range(N):
        idx = np.concatenate((24 * k + np.arange(29), 24 * ((k - 1) % N) + 5 + np.arange(4)))
        r, c = np.nonzero(np.asarray(hblocks[k]))
        R.append(idx[r]); C.append(idx[c]); V.append(np.asarray(hblocks[k])[r, c])
        slots = [s for s in range(33) if row_of(N, k, s, safe) >= 0]
        rows = np.array([row_of(N, k, s, safe) for s in slots])
        colmap = np.concatenate((24 * k + np.arange(29), 24 * (k - 1) + 5 + np.arange(4)))
        ncol = 33 if k > 0 else 29
        sub = np.asarray(blocks[k])[slots][:, :ncol]
        r, c = np.nonzero(sub)
        R += [nw + rows[r], colmap[c]]; C += [colmap[c], nw + rows[r]]; V += [sub[r, c], sub[r, c]]
    p5 = np.arange(5)
    for cols, val in ((p5, 1.0), (24 * N + p5, -1.0)):
        R += [nw + per + p5, cols]; C += [cols, nw + per + p5]; V += [np.full(5, val), np.full(5, val)]
    if grad_energy is not None:
        ge = np.asarray(grad_energy)[:nw]
        c = np.flatnonzero(ge)
        R += [np.full(c.shape, nw + per + 5), c]; C += [c, np.full(c.shape, nw + per + 5)]; V += [ge[c], ge[c]]
    R += [np.arange(nw), nw + np.arange(ng)]; C += [np.arange(nw), nw + np.arange(ng)]
    V += [np.asarray(dw, dtype=np.float64)[:nw], -np.asarray(dg, dtype=np.float64)[:ng]]
    return np.concatenate(R).astype(np.int64), np.concatenate(C).astype(np.int64), np.concatenate(V).astype(np.float64)


def dense(trip, n, dtype=LD):
    A = np.zeros((n, n), dtype)
    np.add.at(A, (trip[0], trip[1]), trip[2].astype(dtype))
    return A


def partition(N, safe, energy):
    """(groups, border): lists of index arrays in the (w, lam_g) numbering"""
    nw, ng, per = sizes(N, safe, energy)

    def path_rows(k):
        return [nw + row_of(N, k, r, safe) for r in range(20, 33) if row_of(N, k, r, safe) >= 0]
    groups = []
    for k in range(N):
        g = []
        if k > 0:
            g += list(24 * (k - 1) + 5 + np.arange(4)) + list(24 * k + np.arange(5))
        g += list(24 * k + 9 + np.arange(15))
        if k > 0:
            g += path_rows(k - 1)
        g += [nw + row_of(N, k, r, safe) for r in range(20)]
        groups.append(np.array(g, dtype=np.int64))
    border = list(24 * N + np.arange(5)) + path_rows(N - 1) + list(range(5)) + list(24 * (N - 1) + 5 + np.arange(4)) + \
        list(nw + per + np.arange(5 + energy))
    return groups, np.array(border, dtype=np.int64)


class Chain:
    """K as a bordered block-tridiagonal matrix in a given sequence of the groups: D[p], C[p] (group p against group p - 1), G[p] (group p
    against the border), T (border), all dense in `dtype`, summed from the triplets in that dtype."""

    def __init__(self, trip, N, safe, energy, reverse=False, dtype=LD):
        groups, border = partition(N, safe, energy)
        if reverse:
            groups = groups[::-1]
        self.groups, self.border, self.dtype = groups, border, dtype
        n = sum(g.shape[0] for g in groups) + border.shape[0]
        self.n = n
        pos, loc = np.full(n, -1, dtype=np.int64), np.zeros(n, dtype=np.int64)
        for p, g in enumerate(groups):
            pos[g], loc[g] = p, np.arange(g.shape[0])
        loc[border] = np.arange(border.shape[0])
        P = len(groups)
        m = [g.shape[0] for g in groups]
        nb, mm = border.shape[0], max(m)
        r, c, v = trip
        v = v.astype(dtype)
        pr, pc, lr, lc = pos[r], pos[c], loc[r], loc[c]
        assert not np.any((pr >= 0) & (pc >= 0) & (np.abs(pr - pc) > 1)), "an entry couples two groups that are not neighbours"
        # every block of a kind in one padded array, summed in one pass over the triplets
        Dall, Call, Gall = np.zeros((P, mm, mm), dtype), np.zeros((P, mm, mm), dtype), np.zeros((P, mm, nb), dtype)
        self.T = np.zeros((nb, nb), dtype)
        sel = (pr < 0) & (pc < 0)
        np.add.at(self.T, (lr[sel], lc[sel]), v[sel])
        sel = (pr >= 0) & (pc == pr)
        np.add.at(Dall, (pr[sel], lr[sel], lc[sel]), v[sel])
        sel = (pr >= 0) & (pc == pr - 1) & (pc >= 0)
        np.add.at(Call, (pr[sel], lr[sel], lc[sel]), v[sel])
        sel = (pr >= 0) & (pc < 0)
        np.add.at(Gall, (pr[sel], lr[sel], lc[sel]), v[sel])
        self.D = [Dall[p, :m[p], :m[p]].copy() for p in range(P)]
        self.C = [None] + [Call[p, :m[p], :m[p - 1]].copy() for p in range(1, P)]
        self.G = [Gall[p, :m[p]].copy() for p in range(P)]

    def split(self, x):
        return [x[..., g] for g in self.groups], x[..., self.border]

    def join(self, xs, xb):
        out = np.zeros(xb.shape[:-1] + (self.n,), self.dtype)
        for g, v in zip(self.groups, xs):
            out[..., g] = v
        out[..., self.border] = xb
        return out

    def matvec(self, x, absolute=False):
        """K x (or |K| |x|) for x [.., n] in the chain's dtype, block by block"""
        f = np.abs if absolute else (lambda a: a)
        xs, xb = self.split(f(np.asarray(x, dtype=self.dtype)))
        P = len(self.groups)
        ys, yb = [], xb @ f(self.T).T
        for p in range(P):
            y = xs[p] @ f(self.D[p]).T + xb @ f(self.G[p]).T
            if p > 0:
                y = y + xs[p - 1] @ f(self.C[p]).T
            if p + 1 < P:
                y = y + xs[p + 1] @ f(self.C[p + 1])
            yb = yb + xs[p] @ f(self.G[p])
            ys.append(y)
        return self.join(ys, yb)

    def nnz_rows(self):
        """non-zeros per row of the assembled K"""
        P = len(self.groups)
        ys, yb = [], (self.T != 0).sum(axis=1).astype(np.float64)
        for p in range(P):
            y = (self.D[p] != 0).sum(axis=1) + (self.G[p] != 0).sum(axis=1)
            if p > 0:
                y = y + (self.C[p] != 0).sum(axis=1)
            if p + 1 < P:
                y = y + (self.C[p + 1] != 0).sum(axis=0)
            yb = yb + (self.G[p] != 0).sum(axis=0)
            ys.append(y.astype(np.float64))
        return np.asarray(self.join([y.astype(self.dtype) for y in ys], yb.astype(self.dtype)), dtype=np.float64)


class Factor:
    """The frontal elimination of a Chain: front p = [group p | the unknowns of group p + 1 it is coupled to | the border columns that are
    non-zero so far]; its first m_p columns are eliminated, with row pivoting among the group's own rows (pivot=True) or in the static order
    (pivot=False: LDL^T, U = D L^T to rounding); what the elimination subtracts from the rest is added to the next group's blocks and the
    border.  pivots: the diagonal of U per front, in elimination order."""

    def __init__(self, ch, pivot):
        self.ch, self.pivot = ch, pivot
        P, dt = len(ch.groups), ch.dtype
        self.fronts, self.pivots, self.growth = [], [], 0.0
        Dn, Gn, T = ch.D[0].copy(), ch.G[0].copy(), ch.T.copy()
        none = np.zeros(0, dtype=np.int64)
        for p in range(P + 1):
            if p < P:
                m = Dn.shape[0]
                idx = np.flatnonzero(np.any(ch.C[p + 1] != 0, axis=1)) if p + 1 < P else none
                act = np.flatnonzero(np.any(Gn != 0, axis=0))
                a, b = m + idx.shape[0], m + idx.shape[0] + act.shape[0]
                F = np.zeros((b, b), dt)
                F[:m, :m] = Dn
                F[:m, a:], F[a:, :m] = Gn[:, act], Gn[:, act].T
                if idx.shape[0]:
                    F[m:a, :m], F[:m, m:a] = ch.C[p + 1][idx], ch.C[p + 1][idx].T
            else:
                m, idx, act = T.shape[0], none, none
                F = T.copy()
            perm = np.arange(m)
            big = float(np.max(np.abs(F))) if F.size else 0.0
            for j in range(m):
                if pivot:
                    q = j + int(np.argmax(np.abs(F[j:m, j])))
                    if q != j:
                        F[[j, q]] = F[[q, j]]
                    perm[j] = q
                F[j + 1:, j] = F[j + 1:, j] / F[j, j]
                F[j + 1:, j + 1:] -= F[j + 1:, j, None] * F[j, None, j + 1:]
            self.growth = max(self.growth, float(np.max(np.abs(F[:, :m]))) / big if big else 0.0)
            self.pivots.append(np.diagonal(F)[:m].copy())
            self.fronts.append((F[:, :m].copy(), F[:m, m:].copy(), perm, m, idx, act))
            if p < P:
                if p + 1 < P:
                    Dn, Gn = ch.D[p + 1].copy(), ch.G[p + 1].copy()
                    Dn[np.ix_(idx, idx)] += F[m:a, m:a]
                    Gn[np.ix_(idx, act)] += F[m:a, a:]
                T[np.ix_(act, act)] += F[a:, a:]

    def solve(self, b):
        """K x = b for b [n] or [r, n] (r right-hand sides at once) in the chain's dtype"""
        ch = self.ch
        b = np.asarray(b, dtype=ch.dtype)
        bs, bb = ch.split(np.atleast_2d(b).copy())
        bs = [v.T.copy() for v in bs]             # [unknowns of the group, r]
        bb = bb.T.copy()
        P = len(ch.groups)
        ys = []
        for p in range(P + 1):
            L, U12, perm, m, idx, act = self.fronts[p]
            v = np.concatenate((bs[p], bs[p + 1][idx] if idx.shape[0] else bb[:0], bb[act])) if p < P else bb
            for j in range(m):             # (the row exchanges first: L is stored as the finished elimination left it)
                if perm[j] != j:
                    v[[j, perm[j]]] = v[[perm[j], j]]
            for j in range(m):
                v[j + 1:] -= np.multiply.outer(L[j + 1:, j], v[j])
            ys.append(v[:m].copy())
            if p < P:
                if idx.shape[0]:
                    bs[p + 1][idx] = v[m:m + idx.shape[0]]
                bb[act] = v[m + idx.shape[0]:]
        xs = [None] * P
        xb = None
        for p in range(P, -1, -1):
            L, U12, perm, m, idx, act = self.fronts[p]
            x = ys[p].copy()
            if p < P:
                x = x - U12 @ np.concatenate((xs[p + 1][idx] if idx.shape[0] else xb[:0], xb[act]))
            for j in range(m - 1, -1, -1):
                x[j] = (x[j] - L[j, j + 1:m] @ x[j + 1:]) / L[j, j]          # (row j of U: the diagonal and what lies right of it in L's storage)
            if p == P:
                xb = x
            else:
                xs[p] = x
        out = ch.join([v.T for v in xs], xb.T)
        return out[0] if b.ndim == 1 else out


def refine(ch, fac, b, steps=None, tol=4.0):
    """x with K x = b (b [n] or [r, n]): fac's solve, then refinement with the chain's own residuals -- `steps` of them, or (None) until the
    componentwise backward error of every right-hand side is below tol x the dtype's eps (at most 12).  Returns (x, backward error)."""
    eps = EPS_LD if ch.dtype == LD else EPS
    b = np.asarray(b, dtype=ch.dtype)
    x = fac.solve(b)
    omega = np.inf
    for it in range(12 if steps is None else steps + 1):
        r = b - ch.matvec(x)
        den = ch.matvec(x, absolute=True) + np.abs(b)
        omega = float(np.max(np.where(den > 0, np.abs(r) / np.where(den > 0, den, 1), 0)))
        if (steps is None and omega <= tol * eps) or (steps is not None and it == steps):
            break
        x = x + fac.solve(r)
    return x, omega


def dense_pivoted(A, b):
    """Gaussian elimination with partial pivoting on a dense matrix, in A's dtype; b [n] or [n, m]"""
    A, b = A.copy(), np.array(b, dtype=A.dtype, copy=True)
    n = A.shape[0]
    for j in range(n):
        q = j + int(np.argmax(np.abs(A[j:, j])))
        if q != j:
            A[[j, q]], b[[j, q]] = A[[q, j]], b[[q, j]]
        l = A[j + 1:, j] / A[j, j]
        A[j + 1:, j:] -= np.outer(l, A[j, j:])
        b[j + 1:] -= np.multiply.outer(l, b[j]) if b.ndim > 1 else l * b[j]
    x = np.zeros_like(b)
    for j in range(n - 1, -1, -1):
        x[j] = (b[j] - A[j, j + 1:] @ x[j + 1:]) / A[j, j]
    return x


def inertia_of(pivots):
    d = np.concatenate(pivots)
    return int(np.sum(d > 0)), int(np.sum(d < 0)), int(np.sum(d == 0))
