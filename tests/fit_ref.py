"""A plain restatement of what mcq_spline_fit_device computes (include/mcq.h): interp_track's re-sampling, scipy's chord-length parameter and
FITPACK's periodic smoothing fit (clocur / fpclos behind scipy.interpolate.splprep(..., per=1)) with unit weights, iopt = 0, tol = 0.001,
maxit = 20.  Written from Dierckx's description; scipy's splprep is the reference it is held to (tests/test_fit_ref.py on the recordings of
scripts/make_golden_spline_fit.py).  Every function takes the number type (numpy.float64 or numpy.longdouble).

The decisions of a fit -- fp - s against +-acc in every knot round and every p round, the truncation in npl1, fpknot's largest interval against
its runner-up -- are returned with their margins (`margins`), so that a case can be shown to be DECIDED (tests/fit_guard.py)."""
import numpy as np

TOL = 0.001
MAXIT = 20
CON1, CON9, CON4 = 0.1, 0.9, 0.04
IER_MESSAGES = {
    1: "The required storage space exceeds the available storage space. Probable causes: data (x,y) size is too small or smoothing parameter"
       " s is too small (fp>s).",
    2: "A theoretically impossible result when finding a smoothing spline with fp = s. Probable cause: s too small. (abs(fp-s)/s>0.001)",
    3: "The maximal number of iterations (20) allowed for finding smoothing spline with fp=s has been reached. Probable cause: s too small."
       " (abs(fp-s)/s>0.001)",
}


class Refused(ValueError):
    """What the device entry answers with MCQ_BAD_INPUT."""


def resample(track, step, T=np.float64):
    """interp_track's rule on the closed raw line, then sample 0 appended again: the closed points [mi, 2]."""
    xy = np.asarray(track, dtype=T)[:, :2]
    n = xy.shape[0]
    if n < 3 or not np.all(np.isfinite(xy.astype(np.float64))):
        raise Refused("n < 3 or a non-finite row")
    if not step > 0.0:
        return np.vstack([xy, xy[:1]])
    cl = np.vstack([xy, xy[:1]])
    d = cl[1:] - cl[:-1]
    el = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
    if np.any(el == 0):
        raise Refused("a zero-length element")
    cum = np.zeros(n + 1, dtype=T)
    acc = T(0)
    for i in range(n):
        acc = acc + el[i]
        cum[i + 1] = acc
    total = cum[n]
    num = int(np.ceil(total / T(step))) + 1
    st = total / T(num - 1)
    out = np.empty((num, 2), dtype=T)
    for j in range(num - 1):
        x = T(j) * st
        lo = int(np.searchsorted(cum, x, side="right")) - 1
        lo = min(max(lo, 0), n - 1)
        out[j] = (cl[lo + 1] - cl[lo]) / (cum[lo + 1] - cum[lo]) * (x - cum[lo]) + cl[lo]
    out[num - 1] = out[0]
    return out


def parameter(pts, T=np.float64):
    pts = np.asarray(pts, dtype=T)
    mi = pts.shape[0]
    u = np.zeros(mi, dtype=T)
    for i in range(1, mi):
        dx, dy = pts[i, 0] - pts[i - 1, 0], pts[i, 1] - pts[i - 1, 1]
        u[i] = u[i - 1] + np.sqrt(dx * dx + dy * dy)
    if not u[mi - 1] > 0 or np.any(u[1:] <= u[:-1]):
        raise Refused("the parameter is not strictly increasing")
    last = u[mi - 1]
    u = u / last
    u[mi - 1] = T(1)
    return u


def bspl(t, k, x, l, T):
    """FITPACK's fpbspl: the k + 1 B-splines of degree k that are not zero on t[l] <= x < t[l + 1]."""
    h = [T(1)] + [T(0)] * k
    for j in range(1, k + 1):
        hh = h[:j]
        h[0] = T(0)
        for i in range(j):
            li, lj = l + 1 + i, l + 1 + i - j
            if t[li] == t[lj]:
                h[i + 1] = T(0)
            else:
                f = hh[i] / (t[li] - t[lj])
                h[i] = h[i] + f * (t[li] - x)
                h[i + 1] = f * (x - t[lj])
    return h


def wrap_knots(t, n, k, T):
    for j in range(1, k + 1):
        t[k - j] = t[n - k - 1 - j] - T(1)
        t[n - k - 1 + j] = t[k + j] + T(1)


def disc_rows(t, n, k, T):
    """fpdisc: the jumps of the k-th derivative of the B-splines at the interior knots t[k + 1 .. n - k - 2], row q on B-splines q .. q + k + 1."""
    nrint = n - 2 * k - 1
    fac = T(nrint) / (t[n - k - 1] - t[k])
    rows = []
    for l in range(k + 1, n - k - 1):
        lmk = l - k - 1
        h = [T(0)] * (2 * k + 2)
        for j in range(k + 1):
            h[j] = t[l] - t[l + j - k - 1]
            h[j + k + 1] = t[l] - t[l + j + 1]
        row = []
        lp = lmk
        for j in range(k + 2):
            jk = j
            prod = h[j]
            for _ in range(k):
                jk += 1
                prod = prod * h[jk] * fac
            lk = lp + k + 1
            row.append((t[lk] - t[lp]) / prod)
            lp += 1
        rows.append(row)
    return rows


class Band:
    """The triangle of the periodic system of n7 coefficients: columns below nb in a band of k + 2, the last kb = n7 - nb columns full."""

    def __init__(self, n7, k, T):
        self.n7, self.k, self.T = n7, k, T
        self.kb = min(k + 1, n7)
        self.nb = n7 - self.kb
        self.a = [[T(0)] * (k + 2) for _ in range(n7)]
        self.b = [[T(0)] * self.kb for _ in range(n7)]
        self.z = [[T(0), T(0)] for _ in range(n7)]

    def copy(self):
        o = Band(self.n7, self.k, self.T)
        o.a = [r[:] for r in self.a]
        o.b = [r[:] for r in self.b]
        o.z = [r[:] for r in self.z]
        return o

    @staticmethod
    def _givens(piv, ww, T):
        store = abs(piv)
        if store >= ww:
            dd = store * np.sqrt(T(1) + (ww / piv) * (ww / piv))
        else:
            dd = ww * np.sqrt(T(1) + (piv / ww) * (piv / ww))
        return ww / dd, piv / dd, dd

    def rotate_in(self, first, vals, rhs):
        """One row with len(vals) entries on the coefficients first, first + 1, ... (mod n7) and the right-hand sides rhs [2]."""
        T, k, nb, kb, n7 = self.T, self.k, self.nb, self.kb, self.n7
        w = k + 2
        h1 = [T(0)] * w
        h2 = [T(0)] * kb
        ws = first if first < nb else 0
        for j, v in enumerate(vals):
            col = (first + j) % n7
            if col < nb:
                h1[col - ws] = h1[col - ws] + v
            else:
                h2[col - nb] = h2[col - nb] + v
        x0, x1 = rhs
        for i in range(ws, nb):
            if i >= ws + w and not any(h1):       # (exact zeros: nothing is left of the row in the band)
                break
            piv = h1[0]
            if piv != 0:
                ai, bi, zi = self.a[i], self.b[i], self.z[i]
                co, si, ai[0] = self._givens(piv, ai[0], T)
                x0, zi[0] = co * x0 - si * zi[0], co * zi[0] + si * x0
                x1, zi[1] = co * x1 - si * zi[1], co * zi[1] + si * x1
                for j in range(kb):
                    h2[j], bi[j] = co * h2[j] - si * bi[j], co * bi[j] + si * h2[j]
                for j in range(1, w):
                    if i + j >= nb:
                        break
                    h1[j], ai[j] = co * h1[j] - si * ai[j], co * ai[j] + si * h1[j]
            h1 = h1[1:] + [T(0)]
        for j in range(kb):
            piv = h2[j]
            if piv == 0:
                continue
            bi, zi = self.b[nb + j], self.z[nb + j]
            co, si, bi[j] = self._givens(piv, bi[j], T)
            x0, zi[0] = co * x0 - si * zi[0], co * zi[0] + si * x0
            x1, zi[1] = co * x1 - si * zi[1], co * zi[1] + si * x1
            for i in range(j + 1, kb):
                h2[i], bi[i] = co * h2[i] - si * bi[i], co * bi[i] + si * h2[i]

    def solve(self):
        T, k, nb, kb, n7 = self.T, self.k, self.nb, self.kb, self.n7
        c = [[T(0), T(0)] for _ in range(n7)]
        for d in range(2):
            for j in range(kb - 1, -1, -1):
                i = nb + j
                s = self.z[i][d]
                for q in range(j + 1, kb):
                    s = s - self.b[i][q] * c[nb + q][d]
                c[i][d] = s / self.b[i][j]
            for i in range(nb - 1, -1, -1):
                s = self.z[i][d]
                for q in range(kb):
                    s = s - self.b[i][q] * c[nb + q][d]
                for j in range(1, k + 2):
                    if i + j >= nb:
                        break
                    s = s - self.a[i][j] * c[i + j][d]
                c[i][d] = s / self.a[i][0]
        return c

    def trace(self):
        s = self.T(0)
        for i in range(self.nb):
            s = s + self.a[i][0]
        for j in range(self.kb):
            s = s + self.b[self.nb + j][j]
        return s


def same_sum(a, b):
    """Whether two residual sums of fpknot's bookkeeping, given by where they come from (the interval they were summed for, then (j, m) of every
    split fpmax * j / m), are the same number in every binary floating-point implementation: the same interval and the same splits in the same
    order, where a split with j and m both powers of two only counts with its exponent -- it scales by a power of two, which rounds nothing and
    commutes with every rounding (so the half of a half, (2, 4) then (1, 2), IS the quarter (1, 4))."""
    def canon(made):
        e, rest = 0, []
        for j, m in made[1:]:
            if j > 0 and j & (j - 1) == 0 and m & (m - 1) == 0:
                e += j.bit_length() - m.bit_length()
            else:
                rest.append((j, m))
        return made[0], e, rest
    return canon(a) == canon(b)


def fit(pts, k, s, nest, T=np.float64, stages=None):
    """fpclos on the closed points [mi, 2].  Returns dict(t, c [2][n - k - 1], n, fp, ier, u, margins, rounds, prounds); `stages`, a list, receives
    (n, knots, fp) of every least-squares stage."""
    pts = np.asarray(pts, dtype=T)
    mi = pts.shape[0]
    if mi <= k:
        raise Refused("m > k must hold")
    u = parameter(pts, T)
    s = T(s)
    m1 = mi - 1
    k1 = k + 1
    nmin, nmax = 2 * k1, mi + 2 * k
    if nest < nmin:
        raise ValueError("nest < 2 k + 2")
    acc = T(TOL) * s
    margins = dict(acc=[], npl1=[], knot=[])
    t = [T(0)] * max(nest, nmin)
    res = dict(u=u, rounds=0, prounds=0, margins=margins)

    def done(n, c7, fp, ier):
        n7 = n - 2 * k - 1
        cc = np.full((2, n - k - 1), T(0), dtype=T)
        for i in range(n - k - 1):
            cc[0, i], cc[1, i] = c7[i % n7][0], c7[i % n7][1]
        res.update(t=np.array(t[:n], dtype=T), c=cc, n=n, fp=fp, ier=ier)
        return res

    # the constant periodic spline
    mean = [T(0), T(0)]
    for d in range(2):
        a = T(0)
        for i in range(m1):
            a = a + pts[i, d]
        mean[d] = a / T(m1)
    fp0 = T(0)
    for i in range(m1):
        fp0 = fp0 + ((pts[i, 0] - mean[0]) * (pts[i, 0] - mean[0]) + (pts[i, 1] - mean[1]) * (pts[i, 1] - mean[1]))

    def interpolation_knots():
        for i in range(1, m1):
            t[i + k] = u[i] if k % 2 else (u[i] + u[i - 1]) * T(0.5)
        return nmax

    if s == 0:
        n = nmax
        if n > nest:
            n = nmin
            t[k], t[n - k - 1] = u[0], u[mi - 1]
            wrap_knots(t, n, k, T)
            return done(n, [mean], fp0, 1)
        interpolation_knots()
    else:
        n = nmin
        t[k], t[n - k - 1] = u[0], u[mi - 1]
        wrap_knots(t, n, k, T)
        fpms = fp0 - s
        margins["acc"].append((float(fp0), float(s), float(acc)))
        if fpms < acc or nmax == nmin:
            return done(n, [mean], fp0, -2)
        if n >= nest:
            return done(n, [mean], fp0, 1)
        mm = (mi + 1) // 2
        t[k + 1] = u[mm - 1]
        n = nmin + 1
        nrdata = [mm - 2, m1 - mm]
    fpold, nplus = fp0, 1
    fpint = [T(0)] * (nest + 2)
    if s != 0:
        nrdata = nrdata + [0] * nest
    for _ in range(mi + 1):
        n7 = n - 2 * k - 1
        nrint = n - nmin + 1
        t[k], t[n - k - 1] = u[0], u[mi - 1]
        wrap_knots(t, n, k, T)
        R = Band(n7, k, T)
        l = k
        q, lidx = [], []
        for it in range(m1):
            while u[it] >= t[l + 1] and l < n - k - 2:
                l += 1
            h = bspl(t, k, u[it], l, T)
            q.append(h)
            lidx.append(l)
            R.rotate_in(l - k, h, (pts[it, 0], pts[it, 1]))
        c7 = R.solve()
        term = []
        fp = T(0)
        for it in range(m1):
            e = T(0)
            for d in range(2):
                a = T(0)
                for j in range(k1):
                    a = a + c7[(lidx[it] - k + j) % n7][d] * q[it][j]
                e = e + (a - pts[it, d]) * (a - pts[it, d])
            term.append(e)
            fp = fp + e
        res["rounds"] += 1
        if stages is not None:
            stages.append((n, np.array(t[:n], dtype=np.float64), fp))
        fpms = fp - s
        margins["acc"].append((float(fp), float(s), float(acc)))
        if s == 0:
            return done(n, c7, fp, -1)
        if abs(fpms) < acc:
            return done(n, c7, fp, 0)
        if fpms < 0:
            break
        if n == nmax:
            return done(n, c7, fp, -1)
        if n == nest:
            return done(n, c7, fp, 1)
        npl1 = nplus * 2
        if fpold - fp > acc:
            r = T(nplus) * fpms / (fpold - fp)
            npl1 = int(r)
            margins["npl1"].append((float(r), float(min(r - np.floor(r), np.floor(r) + 1 - r))))
        nplus = min(nplus * 2, max(npl1, nplus // 2, 1))
        fpold = fp
        # the residual sums per knot interval: a point on a knot is shared half and half; the first point belongs to the last interval
        fpart, i, new, l = T(0), 0, 0, k
        for it in range(m1):
            if u[it] >= t[l]:
                new = 1
                l += 1
            fpart = fpart + term[it]
            if new:
                if l <= k + 1:
                    fpint[nrint - 1] = term[it]
                else:
                    store = term[it] * T(0.5)
                    fpint[i] = fpart - store
                    i += 1
                    fpart = store
                new = 0
        fpint[nrint - 1] = fpint[nrint - 1] + fpart
        full = False
        # where an interval's residual sum comes from, moved along with fpint: the interval of this round it was summed for, then (j, m) of
        # every split fpmax * j / m behind it.  Equal entries are the SAME float operations on the same number in every implementation
        made = [(j,) for j in range(nest + 2)]
        for _add in range(nplus):
            # fpknot
            fpmax, number, second, runner = T(0), -1, T(0), -1
            jbegin = 0
            for j in range(nrint):
                jp = nrdata[j]
                if jp != 0:
                    if fpint[j] > fpmax:
                        second, runner = fpmax, number
                        fpmax, number, maxpt, maxbeg = fpint[j], j, jp, jbegin
                    elif fpint[j] > second:
                        second, runner = fpint[j], j
                jbegin += jp + 1
            if number < 0:
                raise Refused("no interval left to split")
            # (third entry: 1 if the largest and its runner-up are halves of one interval split earlier in this round, or pieces that the same
            #  splits made of such halves: the same arithmetic on the same number)
            margins["knot"].append((float(fpmax), float(second), float(runner >= 0 and len(made[number]) > 1 and same_sum(made[number], made[runner]))))
            ihalf = maxpt // 2 + 1
            nrx = maxbeg + ihalf
            nxt = number + 1
            for j in range(nrint - 1, nxt - 1, -1):
                fpint[j + 1] = fpint[j]
                nrdata[j + 1] = nrdata[j]
                made[j + 1] = made[j]
            for j in range(n - 1, nxt + k - 1, -1):
                t[j + 1] = t[j]
            nrdata[number] = ihalf - 1
            nrdata[nxt] = maxpt - ihalf
            am = T(maxpt)
            fpint[number] = fpmax * T(nrdata[number]) / am
            fpint[nxt] = fpmax * T(nrdata[nxt]) / am
            made[number], made[nxt] = made[number] + ((nrdata[number], maxpt),), made[number] + ((nrdata[nxt], maxpt),)
            t[nxt + k] = u[nrx]
            n += 1
            nrint += 1
            if n == nmax:
                interpolation_knots()
                full = True
                break
            if n == nest:
                break
    # the smoothing spline: f(p) = s by rational interpolation
    D = disc_rows(t, n, k, T)
    p1, f1, p3, f3 = T(0), fp0 - s, T(-1), fpms
    p = T(n7) / R.trace()
    ich1 = ich3 = 0
    ier = 3
    for it in range(1, MAXIT + 1):
        pinv = T(1) / p
        G = R.copy()
        for r, row in enumerate(D):
            G.rotate_in(r, [v * pinv for v in row], (T(0), T(0)))
        c7 = G.solve()
        fp = T(0)
        for i in range(m1):
            for d in range(2):
                a = T(0)
                for j in range(k1):
                    a = a + c7[(lidx[i] - k + j) % n7][d] * q[i][j]
                fp = fp + (a - pts[i, d]) * (a - pts[i, d])
        res["prounds"] += 1
        fpms = fp - s
        margins["acc"].append((float(fp), float(s), float(acc)))
        if abs(fpms) < acc:
            ier = 0
            break
        if it == MAXIT:
            break
        p2, f2 = p, fpms
        if ich3 == 0:
            if f2 - f3 <= acc:
                p3, f3 = p2, f2
                p = p * T(CON4)
                if p <= p1:
                    p = p1 * T(CON9) + p2 * T(CON1)
                continue
            if f2 < 0:
                ich3 = 1
        if ich1 == 0:
            if f1 - f2 <= acc:
                p1, f1 = p2, f2
                p = p / T(CON4)
                if p3 >= 0 and p >= p3:
                    p = p2 * T(CON1) + p3 * T(CON9)
                continue
            if f2 > 0:
                ich1 = 1
        if f2 >= f1 or f2 <= f3:
            ier = 2
            break
        if p3 > 0:
            h1, h2, h3 = f1 * (f2 - f3), f2 * (f3 - f1), f3 * (f1 - f2)
            p = -(p1 * p2 * h3 + p2 * p3 * h1 + p3 * p1 * h2) / (p1 * h1 + p2 * h2 + p3 * h3)
        else:
            p = (p1 * (f1 - f3) * f2 - p2 * (f2 - f3) * f1) / ((f1 - f2) * f3)
        if f2 < 0:
            p3, f3 = p2, f2
        else:
            p1, f1 = p2, f2
    return done(n, c7, fp, ier)


def fit_track(track, k, s, step, nest=None, T=np.float64, stages=None):
    pts = resample(track, step, T)
    if nest is None:
        nest = pts.shape[0] + 2 * k
    out = fit(pts, k, s, nest, T, stages)
    out["pts"] = pts
    return out


def two_lobe(m=41):
    th = 2.0 * np.pi * np.arange(m) / m
    return np.stack([30.0 * np.cos(th) + 3.0 * np.cos(5.0 * th), 20.0 * np.sin(th) + 2.0 * np.sin(3.0 * th)], axis=1)
