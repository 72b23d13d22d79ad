// ---- FITPACK's periodic smoothing fit on the device (mcq_spline_fit_device, include/mcq.h): what scipy.interpolate.splprep(..., k, s, per=1)
//      computes inside tph.spline_approximation [REF helper_funcs_glob/src/prep_track.py:39-45], with interp_track's re-sampling in front of it.
//      Included from mcq_kernels.hip INSIDE its contraction-off section: products and sums are rounded separately, as FITPACK's and numpy's are.
//
//      mcq_spline_fit_kernel: a workgroup per track.  The re-sampling, the B-splines of the data points, the residuals, the jump rows and every
//      copy are spread over the workgroup; the observations of one knot interval are first reduced, sixteen at a time, to triangles of k + 1 rows by a thread each
//      (fit_reduce_segment); the chain of dependent Givens rotations that takes those rows into the periodic triangle (FITPACK's fpgivs / fprota),
//      the back-substitution, the knot bookkeeping (fpknot) and the rational root search for p (fprati) are thread 0's, the other threads wait
//      at the barrier.  The triangle of the periodic system of n7 = n - 2 k - 1 distinct coefficients is held as
//          A [n7][K + 2]   the band: columns i .. i + K + 1 of row i, as far as they lie below nb = n7 - kb
//          B [n7][K + 1]   the border: the last kb = min(K + 1, n7) columns in full (the B-splines that wrap around the seam live here)
//          Z [n7][2]       the rotated right-hand sides, x and y
//      = (2 K + 5) n7 doubles, in LDS while that is at most MCQ_FIT_LDS doubles and in the handle's scratch (L2 / HBM) beyond: the same
//      statements on another pointer type, so both routes return the same bits.  One layout serves the least-squares rows (K + 1 wide) and the
//      smoothing rows (K + 2 wide: FITPACK keeps K border columns for the first and K + 1 for the second; the triangle with a positive
//      diagonal is unique, so only roundings differ).  A row that wraps meets a triangle that is already full and fills in all the way to
//      column nb (FITPACK's loop over all rows with its zero-pivot skip); a row that does not wrap is done after K + 2 rotations. ----

__device__ __forceinline__ void fit_givens(double piv, double& ww, double& co, double& si)
{
    const double store = fabs(piv);
    double dd;
    if (store >= ww) {
        const double r = ww / piv;
        dd = store * sqrt(1.0 + r * r);
    } else {
        const double r = piv / ww;
        dd = ww * sqrt(1.0 + r * r);
    }
    co = ww / dd;
    si = piv / dd;
    ww = dd;
}

#define FIT_ROT(h, a)                           \
    do {                                        \
        const double s1_ = (h), s2_ = (a);      \
        (a) = co * s2_ + si * s1_;              \
        (h) = co * s1_ - si * s2_;              \
    } while (0)

// one row with NV entries on the coefficients first, first + 1, ... (mod n7) and the right-hand sides (x0, x1) into the triangle W
template <int K, int NV, typename PT>
__device__ __forceinline__ void fit_rotate(PT W, int n7, int first, const double* vals, double x0, double x1)
{
    const int kb = n7 < K + 1 ? n7 : K + 1, nb = n7 - kb;
    PT A = W;
    PT B = W + (size_t)n7 * (K + 2);
    PT Z = B + (size_t)n7 * (K + 1);
    double h1[K + 2], h2[K + 1];
    #pragma unroll
    for (int e = 0; e < K + 2; ++e) h1[e] = 0.0;
    #pragma unroll
    for (int e = 0; e < K + 1; ++e) h2[e] = 0.0;
    const int ws = first < nb ? first : 0;
    #pragma unroll
    for (int j = 0; j < NV; ++j) {
        int col = first + j;
        while (col >= n7) col -= n7;
        if (col < nb) {
            #pragma unroll
            for (int e = 0; e < K + 2; ++e)
                if (e == col - ws) h1[e] = h1[e] + vals[j];
        } else {
            #pragma unroll
            for (int e = 0; e < K + 1; ++e)
                if (e == col - nb) h2[e] = h2[e] + vals[j];
        }
    }
    for (int i = ws; i < nb; ++i) {
        if (i >= ws + K + 2) {                  // exact zeros: nothing of the row is left in the band
            bool any = false;
            #pragma unroll
            for (int e = 0; e < K + 2; ++e) any = any || h1[e] != 0.0;
            if (!any) break;
        }
        const double piv = h1[0];
        if (piv != 0.0) {
            PT ai = A + (size_t)i * (K + 2);
            PT bi = B + (size_t)i * (K + 1);
            PT zi = Z + (size_t)i * 2;
            double ww = ai[0], co, si;
            fit_givens(piv, ww, co, si);
            ai[0] = ww;
            FIT_ROT(x0, zi[0]);
            FIT_ROT(x1, zi[1]);
            #pragma unroll
            for (int j = 0; j < K + 1; ++j)
                if (j < kb) FIT_ROT(h2[j], bi[j]);
            #pragma unroll
            for (int j = 1; j < K + 2; ++j)
                if (i + j < nb) FIT_ROT(h1[j], ai[j]);
        }
        #pragma unroll
        for (int e = 0; e < K + 1; ++e) h1[e] = h1[e + 1];
        h1[K + 1] = 0.0;
    }
    #pragma unroll
    for (int j = 0; j < K + 1; ++j) {
        if (j >= kb) continue;
        const double piv = h2[j];
        if (piv == 0.0) continue;
        PT bi = B + (size_t)(nb + j) * (K + 1);
        PT zi = Z + (size_t)(nb + j) * 2;
        double ww = bi[j], co, si;
        fit_givens(piv, ww, co, si);
        bi[j] = ww;
        FIT_ROT(x0, zi[0]);
        FIT_ROT(x1, zi[1]);
        #pragma unroll
        for (int i = j + 1; i < K + 1; ++i)
            if (i < kb) FIT_ROT(h2[i], bi[i]);
    }
}

// the periodic back-substitution: c7 [n7][2]
template <int K, typename PT>
__device__ __forceinline__ void fit_solve(PT W, int n7, gdouble* c7)
{
    const int kb = n7 < K + 1 ? n7 : K + 1, nb = n7 - kb;
    PT A = W;
    PT B = W + (size_t)n7 * (K + 2);
    PT Z = B + (size_t)n7 * (K + 1);
    for (int d = 0; d < 2; ++d) {
        for (int j = kb - 1; j >= 0; --j) {
            const int i = nb + j;
            double s = Z[(size_t)i * 2 + d];
            for (int q = j + 1; q < kb; ++q) s = s - B[(size_t)i * (K + 1) + q] * c7[(size_t)(nb + q) * 2 + d];
            c7[(size_t)i * 2 + d] = s / B[(size_t)i * (K + 1) + j];
        }
        for (int i = nb - 1; i >= 0; --i) {
            double s = Z[(size_t)i * 2 + d];
            for (int q = 0; q < kb; ++q) s = s - B[(size_t)i * (K + 1) + q] * c7[(size_t)(nb + q) * 2 + d];
            #pragma unroll
            for (int j = 1; j < K + 2; ++j)
                if (i + j < nb) s = s - A[(size_t)i * (K + 2) + j] * c7[(size_t)(i + j) * 2 + d];
            c7[(size_t)i * 2 + d] = s / A[(size_t)i * (K + 2)];
        }
    }
}

template <int K, typename PT>
__device__ __forceinline__ double fit_trace(PT W, int n7)
{
    const int kb = n7 < K + 1 ? n7 : K + 1, nb = n7 - kb;
    PT B = W + (size_t)n7 * (K + 2);
    double s = 0.0;
    for (int i = 0; i < nb; ++i) s = s + W[(size_t)i * (K + 2)];
    for (int j = 0; j < kb; ++j) s = s + B[(size_t)(nb + j) * (K + 1) + j];
    return s;
}

// what one track's fit works on (pointers into the handle's scratch and the outputs)
struct FitTrack {
    int mi, m1, nest;
    double s;
    const gdouble* pts;     // [mi][2] closed points
    const gdouble* u;       // [mi]
    gdouble* t;             // [nest] knots (the output row)
    gdouble* q;             // [m1][K + 1] B-splines of the data points
    gint* lidx;             // [m1] their knot intervals
    gdouble* term;          // [m1] squared residuals
    gdouble* R;             // [(2 K + 5) nest] the least-squares triangle, kept for the p rounds
    gdouble* G;             // [(2 K + 5) nest] the working triangle beyond the LDS budget
    gdouble* c7;            // [nest][2]
    gdouble* D;             // [nest][K + 2] fpdisc's rows
    gdouble* fpint;         // [nest + 2]
    gint* nrdata;           // [nest + 2]
    gdouble* qr;            // [m1][K + 1] the segments' reduced rows
    gdouble* zr;            // [m1][2] their right-hand sides
    gint* vf;               // [m1] 1 where qr / zr hold a row
};

// LDS through which thread 0's serial passes read what the workgroup loads or computes a chunk at a time: a dependent chain of rotations or
// additions that fetched its operands from the scratch itself would wait a memory round trip per row
#define MCQ_FIT_CHUNK 128       /* rows of the triangularisation per chunk */
struct FitStage {
    double* q;      // [MCQ_FIT_CHUNK][K + 1] B-splines of the chunk's rows
    double* p;      // [MCQ_FIT_CHUNK][2] their points
    int* l;         // [MCQ_FIT_CHUNK] their knot intervals
    double* e;      // [MCQ_NT] squared residuals of a chunk
    double* u;      // [MCQ_NT] parameters of a chunk
};

// FITPACK's fpbspl for data point `it` on its interval (bisection: the last l in [K, n - K - 2] with t[l] <= x)
template <int K>
__device__ __forceinline__ void fit_bspl(const FitTrack& F, int n, int it)
{
    const gdouble* t = F.t;
    const double x = F.u[it];
    int lo = K, hi = n - K - 2;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (t[mid] <= x) lo = mid;
        else hi = mid - 1;
    }
    const int l = lo;
    double h[K + 1], hh[K];
    h[0] = 1.0;
    #pragma unroll
    for (int j = 1; j <= K; ++j) {
        #pragma unroll
        for (int i = 0; i < j; ++i) hh[i] = h[i];
        h[0] = 0.0;
        #pragma unroll
        for (int i = 0; i < j; ++i) {
            const double tli = t[l + 1 + i], tlj = t[l + 1 + i - j];
            if (tli == tlj) {
                h[i + 1] = 0.0;
            } else {
                const double f = hh[i] / (tli - tlj);
                h[i] = h[i] + f * (tli - x);
                h[i + 1] = f * (x - tlj);
            }
        }
    }
    #pragma unroll
    for (int j = 0; j <= K; ++j) F.q[(size_t)it * (K + 1) + j] = h[j];
    F.lidx[it] = l;
}

// The rows of up to MCQ_FIT_SEG consecutive data points of ONE knot interval share their K + 1 columns: the thread of the segment's first point
// rotates them into a (K + 1) x (K + 1) triangle of its own (registers) and leaves that triangle's rows -- at most as many as the segment has
// points -- in the places of the segment's first rows (qr, zr; vf marks the places that hold a row).  Thread 0 then rotates these few rows into the
// periodic triangle instead of every observation: the same triangle up to roundings (orthogonal transformations of the same rows), a quarter
// of the dependent chain.  What the rotations leave of the right-hand sides is the residual's share and is dropped (fp is summed from the residuals).
#define MCQ_FIT_SEG 16
template <int K>
__device__ __forceinline__ void fit_reduce_segment(const FitTrack& F, int it)
{
    const int l = F.lidx[it];
    if (it != 0 && (it % MCQ_FIT_SEG) != 0 && F.lidx[it - 1] == l) return;        // not a segment's first point
    int end = it + 1;
    while (end < F.m1 && (end % MCQ_FIT_SEG) != 0 && F.lidx[end] == l) ++end;
    double T[K + 1][K + 1], zx[K + 1], zy[K + 1];
    #pragma unroll
    for (int j = 0; j <= K; ++j) {
        zx[j] = 0.0;
        zy[j] = 0.0;
        #pragma unroll
        for (int e = 0; e <= K; ++e) T[j][e] = 0.0;
    }
    for (int r = it; r < end; ++r) {
        double h[K + 1];
        #pragma unroll
        for (int j = 0; j <= K; ++j) h[j] = F.q[(size_t)r * (K + 1) + j];
        double x0 = F.pts[(size_t)r * 2], x1 = F.pts[(size_t)r * 2 + 1];
        #pragma unroll
        for (int j = 0; j <= K; ++j) {
            const double piv = h[j];
            if (piv != 0.0) {
                double ww = T[j][j], co, si;
                fit_givens(piv, ww, co, si);
                T[j][j] = ww;
                FIT_ROT(x0, zx[j]);
                FIT_ROT(x1, zy[j]);
                #pragma unroll
                for (int e = j + 1; e <= K; ++e) FIT_ROT(h[e], T[j][e]);
            }
        }
    }
    #pragma unroll
    for (int j = 0; j <= K; ++j) {
        if (it + j < end) {
            #pragma unroll
            for (int e = 0; e <= K; ++e) F.qr[(size_t)(it + j) * (K + 1) + e] = T[j][e];
            F.zr[(size_t)(it + j) * 2] = zx[j];
            F.zr[(size_t)(it + j) * 2 + 1] = zy[j];
        }
    }
    for (int r = it; r < end; ++r) F.vf[r] = r - it <= K ? 1 : 0;
}

template <int K>
__device__ __forceinline__ void fit_residual(const FitTrack& F, int n7, int it)
{
    const int f0 = F.lidx[it] - K;
    double e = 0.0;
    #pragma unroll
    for (int d = 0; d < 2; ++d) {
        double a = 0.0;
        #pragma unroll
        for (int j = 0; j <= K; ++j) {
            int col = f0 + j;
            while (col >= n7) col -= n7;
            a = a + F.c7[(size_t)col * 2 + d] * F.q[(size_t)it * (K + 1) + j];
        }
        const double r = a - F.pts[(size_t)it * 2 + d];
        e = e + r * r;
    }
    F.term[it] = e;
}

// fpdisc's row for the interior knot t[l], l = K + 1 + r: the jump of the K-th derivative of the B-splines r .. r + K + 1
template <int K>
__device__ __forceinline__ void fit_disc_row(const FitTrack& F, int n, int r)
{
    const gdouble* t = F.t;
    const int l = r + K + 1;
    const double fac = (double)(n - 2 * K - 1) / (t[n - K - 1] - t[K]);
    double h[2 * K + 2];
    #pragma unroll
    for (int j = 0; j <= K; ++j) {
        h[j] = t[l] - t[l + j - K - 1];
        h[j + K + 1] = t[l] - t[l + j + 1];
    }
    #pragma unroll
    for (int j = 0; j < K + 2; ++j) {
        double prod = h[j];
        #pragma unroll
        for (int e = 1; e <= K; ++e) prod = prod * h[j + e] * fac;
        F.D[(size_t)r * (K + 2) + j] = (t[r + j + K + 1] - t[r + j]) / prod;
    }
}

__device__ __forceinline__ void fit_wrap_knots(gdouble* t, int n, int k, double u0, double u1)
{
    t[k] = u0;
    t[n - k - 1] = u1;
    for (int j = 1; j <= k; ++j) {
        t[k - j] = t[n - k - 1 - j] - 1.0;
        t[n - k - 1 + j] = t[k + j] + 1.0;
    }
}

#define FIT_CONTINUE 0
#define FIT_DONE 1
#define FIT_SMOOTH 2

// fpclos with unit weights, iopt = 0, tol = 0.001, maxit = 20 on the closed points of one track; every thread of the workgroup runs it.
// lds: MCQ_FIT_LDS doubles.  Results: n, fp, ier (valid in every thread), the knots in F.t, the n7 distinct coefficients in F.c7.
template <int K>
__device__ __forceinline__ void fit_fpclos(const FitTrack& F, double* lds, const FitStage& L, int* s_state, double* s_val, int& n_out, double& fp_out,
                                           int& ier_out)
{
    const int tid = threadIdx.x;
    const int mi = F.mi, m1 = F.m1, nest = F.nest;
    const int nmin = 2 * (K + 1), nmax = mi + 2 * K;
    const double s = F.s, acc = 0.001 * s;
    gdouble* t = F.t;
    const gdouble* u = F.u;
    // thread 0's registers across the rounds
    double fp0 = 0.0, fpold = 0.0, fp = 0.0, fpms = 0.0;
    int nplus = 1, n = nmin, ier = 0;
    if (tid == 0) {
        double mx = 0.0, my = 0.0;
        for (int i = 0; i < m1; ++i) {
            mx = mx + F.pts[(size_t)i * 2];
            my = my + F.pts[(size_t)i * 2 + 1];
        }
        mx = mx / (double)m1;
        my = my / (double)m1;
        for (int i = 0; i < m1; ++i) {
            const double dx = F.pts[(size_t)i * 2] - mx, dy = F.pts[(size_t)i * 2 + 1] - my;
            fp0 = fp0 + (dx * dx + dy * dy);
        }
        F.c7[0] = mx;
        F.c7[1] = my;
        int state = FIT_CONTINUE;
        fit_wrap_knots(t, nmin, K, u[0], u[mi - 1]);
        if (s == 0.0) {
            if (nmax > nest) {
                state = FIT_DONE; ier = 1; fp = fp0;
            } else {
                n = nmax;
                for (int i = 1; i < m1; ++i) t[i + K] = (K & 1) ? u[i] : (u[i] + u[i - 1]) * 0.5;
            }
        } else {
            fpms = fp0 - s;
            fp = fp0;
            if (fpms < acc || nmax == nmin) {
                state = FIT_DONE; ier = -2;
            } else if (n >= nest) {
                state = FIT_DONE; ier = 1;
            } else {
                const int mm = (mi + 1) / 2;
                t[K + 1] = u[mm - 1];
                n = nmin + 1;
                F.nrdata[0] = mm - 2;
                F.nrdata[1] = m1 - mm;
            }
        }
        fpold = fp0;
        s_state[0] = state;
        s_state[1] = n;
        s_state[2] = ier;
        s_val[0] = fp;
    }
    __syncthreads();
    int state = s_state[0];
    n = s_state[1];
    int n7 = n - 2 * K - 1;
    for (int round = 0; state == FIT_CONTINUE && round <= mi; ++round) {
        n7 = n - 2 * K - 1;
        const int wsz = (2 * K + 5) * n7;
        const bool fits = wsz <= MCQ_FIT_LDS;
        if (tid == 0) fit_wrap_knots(t, n, K, u[0], u[mi - 1]);
        if (fits) for (int i = tid; i < wsz; i += MCQ_NT) lds[i] = 0.0;
        else for (int i = tid; i < wsz; i += MCQ_NT) F.G[i] = 0.0;
        __syncthreads();
        for (int it = tid; it < m1; it += MCQ_NT) fit_bspl<K>(F, n, it);
        __syncthreads();
        for (int it = tid; it < m1; it += MCQ_NT) fit_reduce_segment<K>(F, it);
        __syncthreads();
        for (int base = 0; base < m1; base += MCQ_FIT_CHUNK) {
            const int cnt = m1 - base < MCQ_FIT_CHUNK ? m1 - base : MCQ_FIT_CHUNK;
            if (tid < cnt) {
                const int it = base + tid;
                const bool row = F.vf[it] != 0;
                L.l[tid] = row ? F.lidx[it] : -1;
                if (row) {
                    #pragma unroll
                    for (int j = 0; j <= K; ++j) L.q[tid * (K + 1) + j] = F.qr[(size_t)it * (K + 1) + j];
                    L.p[2 * tid] = F.zr[(size_t)it * 2];
                    L.p[2 * tid + 1] = F.zr[(size_t)it * 2 + 1];
                }
            }
            __syncthreads();
            if (tid == 0) {
                for (int r = 0; r < cnt; ++r) {
                    if (L.l[r] < 0) continue;
                    double v[K + 1];
                    #pragma unroll
                    for (int j = 0; j <= K; ++j) v[j] = L.q[r * (K + 1) + j];
                    const int first = L.l[r] - K;
                    if (fits) fit_rotate<K, K + 1>(lds, n7, first, v, L.p[2 * r], L.p[2 * r + 1]);
                    else fit_rotate<K, K + 1>(F.G, n7, first, v, L.p[2 * r], L.p[2 * r + 1]);
                }
            }
            __syncthreads();
        }
        if (tid == 0) {
            if (fits) fit_solve<K>(lds, n7, F.c7);
            else fit_solve<K>(F.G, n7, F.c7);
        }
        __syncthreads();
        for (int it = tid; it < m1; it += MCQ_NT) fit_residual<K>(F, n7, it);
        __syncthreads();
        // fp, and in the same pass the residual sums per knot interval (kept only if knots are added): a point on a knot is shared half and
        // half, the first point goes to the last interval
        {
            const int nrint = n - nmin + 1;
            double fpart = 0.0, tl = 0.0;
            int i = 0, l = K;
            if (tid == 0) {
                fp = 0.0;
                tl = t[l];
            }
            for (int base = 0; base < m1; base += MCQ_NT) {
                const int cnt = m1 - base < MCQ_NT ? m1 - base : MCQ_NT;
                if (tid < cnt) {
                    L.e[tid] = F.term[base + tid];
                    L.u[tid] = u[base + tid];
                }
                __syncthreads();
                if (tid == 0) {
                    for (int r = 0; r < cnt; ++r) {
                        const double term = L.e[r];
                        fp = fp + term;
                        if (s == 0.0) continue;
                        bool nw = false;
                        if (L.u[r] >= tl) {
                            nw = true;
                            ++l;
                            tl = t[l];
                        }
                        fpart = fpart + term;
                        if (nw) {
                            if (l <= K + 1) {
                                F.fpint[nrint - 1] = term;
                            } else {
                                const double store = term * 0.5;
                                F.fpint[i] = fpart - store;
                                ++i;
                                fpart = store;
                            }
                        }
                    }
                }
                __syncthreads();
            }
            if (tid == 0 && s != 0.0) F.fpint[nrint - 1] = F.fpint[nrint - 1] + fpart;
        }
        if (tid == 0) {
            fpms = fp - s;
            int st = FIT_CONTINUE;
            if (s == 0.0) { st = FIT_DONE; ier = -1; }
            else if (fabs(fpms) < acc) { st = FIT_DONE; ier = 0; }
            else if (fpms < 0.0) st = FIT_SMOOTH;
            else if (n == nmax) { st = FIT_DONE; ier = -1; }
            else if (n == nest) { st = FIT_DONE; ier = 1; }
            else {
                int nrint = n - nmin + 1;
                int npl1 = nplus * 2;
                if (fpold - fp > acc) npl1 = (int)((double)nplus * fpms / (fpold - fp));
                int mxn = npl1 > nplus / 2 ? npl1 : nplus / 2;
                if (mxn < 1) mxn = 1;
                nplus = nplus * 2 < mxn ? nplus * 2 : mxn;
                fpold = fp;
                for (int add = 0; add < nplus; ++add) {
                    // fpknot: the interval with the largest residual sum that holds data points (the lowest index at a tie), split at its middle point
                    double fpmax = 0.0;
                    int number = -1, maxpt = 0, maxbeg = 0, jbegin = 0;
                    for (int j = 0; j < nrint; ++j) {
                        const int jp = F.nrdata[j];
                        if (jp != 0 && F.fpint[j] > fpmax) {
                            fpmax = F.fpint[j];
                            number = j;
                            maxpt = jp;
                            maxbeg = jbegin;
                        }
                        jbegin += jp + 1;
                    }
                    if (number < 0) { st = FIT_DONE; ier = 10; break; }
                    const int ihalf = maxpt / 2 + 1, nrx = maxbeg + ihalf, nxt = number + 1;
                    for (int j = nrint - 1; j >= nxt; --j) {
                        F.fpint[j + 1] = F.fpint[j];
                        F.nrdata[j + 1] = F.nrdata[j];
                    }
                    for (int j = n - 1; j >= nxt + K; --j) t[j + 1] = t[j];
                    F.nrdata[number] = ihalf - 1;
                    F.nrdata[nxt] = maxpt - ihalf;
                    const double am = (double)maxpt;
                    F.fpint[number] = fpmax * (double)(ihalf - 1) / am;
                    F.fpint[nxt] = fpmax * (double)(maxpt - ihalf) / am;
                    t[nxt + K] = u[nrx];
                    ++n;
                    ++nrint;
                    if (n == nmax) {
                        for (int q = 1; q < m1; ++q) t[q + K] = (K & 1) ? u[q] : (u[q] + u[q - 1]) * 0.5;
                        break;
                    }
                    if (n == nest) break;
                }
            }
            s_state[0] = st;
            s_state[1] = n;
            s_state[2] = ier;
            s_val[0] = fp;
        }
        __syncthreads();
        state = s_state[0];
        if (state == FIT_CONTINUE) n = s_state[1];
    }
    if (state == FIT_CONTINUE) {        // (not reached: m rounds bound FITPACK's loop as well)
        state = FIT_DONE;
        if (tid == 0) s_state[2] = 10;
    }
    if (state == FIT_SMOOTH) {
        // the smoothing spline: f(p) = s by rational interpolation on the rows of fpdisc weighted 1 / p
        const int wsz = (2 * K + 5) * n7, n8 = n7 - 1;
        const bool fits = wsz <= MCQ_FIT_LDS;
        for (int i = tid; i < wsz; i += MCQ_NT) F.R[i] = fits ? lds[i] : F.G[i];
        for (int r = tid; r < n8; r += MCQ_NT) fit_disc_row<K>(F, n, r);
        double p = 0.0, p1 = 0.0, f1 = 0.0, p3 = -1.0, f3 = 0.0;
        int ich1 = 0, ich3 = 0;
        if (tid == 0) {
            f1 = fp0 - s;
            f3 = fpms;
            p = (double)n7 / (fits ? fit_trace<K>(lds, n7) : fit_trace<K>(F.G, n7));
            ier = 3;
        }
        for (int it = 1; it <= 20; ++it) {
            __syncthreads();
            if (it > 1) {
                if (fits) for (int i = tid; i < wsz; i += MCQ_NT) lds[i] = F.R[i];
                else for (int i = tid; i < wsz; i += MCQ_NT) F.G[i] = F.R[i];
                __syncthreads();
            }
            if (tid == 0) {
                const double pinv = 1.0 / p;
                for (int r = 0; r < n8; ++r) {
                    double v[K + 2];
                    #pragma unroll
                    for (int j = 0; j < K + 2; ++j) v[j] = F.D[(size_t)r * (K + 2) + j] * pinv;
                    if (fits) fit_rotate<K, K + 2>(lds, n7, r, v, 0.0, 0.0);
                    else fit_rotate<K, K + 2>(F.G, n7, r, v, 0.0, 0.0);
                }
                if (fits) fit_solve<K>(lds, n7, F.c7);
                else fit_solve<K>(F.G, n7, F.c7);
            }
            __syncthreads();
            for (int i = tid; i < m1; i += MCQ_NT) fit_residual<K>(F, n7, i);
            __syncthreads();
            if (tid == 0) fp = 0.0;
            for (int base = 0; base < m1; base += MCQ_NT) {
                const int cnt = m1 - base < MCQ_NT ? m1 - base : MCQ_NT;
                if (tid < cnt) L.e[tid] = F.term[base + tid];
                __syncthreads();
                if (tid == 0)
                    for (int r = 0; r < cnt; ++r) fp = fp + L.e[r];
                __syncthreads();
            }
            if (tid == 0) {
                fpms = fp - s;
                int stop = 0;
                if (fabs(fpms) < acc) { ier = 0; stop = 1; }
                else if (it == 20) stop = 1;
                else {
                    const double p2 = p, f2 = fpms;
                    bool step = true;
                    if (ich3 == 0) {
                        if (f2 - f3 <= acc) {           // the choice of p is too large
                            p3 = p2; f3 = f2;
                            p = p * 0.04;
                            if (p <= p1) p = p1 * 0.9 + p2 * 0.1;
                            step = false;
                        } else if (f2 < 0.0) ich3 = 1;
                    }
                    if (step && ich1 == 0) {
                        if (f1 - f2 <= acc) {           // the choice of p is too small
                            p1 = p2; f1 = f2;
                            p = p / 0.04;
                            if (p3 >= 0.0 && p >= p3) p = p2 * 0.1 + p3 * 0.9;
                            step = false;
                        } else if (f2 > 0.0) ich1 = 1;
                    }
                    if (step) {
                        if (f2 >= f1 || f2 <= f3) { ier = 2; stop = 1; }
                        else {
                            if (p3 > 0.0) {
                                const double h1 = f1 * (f2 - f3), h2 = f2 * (f3 - f1), h3 = f3 * (f1 - f2);
                                p = -(p1 * p2 * h3 + p2 * p3 * h1 + p3 * p1 * h2) / (p1 * h1 + p2 * h2 + p3 * h3);
                            } else {
                                p = (p1 * (f1 - f3) * f2 - p2 * (f2 - f3) * f1) / ((f1 - f2) * f3);
                            }
                            if (f2 < 0.0) { p3 = p2; f3 = f2; }
                            else { p1 = p2; f1 = f2; }
                        }
                    }
                }
                s_state[0] = stop;
                s_state[2] = ier;
                s_val[0] = fp;
            }
            __syncthreads();
            if (s_state[0]) break;
        }
    }
    __syncthreads();
    n_out = n;
    fp_out = s_val[0];
    ier_out = s_state[2];
}

template <int K>
__device__ __forceinline__ void fit_track_body(const McqFit& P, int tr, int mi, const gdouble* pts, const gdouble* u, double* lds, const FitStage& L,
                                               int* s_state, double* s_val)
{
    const int tid = threadIdx.x;
    const size_t nk = (size_t)P.nkmax, mm = (size_t)P.mimax;
    const size_t wmax = (size_t)(2 * K + 5) * nk;
    gdouble* base = (gdouble*)(P.work + (size_t)tr * P.work_per);
    FitTrack F;
    F.mi = mi; F.m1 = mi - 1; F.nest = P.nkmax; F.s = P.s;
    F.pts = pts; F.u = u;
    F.t = (gdouble*)(P.knots_out + (size_t)tr * nk);
    F.q = base;
    F.term = F.q + mm * (K + 1);
    F.R = F.term + mm;
    F.G = F.R + wmax;
    F.c7 = F.G + wmax;
    F.D = F.c7 + 2 * nk;
    F.fpint = F.D + nk * (K + 2);
    F.lidx = (gint*)(F.fpint + nk + 2);
    F.nrdata = F.lidx + mm;
    F.vf = F.nrdata + nk + 2;
    F.qr = (gdouble*)(P.work + (size_t)tr * P.work_per + P.work_per - mm * (K + 3));
    F.zr = F.qr + mm * (K + 1);
    int n, ier;
    double fp;
    fit_fpclos<K>(F, lds, L, s_state, s_val, n, fp, ier);
    gdouble* co = (gdouble*)(P.coef_out + (size_t)tr * 2 * nk);
    const bool good = ier != 10;
    const int n7 = n - 2 * K - 1, nc = n - K - 1;
    for (int i = tid; i < P.nkmax; i += MCQ_NT) {
        int col = i;
        if (good && i < nc) while (col >= n7) col -= n7;
        co[i] = good && i < nc ? F.c7[(size_t)col * 2] : NAN;
        co[nk + i] = good && i < nc ? F.c7[(size_t)col * 2 + 1] : NAN;
        if (!good || i >= n) F.t[i] = NAN;
    }
    if (!good && P.pts_out) {       // a refused track keeps no finite output: the points were written before the fit (each thread its own entries again)
        gdouble* po = (gdouble*)(P.pts_out + (size_t)tr * mm * 2);
        for (size_t i = tid; i < mm * 2; i += MCQ_NT) po[i] = NAN;
    }
    if (tid == 0) {
        ((gint*)P.nk_out)[tr] = good ? n : 0;
        ((gint*)P.ier_out)[tr] = ier;
        if (P.fp_out) ((gdouble*)P.fp_out)[tr] = good ? fp : NAN;
        ((gint*)P.status)[tr] = good ? MCQ_OK : MCQ_BAD_INPUT;
    }
}

__global__ void __launch_bounds__(MCQ_NT) mcq_spline_fit_kernel(McqFit P)
{
    __shared__ double s_w[MCQ_FIT_LDS];
    __shared__ double s_el[MCQ_NT];
    __shared__ double s_u[MCQ_NT];
    __shared__ double s_rq[MCQ_FIT_CHUNK * 6];
    __shared__ double s_rp[MCQ_FIT_CHUNK * 2];
    __shared__ int s_rl[MCQ_FIT_CHUNK];
    __shared__ double s_carry;
    __shared__ double s_val[2];
    __shared__ int s_state[4];
    __shared__ int s_bad;
    const int tid = threadIdx.x, tr = blockIdx.x;
    const size_t nm = (size_t)P.nmax, nk = (size_t)P.nkmax, mm = (size_t)P.mimax;
    const int n = P.n_list ? P.n_list[tr] : P.nmax;
    const gdouble* trk = (const gdouble*)(P.track + (size_t)tr * nm * 4);
    gdouble* cum = (gdouble*)(P.cum + (size_t)tr * (nm + 1));
    gdouble* pts = (gdouble*)(P.pts + (size_t)tr * mm * 2);
    gdouble* u = (gdouble*)(P.u + (size_t)tr * mm);
    gdouble* po = P.pts_out ? (gdouble*)(P.pts_out + (size_t)tr * mm * 2) : nullptr;
    if (tid == 0) {
        s_bad = 0;
        s_carry = 0.0;
    }
    __syncthreads();
    int need = 0;               // the closed sample count, where it is known
    bool bad = n < 3 || n > P.nmax;
    if (!bad) {
        int b = 0;
        for (int i = tid; i < n; i += MCQ_NT)
            if (!finite_d(trk[4 * (size_t)i]) || !finite_d(trk[4 * (size_t)i + 1])) b = 1;
        if (b) s_bad = 1;
        __syncthreads();
        bad = s_bad != 0;
    }
    if (!bad && P.step > 0.0) {
        // interp_track's rule: the closed raw line's running sum, numpy.linspace, numpy.interp -- mcq_bound_points_kernel's rule, written here
        // a second time because this file is compiled without contraction and that kernel fuses slope * (x - xp) + fp: one function would
        // round one of the two differently from what it returns today
        if (tid == 0) cum[0] = 0.0;
        int b = 0;
        running_sum<MCQ_NT>(n, s_el, s_carry, cum + 1, [&](int i) {
            const int j = i + 1 < n ? i + 1 : 0;
            const double dx = trk[4 * (size_t)j] - trk[4 * (size_t)i], dy = trk[4 * (size_t)j + 1] - trk[4 * (size_t)i + 1];
            const double e = sqrt(dx * dx + dy * dy);
            if (!(e > 0.0)) b = 1;
            return e;
        });
        if (b) s_bad = 1;
        __syncthreads();
        const double total = s_carry;
        const double cnt = ceil(total / P.step);
        if (s_bad || !finite_d(cnt) || !(cnt >= 1.0)) bad = true;
        else if (cnt + 1.0 > (double)P.mimax) {
            bad = true;
            need = cnt < 2147483646.0 ? (int)cnt + 1 : 0;
        } else {
            const int nb = (int)cnt;
            need = nb + 1;
            const double dl = total / (double)nb;
            for (int j = tid; j < nb; j += MCQ_NT) {
                const double x = (double)j * dl;
                int lo = 0, hi = n - 1;
                while (lo < hi) {
                    const int mid = (lo + hi + 1) >> 1;
                    if (cum[mid] <= x) lo = mid;
                    else hi = mid - 1;
                }
                const int k1 = lo + 1 < n ? lo + 1 : 0;
                const double x0 = cum[lo], den = cum[(size_t)lo + 1] - x0;
                const double fx = trk[4 * (size_t)lo], fy = trk[4 * (size_t)lo + 1];
                const double sx = (trk[4 * (size_t)k1] - fx) / den, sy = (trk[4 * (size_t)k1 + 1] - fy) / den;
                pts[2 * (size_t)j] = sx * (x - x0) + fx;
                pts[2 * (size_t)j + 1] = sy * (x - x0) + fy;
            }
            __syncthreads();
            if (tid == 0) {
                pts[2 * (size_t)nb] = pts[0];
                pts[2 * (size_t)nb + 1] = pts[1];
            }
        }
    } else if (!bad) {
        need = n + 1;
        if (need > P.mimax) bad = true;
        else
            for (int i = tid; i <= n; i += MCQ_NT) {
                const int r = i < n ? i : 0;
                pts[2 * (size_t)i] = trk[4 * (size_t)r];
                pts[2 * (size_t)i + 1] = trk[4 * (size_t)r + 1];
            }
    }
    const int mi = need;
    if (!bad && mi <= P.k) bad = true;              // scipy: "m > k must hold"
    __syncthreads();
    if (!bad) {
        // the parameter: u_0 = 0, u_i = u_(i-1) + the chord, each divided by the last, u_(mi-1) = 1
        if (tid == 0) {
            s_carry = 0.0;
            s_bad = 0;
            u[0] = 0.0;
        }
        __syncthreads();
        running_sum<MCQ_NT>(mi - 1, s_el, s_carry, u + 1, [&](int i) {
            const double dx = pts[2 * (size_t)(i + 1)] - pts[2 * (size_t)i], dy = pts[2 * (size_t)(i + 1) + 1] - pts[2 * (size_t)i + 1];
            return sqrt(dx * dx + dy * dy);
        });
        const double last = s_carry;
        if (!(last > 0.0) || !finite_d(last)) bad = true;          // (uniform)
        if (!bad) {
            for (int i = tid; i < mi; i += MCQ_NT) u[i] = i == mi - 1 ? 1.0 : u[i] / last;
            __syncthreads();
            int b = 0;
            for (int i = tid; i < mi - 1; i += MCQ_NT)
                if (!(u[i] < u[i + 1])) b = 1;
            if (b) s_bad = 1;
            __syncthreads();
            bad = s_bad != 0;
        }
    }
    if (po) for (size_t i = tid; i < mm * 2; i += MCQ_NT) po[i] = (!bad && i < (size_t)mi * 2) ? pts[i] : NAN;
    if (tid == 0 && P.mi_out) ((gint*)P.mi_out)[tr] = need;
    if (bad) {
        gdouble* kn = (gdouble*)(P.knots_out + (size_t)tr * nk);
        gdouble* co = (gdouble*)(P.coef_out + (size_t)tr * 2 * nk);
        for (size_t i = tid; i < nk; i += MCQ_NT) kn[i] = NAN;
        for (size_t i = tid; i < 2 * nk; i += MCQ_NT) co[i] = NAN;
        if (tid == 0) {
            ((gint*)P.nk_out)[tr] = 0;
            ((gint*)P.ier_out)[tr] = 10;
            if (P.fp_out) ((gdouble*)P.fp_out)[tr] = NAN;
            ((gint*)P.status)[tr] = MCQ_BAD_INPUT;
        }
        return;
    }
    FitStage L;
    L.q = s_rq; L.p = s_rp; L.l = s_rl; L.e = s_el; L.u = s_u;
    switch (P.k) {
    case 1: fit_track_body<1>(P, tr, mi, pts, u, s_w, L, s_state, s_val); break;
    case 2: fit_track_body<2>(P, tr, mi, pts, u, s_w, L, s_state, s_val); break;
    case 3: fit_track_body<3>(P, tr, mi, pts, u, s_w, L, s_state, s_val); break;
    case 4: fit_track_body<4>(P, tr, mi, pts, u, s_w, L, s_state, s_val); break;
    default: fit_track_body<5>(P, tr, mi, pts, u, s_w, L, s_state, s_val); break;
    }
}
#undef FIT_ROT
#undef MCQ_FIT_CHUNK
#undef MCQ_FIT_SEG
#undef FIT_CONTINUE
#undef FIT_DONE
#undef FIT_SMOOTH
