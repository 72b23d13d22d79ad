// ---- friction maps on the device (mcq_fmap_query_device, mcq_friction_grid_device; include/mcq.h): the nearest cell of a point
//      [REF opt_mintime_traj/src/friction_map_interface.py:61, a cKDTree query], the grids of friction under the four wheels along every normal
//      [REF opt_mintime_traj/src/extract_friction_coeffs.py:81-104] and their line per waypoint [REF opt_mintime_traj/src/approx_friction_map.py:97-100].
//      Included from mcq_kernels.hip INSIDE its contraction-off section: the counts, numpy.linspace's positions and the wheels' coordinates are
//      Python's and numpy's roundings only while every product and sum is rounded on its own, and the bin edges are the bits the host sorted the
//      cells by (mcq_fmap_create).
//
//      The index (McqFmap): a uniform grid of nbx x nby bins of one side over the cells' bounding box, in CSR form.  bin_start[iy * nbx + ix] is
//      the first of the bin's cells in sxy / sidx (coordinates and original index, sorted by bin); a ROW of bins is one contiguous span of cells,
//      so a block of bins is scanned as one span per row.  A cell of bin ix lies between fric_edge(ix) and fric_edge(ix + 1), both included; the
//      first and the last bin of an axis are open to the outside.
//
//      The search (fric_nearest) is exact: the 3 x 3 block around the query's bin (clamped into the grid), then ring after ring, until the best
//      squared distance is STRICTLY below the squared distance from the query to the nearest side of the block -- sides on the grid's border do
//      not count, nothing lies beyond them -- or the grid is exhausted.  Every cell outside the block has a computed squared distance of at least
//      that bound (rounding is monotonic), so with the strict comparison none of them can even tie.  Among cells at exactly equal computed squared
//      distance the lowest original index wins. ----

// the lower edge of bin k along an axis that starts at o: the same two roundings as the host's (mcq_fmap_create)
__device__ __forceinline__ double fric_edge(double o, double side, int k) { return o + (double)k * side; }

__device__ __forceinline__ int fric_bin(double q, double o, double side, int nb)
{
    const double t = floor((q - o) / side);
    return t >= (double)(nb - 1) ? nb - 1 : (t > 0.0 ? (int)t : 0);
}

// the cells of bins ix0 .. ix1 of bin row iy: one span
__device__ __forceinline__ void fric_span(const McqFmap& F, int iy, int ix0, int ix1, double qx, double qy, double& best, int& bi)
{
    const int* bs = F.bin_start + (size_t)iy * F.nbx;
    const int c1 = bs[ix1 + 1];
    for (int c = bs[ix0]; c < c1; ++c) {
        const double dx = F.sxy[2 * (size_t)c] - qx, dy = F.sxy[2 * (size_t)c + 1] - qy;
        const double d2 = dx * dx + dy * dy;
        if (d2 <= best) {
            const int id = F.sidx[c];
            if (d2 < best || id < bi) { best = d2; bi = id; }
        }
    }
}

// idx = the nearest cell's original index and d2 its squared distance; -1 and NaN for a query that is not finite
__device__ __forceinline__ void fric_nearest(const McqFmap& F, double qx, double qy, int& idx, double& d2)
{
    if (!(finite_d(qx) && finite_d(qy))) { idx = -1; d2 = NAN; return; }
    const int nbx = F.nbx, nby = F.nby;
    const int bx = fric_bin(qx, F.x0, F.side, nbx), by = fric_bin(qy, F.y0, F.side, nby);
    double best = INFINITY;
    int bi = 0x7fffffff;
    for (int r = 1;; ++r) {
        const int x_lo = bx - r, x_hi = bx + r, y_lo = by - r, y_hi = by + r;
        const int cx0 = x_lo > 0 ? x_lo : 0, cx1 = x_hi < nbx - 1 ? x_hi : nbx - 1;
        const int cy0 = y_lo > 0 ? y_lo : 0, cy1 = y_hi < nby - 1 ? y_hi : nby - 1;
        if (r == 1) {       // the 3 x 3 block: three spans
            for (int iy = cy0; iy <= cy1; ++iy) fric_span(F, iy, cx0, cx1, qx, qy, best, bi);
        } else {            // a ring: its two outer rows whole, of the rows between them the two new bins -- whatever of it lies inside the grid
            if (y_lo >= 0) fric_span(F, y_lo, cx0, cx1, qx, qy, best, bi);
            if (y_hi < nby) fric_span(F, y_hi, cx0, cx1, qx, qy, best, bi);
            if (x_lo >= 0 || x_hi < nbx) {
                const int iy1 = y_hi - 1 < nby - 1 ? y_hi - 1 : nby - 1;
                for (int iy = y_lo + 1 > 0 ? y_lo + 1 : 0; iy <= iy1; ++iy) {
                    if (x_lo >= 0) fric_span(F, iy, x_lo, x_lo, qx, qy, best, bi);
                    if (x_hi < nbx) fric_span(F, iy, x_hi, x_hi, qx, qy, best, bi);
                }
            }
        }
        bool open = false;
        double dmin = INFINITY;
        if (x_lo > 0) { open = true; dmin = fmin(dmin, qx - fric_edge(F.x0, F.side, x_lo)); }
        if (x_hi < nbx - 1) { open = true; dmin = fmin(dmin, fric_edge(F.x0, F.side, x_hi + 1) - qx); }
        if (y_lo > 0) { open = true; dmin = fmin(dmin, qy - fric_edge(F.y0, F.side, y_lo)); }
        if (y_hi < nby - 1) { open = true; dmin = fmin(dmin, fric_edge(F.y0, F.side, y_hi + 1) - qy); }
        if (!open) break;                                   // the whole grid has been scanned
        if (dmin > 0.0 && best < dmin * dmin) break;        // (a query outside the block -- outside the box -- keeps widening)
    }
    idx = bi;
    d2 = best;
}

__global__ void __launch_bounds__(MCQ_NT) mcq_fmap_query_kernel(McqFmap F, int count, const double* xy, double* mue_out, int* idx_out, double* dist_out)
{
    const int q = blockIdx.x * MCQ_NT + threadIdx.x;
    if (q >= count) return;
    int idx;
    double d2;
    fric_nearest(F, xy[2 * (size_t)q], xy[2 * (size_t)q + 1], idx, d2);
    mue_out[q] = idx >= 0 ? F.mue[idx] : NAN;
    if (idx_out) idx_out[q] = idx;
    if (dist_out) dist_out[q] = sqrt(d2);
}

// Python's math.floor((w - 0.5 * width - 0.5) / dn), held inside int range (a count above jmax is refused anyway)
__device__ __forceinline__ int fric_steps(double w, double hw, double dn)
{
    const double f = floor((w - hw - 0.5) / dn);
    return f > 1.0e9 ? 1000000000 : (f < -1.0e9 ? -1000000000 : (int)f);
}

// a workgroup per MCQ_FG_ROWS rows of a track, a wave per row, sixteen lanes per wheel.  Every workgroup forms the track's verdict itself (the rows
// are few and sit in the cache): the outputs of a refused track are NaN in every row.  The sums of a line run over each lane's positions in
// rising order and then over the sixteen lanes by four exchanges: one order, whatever the grid.
__global__ void __launch_bounds__(MCQ_NT) mcq_friction_grid_kernel(McqFricGrid G)
{
    __shared__ int s_bad, s_over;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int nblk = (G.nmax + MCQ_FG_ROWS) / MCQ_FG_ROWS;      // blocks of a track's nmax + 1 rows
    const int t = blockIdx.x / nblk, rb = blockIdx.x % nblk;
    const int n = G.n_list ? G.n_list[t] : G.nmax;
    const double width = G.width_list ? G.width_list[t] : G.width;
    const double hw = 0.5 * width, dn = G.dn;
    const double* ref = G.ref + (size_t)t * G.nmax * 4;
    const double* nv = G.nv + (size_t)t * G.nmax * 2;
    if (tid == 0) { s_bad = 0; s_over = 0; }
    __syncthreads();
    bool bad = n < 1 || n > G.nmax || !(finite_d(width) && finite_d(G.wbf) && finite_d(G.wbr));
    if (!bad) {
        bool any_bad = false, any_over = false;
        for (int r = tid; r < n; r += MCQ_NT) {
            const double x = ref[4 * r], y = ref[4 * r + 1], wr = ref[4 * r + 2], wl = ref[4 * r + 3], nx = nv[2 * r], ny = nv[2 * r + 1];
            if (!(finite_d(x) && finite_d(y) && finite_d(wr) && finite_d(wl) && finite_d(nx) && finite_d(ny))) any_bad = true;
            else if (fric_steps(wr, hw, dn) + fric_steps(wl, hw, dn) + 1 > G.jmax) any_over = true;
        }
        if (any_bad) s_bad = 1;
        if (any_over) s_over = 1;
    }
    __syncthreads();
    bad = bad || s_bad != 0;
    const bool over = !bad && s_over != 0;      // refused for a count above jmax: cnt_out reports the counts it needs
    if (rb == 0 && tid == 0) G.status[t] = (bad || over) ? MCQ_BAD_INPUT : MCQ_OK;
    const int row = rb * MCQ_FG_ROWS + wv;
    if (row > G.nmax) return;       // (the whole wave; no barrier follows)
    const size_t ro = (size_t)t * (G.nmax + 1) + row;
    int cnt = 0, nr = 0, nl = 0;
    double x = 0.0, y = 0.0, nx = 0.0, ny = 0.0;
    if (!bad && row <= n) {
        const int i = row == n ? 0 : row;       // the reference closes the track with row 0 again
        x = ref[4 * i]; y = ref[4 * i + 1]; nx = nv[2 * i]; ny = nv[2 * i + 1];
        nr = fric_steps(ref[4 * i + 2], hw, dn);
        nl = fric_steps(ref[4 * i + 3], hw, dn);
        cnt = nr + nl + 1;
    }
    if (lane == 0) G.cnt_out[ro] = cnt;
    const int c = (!over && cnt > 0) ? cnt : 0;         // positions delivered; the rest of the row is NaN
    const size_t wstride = (size_t)(G.nmax + 1) * G.jmax;
    double* n_row = G.n_out + ro * G.jmax;
    double* m_row = G.mue_out + (size_t)t * 4 * wstride + (size_t)row * G.jmax;
    int* i_row = G.idx_out ? G.idx_out + (size_t)t * 4 * wstride + (size_t)row * G.jmax : nullptr;
    for (int j = c + lane; j < G.jmax; j += 64) {
        n_row[j] = NAN;
        for (int w = 0; w < 4; ++w) {
            m_row[w * wstride + j] = NAN;
            if (i_row) i_row[w * wstride + j] = -1;
        }
    }
    // numpy.linspace(-dn * num_right, dn * num_left, count): arange * step + start, the last entry set to stop
    const double start = -dn * (double)nr, stop = dn * (double)nl, delta = stop - start;
    const double step = c > 1 ? delta / (double)(c - 1) : delta;       // (a single position: numpy forms 0 * delta + start)
    const int wheel = lane >> 4, jj = lane & 15;                        // fl, fr, rl, rr
    const double along = wheel < 2 ? G.wbf : -G.wbr, side = (wheel & 1) ? -hw : hw;
    const double tx = -ny, ty = nx;
    const double ax = x + along * tx, ay = y + along * ty;
    double* m_w = m_row + wheel * wstride;
    double sm = 0.0, sn = 0.0;
    for (int j = jj; j < c; j += 16) {
        double nj = (double)j * step + start;
        if (c > 1 && j == c - 1) nj = stop;
        if (wheel == 0) n_row[j] = nj;
        const double lat = nj + side;
        int idx;
        double d2;
        fric_nearest(G.F, ax - lat * nx, ay - lat * ny, idx, d2);
        const double mu = idx >= 0 ? G.F.mue[idx] : NAN;
        m_w[j] = mu;
        if (i_row) i_row[wheel * wstride + j] = idx;
        sm += mu;
        sn += nj;
    }
    if (!G.w_out) return;           // (uniform)
    for (int m = 1; m < 16; m <<= 1) { sm += __shfl_xor(sm, m); sn += __shfl_xor(sn, m); }
    const double mm = sm / (double)c, mn = sn / (double)c;
    double sxy = 0.0, sxx = 0.0;
    for (int j = jj; j < c; j += 16) {
        double nj = (double)j * step + start;
        if (c > 1 && j == c - 1) nj = stop;
        const double dnj = nj - mn;
        sxy += dnj * (m_w[j] - mm);         // (the lane's own stores)
        sxx += dnj * dnj;
    }
    for (int m = 1; m < 16; m <<= 1) { sxy += __shfl_xor(sxy, m); sxx += __shfl_xor(sxx, m); }
    if (jj == 0) {
        double* w = G.w_out + ((size_t)t * 4 * (G.nmax + 1) + (size_t)wheel * (G.nmax + 1) + row) * 2;
        const double slope = c > 1 ? sxy / sxx : NAN;
        w[0] = slope;
        w[1] = c > 1 ? mm - slope * mn : NAN;
    }
}

// ---- the Gaussian-basis fit and the models' evaluation (mcq_friction_gauss_device, mcq_friction_model_device; include/mcq.h)
//      [REF opt_mintime_traj/src/approx_friction_map.py:102-127 and its GaussianFeatures, opt_mintime.py:733-747].  Per row the minimum-norm
//      least-squares solution of the centred cnt x N system, N = 2 n_gauss + 1, by a one-sided Jacobi (Hestenes) decomposition: plane rotations
//      from the right make the columns of A orthogonal and are accumulated in V, so that A_end = U S and x = V S^+ U^T b; the Gram matrix, whose
//      condition is the square of an already large one, is never formed.
//
//      Lanes (DESIGN.md "Gaussian friction fit"): a wave per row.  Lane l owns the samples j = l, l + 64, ... of every column of A (column-major
//      in LDS, stride jmax) and, where l < N, row l of V (V[k * N + l]).  A rotation of the pair (p, q) therefore touches only a lane's own
//      entries, and the one thing lanes exchange is the pair's three inner products: every lane stores its partial sums (over its samples, rising)
//      into one of two alternating buffers, and after a wave barrier EVERY lane adds the first min(cnt, 64) partials in rising lane order -- one
//      order, all lanes hold the same bits, every branch on them is uniform.  The pairs are taken one after another in the row-cyclic order
//      (0,1) (0,2) .. (0,N-1) (1,2) .. (N-2,N-1).  Nothing depends on which rows share the workgroup.
//
//      A pair is rotated while its columns are not orthogonal to sqrt(cnt) eps AND both lie above 2^-20 of the cut rcond * (the largest column
//      norm seen so far): the columns of a structurally rank-deficient row (cnt <= N) that converge to zero never pass the first test, and frozen
//      that far below the cut they leave the rank to the problem, not to the sweep that happened to cross the cut. ----
#define MCQ_FGS_SWEEPS 40       /* a row that has not settled by then delivers NaN and rank -1 */

// the sum of one value per lane over the lanes 0 .. nl-1 in rising order, the same bits in every lane
__device__ __forceinline__ double fgs_wsum(double* part, int lane, int nl, double v)
{
    part[lane] = v;
    __builtin_amdgcn_wave_barrier();
    double s = 0.0;
    for (int l = 0; l < nl; ++l) s += part[l];
    __builtin_amdgcn_wave_barrier();
    return s;
}

// exp(x) to about half a unit in the last place (0.53 at worst over 4e6 arguments in [-120, 0] against long double, on the host).  The weights
// carry the features' rounding times the problem's conditioning, so the feature is formed as the host's exp forms it, not to the device library's one unit:
// x = k ln2 + r with ln2 in two pieces (k * LN2_HI and the difference are exact), exp(r) = 1 + r + r^2 / 2 + tail, the tail (below 0.008, a
// polynomial to r^14 in plain double) and the low pieces added first, the leading three terms through two exact sums, one final rounding.
// KEEP THESE TWO FUNCTIONS INSIDE THE CONTRACTION-OFF SECTION (mcq_kernels.hip includes this file behind `#pragma clang fp contract(off)`), and
// build them without fast-math: fgs_two_sum's error term is exact only while every sum is rounded on its own, r_hi is exact only because
// kd * LN2_HI is a plain exact product followed by an exact difference, and the low pieces mean what the comments say only while no product is
// fused into the sum next to it (the one fma is asked for by name).  Moved elsewhere the function still compiles and silently returns other
// bits; tests/fgauss_checks.py (check_model, "a feature alone") holds it to 0.55 units in the last place on the device and on the interpreter.
__device__ __forceinline__ void fgs_two_sum(double a, double b, double& s, double& e)
{
    s = a + b;
    const double bb = s - a;
    e = (a - (s - bb)) + (b - bb);
}

__device__ __forceinline__ double fgs_exp(double x)
{
    if (!(x > -745.0)) return x < 0.0 ? 0.0 : x;           // (underflow; a NaN stays)
    if (x > 709.0) return INFINITY;
    const double kd = rint(x * 1.4426950408889634);
    const double r_hi = x - kd * 6.93147180369123816490e-01;        // LN2_HI: 21 bits below its leading one are zero, |k| < 2^11
    const double r_lo = -(kd * 1.90821492927058770002e-10);         // LN2_LO
    const double r = r_hi + r_lo;
    double p = 1.0 / 87178291200.0;                                 // 1 / 14!
    p = p * r + 1.0 / 6227020800.0;
    p = p * r + 1.0 / 479001600.0;
    p = p * r + 1.0 / 39916800.0;
    p = p * r + 1.0 / 3628800.0;
    p = p * r + 1.0 / 362880.0;
    p = p * r + 1.0 / 40320.0;
    p = p * r + 1.0 / 5040.0;
    p = p * r + 1.0 / 720.0;
    p = p * r + 1.0 / 120.0;
    p = p * r + 1.0 / 24.0;
    p = p * r + 1.0 / 6.0;
    const double tail = ((r * r) * r) * p;
    const double s_hi = r_hi * r_hi, s_lo = fma(r_hi, r_hi, -s_hi);         // r_hi^2 in two pieces (an fma asked for by name; nothing is contracted)
    const double sq_lo = (0.5 * s_lo + r_hi * r_lo) + 0.5 * (r_lo * r_lo);  // r^2 / 2 = 0.5 s_hi + sq_lo
    double h1, l1, h2, l2;
    fgs_two_sum(1.0, r_hi, h1, l1);
    fgs_two_sum(h1, 0.5 * s_hi, h2, l2);
    return ldexp(h2 + ((((l1 + l2) + r_lo) + sq_lo) + tail), (int)kd);
}

// numpy.linspace(start, stop, num)[k] for num >= 2: k * step + start in two roundings, the last entry the stop value itself
__device__ __forceinline__ double fgs_linspace(double start, double stop, double step, int num, int k) { return k == num - 1 ? stop : (double)k * step + start; }

__global__ void __launch_bounds__(MCQ_NT) mcq_friction_gauss_kernel(McqFricGauss G)
{
    HIP_DYNAMIC_SHARED(double, fgs_lds)
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int N = G.N, jmax = G.jmax, P1 = N + 1;
    const int nblk = (G.nmax + G.rows_wg) / G.rows_wg;
    const int t = blockIdx.x / nblk, row = (blockIdx.x % nblk) * G.rows_wg + wv;
    if (row > G.nmax) return;           // (the whole wave; the kernel has no workgroup barrier)
    double* A = fgs_lds + (size_t)wv * ((size_t)N * ((size_t)jmax + N + 6) + MCQ_FGS_PART);       // (mcq_fgs_row_doubles) [N][jmax]
    double* V = A + (size_t)N * jmax;                                   // [N][N]: V[k * N + i] = entry i of column k
    double* cm = V + N * N;                                             // [N] column means of the features
    double* s2 = cm + N;                                                // [N] squared singular values
    double* Z = s2 + N;                                                 // [4][N] U^T b / S per wheel (0 where the singular value is cut)
    double* part = Z + 4 * N;                                           // [MCQ_FGS_PART]
    const size_t ro = (size_t)t * (G.nmax + 1) + row;
    const size_t wstride = (size_t)(G.nmax + 1) * jmax;
    const int cnt = G.cnt[ro];
    const int c = (G.status[t] == MCQ_OK && cnt >= 1 && cnt <= jmax) ? cnt : 0;
    double* w_row = G.w_out + ((size_t)t * 4 * (G.nmax + 1) + row) * P1;             // wheel w: + w * (nmax + 1) * P1
    const size_t w_wheel = (size_t)(G.nmax + 1) * P1;
    if (c < 2) {        // no row, or one position (the reference's width is 0 and its features NaN)
        for (int i = lane; i < 4 * P1; i += 64) w_row[(size_t)(i / P1) * w_wheel + i % P1] = NAN;
        if (lane == 0) {
            G.cd_out[ro] = c == 1 ? 0.0 : NAN;
            if (G.rank_out) G.rank_out[ro] = 0;
            if (G.sweeps_out) G.sweeps_out[ro] = 0;
        }
        return;
    }
    const double* n_row = G.n + ro * jmax;
    const double* m_row = G.mue + (size_t)t * 4 * wstride + (size_t)row * jmax;
    const int nl = c < 64 ? c : 64;
    const double n0 = n_row[0], n1 = n_row[c - 1];
    const double cstep = (n1 - n0) / (double)(N - 1);
    const double width = 2.0 * (fgs_linspace(n0, n1, cstep, N, 1) - n0);
    // features, their column means, the centred columns; V = I
    for (int k = 0; k < N; ++k) {
        const double ck = fgs_linspace(n0, n1, cstep, N, k);
        double s = 0.0;
        for (int j = lane; j < c; j += 64) {
            const double arg = (n_row[j] - ck) / width;
            const double f = fgs_exp(-0.5 * (arg * arg));
            A[(size_t)k * jmax + j] = f;
            s += f;
        }
        const double mean = fgs_wsum(part, lane, nl, s) / (double)c;
        for (int j = lane; j < c; j += 64) A[(size_t)k * jmax + j] -= mean;
        if (lane == 0) cm[k] = mean;
        if (lane < N) V[k * N + lane] = lane == k ? 1.0 : 0.0;
    }
    const double rc = G.rcond > 0.0 ? G.rcond : (double)(c > N ? c : N) * 2.220446049250313e-16;
    const double tol = 2.220446049250313e-16 * sqrt((double)c);
    double smax2 = 0.0;
    int sweeps = 0, buf = 0;
    bool settled = false;
    while (!settled && sweeps < MCQ_FGS_SWEEPS) {
        settled = true;
        ++sweeps;
        for (int p = 0; p < N - 1; ++p) {
            for (int q = p + 1; q < N; ++q) {
                double* ap = A + (size_t)p * jmax;
                double* aq = A + (size_t)q * jmax;
                double pa = 0.0, pb = 0.0, pg = 0.0;
                for (int j = lane; j < c; j += 64) {
                    const double x = ap[j], y = aq[j];
                    pa += x * x; pb += y * y; pg += x * y;
                }
                double* pp = part + buf * 192;
                buf ^= 1;
                pp[lane] = pa; pp[64 + lane] = pb; pp[128 + lane] = pg;
                __builtin_amdgcn_wave_barrier();
                double alpha = 0.0, beta = 0.0, gamma = 0.0;
                for (int l = 0; l < nl; ++l) { alpha += pp[l]; beta += pp[64 + l]; gamma += pp[128 + l]; }
                smax2 = fmax(smax2, fmax(alpha, beta));
                const double cut2 = ((rc * rc) * smax2) * 0x1p-40;
                if (!(alpha > cut2 && beta > cut2)) continue;           // a column 2^-20 below the cut-off: the pair counts as settled
                if (!(fabs(gamma) > tol * sqrt(alpha * beta))) continue;
                settled = false;
                const double zeta = (beta - alpha) / (2.0 * gamma);
                const double tn = (zeta < 0.0 ? -1.0 : 1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double cs = 1.0 / sqrt(1.0 + tn * tn), sn = cs * tn;
                for (int j = lane; j < c; j += 64) {
                    const double x = ap[j], y = aq[j];
                    ap[j] = cs * x - sn * y;
                    aq[j] = sn * x + cs * y;
                }
                if (lane < N) {
                    const double x = V[p * N + lane], y = V[q * N + lane];
                    V[p * N + lane] = cs * x - sn * y;
                    V[q * N + lane] = sn * x + cs * y;
                }
            }
        }
    }
    __builtin_amdgcn_wave_barrier();
    if (lane == 0) {
        G.cd_out[ro] = (n1 - n0) / (double)(2 * G.n_gauss);
        if (G.sweeps_out) G.sweeps_out[ro] = sweeps;
    }
    if (!settled) {
        for (int i = lane; i < 4 * P1; i += 64) w_row[(size_t)(i / P1) * w_wheel + i % P1] = NAN;
        if (lane == 0 && G.rank_out) G.rank_out[ro] = -1;
        return;
    }
    // the singular values, the cut, the rank
    double sig_max = 0.0;
    for (int k = 0; k < N; ++k) {
        double s = 0.0;
        for (int j = lane; j < c; j += 64) { const double x = A[(size_t)k * jmax + j]; s += x * x; }
        const double v = fgs_wsum(part, lane, nl, s);
        if (lane == 0) s2[k] = v;
        sig_max = fmax(sig_max, sqrt(v));
    }
    __builtin_amdgcn_wave_barrier();
    const double thr = rc * sig_max;
    int rank = 0;
    for (int k = 0; k < N; ++k) rank += sqrt(s2[k]) > thr ? 1 : 0;
    if (lane == 0 && G.rank_out) G.rank_out[ro] = rank;
    // the four right-hand sides: their means, U^T b / S = A_k . b / s2_k
    double mb[4];
    for (int w = 0; w < 4; ++w) {
        double s = 0.0;
        for (int j = lane; j < c; j += 64) s += m_row[w * wstride + j];
        mb[w] = fgs_wsum(part, lane, nl, s) / (double)c;
    }
    for (int k = 0; k < N; ++k) {
        const double* ak = A + (size_t)k * jmax;
        double s[4] = {0.0, 0.0, 0.0, 0.0};
        for (int j = lane; j < c; j += 64) {
            const double x = ak[j];
            for (int w = 0; w < 4; ++w) s[w] += x * (m_row[w * wstride + j] - mb[w]);
        }
        for (int w = 0; w < 4; ++w) part[w * 64 + lane] = s[w];
        __builtin_amdgcn_wave_barrier();
        if (lane < 4) {
            double g = 0.0;
            for (int l = 0; l < nl; ++l) g += part[lane * 64 + l];
            const double v = s2[k];
            Z[lane * N + k] = sqrt(v) > thr ? g / v : 0.0 * g;         // (0 * g: a NaN right-hand side stays NaN)
        }
        __builtin_amdgcn_wave_barrier();
    }
    // x = V z, entry i by lane i, over the columns in rising order; then the intercept
    double x[4] = {0.0, 0.0, 0.0, 0.0};
    if (lane < N) {
        for (int k = 0; k < N; ++k) {
            const double v = V[k * N + lane];
            for (int w = 0; w < 4; ++w) x[w] += v * Z[w * N + k];
        }
        for (int w = 0; w < 4; ++w) {
            w_row[(size_t)w * w_wheel + lane] = x[w];
            part[w * 64 + lane] = cm[lane] * x[w];
        }
    }
    __builtin_amdgcn_wave_barrier();
    if (lane < 4) {
        double d = 0.0;
        for (int i = 0; i < N; ++i) d += part[lane * 64 + i];
        w_row[(size_t)lane * w_wheel + N] = mb[lane] - d;
    }
}

// a thread per (track, row, position): the four wheels' models at q
__global__ void __launch_bounds__(MCQ_NT) mcq_friction_model_kernel(McqFricModel M)
{
    const size_t e = (size_t)blockIdx.x * MCQ_NT + threadIdx.x;
    const size_t rows = (size_t)M.nmax + 1, total = (size_t)M.tracks * rows * M.qmax;
    if (e >= total) return;
    const int j = (int)(e % M.qmax);
    const size_t ro = e / M.qmax;              // t * rows + row
    const size_t t = ro / rows, row = ro % rows;
    double* out = M.mue_out + (t * 4 * rows + row) * M.qmax + j;           // wheel w: + w * rows * qmax
    const size_t ostride = rows * M.qmax;
    const int P = M.model == MCQ_FRIC_LINEAR ? 2 : M.N + 1;
    const double* w = M.w + (t * 4 * rows + row) * P;
    const size_t wstride = rows * P;
    const int qc = M.qcnt ? M.qcnt[ro] : M.qmax;
    if (j >= qc) {
        for (int k = 0; k < 4; ++k) out[k * ostride] = NAN;
        return;
    }
    const double q = M.q[ro * M.qmax + j];
    if (M.model == MCQ_FRIC_LINEAR) {
        for (int k = 0; k < 4; ++k) out[k * ostride] = w[k * wstride] * q + w[k * wstride + 1];
        return;
    }
    const int N = M.N;
    const double cd = M.cd[ro];
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    if (M.centres == MCQ_FRIC_CENTRES_FIT) {
        const int c = M.cnt[ro];
        const bool have = c >= 2 && c <= M.jmax;
        const double n0 = have ? M.n[ro * M.jmax] : NAN, n1 = have ? M.n[ro * M.jmax + c - 1] : NAN;
        const double width = 2.0 * ((cd + n0) - n0);
        for (int k = 0; k < N; ++k) {
            const double arg = (q - fgs_linspace(n0, n1, cd, N, k)) / width;
            const double f = fgs_exp(-0.5 * (arg * arg));
            for (int v = 0; v < 4; ++v) acc[v] += f * w[v * wstride + k];
        }
    } else {
        const double sigma = 2.0 * cd;
        for (int k = 0; k < N; ++k) {
            const double d = q - (double)(k - M.n_gauss) * cd;
            const double f = fgs_exp(-(d * d) / (2.0 * (sigma * sigma)));
            for (int v = 0; v < 4; ++v) acc[v] += f * w[v * wstride + k];
        }
    }
    for (int v = 0; v < 4; ++v) out[v * ostride] = acc[v] + w[v * wstride + N];
}
