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

__device__ __forceinline__ bool fric_finite(double a) { return fabs(a) < (double)INFINITY; }      // (false for a NaN)

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
    if (!(fric_finite(qx) && fric_finite(qy))) { idx = -1; d2 = NAN; return; }
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
    bool bad = n < 1 || n > G.nmax || !(fric_finite(width) && fric_finite(G.wbf) && fric_finite(G.wbr));
    if (!bad) {
        bool any_bad = false, any_over = false;
        for (int r = tid; r < n; r += MCQ_NT) {
            const double x = ref[4 * r], y = ref[4 * r + 1], wr = ref[4 * r + 2], wl = ref[4 * r + 3], nx = nv[2 * r], ny = nv[2 * r + 1];
            if (!(fric_finite(x) && fric_finite(y) && fric_finite(wr) && fric_finite(wl) && fric_finite(nx) && fric_finite(ny))) any_bad = true;
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
