// ---- friction map generation (mcq_points_in_path_device, mcq_friction_gen_device; include/mcq.h): the cells of a track's friction map
//      [REF main_gen_frictionmap.py:64-130, frictionmap/src/reftrack_functions.py].  The reference decides a cell with matplotlib's
//      Path.contains_points(points, radius): agg's CONTOUR of the polygon at half the radius (miter joins, limit 4; inner joins reverted, limit
//      1.01; the side follows the polygon's orientation), then a crossing test.  Both are restated here operation by operation.
//      Included from mcq_kernels.hip INSIDE its contraction-off section: the contour's a + r (b - a), dx dx + dy dy, the cross products and
//      numpy.arange's start + i delta change bits under a fused multiply-add, and the comparisons downstream are exact -- one bit is a flipped cell.
//
//      Stages: mcq_fgen_bounds_kernel (a workgroup per track: closed or open, boundaries, the polygons to test, the grid's range and counts),
//      mcq_fgen_contour_kernel (a workgroup per polygon: drop coincident vertices, then a join per kept vertex, placed by a prefix sum),
//      mcq_fgen_mask_kernel (all pairs: every grid point against every contour edge, the contour staged through LDS in tiles that every lane reads
//      at the same address; a thread takes MCQ_FGEN_PPT points that share x), mcq_fgen_scan_kernel and mcq_fgen_scatter_kernel (the stable
//      compaction: counts per block, their running sum per track, the scatter).  mcq_fgen_points_kernel is the crossing test for any points. ----

#define FGEN_EPS 1e-14              /* agg's vertex_dist_epsilon */
#define FGEN_DEN_EPS 1e-30          /* agg's intersection_epsilon */

__device__ __forceinline__ double fgen_dist(double ax, double ay, double bx, double by)
{
    const double dx = bx - ax, dy = by - ay;
    return sqrt(dx * dx + dy * dy);
}

__device__ __forceinline__ double fgen_cross(double ax, double ay, double bx, double by, double qx, double qy)
{
    return (qx - bx) * (by - ay) - (qy - by) * (bx - ax);
}

// numpy.arange's entry i: start, start + step, then start + i * ((start + step) - start)
__device__ __forceinline__ double fgen_coord(double start, double step, int i)
{
    const double nxt = start + step;
    return i == 0 ? start : (i == 1 ? nxt : start + (double)i * (nxt - start));
}

// exclusive prefix sum of one int per thread over the workgroup (MCQ_NT threads, all must call); total = the sum.  s: 2 * MCQ_NT ints of LDS.
__device__ int fgen_scan(int val, int* s, int& total)
{
    const int tid = threadIdx.x;
    int src = 0;
    s[tid] = val;
    __syncthreads();
    for (int off = 1; off < MCQ_NT; off <<= 1) {
        const int t = s[src * MCQ_NT + tid] + (tid >= off ? s[src * MCQ_NT + tid - off] : 0);
        s[(src ^ 1) * MCQ_NT + tid] = t;
        src ^= 1;
        __syncthreads();
    }
    const int incl = s[src * MCQ_NT + tid];
    total = s[src * MCQ_NT + MCQ_NT - 1];
    __syncthreads();        // (the buffers are free again)
    return incl - val;
}

// agg's calc_miter: the points a join contributes (1 or 2), into o[4]
__device__ __forceinline__ int fgen_miter(double* o, double v0x, double v0y, double v1x, double v1y, double v2x, double v2y, double dx1, double dy1,
                                          double dx2, double dy2, bool revert, double mlimit, double dbevel, double wabs, double wsign)
{
    const double lim = wabs * mlimit;
    const double ax = v0x + dx1, ay = v0y - dy1, bx = v1x + dx1, by = v1y - dy1;
    const double cx = v1x + dx2, cy = v1y - dy2, dx = v2x + dx2, dy = v2y - dy2;
    const double num = (ay - cy) * (dx - cx) - (ax - cx) * (dy - cy);
    const double den = (bx - ax) * (dy - cy) - (by - ay) * (dx - cx);
    bool failed = true;
    double di = 1.0, px = v1x, py = v1y;
    if (!(fabs(den) < FGEN_DEN_EPS)) {
        const double r = num / den;
        px = ax + r * (bx - ax);
        py = ay + r * (by - ay);
        di = fgen_dist(v1x, v1y, px, py);
        if (di <= lim) { o[0] = px; o[1] = py; return 1; }
        failed = false;
    } else {
        const double qx = v1x + dx1, qy = v1y - dy1;
        if ((fgen_cross(v0x, v0y, v1x, v1y, qx, qy) < 0.0) == (fgen_cross(v1x, v1y, v2x, v2y, qx, qy) < 0.0)) { o[0] = qx; o[1] = qy; return 1; }
    }
    if (revert) {
        o[0] = v1x + dx1; o[1] = v1y - dy1;
        o[2] = v1x + dx2; o[3] = v1y - dy2;
    } else if (failed) {
        const double ml = mlimit * wsign;
        o[0] = v1x + dx1 + dy1 * ml; o[1] = v1y - dy1 + dx1 * ml;
        o[2] = v1x + dx2 - dy2 * ml; o[3] = v1y - dy2 - dx2 * ml;
    } else {
        const double x1 = v1x + dx1, y1 = v1y - dy1, x2 = v1x + dx2, y2 = v1y - dy2;
        const double t = (lim - dbevel) / (di - dbevel);
        o[0] = x1 + (px - x1) * t; o[1] = y1 + (py - y1) * t;
        o[2] = x2 + (px - x2) * t; o[3] = y2 + (py - y2) * t;
    }
    return 2;
}

// agg's calc_join at the kept vertex v1 between v0 and v2: 1 or 2 contour points
__device__ __forceinline__ int fgen_join(double* o, double v0x, double v0y, double v1x, double v1y, double v2x, double v2y, double w, double wabs,
                                         double wsign)
{
    const double len1 = fgen_dist(v0x, v0y, v1x, v1y), len2 = fgen_dist(v1x, v1y, v2x, v2y);
    const double dx1 = w * (v1y - v0y) / len1, dy1 = w * (v1x - v0x) / len1;
    const double dx2 = w * (v2y - v1y) / len2, dy2 = w * (v2x - v1x) / len2;
    const double cp = (v2x - v1x) * (v1y - v0y) - (v2y - v1y) * (v1x - v0x);
    if ((cp > FGEN_EPS && w > 0.0) || (cp < -FGEN_EPS && w < 0.0)) {       // inner join
        double limit = (len1 < len2 ? len1 : len2) / wabs;
        if (limit < 1.01) limit = 1.01;
        return fgen_miter(o, v0x, v0y, v1x, v1y, v2x, v2y, dx1, dy1, dx2, dy2, true, limit, 0.0, wabs, wsign);
    }
    const double dx = (dx1 + dx2) / 2.0, dy = (dy1 + dy2) / 2.0;
    return fgen_miter(o, v0x, v0y, v1x, v1y, v2x, v2y, dx1, dy1, dx2, dy2, false, 4.0, sqrt(dx * dx + dy * dy), wabs, wsign);
}

// A workgroup per polygon.  cont / ccount: the polygon the crossing test runs on -- the path itself for radius 0, nothing for a path of fewer than
// 3 vertices (matplotlib answers False everywhere) or fewer than 2 kept ones.  A vertex within FGEN_EPS of the previous KEPT one is dropped: where
// no two neighbours are that close every vertex is kept (the usual case); otherwise one thread walks the path.
__global__ void __launch_bounds__(MCQ_NT) mcq_fgen_contour_kernel(McqContour C)
{
    __shared__ int s_scan[2 * MCQ_NT];
    __shared__ int s_bad, s_dup;
    const int tid = threadIdx.x, p = blockIdx.x;
    const size_t vm = (size_t)C.vmax;
    const int v = C.v_list ? C.v_list[p] : C.vmax;
    const double* V = C.verts + (size_t)p * vm * 2;
    double* K = C.kept + (size_t)p * vm * 2;
    int* F = C.flag + (size_t)p * vm;
    double* O = C.cont + (size_t)p * vm * 4;
    const double radius = C.radius[p];
    if (tid == 0) { s_bad = 0; s_dup = 0; }
    __syncthreads();
    const bool range = v >= 0 && v <= C.vmax;
    if (range) {
        bool bad = false;
        for (int i = tid; i < v; i += MCQ_NT) bad = bad || !(finite_d(V[2 * (size_t)i]) && finite_d(V[2 * (size_t)i + 1]));
        if (bad) s_bad = 1;
    }
    __syncthreads();
    const bool nonfinite = range && (s_bad != 0 || !finite_d(radius));
    if (C.status && tid == 0) C.status[p] = !range ? MCQ_FGEN_FEW : (nonfinite ? MCQ_FGEN_NONFINITE : 0);
    if (!range || nonfinite || v < 3) {
        if (tid == 0) C.ccount[p] = 0;
        return;
    }
    if (radius == 0.0) {
        for (size_t i = tid; i < 2 * (size_t)v; i += MCQ_NT) O[i] = V[i];
        if (tid == 0) C.ccount[p] = v;
        return;
    }
    bool dup = false;
    for (int i = tid; i < v; i += MCQ_NT) {
        const bool keep = i == 0 || fgen_dist(V[2 * (size_t)i - 2], V[2 * (size_t)i - 1], V[2 * (size_t)i], V[2 * (size_t)i + 1]) > FGEN_EPS;
        F[i] = keep ? 1 : 0;
        dup = dup || !keep;
    }
    if (dup) s_dup = 1;
    __syncthreads();
    if (s_dup != 0) {
        if (tid == 0) {
            double lx = V[0], ly = V[1];
            for (int i = 1; i < v; ++i) {
                const double x = V[2 * (size_t)i], y = V[2 * (size_t)i + 1];
                const bool keep = fgen_dist(lx, ly, x, y) > FGEN_EPS;
                F[i] = keep ? 1 : 0;
                if (keep) { lx = x; ly = y; }
            }
        }
        __syncthreads();
    }
    int m = 0;
    for (int c0 = 0; c0 < v; c0 += MCQ_NT) {
        const int i = c0 + tid;
        const int f = i < v ? F[i] : 0;
        int total;
        const int at = m + fgen_scan(f, s_scan, total);
        if (f) { K[2 * (size_t)at] = V[2 * (size_t)i]; K[2 * (size_t)at + 1] = V[2 * (size_t)i + 1]; }
        m += total;
    }
    __syncthreads();            // the kept vertices are this workgroup's own stores
    while (m > 1 && !(fgen_dist(K[2 * (size_t)m - 2], K[2 * (size_t)m - 1], K[0], K[1]) > FGEN_EPS)) --m;      // (every thread reads the same values)
    if (m < 2) {
        if (tid == 0) C.ccount[p] = 0;
        return;
    }
    const double w = radius * 0.5;
    const double wabs = w < 0.0 ? -w : w, wsign = w < 0.0 ? -1.0 : 1.0;
    int cc = 0;
    for (int c0 = 0; c0 < m; c0 += MCQ_NT) {
        const int i = c0 + tid;
        double o[4];
        int cnt = 0;
        if (i < m) {
            const size_t a = i == 0 ? (size_t)m - 1 : (size_t)i - 1, b = i == m - 1 ? 0 : (size_t)i + 1;
            cnt = fgen_join(o, K[2 * a], K[2 * a + 1], K[2 * (size_t)i], K[2 * (size_t)i + 1], K[2 * b], K[2 * b + 1], w, wabs, wsign);
        }
        int total;
        const size_t at = (size_t)cc + fgen_scan(cnt, s_scan, total);
        for (int k = 0; k < cnt; ++k) { O[2 * (at + k)] = o[2 * k]; O[2 * (at + k) + 1] = o[2 * k + 1]; }
        cc += total;
    }
    if (tid == 0) C.ccount[p] = cc;
}

// matplotlib's crossing test of P points that share tx against the closed polygon cv[cc]: bit k of the result = point k is inside.  Every thread
// of the workgroup must call (the tiles are staged between barriers); s_v: 2 * (MCQ_FGEN_TILE + 1) doubles of LDS.
template <int P> __device__ __forceinline__ unsigned fgen_parity(const double* cv, int cc, double tx, const double* ty, double* s_v)
{
    unsigned par = 0;
    for (int j0 = 0; j0 < cc; j0 += MCQ_FGEN_TILE) {
        const int cnt = cc - j0 < MCQ_FGEN_TILE ? cc - j0 : MCQ_FGEN_TILE;
        __syncthreads();
        for (int j = threadIdx.x; j <= cnt; j += MCQ_NT) {
            const size_t g = j0 + j < cc ? (size_t)(j0 + j) : 0;        // (the closing edge returns to vertex 0)
            s_v[2 * j] = cv[2 * g];
            s_v[2 * j + 1] = cv[2 * g + 1];
        }
        __syncthreads();
        for (int j = 0; j < cnt; ++j) {
            const double x0 = s_v[2 * j], y0 = s_v[2 * j + 1], x1 = s_v[2 * j + 2], y1 = s_v[2 * j + 3];
            const double ex = x0 - x1, rhs = (x1 - tx) * (y0 - y1);
            #pragma unroll
            for (int k = 0; k < P; ++k) {
                const bool f0 = y0 >= ty[k], f1 = y1 >= ty[k];
                if (f0 != f1 && (((y1 - ty[k]) * ex >= rhs) == f1)) par ^= 1u << k;
            }
        }
    }
    return par;
}

// grid (point blocks, paths)
__global__ void __launch_bounds__(MCQ_NT) mcq_fgen_points_kernel(McqContour C, int count, const double* xy, unsigned char* inside_out)
{
    __shared__ double s_v[2 * (MCQ_FGEN_TILE + 1)];
    const int p = blockIdx.y;
    const size_t q = (size_t)blockIdx.x * MCQ_NT + threadIdx.x;
    const bool has = q < (size_t)count;
    const double tx = has ? xy[2 * q] : 0.0, ty = has ? xy[2 * q + 1] : 0.0;
    const unsigned par = fgen_parity<1>(C.cont + (size_t)p * C.vmax * 4, C.ccount[p], tx, &ty, s_v);
    if (has) inside_out[(size_t)p * count + q] = (par != 0 && finite_d(tx) && finite_d(ty)) ? 1 : 0;
}

// A workgroup per track: calc_trackboundaries, the polygons, the grid.  rec[t] = nx, ny -- zero for a refused track.
__global__ void __launch_bounds__(MCQ_NT) mcq_fgen_bounds_kernel(McqFgen G)
{
    __shared__ double s_red[2 * MCQ_NW];
    __shared__ int s_bad;
    const int tid = threadIdx.x, t = blockIdx.x;
    const size_t nm = (size_t)G.nmax;
    const int n = G.n_list ? G.n_list[t] : G.nmax;
    const double* ref = G.ref + (size_t)t * nm * 4;
    double* P0 = G.poly + (size_t)t * nm * 8;
    double* P1 = P0 + nm * 4;
    double* br = G.bound_r ? G.bound_r + (size_t)t * nm * 2 : nullptr;
    double* bl = G.bound_l ? G.bound_l + (size_t)t * nm * 2 : nullptr;
    int st = (n < 3 || n > G.nmax) ? MCQ_FGEN_FEW : 0;
    if (tid == 0) s_bad = 0;
    __syncthreads();
    double minx = INFINITY, maxx = -INFINITY, miny = INFINITY, maxy = -INFINITY, maxr = -INFINITY, maxl = -INFINITY;
    if (st == 0) {
        bool bad = false;
        for (int i = tid; i < n; i += MCQ_NT) {
            const double x = ref[4 * (size_t)i], y = ref[4 * (size_t)i + 1], wr = ref[4 * (size_t)i + 2], wl = ref[4 * (size_t)i + 3];
            bad = bad || !(finite_d(x) && finite_d(y) && finite_d(wr) && finite_d(wl));
            minx = fmin(minx, x); maxx = fmax(maxx, x); miny = fmin(miny, y); maxy = fmax(maxy, y); maxr = fmax(maxr, wr); maxl = fmax(maxl, wl);
        }
        if (bad) s_bad = 1;
    }
    __syncthreads();
    if (st == 0 && s_bad != 0) st = MCQ_FGEN_NONFINITE;
    __syncthreads();
    if (st != 0) {      // refused on its inputs: the rows it has are NaN
        const int rows = n < 0 ? 0 : (n > G.nmax ? G.nmax : n);
        for (int i = tid; i < 2 * rows; i += MCQ_NT) {
            if (br) br[i] = NAN;
            if (bl) bl[i] = NAN;
        }
        if (tid == 0) { G.prad[2 * t] = 0.0; G.prad[2 * t + 1] = 0.0; }
    }
    bool closed = false;
    const double d = G.cw * 1.1;
    if (st == 0) {
        const double ex = ref[4 * (size_t)(n - 1)] - ref[0], ey = ref[4 * (size_t)(n - 1) + 1] - ref[1];
        closed = sqrt(ex * ex + ey * ey) <= 10.0;
        const bool in_right = closed && (G.inside_right ? G.inside_right[t] != 0 : true);
        bool bad = false;
        for (int i = tid; i < n; i += MCQ_NT) {
            int a, b;
            double h = 2.0;
            if (closed) { a = i == 0 ? n - 1 : i - 1; b = i == n - 1 ? 0 : i + 1; }
            else if (i == 0) { a = 0; b = 1; h = 1.0; }
            else if (i == n - 1) { a = n - 2; b = n - 1; h = 1.0; }
            else { a = i - 1; b = i + 1; }
            const double gx = (ref[4 * (size_t)b] - ref[4 * (size_t)a]) / h, gy = (ref[4 * (size_t)b + 1] - ref[4 * (size_t)a + 1]) / h;
            const double nf = 1.0 / sqrt((gy * gy + gx * gx) + 0.0);
            const double nx = gy * nf, ny = -gx * nf;
            const double x = ref[4 * (size_t)i], y = ref[4 * (size_t)i + 1], wr = ref[4 * (size_t)i + 2], wl = ref[4 * (size_t)i + 3];
            const double rx = x + nx * wr, ry = y + ny * wr, lx = x - nx * wl, ly = y - ny * wl;
            bad = bad || !(finite_d(rx) && finite_d(ry) && finite_d(lx) && finite_d(ly));
            if (br) { br[2 * (size_t)i] = rx; br[2 * (size_t)i + 1] = ry; }
            if (bl) { bl[2 * (size_t)i] = lx; bl[2 * (size_t)i + 1] = ly; }
            if (!closed) {          // one polygon: the left boundary, then the right one backwards
                P0[2 * (size_t)i] = lx; P0[2 * (size_t)i + 1] = ly;
                const size_t j = 2 * (size_t)n - 1 - (size_t)i;
                P0[2 * j] = rx; P0[2 * j + 1] = ry;
            } else {                // P0 the outside boundary, P1 the inside one
                double* R = in_right ? P1 : P0;
                double* L = in_right ? P0 : P1;
                R[2 * (size_t)i] = rx; R[2 * (size_t)i + 1] = ry;
                L[2 * (size_t)i] = lx; L[2 * (size_t)i + 1] = ly;
            }
        }
        if (bad) s_bad = 1;
        if (tid == 0) {
            const double sign = in_right ? -1.0 : 1.0;
            G.prad[2 * t] = closed ? d * sign : -d;
            G.prad[2 * t + 1] = closed ? -(d * sign) : 0.0;
        }
    }
    __syncthreads();
    if (st == 0 && s_bad != 0) st = MCQ_FGEN_NONFINITE;      // a boundary that is not finite (a zero gradient)
    block_reduce2_(minx, 1, maxx, 2, s_red);
    block_reduce2_(miny, 1, maxy, 2, s_red);
    block_reduce2_(maxr, 2, maxl, 2, s_red);
    if (tid != 0) return;
    double g[6] = {NAN, NAN, NAN, NAN, 0.0, 0.0};
    int nx = 0, ny = 0;
    if (st == 0) {
        const double dd = ceil(maxr + maxl + 5.0);
        g[0] = floor(minx - dd); g[1] = ceil(maxx + dd); g[2] = floor(miny - dd); g[3] = ceil(maxy + dd);
        const double kx = ceil(((g[1] + 0.1) - g[0]) / G.cw), ky = ceil(((g[3] + 0.1) - g[2]) / G.cw);
        g[4] = kx > 0.0 ? kx : 0.0;
        g[5] = ky > 0.0 ? ky : 0.0;
        if (!(g[4] * g[5] <= 2147483647.0)) st = MCQ_FGEN_GRID;       // (also a range that is not finite)
        else { nx = (int)g[4]; ny = (int)g[5]; }
    }
    for (int k = 0; k < 6; ++k) G.grid[6 * (size_t)t + k] = g[k];
    G.rec[2 * t] = nx;
    G.rec[2 * t + 1] = ny;
    G.pcount[2 * t] = st != 0 ? 0 : (closed ? n : 2 * n);
    G.pcount[2 * t + 1] = (st == 0 && closed) ? n : 0;
    G.status[t] = st;
}

// the items of a track: nx columns of ceil(ny / MCQ_FGEN_PPT) runs of points; item = ix * runs + run, rising with the point's index ix * ny + iy
__device__ __forceinline__ int fgen_runs(int ny) { return (ny + MCQ_FGEN_PPT - 1) / MCQ_FGEN_PPT; }

// grid (item blocks, tracks): bits[item] = the on-track flags of the item's points, bcount[block] = how many the block has
__global__ void __launch_bounds__(MCQ_NT) mcq_fgen_mask_kernel(McqFgen G)
{
    __shared__ double s_v[2 * (MCQ_FGEN_TILE + 1)];
    __shared__ int s_scan[2 * MCQ_NT];
    const int tid = threadIdx.x, t = blockIdx.y;
    const int nx = G.rec[2 * t], ny = G.rec[2 * t + 1];
    const int runs = fgen_runs(ny);
    const size_t items = (size_t)nx * runs, item = (size_t)blockIdx.x * MCQ_NT + tid;
    if ((size_t)blockIdx.x * MCQ_NT >= items) return;       // (the whole workgroup)
    const bool has = item < items;
    const int ix = has ? (int)(item / runs) : 0, iy0 = has ? (int)(item % runs) * MCQ_FGEN_PPT : 0;
    const double tx = fgen_coord(G.grid[6 * (size_t)t], G.cw, ix);
    double ty[MCQ_FGEN_PPT];
    #pragma unroll
    for (int k = 0; k < MCQ_FGEN_PPT; ++k) ty[k] = fgen_coord(G.grid[6 * (size_t)t + 2], G.cw, iy0 + k);
    const size_t cstride = (size_t)G.nmax * 8;              // doubles per contour: 2 * (2 nmax) vertices
    const double* c0 = G.cont + (size_t)t * 2 * cstride;
    const unsigned in0 = fgen_parity<MCQ_FGEN_PPT>(c0, G.ccount[2 * t], tx, ty, s_v);
    const unsigned in1 = fgen_parity<MCQ_FGEN_PPT>(c0 + cstride, G.ccount[2 * t + 1], tx, ty, s_v);
    unsigned m = has ? (in0 & ~in1) : 0u;
    #pragma unroll
    for (int k = 0; k < MCQ_FGEN_PPT; ++k) if (iy0 + k >= ny) m &= ~(1u << k);
    if (has) G.bits[(size_t)t * G.maxblk * MCQ_NT + item] = (unsigned char)m;
    int total;
    (void)fgen_scan(__builtin_popcount(m), s_scan, total);
    if (tid == 0) G.bcount[(size_t)t * G.maxblk + blockIdx.x] = total;
}

// A workgroup per track: the blocks' counts become their offsets; the track's count, and the overflow bit where cells are written
__global__ void __launch_bounds__(MCQ_NT) mcq_fgen_scan_kernel(McqFgen G)
{
    __shared__ int s_scan[2 * MCQ_NT];
    const int tid = threadIdx.x, t = blockIdx.x;
    const size_t items = (size_t)G.rec[2 * t] * fgen_runs(G.rec[2 * t + 1]);
    const int nblk = (int)((items + MCQ_NT - 1) / MCQ_NT);
    int* bc = G.bcount + (size_t)t * G.maxblk;
    int sum = 0;
    for (int b0 = 0; b0 < nblk; b0 += MCQ_NT) {
        const int b = b0 + tid;
        const int c = b < nblk ? bc[b] : 0;
        int total;
        const int at = sum + fgen_scan(c, s_scan, total);
        if (b < nblk) bc[b] = at;
        sum += total;
    }
    if (tid == 0) {
        G.count[t] = sum;
        if (G.cells && sum > G.cmax) G.status[t] |= MCQ_FGEN_OVERFLOW;
    }
}

// grid (item blocks, tracks): the cells in the order of their points, the first cmax of them
__global__ void __launch_bounds__(MCQ_NT) mcq_fgen_scatter_kernel(McqFgen G)
{
    __shared__ int s_scan[2 * MCQ_NT];
    const int tid = threadIdx.x, t = blockIdx.y;
    const int nx = G.rec[2 * t], ny = G.rec[2 * t + 1];
    const int runs = fgen_runs(ny);
    const size_t items = (size_t)nx * runs, item = (size_t)blockIdx.x * MCQ_NT + tid;
    if ((size_t)blockIdx.x * MCQ_NT >= items) return;       // (the whole workgroup)
    const unsigned m = item < items ? G.bits[(size_t)t * G.maxblk * MCQ_NT + item] : 0u;
    int total;
    int at = G.bcount[(size_t)t * G.maxblk + blockIdx.x] + fgen_scan(__builtin_popcount(m), s_scan, total);
    if (m == 0u) return;
    const int ix = (int)(item / runs), iy0 = (int)(item % runs) * MCQ_FGEN_PPT;
    const double tx = fgen_coord(G.grid[6 * (size_t)t], G.cw, ix);
    double* out = G.cells + (size_t)t * G.cmax * 2;
    for (int k = 0; k < MCQ_FGEN_PPT; ++k) {
        if (!((m >> k) & 1u)) continue;
        if (at < G.cmax) {
            out[2 * (size_t)at] = tx;
            out[2 * (size_t)at + 1] = fgen_coord(G.grid[6 * (size_t)t + 2], G.cw, iy0 + k);
        }
        ++at;
    }
}
