// mcq_tri.inc -- included by mcq_kernels.hip (saddle-point translation unit only).
// ---------------------------------------------------------------------------------------------------------------------
// E and E' applied WITHOUT their bands:   E = a T^-1 R Nx + b T^-1 R Ny   (a = -2 c y', b = 2 c x', c = |p'|^-3;  T, R the cyclic tridiagonal
// spline matrix and its right-hand-side operator, sections 3 of DESIGN.md), so   E x = a (T^-1 R (nx x)) + b (T^-1 R (ny x))   and
// E' y = nx R' T^-T (a y) + ny R' T^-T (b y):  four solves with a diagonally dominant cyclic tridiagonal matrix instead of two passes over
// 2 x 65 doubles per row (1 MB each at N = 2000).  The solves use the periodic-pivot form of the assembly kernel: the pivots delta_m of the
// LU sweep around the ring are a contraction (ratio ~0.27 per step), so a sweep started TRI_W waypoints upstream with zero has converged
// to the ring's periodic solution when it reaches a thread's own eight waypoints -- every thread runs its own short chain, no reduced
// system, three barriers per solve.      T c = r :   y_m = r_m - y_(m-1) / delta_(m-1),        c_m = (y_m - u_m c_(m+1)) / delta_m
//                                      T' x = q :   y_m = q_m - u_(m-1) y_(m-1) / delta_(m-1), x_m = (y_m - x_(m+1)) / delta_m
// with T[m, m-1] = 1, T[m, m] = d_m = 2 s_(m-1)^2 + 2 s_(m-1), T[m, m+1] = u_m = s_(m-1) s_m^2, delta_m = d_m - u_(m-1) / delta_(m-1)
// (the same pivots for T and T').  1 / delta and u live in two vectors of the workspace (tri_prepare, once per problem) and are staged into
// LDS per call next to the right-hand side; LDS rows are padded by one double per eight (a thread walks consecutive entries).
// Rings up to TRI_MAXN = 8 x 256 waypoints: one thread, eight waypoints, everything in LDS.  Longer rings (round 4; rounds 1-3 kept three
// 66-diagonal bands per problem for them): the same sweeps chunk after chunk on vectors of the workspace (tri_solve_long) -- every
// waypoint of the ring has its y before the first backward sweep starts, which the LDS route gets for free from its single chunk.
// ---------------------------------------------------------------------------------------------------------------------
#define TRI_W 64
#define TRI_LD 2488                                  /* doubles per LDS array: OVL_SIZE / 3 */
#define TRI_MAXN MCQ_TRI_MAXN                        /* rings the LDS route holds: one chunk of eight waypoints per thread */
#define TRI_PAD(m) ((m) + ((m) >> 3))
// The LDS arrays of the sweeps carry a HALO: extended index e = ring index + TRI_H, e in [0, n + 2 TRI_H), the entries below TRI_H and from
// n + TRI_H on being copies of the ring's other end.  A thread's window -- TRI_W + 1 waypoints upstream of its first, 7 + TRI_W downstream --
// then never wraps, and with one pad double per eight its slots are  9 tid + constant : the sweeps' steps are two LDS reads at immediate
// offsets and one multiply-add (they had spent seven instructions per step on the wrap-around and on the padding).
#define TRI_H (TRI_W + 8)
#define TRI_PE(e) ((e) + ((e) >> 3))                  /* slot of extended index e */
#define TRI_X(i) TRI_PE((i) + TRI_H)                  /* slot of ring index i (the copy inside the ring's own range) */
__device__ __forceinline__ int tri_ring(int e, int n)
{
    int i = e - TRI_H;
    if (n >= TRI_H) return i < 0 ? i + n : i >= n ? i - n : i;          // (uniform branch: one wrap at most)
    i %= n;
    return i < 0 ? i + n : i;
}
#ifndef TRI_UNR
#define TRI_UNR 8
#endif
static_assert(TRI_MAXN == 8 * MCQ_NT && TRI_PE(TRI_MAXN + 2 * TRI_H - 1) < TRI_LD && TRI_W % 8 == 0, "padded LDS rows of the tridiagonal solves, halo included");
static_assert(3 * TRI_LD <= OVL_SIZE, "right-hand side, 1 / delta and u of the tridiagonal solves must fit the LDS overlay");


// Open chains (SolveCtx.chain; n <= TRI_MAXN): T loses its corners, row 0 is  2 c_0 + s_0^2 c_1  and row n - 1 is  c_(n-2) + 2 c_(n-1)
// (d = 2, u_(n-1) = 0).  The pivots are then the chain's own, from delta_0 = 2: a thread's pivot sweep starts at waypoint max(0, m0 - TRI_W),
// exactly at the chain's first row where it reaches it.  The solves keep their code: the halo of every LDS array -- right-hand side, 1 / delta
// and u at the extended indices outside [0, n) -- is zero instead of a copy of the ring's other end.  A forward step into waypoint 0 then
// multiplies by 1 / delta_(-1) = 0 (y_0 = r_0, the chain's first step), a backward step into waypoint n - 1 starts from x_n = y_n / delta_n = 0,
// and the warm-up sweeps of the threads further in are the same contraction as on a ring.
// 1 / delta_m and u_m into V_IDL, V_TUC (once per problem)
__device__ void tri_prepare(const LCtx& c)
{
    const int n = c.d.n, tid = threadIdx.x;
    const gdouble* SC = VEC(c.w, c.nm, V_SC);
    gdouble* IDL = VEC(c.w, c.nm, V_IDL);
    gdouble* TUC = VEC(c.w, c.nm, V_TUC);
    __syncthreads();
    if (c.chain) {
        for (int m0 = 8 * tid; m0 < n; m0 += 8 * MCQ_NT) {
            const int mb = m0 >= TRI_W ? m0 - TRI_W : 0;
            double idl = 0.0, uprev = 0.0;
            for (int m = mb; m < m0 + 8 && m < n; ++m) {
                const double sp = m > 0 ? SC[m - 1] : 1.0, sm = SC[m];        // (S[n-2] = 1: u_(n-2) = s_(n-3))
                const double d = (m == 0 || m == n - 1) ? 2.0 : 2.0 * sp * sp + 2.0 * sp;
                const double u = m == n - 1 ? 0.0 : sp * sm * sm;
                const double delta = d - uprev * idl;
                idl = 1.0 / delta;
                uprev = u;
                if (m >= m0) { IDL[m] = idl; TUC[m] = u; }
            }
        }
        __syncthreads();
        return;
    }
    for (int base = 0; base < n; base += 8 * MCQ_NT) {
        const int m0 = base + 8 * tid;
        if (m0 < n) {
            int m = m0 - TRI_W;
            m %= n;
            if (m < 0) m += n;
            int mp = m > 0 ? m - 1 : n - 1;
            double sp = SC[mp];                     // s_(m-1)
            double idl = 0.0, uprev = 0.0;          // 1 / delta_(m-1), u_(m-1): the sweep starts with delta = d
            for (int k = -TRI_W; k < 8; ++k) {
                const double sm = SC[m];
                const double d = 2.0 * sp * sp + 2.0 * sp, u = sp * sm * sm;
                const double delta = d - uprev * idl;
                idl = 1.0 / delta;
                uprev = u;
                if (k >= 0 && m0 + k < n) { IDL[m0 + k] = idl; TUC[m0 + k] = u; }
                sp = sm;
                m = m + 1 < n ? m + 1 : 0;
            }
        }
    }
    __syncthreads();
}

struct TriLds {
    double* ry;
    double* idl;
    double* tu;
};
__device__ __forceinline__ TriLds tri_lds()
{
    TriLds t;
    t.ry = g_sm + SM_OVL;
    t.idl = g_sm + SM_OVL + TRI_LD;
    t.tu = g_sm + SM_OVL + 2 * TRI_LD;
    return t;
}
// Staging is thread-contiguous: a thread loads what its own eight waypoints (8 tid ..) need -- every load issued before the first use, ONE
// memory latency per staged vector (a strided loop over the ring paid one per trip, nine trips per vector) -- and writes each value to the
// ring's own range and to the halo copies it has.
__device__ __forceinline__ void tri_put(double* arr, int n, int i, double v, bool chain)
{
    const int e = i + TRI_H;
    if (chain) {
        arr[TRI_PE(e)] = v;                                  // (open chain: the halo stays zero, tri_stage_factors)
    } else if (n >= TRI_H) {
        arr[TRI_PE(e)] = v;
        if (e >= n) arr[TRI_PE(e - n)] = v;                  // upstream halo: the ring's last TRI_H waypoints
        if (i < TRI_H) arr[TRI_PE(e + n)] = v;               // downstream halo: its first TRI_H
    } else {
        for (int q = e % n; q < n + 2 * TRI_H; q += n) arr[TRI_PE(q)] = v;
    }
}
// ring index of waypoint m0 + k of a thread's window, k in [-1, 8]: one wrap at either end; entries beyond the ring's end + 1 (never used) -> 0
__device__ __forceinline__ int tri_win(int m0, int k, int n)
{
    const int j = m0 + k;
    return j < 0 ? n - 1 : j < n ? j : 0;
}
// 1 / delta and u into LDS (once per call of tri_apply_*); open chain: the halos of all three arrays to zero
__device__ __forceinline__ void tri_stage_factors(const LCtx& c, const TriLds& L)
{
    const int n = c.d.n, m0 = 8 * threadIdx.x;
    const gdouble* IDL = VEC(c.w, c.nm, V_IDL);
    const gdouble* TUC = VEC(c.w, c.nm, V_TUC);
    const bool chain = c.chain != 0;
    if (chain) {
        for (int q = threadIdx.x; q < 2 * TRI_H; q += MCQ_NT) {
            const int e = q < TRI_H ? q : n + q;             // [0, TRI_H) and [n + TRI_H, n + 2 TRI_H)
            L.ry[TRI_PE(e)] = 0.0;
            L.idl[TRI_PE(e)] = 0.0;
            L.tu[TRI_PE(e)] = 0.0;
        }
    }
    if (m0 >= n) return;
    double a[8], b[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) { a[k] = IDL[tri_win(m0, k, n)]; b[k] = TUC[tri_win(m0, k, n)]; }
#pragma unroll
    for (int k = 0; k < 8; ++k)
        if (m0 + k < n) { tri_put(L.idl, n, m0 + k, a[k], chain); tri_put(L.tu, n, m0 + k, b[k], chain); }
}

// Solves  T c = r  (TRANS = false)  or  T' x = q  (TRANS = true)  for the right-hand side in L.ry (all n + 2 TRI_H extended entries written,
// barrier passed); returns this thread's eight entries (waypoints 8 tid ..) in own[]; L.ry holds y afterwards (the ring's own range and the
// halo downstream of it).  Uniform over the block.  n <= TRI_MAXN.
template <bool TRANS>
__device__ __forceinline__ void tri_solve_chunk(const TriLds& L, int n, double (&own)[8], bool chain)
{
    const int tid = threadIdx.x, m0 = 8 * tid;
    const bool valid = m0 < n;
    const int t9 = valid ? 9 * tid : 0;          // slot of extended index 8 tid = waypoint m0 - TRI_H (threads beyond the ring shadow thread 0)
    // ---- forward sweep: warm-up upstream (TRI_W steps from waypoint m0 - TRI_W), then the own entries; eight steps = one padded row
    // (the rows are NOT unrolled: a fully unrolled warm-up takes every VGPR there is, and a __noinline__ function pays for the callee-saved
    //  half of them with scratch traffic in its prologue and epilogue -- or pushes the kernel beyond 256 registers, one workgroup per CU)
    double y = 0.0;
#pragma unroll 1
    for (int a = 1; a <= TRI_W / 8; ++a) {
        const int q = t9 + 9 * a;
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) {
            const int sp = kk == 0 ? q - 2 : q + kk - 1;             // the previous waypoint's slot (a pad slot lies between two rows)
            const double f = TRANS ? L.tu[sp] * L.idl[sp] : L.idl[sp];
            y = fma(-f, y, L.ry[q + kk]);
        }
    }
    const int qo = t9 + 9 * (TRI_W / 8 + 1);      // the own entries' row
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) {
        const int sp = kk == 0 ? qo - 2 : qo + kk - 1;
        const double f = TRANS ? L.tu[sp] * L.idl[sp] : L.idl[sp];
        y = fma(-f, y, L.ry[qo + kk]);
        own[kk] = y;
    }
    __syncthreads();
    if (valid)
        for (int k = 0; k < 8; ++k)
            if (m0 + k < n)
                for (int e = m0 + k + TRI_H; e < (chain ? m0 + k + TRI_H + 1 : n + 2 * TRI_H); e += n) L.ry[TRI_PE(e)] = own[k];      // (the copy downstream of the ring as well; a chain has none)
    __syncthreads();
    // ---- backward sweep: warm-up downstream of the own entries (from waypoint m0 + 7 + TRI_W)
    double x = 0.0;
#pragma unroll 1
    for (int a = TRI_W / 8; a >= 1; --a) {
        const int q = qo + 9 * a;
#pragma unroll
        for (int kk = 7; kk >= 0; --kk) {
            const double yk = L.ry[q + kk];
            x = TRANS ? (yk - x) * L.idl[q + kk] : (yk - L.tu[q + kk] * x) * L.idl[q + kk];
        }
    }
#pragma unroll
    for (int kk = 7; kk >= 0; --kk) {
        const double yk = (valid && m0 + kk < n) ? own[kk] : L.ry[qo + kk];
        x = TRANS ? (yk - x) * L.idl[qo + kk] : (yk - L.tu[qo + kk] * x) * L.idl[qo + kk];
        own[kk] = x;
    }
}

// ---- long rings (n > TRI_MAXN): T c = r / T' x = q on vectors of the workspace.  R: right-hand side, Y: scratch (the forward sweep's y of
//      EVERY waypoint before the first backward sweep), X: solution (may be R).  Uniform over the block; barriers on entry and exit.
template <bool TRANS>
__device__ void tri_solve_long(const LCtx& c, const gdouble* R, gdouble* Y, gdouble* X)
{
    const int n = c.d.n, tid = threadIdx.x;
    const gdouble* IDL = VEC(c.w, c.nm, V_IDL);
    const gdouble* TU = VEC(c.w, c.nm, V_TUC);
    __syncthreads();
    for (int base = 0; base < n; base += 8 * MCQ_NT) {
        const int m0 = base + 8 * tid;
        if (m0 >= n) continue;
        int m = (m0 - TRI_W) % n;
        if (m < 0) m += n;
        int mp = m > 0 ? m - 1 : n - 1;
        double y = 0.0;
#pragma unroll 8
        for (int k = -TRI_W; k < 8; ++k) {
            const double f = TRANS ? TU[mp] * IDL[mp] : IDL[mp];
            y = fma(-f, y, R[m]);
            if (k >= 0 && m0 + k < n) Y[m0 + k] = y;
            mp = m;
            m = m + 1 < n ? m + 1 : 0;
        }
    }
    __syncthreads();
    for (int base = 0; base < n; base += 8 * MCQ_NT) {
        const int m0 = base + 8 * tid;
        if (m0 >= n) continue;
        int mm = (m0 + 7 + TRI_W) % n;
        double x = 0.0;
#pragma unroll 8
        for (int k = 7 + TRI_W; k >= 0; --k) {
            const double yk = Y[mm];
            x = TRANS ? (yk - x) * IDL[mm] : (yk - TU[mm] * x) * IDL[mm];
            if (k < 8 && m0 + k < n) X[m0 + k] = x;
            mm = mm > 0 ? mm - 1 : n - 1;
        }
    }
    __syncthreads();
}

// out = T^-1 rhs  (the assembly kernel's second derivatives: x'' = 2 T^-1 r_x)
__device__ __noinline__ void tri_solve_T(const LCtx& c, const gdouble* rhs, gdouble* out)
{
    const int n = c.d.n, tid = threadIdx.x;
    if (n > TRI_MAXN) { tri_solve_long<false>(c, rhs, K_TS(c, 1), out); return; }
    const TriLds L = tri_lds();
    __syncthreads();
    tri_stage_factors(c, L);
    const int m0 = 8 * tid;
    double own[8];
    if (m0 < n) {
#pragma unroll
        for (int k = 0; k < 8; ++k) own[k] = rhs[tri_win(m0, k, n)];
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (m0 + k < n) tri_put(L.ry, n, m0 + k, own[k], c.chain != 0);
    }
    __syncthreads();
    tri_solve_chunk<false>(L, n, own, c.chain != 0);
    if (m0 < n) {
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (m0 + k < n) out[m0 + k] = own[k];
    }
    __syncthreads();
}

// dst = E src + addc * add        (add may be nullptr);   optionally also  d1 = D (nx src), d2 = D (ny src),  D = 2 T^-1 R  (the second
// derivatives of the spline through the displaced points: what the curvature-error post-check needs).  dst, d1, d2 must not alias src.
__device__ __noinline__ void tri_apply_E_lds(const LCtx& c, const gdouble* src, const gdouble* add, double addc, gdouble* dst,
                                             gdouble* d1, gdouble* d2)
{
    const int n = c.d.n, tid = threadIdx.x;
    const gdouble* SC = VEC(c.w, c.nm, V_SC);
    const gdouble* NX = VEC(c.w, c.nm, V_NX);
    const gdouble* NY = VEC(c.w, c.nm, V_NY);
    const gdouble* XP = VEC(c.w, c.nm, V_XP);
    const gdouble* YP = VEC(c.w, c.nm, V_YP);
    const gdouble* CP = VEC(c.w, c.nm, V_CP);
    const TriLds L = tri_lds();
    const bool chain = c.chain != 0;
    __syncthreads();
    tri_stage_factors(c, L);
    double c1[8], c2[8];
    const int m0 = 8 * tid;
    const bool mine = m0 < n;
    // the window's source values and spline scalings once, for both passes
    double sv[10], sc[8];
    if (mine) {
#pragma unroll
        for (int k = -1; k <= 8; ++k) sv[k + 1] = src[tri_win(m0, k, n)];
#pragma unroll
        for (int k = 0; k < 8; ++k) sc[k] = SC[tri_win(m0, k - 1, n)];            // s_(m-1)
    }
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        const gdouble* NV = pass == 0 ? NX : NY;
        __syncthreads();
        // r_m = 3 q_(m-1) - 3 (s_(m-1) + 1) q_m + 3 s_(m-1) q_(m+1),   q = n . x
        if (mine) {
            double q[10];
#pragma unroll
            for (int k = -1; k <= 8; ++k) q[k + 1] = NV[tri_win(m0, k, n)] * sv[k + 1];
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (m0 + k < n) tri_put(L.ry, n, m0 + k, 3.0 * q[k] - 3.0 * (sc[k] + 1.0) * q[k + 1] + 3.0 * sc[k] * q[k + 2], chain);
            // open chain, the heading rows: 3 (q_1 - q_0) and -3 (q_(n-1) - q_(n-2)) overwrite the ring formula's values (a block of its own
            // after the ring's stores: the ring's arithmetic stays what it was, contractions included)
            if (chain) {
                if (m0 == 0) L.ry[TRI_X(0)] = 3.0 * (q[2] - q[1]);
#pragma unroll
                for (int k = 0; k < 8; ++k)
                    if (m0 + k == n - 1) L.ry[TRI_X(n - 1)] = 3.0 * (q[k] - q[k + 1]);
            }
        }
        __syncthreads();
        if (pass == 0) tri_solve_chunk<false>(L, n, c1, chain);
        else tri_solve_chunk<false>(L, n, c2, chain);
    }
    if (mine) {
        double cp[8], xp[8], yp[8], ad[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int m = tri_win(m0, k, n);
            cp[k] = CP[m]; xp[k] = XP[m]; yp[k] = YP[m];
            ad[k] = add ? add[m] : 0.0;
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int m = m0 + k;
            if (m < n) {
                double v = (-2.0 * cp[k] * yp[k]) * c1[k] + (2.0 * cp[k] * xp[k]) * c2[k];
                if (add) v += addc * ad[k];
                dst[m] = v;
                if (d1) { d1[m] = 2.0 * c1[k]; d2[m] = 2.0 * c2[k]; }
            }
        }
    }
    __syncthreads();
}
__device__ __noinline__ void tri_apply_E_long(const LCtx& c, const gdouble* src, const gdouble* add, double addc, gdouble* dst,
                                              gdouble* d1, gdouble* d2)
{
    const int n = c.d.n, tid = threadIdx.x;
    const gdouble* SC = VEC(c.w, c.nm, V_SC);
    const gdouble* XP = VEC(c.w, c.nm, V_XP);
    const gdouble* YP = VEC(c.w, c.nm, V_YP);
    const gdouble* CP = VEC(c.w, c.nm, V_CP);
    gdouble* R = K_TS(c, 0);
    gdouble* Y = K_TS(c, 1);
    gdouble* C = K_TS(c, 2);
    for (int pass = 0; pass < 2; ++pass) {
        const gdouble* NV = VEC(c.w, c.nm, pass == 0 ? V_NX : V_NY);
        __syncthreads();
        for (int i = tid; i < n; i += MCQ_NT) {
            const int im = i > 0 ? i - 1 : n - 1, ip = i + 1 < n ? i + 1 : 0;
            const double s1 = SC[im];
            R[i] = 3.0 * (NV[im] * src[im]) - 3.0 * (s1 + 1.0) * (NV[i] * src[i]) + 3.0 * s1 * (NV[ip] * src[ip]);
        }
        tri_solve_long<false>(c, R, Y, C);
        for (int i = tid; i < n; i += MCQ_NT) {
            const double cp = CP[i], ci = C[i];
            if (pass == 0) {
                dst[i] = (-2.0 * cp * YP[i]) * ci + (add ? addc * add[i] : 0.0);
                if (d1) d1[i] = 2.0 * ci;
            } else {
                dst[i] += (2.0 * cp * XP[i]) * ci;
                if (d2) d2[i] = 2.0 * ci;
            }
        }
    }
    __syncthreads();
}
__device__ __forceinline__ void tri_apply_E(const LCtx& c, const gdouble* src, const gdouble* add, double addc, gdouble* dst,
                                            gdouble* d1 = nullptr, gdouble* d2 = nullptr)
{
    if (c.d.n <= TRI_MAXN) tri_apply_E_lds(c, src, add, addc, dst, d1, d2);
    else tri_apply_E_long(c, src, add, addc, dst, d1, d2);
}

// dst = E' src   (dst must not alias src)
__device__ __noinline__ void tri_apply_Et_lds(const LCtx& c, const gdouble* src, gdouble* dst)
{
    const int n = c.d.n, tid = threadIdx.x;
    const gdouble* SC = VEC(c.w, c.nm, V_SC);
    const gdouble* NX = VEC(c.w, c.nm, V_NX);
    const gdouble* NY = VEC(c.w, c.nm, V_NY);
    const gdouble* XP = VEC(c.w, c.nm, V_XP);
    const gdouble* YP = VEC(c.w, c.nm, V_YP);
    const gdouble* CP = VEC(c.w, c.nm, V_CP);
    const TriLds L = tri_lds();
    const bool chain = c.chain != 0;
    __syncthreads();
    tri_stage_factors(c, L);
    double acc[8], ce0 = 0.0, cen = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] = 0.0;
    const int m0 = 8 * tid;
    const bool mine = m0 < n;
    // per waypoint of the window: c y' and c x' times the source; the scalings the R' product needs (s_(m-2), s_(m-1))
    double wy[8], wx[8], sc[9];
    if (mine) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int m = tri_win(m0, k, n);
            const double cp = CP[m], sm = src[m];
            wy[k] = (-2.0 * cp * YP[m]) * sm;
            wx[k] = (2.0 * cp * XP[m]) * sm;
        }
        // s_(m0-2) .. s_(m0+6): the first may lie two waypoints before the ring's start
        sc[0] = SC[m0 >= 2 ? m0 - 2 : (m0 - 2 + n) % n];
#pragma unroll
        for (int k = 1; k < 9; ++k) sc[k] = SC[tri_win(m0, k - 2, n)];
    }
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        const gdouble* NV = pass == 0 ? NX : NY;
        __syncthreads();
        if (mine) {
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (m0 + k < n) tri_put(L.ry, n, m0 + k, pass == 0 ? wy[k] : wx[k], chain);
        }
        __syncthreads();
        double u[8];
        tri_solve_chunk<true>(L, n, u, chain);
        __syncthreads();
        double nv[8];
        if (mine) {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                nv[k] = NV[tri_win(m0, k, n)];
                if (m0 + k < n) L.ry[TRI_X(m0 + k)] = u[k];
            }
        }
        __syncthreads();
        // (R'u)_m = R[m-1, m] u_(m-1) + R[m, m] u_m + R[m+1, m] u_(m+1) = 3 s_(m-2) u_(m-1) - 3 (s_(m-1) + 1) u_m + 3 u_(m+1)
        if (mine) {
            const double ub = L.ry[TRI_X(m0 > 0 ? m0 - 1 : n - 1)];                       // the neighbours' entries either side of the own eight
            const int ml = m0 + 7 < n ? m0 + 7 : n - 1;
            const double ua = L.ry[TRI_X(ml + 1 < n ? ml + 1 : 0)];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int m = m0 + k;
                if (m < n) {
                    const double um = k > 0 ? u[k - 1] : ub;
                    const double up = m == ml ? ua : u[k < 7 ? k + 1 : 7];
                    const double rt = 3.0 * sc[k] * um - 3.0 * (sc[k + 1] + 1.0) * u[k] + 3.0 * up;
                    acc[k] += nv[k] * rt;
                }
            }
            // open chain: the columns of R' at the ends, (R'u)_0 = 3 (u_1 - u_0) and (R'u)_(n-1) = 3 s_(n-3) u_(n-2) - 3 u_(n-1) (waypoint 1
            // is the ring formula: s_(-1) = S[n-1] = 1) -- by thread 0 from the u in LDS, accumulated apart and stored over the ring formula's
            // values at the end: the ring's arithmetic and registers stay what they were
            if (chain && tid == 0) {
                ce0 += NV[0] * (3.0 * (L.ry[TRI_X(1)] - L.ry[TRI_X(0)]));
                cen += NV[n - 1] * (3.0 * (SC[n - 3] * L.ry[TRI_X(n - 2)] - L.ry[TRI_X(n - 1)]));
            }
        }
    }
    if (mine) {
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (m0 + k < n) dst[m0 + k] = acc[k];
    }
    __syncthreads();
    if (chain) {                     // open chain: the two end entries (above), over what the owners of waypoints 0 and n - 1 stored
        if (tid == 0) { dst[0] = ce0; dst[n - 1] = cen; }
        __syncthreads();
    }
}
// (Round 4, measured and NOT kept: E then E' as ONE function -- one batch of loads, factors staged once, E x in registers between the
//  halves: 34 us per gradient instead of 40, bench +0.5 %.  Same mathematics, other rounding order -- and the block-pivoting phase of the
//  720-point stadium (270 adjacent active curvature rows: intermediate multipliers of 1e14 whose E' cancels to 1e-1, i.e. to rounding noise)
//  then needs 67 rounds and hits the cap where the two-call order needs 40.  That phase's robustness on such plateaus is the open item, not
//  the gradient; docs/NOTEBOOK.md.)
__device__ __noinline__ void tri_apply_Et_long(const LCtx& c, const gdouble* src, gdouble* dst)
{
    const int n = c.d.n, tid = threadIdx.x;
    const gdouble* SC = VEC(c.w, c.nm, V_SC);
    const gdouble* XP = VEC(c.w, c.nm, V_XP);
    const gdouble* YP = VEC(c.w, c.nm, V_YP);
    const gdouble* CP = VEC(c.w, c.nm, V_CP);
    gdouble* R = K_TS(c, 0);
    gdouble* Y = K_TS(c, 1);
    gdouble* U = K_TS(c, 2);
    for (int pass = 0; pass < 2; ++pass) {
        const gdouble* NV = VEC(c.w, c.nm, pass == 0 ? V_NX : V_NY);
        __syncthreads();
        for (int i = tid; i < n; i += MCQ_NT) {
            const double cp = CP[i];
            R[i] = (pass == 0 ? -2.0 * cp * YP[i] : 2.0 * cp * XP[i]) * src[i];
        }
        tri_solve_long<true>(c, R, Y, U);
        for (int m = tid; m < n; m += MCQ_NT) {
            const int mm = m > 0 ? m - 1 : n - 1, m2 = mm > 0 ? mm - 1 : n - 1, mp = m + 1 < n ? m + 1 : 0;
            const double rt = 3.0 * SC[m2] * U[mm] - 3.0 * (SC[mm] + 1.0) * U[m] + 3.0 * U[mp];
            dst[m] = pass == 0 ? NV[m] * rt : dst[m] + NV[m] * rt;
        }
    }
    __syncthreads();
}
__device__ __forceinline__ void tri_apply_Et(const LCtx& c, const gdouble* src, gdouble* dst)
{
    if (c.d.n <= TRI_MAXN) tri_apply_Et_lds(c, src, dst);
    else tri_apply_Et_long(c, src, dst);
}

// =====================================================================================================================
// Shortest-path objective (SURVEY.md section 8 row f-4; tph.opt_shortest_path [REF main_globaltraj.py:286-290]): H itself is a symmetric
// cyclic TRIDIAGONAL matrix, given entry by entry (V_SPD: H[i, i], V_SPU: H[i, i + 1 mod n]).  The systems of the interior point / active
// set,  (H + diag(sig)) x = r  with pinned rows and columns replaced by identity, are scalar tridiagonal: no saddle-point form, no stored
// factor.  (Rounds 1-3 ran them through a 129-wide bordered-band Cholesky on the matrix cores -- a second 2000-line solver core for 3 N
// numbers.)  A "factorisation" keeps two pointers and one vector; every solve redoes the elimination:
//   * ring -> chain by Sherman-Morrison:  T = T' + u v',  u = (g, 0 .. 0, c0)',  v = (1, 0 .. 0, c0 / g)',  g = -T[0, 0],  c0 = T[n-1, 0]:
//     T' is T without its corners, T'[0, 0] = 2 T[0, 0], T'[n-1, n-1] = T[n-1, n-1] + c0^2 / T[0, 0] -- T plus a positive semidefinite rank-one
//     term, so still positive definite;   x = y - z (v'y) / (1 + v'z),  T'y = r,  T'z = u  (z: once per factorisation, V_SPZ);
//   * the chain in three phases: every thread owns m = ceil(n / 256) consecutive rows, the last one its SEPARATOR; two sweeps over its
//     interior rows (top-down, bottom-up) give its first and last interior unknown as affine functions of the two separators around it,
//     which turns the separators' rows into a tridiagonal system of <= 256 unknowns; that one by parallel cyclic reduction in LDS
//     (8 levels); the interior rows by a Thomas sweep with both neighbours known.  All pivots are pivots of a positive definite matrix:
//     no pivoting; a non-positive or non-finite one is MCQ_NOT_PD (an iterate ON a bound: sig = inf).
// Coefficients and right-hand side are staged into the LDS arrays of the sweeps above (rings up to TRI_MAXN) or into three scratch
// vectors of the workspace (longer rings: same code, global pointers).
// =====================================================================================================================
#define V_SPD V_XP      /* diagonal of H */
#define V_SPU V_YP      /* H[i, i + 1 mod n] */
#define V_SPZ V_IDL     /* z = T'^-1 u of the current factorisation */
#define V_SPA V_XPP     /* scratch of the long-ring route: diagonal, off-diagonal, right-hand side */
#define V_SPB V_YPP
#define V_SPC V_TUC
#define SP_PA 0              /* PCR rows of the separators: a, b, c, d */
#define SP_PP (4 * MCQ_NT)   /* first interior unknown of a block = pp - pq x_left - pw x_right */
static_assert(7 * MCQ_NT <= SPK, "separator system of the scalar tridiagonal solves must fit the persistent LDS region");

template <typename P, bool PAD>
__device__ __forceinline__ bool sp_chain_solve(P d, P o, P r, int n)
{
#define SPX(i) (PAD ? TRI_PAD(i) : (i))
    const int tid = threadIdx.x;
    const int m = (n + MCQ_NT - 1) / MCQ_NT, nb = (n + m - 1) / m;
    double* pa = g_sm + SM_S + SP_PA;
    double* pb = pa + MCQ_NT;
    double* pc = pb + MCQ_NT;
    double* pd = pc + MCQ_NT;
    double* pp = g_sm + SM_S + SP_PP;
    double* pq = pp + MCQ_NT;
    double* pw = pq + MCQ_NT;
    const bool has = tid < nb;
    const int s = tid * m;
    const int e = has ? ((s + m < n ? s + m : n) - 1) : 0;        // separator row; interior rows s .. e - 1
    const int mi = has ? e - s : 0;
    bool bad = false;
    // ---- phase A: first / last interior unknown as functions of the two separators -------------------------------------------------
    double p = 0.0, q = 0.0, w = 0.0, p1 = 0.0, q1 = 0.0, w1 = 0.0;
    if (mi > 0) {
        const double cl = tid > 0 ? o[SPX(s - 1)] : 0.0;
        double u = d[SPX(s)], rr = r[SPX(s)], ff = cl;
        for (int k = s + 1; k < e; ++k) {
            const double ok = o[SPX(k - 1)];
            bad |= !(u > 0.0);
            const double mlt = ok * kkt_rcp(u);
            u = fma(-mlt, ok, d[SPX(k)]);
            rr = fma(-mlt, rr, r[SPX(k)]);
            ff = -mlt * ff;
        }
        bad |= !(u > 0.0);
        double iu = kkt_rcp(u);
        p = rr * iu; q = ff * iu; w = o[SPX(e - 1)] * iu;
        double u2 = d[SPX(e - 1)], r2 = r[SPX(e - 1)], gg = o[SPX(e - 1)];
        for (int k = e - 2; k >= s; --k) {
            const double ok = o[SPX(k)];
            bad |= !(u2 > 0.0);
            const double mlt = ok * kkt_rcp(u2);
            u2 = fma(-mlt, ok, d[SPX(k)]);
            r2 = fma(-mlt, r2, r[SPX(k)]);
            gg = -mlt * gg;
        }
        bad |= !(u2 > 0.0);
        iu = kkt_rcp(u2);
        p1 = r2 * iu; q1 = cl * iu; w1 = gg * iu;
    }
    pp[tid] = p1; pq[tid] = q1; pw[tid] = w1;
    __syncthreads();
    // ---- the separators' rows ------------------------------------------------------------------------------------------------
    double ra = 0.0, rb = 1.0, rc = 0.0, rd = 0.0;
    if (has) {
        const double ae = e > 0 ? o[SPX(e - 1)] : 0.0;
        const double ce = e < n - 1 ? o[SPX(e)] : 0.0;
        const int tn = tid + 1;
        const int min_ = tn < nb ? ((tn * m + m < n ? tn * m + m : n) - 1 - tn * m) : 0;      // interior rows of the next block
        rb = d[SPX(e)];
        rd = r[SPX(e)];
        if (mi > 0) { ra = -ae * q; rb = fma(-ae, w, rb); rd = fma(-ae, p, rd); }
        else ra = ae;
        if (min_ > 0) { rc = -ce * pw[tn]; rb = fma(-ce, pq[tn], rb); rd = fma(-ce, pp[tn], rd); }
        else rc = ce;
    }
    pa[tid] = ra; pb[tid] = rb; pc[tid] = rc; pd[tid] = rd;
    __syncthreads();
    // ---- phase B: parallel cyclic reduction of the separators' chain (rows beyond nb are identity rows) ------------------------------
    for (int st = 1; st < nb; st <<= 1) {
        const int il = tid - st, ir = tid + st;
        double al = 0.0, bl = 1.0, cl_ = 0.0, dl = 0.0, ar = 0.0, br = 1.0, cr = 0.0, dr = 0.0;
        if (il >= 0) { al = pa[il]; bl = pb[il]; cl_ = pc[il]; dl = pd[il]; }
        if (ir < MCQ_NT) { ar = pa[ir]; br = pb[ir]; cr = pc[ir]; dr = pd[ir]; }
        const double k1 = ra * kkt_rcp(bl), k2 = rc * kkt_rcp(br);
        const double na = -al * k1, nc = -cr * k2;
        const double nbv = rb - cl_ * k1 - ar * k2, nd = rd - dl * k1 - dr * k2;
        __syncthreads();
        ra = na; rb = nbv; rc = nc; rd = nd;
        pa[tid] = ra; pb[tid] = rb; pc[tid] = rc; pd[tid] = rd;
        __syncthreads();
    }
    bad |= has && !(rb > 0.0);
    const double xs = rd * kkt_rcp(rb);
    __syncthreads();
    pd[tid] = xs;
    __syncthreads();
    // ---- phase C: interior rows with both separators known (in place: d <- pivots, r <- solution) --------------------------------
    if (mi > 0) {
        const double xl = tid > 0 ? pd[tid - 1] : 0.0;
        double u = d[SPX(s)];
        double rr = r[SPX(s)] - (tid > 0 ? o[SPX(s - 1)] * xl : 0.0) - (mi == 1 ? o[SPX(e - 1)] * xs : 0.0);
        r[SPX(s)] = rr;
        for (int k = s + 1; k < e; ++k) {
            const double ok = o[SPX(k - 1)];
            const double mlt = ok * kkt_rcp(u);
            u = fma(-mlt, ok, d[SPX(k)]);
            rr = fma(-mlt, rr, r[SPX(k)] - (k == e - 1 ? o[SPX(e - 1)] * xs : 0.0));
            d[SPX(k)] = u;
            r[SPX(k)] = rr;
        }
        double x = rr * kkt_rcp(u);
        r[SPX(e - 1)] = x;
        for (int k = e - 2; k >= s; --k) {
            x = (r[SPX(k)] - o[SPX(k)] * x) * kkt_rcp(d[SPX(k)]);
            r[SPX(k)] = x;
        }
    }
    if (has) r[SPX(e)] = xs;
    __syncthreads();
    return bad;
#undef SPX
}

// dst = (H + diag(sig))^-1 rhs  with the working set of the last factor_sp() pinned;  rhs == nullptr: the Sherman-Morrison vector z
// (factor_sp).  Returns true if a pivot was not positive (uniform over the block).
__device__ __noinline__ bool sp_solve(const LCtx& c, const gdouble* rhs, gdouble* dst)
{
    const int n = c.d.n, tid = threadIdx.x;
    const gdouble* HD = VEC(c.w, c.nm, V_SPD);
    const gdouble* HU = VEC(c.w, c.nm, V_SPU);
    const gdouble* sig = c.sp_sig;
    const gschar* mk = c.sp_mk;
    const bool lds = n <= TRI_MAXN;
    const TriLds L = tri_lds();
    gdouble* GA = VEC(c.w, c.nm, V_SPA);
    gdouble* GB = VEC(c.w, c.nm, V_SPB);
    gdouble* GC = VEC(c.w, c.nm, V_SPC);
    // corner data (uniform): d0 = T[0, 0], c0 = T[n-1, 0]
    const bool f0 = !(mk && mk[0] != 0), fl = !(mk && mk[n - 1] != 0);
    const double d0 = f0 ? HD[0] + (sig ? sig[0] : 0.0) : 1.0;
    const double c0 = (f0 && fl) ? HU[n - 1] : 0.0;
    const double gam = -d0, c0g = c0 / gam;
    __syncthreads();
    for (int i = tid; i < n; i += MCQ_NT) {
        const int ip = i + 1 < n ? i + 1 : 0;
        const bool fi = !(mk && mk[i] != 0), fp = !(mk && mk[ip] != 0);
        double dv = fi ? HD[i] + (sig ? sig[i] : 0.0) : 1.0;
        if (i == 0) dv = 2.0 * d0;
        if (i == n - 1) dv -= c0 * c0g;
        const double ov = (fi && fp && i < n - 1) ? HU[i] : 0.0;
        const double rv = rhs ? rhs[i] : (i == 0 ? gam : (i == n - 1 ? c0 : 0.0));
        if (lds) { L.idl[TRI_PAD(i)] = dv; L.tu[TRI_PAD(i)] = ov; L.ry[TRI_PAD(i)] = rv; }
        else { GA[i] = dv; GB[i] = ov; GC[i] = rv; }
    }
    __syncthreads();
    bool bad;
    if (lds) bad = sp_chain_solve<double*, true>(L.idl, L.tu, L.ry, n);
    else bad = sp_chain_solve<gdouble*, false>(GA, GB, GC, n);
    double* flag = g_sm + SM_RED + 32;
    if (tid == 0) *flag = 0.0;
    __syncthreads();
    if (bad) *flag = 1.0;
    __syncthreads();
    const bool any_bad = *flag != 0.0;
    if (!rhs) {
        for (int i = tid; i < n; i += MCQ_NT) dst[i] = lds ? L.ry[TRI_PAD(i)] : GC[i];
    } else {
        const gdouble* Z = VEC(c.w, c.nm, V_SPZ);
        const double y0 = lds ? L.ry[TRI_PAD(0)] : GC[0], yl = lds ? L.ry[TRI_PAD(n - 1)] : GC[n - 1];
        const double fac = (y0 + c0g * yl) / (1.0 + Z[0] + c0g * Z[n - 1]);
        for (int i = tid; i < n; i += MCQ_NT) dst[i] = (lds ? L.ry[TRI_PAD(i)] : GC[i]) - fac * Z[i];
    }
    __syncthreads();
    return any_bad;
}

__device__ __noinline__ int factor_sp(const LCtx& c, const gdouble* sig, const gschar* mk)
{
    c.sp_sig = sig;
    c.sp_mk = mk;
    const bool bad = sp_solve(c, nullptr, VEC(c.w, c.nm, V_SPZ));
    // (1 + v'z = 0 cannot happen for a positive definite T; a non-finite z can: sig = inf)
    const gdouble* Z = VEC(c.w, c.nm, V_SPZ);
    const bool fin = isfinite(Z[0]) && isfinite(Z[c.d.n - 1]);
    return (bad || !fin) ? MCQ_NOT_PD : 0;
}
