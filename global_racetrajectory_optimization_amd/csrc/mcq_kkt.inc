// mcq_kkt.inc -- included by mcq_kernels.hip (after the helpers and the LDS map, before the interior point).
// ---------------------------------------------------------------------------------------------------------------------
// The reduced system of the interior point / active set,   (E' diag(w) E + diag(sig)) dx = r   with pinned rows replaced by identity,
// solved WITHOUT the band of H = E'E: through the sparse saddle-point system it is the Schur complement of.  With the spline second
// derivatives as unknowns,
//     kappa_m = k_ref_m + a_m cx_m + b_m cy_m,     T cx = R (px + Nx alpha),   T cy = R (py + Ny alpha)      (T, R cyclic tridiagonal),
// the stationarity conditions in z_m = (alpha_m, cx_m, cy_m, lx_m, ly_m) form a cyclic BLOCK-tridiagonal system with 5 x 5 blocks
//     Lo_m z_(m-1) + Dg_m z_m + Up_m z_(m+1) = (r_m, 0, 0, 0, 0),        Up_m = Lo_(m+1)',
//     Dg = [ d00  .   .  d03 d04 ]   Lo = [  .   .  .  lo0 lo1 ]     d00 = sig_m (1 if pinned),  d03 = 3 (s_(m-1) + 1) nx_m,  d04 = .. ny_m
//          [  .  d11 d12  td  .  ]        [  .   .  .  lo2  .  ]     d11 = w a a, d12 = w a b, d22 = w b b,   td = 2 s_(m-1)^2 + 2 s_(m-1)
//          [  .  d12 d22  .   td ]        [  .   .  .   .  lo2 ]     lo0 = -3 s_(m-2) nx_m,  lo1 = .. ny_m,  lo2 = s_(m-2) s_(m-1)^2
//          [ d03  td  .   .   .  ]        [ lo3  1  .   .   .  ]     lo3 = -3 nx_(m-1),  lo4 = -3 ny_(m-1)
//          [ d04  .   td  .   .  ]        [ lo4  .  1   .   .  ]     (entries that carry n_k vanish when alpha_k is pinned)
// -- 2 000 blocks of 25 numbers where the band of H has 2 000 rows of 65 + a 64-wide border, and the conditioning of E instead of E'E.
// (scripts/proto_kkt.py is the numpy model of exactly this algorithm: backward error 1e-16 .. 5e-15 at cond(M) = 1e15.)
//
// Elimination.  The ring is cut at nseg <= 16 SEPARATOR waypoints; the segments between them are independent block-tridiagonal chains,
// one per 16-lane group of the workgroup (4 waves x 4 DPP rows).  A group holds the 5 x 16 working matrix of a step one column per lane:
//     [ D~_k | Up_k | left spike | - ]   with  D~_k = Dg_k - Lo_k G_(k-1),   spike_k = -Lo_k Y_(k-1)  (Lo_0 itself at the first point),
// and reduces it by an in-place Gauss-Jordan elimination with a STATIC pivot order inside the block (kkt_gj: no search, no swaps; every row
// takes  - (its raw pivot-column entry, broadcast) x (the lane's scaled pivot-row entry)  as one v_fmac_f64_dpp): columns 0..4 become
// D~^-1 (symmetric: its packed lower triangle is stored, un-permuted, so the solves apply it as a plain 5 x 5 product), 5..9 become
// G_k = D~^-1 Up_k (registers only), 10..14 the forward-eliminated coupling to the left separator.  The records of two steps leave
// through an LDS slice of the group as contiguous 16-byte items.
// A backward pass turns the latter and the coupling to the right separator into the spikes X^L, X^R (only their alpha rows are kept,
// plus the full blocks at both ends of the segment); the separators' own block-cyclic system (nseg x nseg blocks) is eliminated the same
// way by one wave with both spikes pointing at separator 0; its step records keep D_k^-1, G_k, M_k = D_k^-1 RL_k and the spike to 0.
// A solve is: forward chain y_k = D~^-1 (r_k e_0 - Lo_k y_(k-1)), backward chain x_k = y_k - G_k x_(k+1), the separators' system,
// alpha_m -= X^L_m xs_j + X^R_m xs_(j+1).   Chains read their blocks from LDS chunks staged by the group's own lanes one chunk ahead; the
// correction, issued after the barrier that follows the separators' system, has the loads of four (float records: eight) of a lane's
// waypoints in flight at once -- two round trips to memory per segment of 124 waypoints (one for float records).
// ---------------------------------------------------------------------------------------------------------------------
#ifndef MCQ_KKT
#define MCQ_KKT 1
#endif
// MCQ_KKT_CORR_BATCH (default 1): the correction at the end of solve_kkt<> loads the spike rows and the alpha of several of a lane's
// waypoints before it uses the first (0: the earlier form, one waypoint per trip -- same results bit for bit, tests/test_emu_entry_batch.py).
// Trips per batch: what keeps solve_kkt<> free of scratch memory (fp64 records: eight trips need 248 VGPRs and spill, four do not).
#ifndef MCQ_KKT_CORR_BATCH
#define MCQ_KKT_CORR_BATCH 1
#endif
#define KKT_CORR_TRIPS_F64 4
#define KKT_CORR_TRIPS_F32 8
#define KKT_FN __device__ __noinline__
#ifndef KKT_TIMERS
#define KKT_TIMERS 0     /* scripts/kkt_check.hip: wall-clock ticks of the phases of factor_kkt / solve_kkt summed into SolveCtx.tk[0..7] */
#endif
#define KT(k) do { if (KKT_TIMERS) { const long long t_ = (long long)wall_clock64(); if (threadIdx.x == 0) c.tk[(k)] += t_ - kt_last; kt_last = t_; } } while (0)
#define KRS 32                     /* record stride (doubles) of the per-point arrays */
#define KCK 8                      /* points per staged chunk of the solve chains */
#define KCKF 16                    /* coefficient records of the elimination per chunk: one per lane of the group, so a 128-byte line of a coefficient
                                      vector (sixteen waypoints) is touched by ONE load phase -- touched again a chunk later it has left the L2 */
#define KCK2 6                     /* points per staged chunk of the spike pass (two arrays) */
#define KCOEF 20                   /* d00 d03 d04 d11 d12 d22 td lo[5] up[5] r 0 1 */
// global scratch inside McqWork.L (nm x MCQ_LLD doubles per problem)
#define KAD 20                     /* record of D~^-1: it is SYMMETRIC (D~_k = Dg_k - Lo_k D~_(k-1)^-1 Lo_k'), 15 packed lower-triangle entries + Lo's five */
#define KTRI(r, c) ((r) >= (c) ? (r) * ((r) + 1) / 2 + (c) : (c) * ((c) + 1) / 2 + (r))
#define K_AD(c) ((c).w.L)                                   /* [n][20]: D~^-1 packed (15), lo[5] at 15..19.  G_k = D~_k^-1 Up_k is NOT stored: Up_k is Lo_(k+1)' */
#define KAY 26                     /* record of the forward-eliminated left spike, columns 1..4 (20: column 0 is lo3 col1 + lo4 col2 with the segment's
                                      first Lo -- Lo's first column is a combination of its second and third) | y of the fused right-hand side (5) | pad */
#define K_OFF(c) ((c).nm >= 64 ? 64 : 0)                    /* (short rings: the records must stay inside nm x MCQ_LLD doubles) */
#define K_AY(c) ((c).w.L + (size_t)20 * (c).nm + K_OFF(c))        /* [n][26] */
#define KAS 8                      /* record of the spikes' alpha rows: columns 1..4 of X^L, columns 1..4 of X^R.  Both spikes have rank 4: column 0
                                      of X^L is lo3 col1 + lo4 col2 with the segment's first Lo (as for the forward-eliminated spike above), column 0
                                      of X^R is (lo0 col1 + lo1 col2) / lo2 with the right separator's Lo (Up = Lo': its first column is a combination
                                      of the second and third) -- the correction of a solve folds both into the separators' values it multiplies by */
#define K_AS(c) ((c).w.L + (size_t)50 * (c).nm + K_OFF(c))        /* [n][8] */
#define K_YV(c) ((c).w.L + (size_t)60 * (c).nm + K_OFF(c))        /* [n][5]: y of a solve's forward chain */
#define K_TS(c, j) ((c).w.L + (size_t)(66 + (j)) * (c).nm + 64)   /* [n] x 3: scratch vectors of the long-ring tridiagonal route (mcq_tri.inc; n > 2048) */
static_assert(MCQ_LLD >= 72, "the factor arrays of the saddle-point form (65 doubles per waypoint + 64) and three scratch vectors must fit McqWork.L");
// LDS, persistent part (SM_S .. SM_S + SPK): what a solve needs of the separators' system
#define KP_SEP 0                   /* [16][10]: lo, up of separator j */
#define KP_R0I 160                 /* inverse of separator 0's final block */
#define KP_RU0 185
#define KP_RL0 210
#define KP_STEP 240                /* [15][100]: D^-1, G, RL, XL + XR of the separator chain */
#define KP_X0 (KP_STEP + 15 * 100) /* [16][10]: X0 = A_int^-1 r at the first / last interior point of every segment */
static_assert(KP_X0 + 160 <= SPK, "separator chain must fit the persistent LDS region");
// LDS, scratch part (overlay)
#define KO_CH 0                    /* chunk buffers [16][KCK][KRS] (solves); the coefficient records [16][KCKF][KCOEF] of the elimination (into KO_AUX's footprint, idle then) */
#define KO_CH2 (16 * (KCK2 * KAD + 32)) /* second array of the spike pass (behind the first; reaches into KO_AUX's footprint, idle then) */
#define KO_AUX (16 * KCK * KRS)    /* right-hand sides / y of a chunk [16][KCK * 8] (solves);  [16][3][25]: RD, RL, RU (factorisation) */
#define KO_RB KO_AUX
#define KO_SPK (KO_AUX + 1280)     /* [16][4][25]: XL, XR at the first and the last interior point */
#define KO_RR (KO_SPK + 16 * 100)  /* [16][5] right-hand sides of the separators, then their solution */
#define KO_YR (KO_RR + 80)         /* [16][5] forward chain of the separators */
#define KO_SREC (KO_YR + 80)       /* [16][KCOEF] coefficient records of the separators */
#define KO_FLAG (KO_SREC + 16 * KCOEF)
#define KO_TOTAL (KO_FLAG + 8)
// Per-group strides of the chunk buffers (doubles).  A wave holds four consecutive groups, and its LDS reads are broadcasts within a group
// (or a handful of neighbouring doubles): the four groups must not sit a multiple of 32 doubles (64 banks x 4 bytes) apart, or every such
// read is a four-way bank conflict (round 3: strides 320 / 256 / 128 / 64 -- SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE = 0.30).  A stride of
// 8 modulo 32 doubles puts them 16 banks apart: KS_STRIDE pads the payload up to the next such number.
#define KS_STRIDE(payload) ((payload) + (8 + 32 - (payload) % 32) % 32)
#define KS_COEF KS_STRIDE(KCKF * KCOEF)    /* coefficient records of the elimination */
#define KS_CH KS_STRIDE(KCK * KAD)         /* D~^-1 | Lo records of a solve's chunk */
#define KS_AUX KS_STRIDE(KCK * 8)          /* right-hand sides / y of a solve's chunk */
#define KS_CH2G KS_STRIDE(KCK2 * KAD)      /* spike pass: D~^-1 | Lo */
#define KS_CH2Y KS_STRIDE(KCK2 * 28)       /* spike pass: forward-eliminated spike | y (28: the float record's stride) */
static_assert(KS_COEF % 32 == 8 && KS_CH % 32 == 8 && KS_AUX % 32 == 8 && KS_CH2G % 32 == 8 && KS_CH2Y % 32 == 8, "group strides: 16 banks apart");
#define KS_STG KS_STRIDE(2 * (KAD + KAY))      /* elimination: the records of two steps on their way out (in KO_SPK .. KO_SREC, idle until the backward pass) */
static_assert(16 * KS_STG <= KO_SREC - KO_SPK && KS_STG % 2 == 0, "staged records of the elimination fit the idle spike / separator regions, 16-byte aligned");
static_assert(16 * KS_AUX <= 1280 && 16 * 75 <= 1280 && 16 * KS_COEF <= 16 * KCK * KRS + 1280 && 16 * KS_CH <= 16 * KCK * KRS
              && 16 * KS_CH2G <= KO_CH2 && KO_CH2 + 16 * KS_CH2Y <= KO_SPK, "overlay regions of the saddle-point elimination");
static_assert(KO_TOTAL <= OVL_SIZE, "scratch of the saddle-point elimination must fit the LDS overlay");

__device__ __forceinline__ double dpp_shl1(double v) { return __builtin_amdgcn_update_dpp(0.0, v, 0x101, 0xf, 0xf, true); }
__device__ __forceinline__ double dpp_shl2(double v) { return __builtin_amdgcn_update_dpp(0.0, v, 0x102, 0xf, 0xf, true); }
__device__ __forceinline__ double dpp_shl5(double v) { return __builtin_amdgcn_update_dpp(0.0, v, 0x105, 0xf, 0xf, true); }
// lanes 0..7 of every row take lane + 5, lanes 8..15 keep their own value (bank mask 0x3): the source of  Lo x  in one move
__device__ __forceinline__ double dpp_shl5_low8(double v) { return __builtin_amdgcn_update_dpp(v, v, 0x105, 0xf, 0x3, false); }
// Which entry of a step's coefficient record is row r of this lane's column of [ Dg | Up | Lo (first step only) | r e_0 ] (18: the zero slot)
__device__ __forceinline__ int kkt_base_index(int c, int r, bool first)
{
    if (r == 0) return c == 0 ? 0 : c == 3 ? 1 : c == 4 ? 2 : c == 8 ? 15 : c == 9 ? 16 : c == 15 ? 17 : (first && c == 13) ? 7 : (first && c == 14) ? 8 : 18;
    if (r == 1) return c == 1 ? 3 : c == 2 ? 4 : c == 3 ? 6 : c == 8 ? 19 : (first && c == 13) ? 9 : 18;
    if (r == 2) return c == 1 ? 4 : c == 2 ? 5 : c == 4 ? 6 : c == 9 ? 19 : (first && c == 14) ? 9 : 18;
    if (r == 3) return c == 0 ? 1 : c == 1 ? 6 : c == 5 ? 12 : c == 6 ? 14 : (first && c == 10) ? 10 : (first && c == 11) ? 19 : 18;
    return c == 0 ? 2 : c == 2 ? 6 : c == 5 ? 13 : c == 7 ? 14 : (first && c == 10) ? 11 : (first && c == 12) ? 19 : 18;
}
__device__ __forceinline__ double kkt_rcp(double x)
{
    double r = __builtin_amdgcn_rcp(x);
    r = fma(fma(-x, r, 1.0), r, r);
    r = fma(fma(-x, r, 1.0), r, r);
    return r;
}

struct KktGeom {
    int nseg, Lmax;
};
__device__ __forceinline__ KktGeom kkt_geom(int n)
{
    KktGeom g;
    g.nseg = (n / 16 >= 3) ? (n / 16 < 16 ? n / 16 : 16) : 1;
    g.Lmax = (n + g.nseg - 1) / g.nseg - 1;
    return g;
}
#define KSEP(j, n, nseg) (((j) * (n)) / (nseg))

// coefficient record of waypoint m (see the header): into rec[0 .. KCOEF) -- in two halves, so that the elimination can have the loads of
// its next sixteen records in flight while it works through the current sixteen
struct KktRaw {
    double s2, s1, s0, nx0, ny0, nxm, nym, nxp, nyp, xp, yp, cp, w, sg, fv;
    int k0, km, kp;         // mask bytes of m, m - 1, m + 1
};
__device__ __forceinline__ void kkt_point_load(const LCtx& c, const gdouble* sig, const gschar* mk, const gdouble* wgt, const gdouble* fv, int m, KktRaw& r)
{
    const int n = c.d.n;
    const int m1 = m > 0 ? m - 1 : n - 1, m2 = m1 > 0 ? m1 - 1 : n - 1, p1 = m + 1 < n ? m + 1 : 0;
    const gdouble* SC = VEC(c.w, c.nm, V_SC);
    const gdouble* NX = VEC(c.w, c.nm, V_NX);
    const gdouble* NY = VEC(c.w, c.nm, V_NY);
    r.s2 = SC[m2]; r.s1 = SC[m1]; r.s0 = SC[m];
    r.nx0 = NX[m]; r.ny0 = NY[m]; r.nxm = NX[m1]; r.nym = NY[m1]; r.nxp = NX[p1]; r.nyp = NY[p1];
    r.xp = VEC(c.w, c.nm, V_XP)[m]; r.yp = VEC(c.w, c.nm, V_YP)[m]; r.cp = VEC(c.w, c.nm, V_CP)[m];
    r.w = wgt ? wgt[m] : 1.0;
    r.sg = sig ? sig[m] : 0.0;
    r.fv = fv ? fv[m] : 0.0;
    r.k0 = mk ? (int)mk[m] : 0; r.km = mk ? (int)mk[m1] : 0; r.kp = mk ? (int)mk[p1] : 0;
}
__device__ __forceinline__ void kkt_point_make(const KktRaw& r, double* rec)
{
    const double s2 = r.s2, s1 = r.s1, s0 = r.s0;
    const double nx0 = r.nx0, ny0 = r.ny0, nxm = r.nxm, nym = r.nym, nxp = r.nxp, nyp = r.nyp;
    const double w = r.w, sg = r.sg;
    const double f0 = r.k0 != 0 ? 0.0 : 1.0, fm = r.km != 0 ? 0.0 : 1.0, fp = r.kp != 0 ? 0.0 : 1.0;
    const double a = -2.0 * r.cp * r.yp, b = 2.0 * r.cp * r.xp;
    rec[0] = f0 != 0.0 ? sg : 1.0;
    rec[1] = 3.0 * (s1 + 1.0) * nx0 * f0;
    rec[2] = 3.0 * (s1 + 1.0) * ny0 * f0;
    rec[3] = w * a * a;
    rec[4] = w * a * b;
    rec[5] = w * b * b;
    rec[6] = 2.0 * s1 * s1 + 2.0 * s1;
    rec[7] = -3.0 * s2 * nx0 * f0;
    rec[8] = -3.0 * s2 * ny0 * f0;
    rec[9] = s2 * s1 * s1;
    rec[10] = -3.0 * nxm * fm;
    rec[11] = -3.0 * nym * fm;
    rec[12] = -3.0 * s1 * nxp * fp;
    rec[13] = -3.0 * s1 * nyp * fp;
    rec[14] = s1 * s0 * s0;
    rec[15] = -3.0 * nx0 * f0;
    rec[16] = -3.0 * ny0 * f0;
    rec[17] = r.fv;
    rec[18] = 0.0;
    rec[19] = 1.0;
}
// Open chain (DESIGN.md "Open chains"; with S[n-2] = S[n-1] = 1 every other waypoint's record is the ring formula): the records of waypoints 0
// and n - 1 after kkt_point_make.  R[0, .] = 3 (q_1 - q_0), R[n-1, .] = -3 (q_(n-1) - q_(n-2)): d03, d04 = 3 n (= -rec[15], -rec[16] of the ring
// formula, exactly); T[0, 0] = T[n-1, n-1] = 2.  Lo_0 = 0 (nothing couples waypoint 0 to waypoint n - 1), and so is Up_(n-1) = Lo_0', the 1 of
// T[0, n-1] (rec[19] as an Up entry) included.  (Waypoint 0 is always separator 0 and waypoint n - 1 is never a segment's first step, so rec[19]
// is not needed as the 1 of a Lo there.)  Called only for chains: the rings' records are kkt_point_make's, instruction for instruction.
__device__ __forceinline__ void kkt_chain_ends(double* rec, int m, int n)
{
    if (m == 0) {
        rec[1] = -rec[15];
        rec[2] = -rec[16];
        rec[6] = 2.0;
        rec[7] = rec[8] = rec[9] = rec[10] = rec[11] = 0.0;
    } else if (m == n - 1) {
        rec[1] = -rec[15];
        rec[2] = -rec[16];
        rec[6] = 2.0;
        rec[12] = rec[13] = rec[14] = rec[15] = rec[16] = 0.0;
        rec[19] = 0.0;
    }
}
__device__ __forceinline__ int kkt_rec_point(int m, int s1, int n) { m = m < s1 ? m : s1 - 1; return m < n ? m : n - 1; }
__device__ __forceinline__ void kkt_point_record(const LCtx& c, const gdouble* sig, const gschar* mk, const gdouble* wgt, const gdouble* fv, int m, double* rec)
{
    KktRaw r;
    kkt_point_load(c, sig, mk, wgt, fv, m, r);
    kkt_point_make(r, rec);
    if (c.chain) kkt_chain_ends(rec, m, c.d.n);
}

// t = Lo s  for the sparse coupling block given by lo[0..4]
#define KKT_LO_APPLY(lo, s, t)                                                                                 \
    do {                                                                                                       \
        t[0] = lo[0] * s[3] + lo[1] * s[4];                                                                    \
        t[1] = lo[2] * s[3];                                                                                   \
        t[2] = lo[2] * s[4];                                                                                   \
        t[3] = fma(lo[3], s[0], s[1]);                                                                         \
        t[4] = fma(lo[4], s[0], s[2]);                                                                         \
    } while (0)
// t = Up s,  Up = (Lo of the next point)' given by up[0..4]
#define KKT_UP_APPLY(up, s, t)                                                                                 \
    do {                                                                                                       \
        t[0] = up[3] * s[3] + up[4] * s[4];                                                                    \
        t[1] = s[3];                                                                                           \
        t[2] = s[4];                                                                                           \
        t[3] = up[0] * s[0] + up[2] * s[1];                                                                    \
        t[4] = up[1] * s[0] + up[2] * s[2];                                                                    \
    } while (0)

// In-place Gauss-Jordan elimination of a 5 x 16 working matrix held one column per lane of a 16-lane row, with a STATIC pivot order:
// (lx row, cx column), (ly, cy), (cx, lx), (cy, ly), (alpha, alpha).  The first four pivots are pivots of the diagonally dominant spline
// matrix T (its diagonal td = 2 s^2 + 2 s against off-diagonals 1 and s s'^2), the last one is the pivot of the positive definite
// reduced system: no search, no row swaps (scripts/proto_kkt.py --static: backward errors 1e-16 .. 4e-15, the same as with partial pivoting
// inside the block, curvature-row weights up to 1e10 included).  Rows and columns come out permuted by pi = (0 3 4 1 2), which is
// undone by renaming registers (rows) and by the column slot a lane stores to (kkt_col_of_lane).
template <int K> __device__ __forceinline__ void kkt_gj_stage(double (&v)[5], int c, bool& bad)
{
    constexpr int RHO = K == 0 ? 3 : K == 1 ? 4 : K == 2 ? 1 : K == 3 ? 2 : 0;
    constexpr int GAM = K == 0 ? 1 : K == 1 ? 2 : K == 2 ? 3 : K == 3 ? 4 : 0;
    const double piv = bcast_row16<GAM>(v[RHO]);
#ifdef IPM_TRACE
    if ((threadIdx.x & 15) == 0 && !(fabs(piv) > 1e-6) ) printf("   gj stage %d pivot %.3e (tid %d)\n", K, piv, (int)threadIdx.x);
#endif
    bad |= !(fabs(piv) > 1e-290);
    const double inv = kkt_rcp(piv);
    // the lane that owns the pivot column takes the multipliers themselves (in-place inverse): it runs the same update on the unit
    // column -- pivot entry 1, the others 0 -- instead of selecting: one select and four multiplications where ten selects were
    // Row j takes  - a_j (pivot row / pivot):  the lanes broadcast the RAW entry a_j of the pivot column and multiply it by their own entry of
    // the scaled pivot row -- one multiplication per stage where the four multipliers -a_j / pivot were formed before broadcasting
    const bool own = (c == GAM);
    const double keep = own ? 0.0 : 1.0;
    const double vk = own ? 1.0 : v[RHO];
    const double pr = vk * inv;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        if (j == RHO) continue;
        v[j] = fnma_bcast_row16<GAM>(v[j], pr, v[j] * keep);
    }
    v[RHO] = pr;
}
__device__ __forceinline__ void kkt_gj(double (&v)[5], int c, bool& bad)
{
    kkt_gj_stage<0>(v, c, bad);
    kkt_gj_stage<1>(v, c, bad);
    kkt_gj_stage<2>(v, c, bad);
    kkt_gj_stage<3>(v, c, bad);
    kkt_gj_stage<4>(v, c, bad);
    const double r1 = v[3], r2 = v[4], r3 = v[1], r4 = v[2];      // register rho holds row pi(rho)
    v[1] = r1; v[2] = r2; v[3] = r3; v[4] = r4;
}
// lanes 0..4 hold the columns of the inverse permuted the same way: lane c holds column pi(c)
__device__ __forceinline__ int kkt_col_of_lane(int c) { return c == 1 ? 3 : c == 2 ? 4 : c == 3 ? 1 : c == 4 ? 2 : c; }

// Record precision (round 4).  F32: the records of a factorisation -- D~^-1 | Lo, the forward-eliminated spike | y, the spikes' alpha rows,
// the forward chain's y -- are STORED as floats: half the bytes in every pass that streams them (spike pass, chains, correction).  The
// arithmetic does not change: the elimination runs in fp64 registers, and the passes widen a record when they stage it into LDS, so the
// recursions work on doubles as before.  What is lost is the last 29 bits of the STORED numbers, i.e. the solve applies the inverse of a
// matrix within 6e-8 (relative, entrywise on the blocks) of the one asked for: an inexact Newton direction with a residual of that size.
// The interior point can live with it (its iterates are corrected by the next step, and convergence is only ever declared on a gradient
// recomputed exactly through E); the exact phases -- active-set vertex, refinement, resumed interior point, curvature rows -- keep fp64.
typedef __attribute__((address_space(1))) float gfloat;
typedef float f4 __attribute__((vector_size(16)));
union KItem { d2 d; f4 f; };
template <bool F32> struct KRec;
template <> struct KRec<false> {
    typedef gdouble G;
    typedef double T;
    static constexpr int AY = KAY;       // elements per record of K_AY
    static constexpr int PER = 2;        // elements per 16-byte item
};
template <> struct KRec<true> {
    typedef gfloat G;
    typedef float T;
    static constexpr int AY = 28;        // 25 used; records stay multiples of 16 bytes
    static constexpr int PER = 4;
};
// Chunks of packed records are staged as contiguous copies: NEL elements (16-byte items) starting at `src`, this group's 16 lanes -- issue /
// commit halves; the commit widens float records.
template <bool F32, int NEL> __device__ __forceinline__ void kkt_stage_issue(const typename KRec<F32>::G* src, int c, KItem (&regs)[(NEL / KRec<F32>::PER + 15) / 16])
{
    constexpr int NI = NEL / KRec<F32>::PER;
    static_assert(NEL % KRec<F32>::PER == 0, "whole 16-byte items");
#pragma unroll
    for (int i = 0; i < (NI + 15) / 16; ++i) {
        const int idx = c + 16 * i;
        regs[i].d = *(const gd2*)((const gdouble*)src + 2 * (idx < NI ? idx : 0));
    }
}
template <bool F32, int NEL> __device__ __forceinline__ void kkt_stage_commit(double* dst, int c, const KItem (&regs)[(NEL / KRec<F32>::PER + 15) / 16])
{
    constexpr int NI = NEL / KRec<F32>::PER;
#pragma unroll
    for (int i = 0; i < (NI + 15) / 16; ++i) {
        const int idx = c + 16 * i;
        if (NI % 16 == 0 || idx < NI) {
            if (!F32) *(d2*)(dst + 2 * idx) = regs[i].d;
            else {
                const f4 v = regs[i].f;
                d2 lo, hi;
                lo[0] = (double)v[0]; lo[1] = (double)v[1]; hi[0] = (double)v[2]; hi[1] = (double)v[3];
                *(d2*)(dst + 4 * idx) = lo;
                *(d2*)(dst + 4 * idx + 2) = hi;
            }
        }
    }
}

// ---- factorisation --------------------------------------------------------------------------------------------------
// fv (optional): right-hand side of the solve that follows.  It rides through the elimination as the 16th column of the working matrix and
// through the backward pass as an 11th column next to the spikes: solve_kkt(c, fv, fwd_done = true) then only has the separators' system and
// the spike correction left (fv holds the alpha components of A_int^-1 r at the interior points, r at the separators).
template <bool F32>
KKT_FN int factor_kkt(const LCtx& c, const gdouble* sig, const gschar* mk, const gdouble* wgt, gdouble* fv)
{
    typedef typename KRec<F32>::G RG;
    typedef typename KRec<F32>::T RT;
    constexpr int KAYR = KRec<F32>::AY;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int cl = lane & 15, g = 4 * wv + (lane >> 4);
    const int n = c.d.n;
    const KktGeom G = kkt_geom(n);
    const int nseg = G.nseg, Lmax = G.Lmax;
    double* per = g_sm + SM_S;
    double* ovl = g_sm + SM_OVL;
    const bool has = g < nseg;
    const int s0 = has ? KSEP(g, n, nseg) : 0;
    const int s1 = has ? (g + 1 < nseg ? KSEP(g + 1, n, nseg) : n) : 1;
    const int lo_pt = s0 + 1, L = s1 - s0 - 1;
    RG* AD = (RG*)K_AD(c);
    RG* AS = (RG*)K_AS(c);
    RG* AY = (RG*)K_AY(c);
    const bool chain = c.chain != 0;
    bool bad = false;
    long long kt_last = KKT_TIMERS ? (long long)wall_clock64() : 0;

    __syncthreads();
    if (tid == 0) ovl[KO_FLAG] = 0.0;
    // separators' coefficient records
    if (tid < nseg) {
        double rec[KCOEF];
        kkt_point_record(c, sig, mk, wgt, nullptr, KSEP(tid, n, nseg), rec);
#pragma unroll
        for (int q = 0; q < KCOEF; ++q) ovl[KO_SREC + tid * KCOEF + q] = rec[q];
#pragma unroll
        for (int q = 0; q < 10; ++q) per[KP_SEP + tid * 10 + q] = rec[7 + q];
    }

    // ---- forward elimination of the segments --------------------------------------------------------------------------
    double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    double* coef = ovl + KO_CH + g * KS_COEF;
    int ixF[5], ixN[5];
#pragma unroll
    for (int r = 0; r < 5; ++r) { ixF[r] = kkt_base_index(cl, r, true); ixN[r] = kkt_base_index(cl, r, false); }
    // where a lane's column of a step goes: D~^-1 (lanes 0..4: the lower triangle of its column, packed), left spike (11..14), y (15)
    // (lanes 5..9: G stays in registers; lane 10: column 0 of the spike is not stored).
    const int colp = kkt_col_of_lane(cl);
    RG* const st_base = cl < 5 ? AD : cl < 15 ? AY + (cl - 11) : AY + 20;
    const int st_rec = cl < 5 ? KAD : KAYR;
    int st_off[5];
    bool st_en[5];
#pragma unroll
    for (int r = 0; r < 5; ++r) {
        st_off[r] = cl < 5 ? KTRI(r, colp) : cl < 15 ? r * 4 : r;
        st_en[r] = cl < 5 ? r >= colp : (cl >= 11 && cl < 15) || (cl == 15 && fv != nullptr);
    }
    // The records of TWO steps are assembled in LDS (in the spike blocks' region, idle until the backward pass) and leave as contiguous 16-byte
    // items, three store instructions per pair of steps and lane: the per-step stores above -- 8-byte pieces, twenty-odd lanes scattered
    // over six or more cache lines per instruction -- had bounded the elimination (126 us; 66 us without them, the arithmetic's share;
    // scripts/write_bw.hip: that pattern tops out at 3.4 TB/s chip-wide, contiguous 16-byte items at 5.6).  Staged: 102 us.  (The same
    // staging changed nothing while the step still had 207 VALU instructions -- the elimination was then bound by those.)
    constexpr int PER = KRec<F32>::PER;
    constexpr int STG_SLOT = KAD + KAYR;                    // entries of one step: its D~^-1 | Lo record, then its spike | y record
    constexpr int NI_AD = KAD / PER, NI_AY = KAYR / PER;    // 16-byte items per record
    constexpr int NJ = (2 * (NI_AD + NI_AY) + 15) / 16;     // items per lane and pair of steps
    static_assert(KAD % PER == 0 && KAYR % PER == 0 && 2 * STG_SLOT * sizeof(RT) <= KS_STG * sizeof(double), "staged records: whole items, inside the group's slice");
    RT* const stg = (RT*)(ovl + KO_SPK + g * KS_STG);
    RT* const stg_lane = stg + (cl < 5 ? 0 : KAD + (cl < 15 ? cl - 11 : 20));          // (lanes 5..10 store nothing)
    const RT* fl_src[NJ];
    RG* fl_dst[NJ];
    int fl_rec[NJ];
    bool fl_on[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int i = cl + 16 * j;                          // items 0 .. 2 NI_AD - 1: the two D~^-1 | Lo records, consecutive in memory; then the two others
        const bool ad = i < 2 * NI_AD;
        const int q = ad ? i : i - 2 * NI_AD;
        const int pp = ad ? q / NI_AD : q / NI_AY, w = ad ? q % NI_AD : q % NI_AY;
        fl_on[j] = has && i < 2 * (NI_AD + NI_AY);
        fl_src[j] = stg + pp * STG_SLOT + (ad ? 0 : KAD) + w * PER;
        fl_dst[j] = (ad ? AD + (size_t)lo_pt * KAD : AY + (size_t)lo_pt * KAYR) + q * PER;
        fl_rec[j] = ad ? KAD : KAYR;
    }
    const double msub = (cl < 5 || cl >= 10) ? 1.0 : 0.0;      // the columns that take  - Lo (previous columns): D~, the left spike, the right-hand side
    // the loads of a chunk's sixteen records are issued a chunk ahead (KktRaw in registers across the sixteen steps)
#define KKT_REC_POINT(k0_) kkt_rec_point(lo_pt + (k0_) + cl, s1, n)
    KktRaw raw;
    kkt_point_load(c, sig, mk, wgt, fv, KKT_REC_POINT(0), raw);
    for (int k0 = 0; k0 < Lmax; k0 += KCKF) {
        {
            __builtin_amdgcn_wave_barrier();
            {
                double rec[KCOEF];
                kkt_point_make(raw, rec);
#pragma unroll
                for (int q = 0; q < KCOEF; ++q) coef[cl * KCOEF + q] = rec[q];
            }
            if (chain) kkt_chain_ends(coef + cl * KCOEF, KKT_REC_POINT(k0), n);      // (on the staged record: nothing more stays live in the loop)
            __builtin_amdgcn_wave_barrier();
            if (k0 + KCKF < Lmax) kkt_point_load(c, sig, mk, wgt, fv, KKT_REC_POINT(k0 + KCKF), raw);
        }
        // a step reads five entries of its coefficient record through per-lane indices (its column of [ Dg | Up | Lo | r e_0 ]) and the five
        // entries of Lo -- from LDS one step ahead, during the previous step's elimination
        // Steps 0 .. Lmax-2 exist in every segment (the segments' lengths differ by at most one): they run unguarded -- the state v is
        // overwritten in place, which saves the copy a kept-alive v costs in front of every DPP merge -- and only the last step asks
        // whether the segment has it.
        double bs[5], lo[5];
#define KKT_ELIM_STEP(GUARD_, kk_, SLOT_)                                                                                       \
        {                                                                                                                       \
            const int k = k0 + (kk_);                                                                                           \
            const bool active = (GUARD_) ? (has && k < L) : has;                                                                \
            if ((kk_) == 0) {                                                                                                   \
                _Pragma("unroll") for (int r = 0; r < 5; ++r) { bs[r] = coef[k == 0 ? ixF[r] : ixN[r]]; lo[r] = coef[7 + r]; }  \
            }                                                                                                                   \
            double s[5], t[5];                                                                                                  \
            _Pragma("unroll") for (int r = 0; r < 5; ++r) s[r] = dpp_shl5_low8(v[r]);                                           \
            KKT_LO_APPLY(lo, s, t);                                                                                             \
            double nvv[5];                                                                                                      \
            _Pragma("unroll") for (int r = 0; r < 5; ++r) nvv[r] = fma(-msub, t[r], bs[r]);                                     \
            const double lov = cl == 0 ? lo[0] : cl == 1 ? lo[1] : cl == 2 ? lo[2] : cl == 3 ? lo[3] : lo[4];                   \
            if ((kk_) + 1 < KCKF) {                                                                                             \
                const double* cn = coef + ((kk_) + 1) * KCOEF;                                                                  \
                _Pragma("unroll") for (int r = 0; r < 5; ++r) { bs[r] = cn[ixN[r]]; lo[r] = cn[7 + r]; }                        \
            }                                                                                                                   \
            bool bad_step = false;                                                                                              \
            kkt_gj(nvv, cl, bad_step);                                                                                          \
            if (active) {                                                                                                       \
                bad |= bad_step;                                                                                                \
                /* every lane stores its column through its own base pointer and row stride (set up once: no branching by lane class here) */ \
                if ((SLOT_) < 0) {       /* a step without a partner: straight to memory */                                     \
                    RG* o = st_base + (size_t)(lo_pt + k) * st_rec;                                                             \
                    _Pragma("unroll") for (int r = 0; r < 5; ++r)                                                               \
                        if (st_en[r]) o[st_off[r]] = (RT)nvv[r];                                                                \
                    if (cl < 5) o[15 + cl] = (RT)lov;                                                                           \
                } else {                                                                                                        \
                    RT* o = stg_lane + ((SLOT_) < 0 ? 0 : (SLOT_)) * STG_SLOT;                                                  \
                    _Pragma("unroll") for (int r = 0; r < 5; ++r)                                                               \
                        if (st_en[r]) o[st_off[r]] = (RT)nvv[r];                                                                \
                    if (cl < 5) o[15 + cl] = (RT)lov;                                                                           \
                }                                                                                                               \
            }                                                                                                                   \
            if (!(GUARD_) || active) {                                                                                          \
                _Pragma("unroll") for (int r = 0; r < 5; ++r) v[r] = nvv[r];                                                    \
            }                                                                                                                   \
        }
        const int kend = Lmax - 1 - k0 < KCKF ? Lmax - 1 - k0 : KCKF;
        // (two steps per trip, written out: the next step's coefficients are read into the registers the step after it works in -- a one-step
        //  loop body copies them across, ten 64-bit moves per step; hipcc does not unroll loops with DPP operations by itself)
        int kk = 0;
        for (; kk + 1 < kend; kk += 2) {
            KKT_ELIM_STEP(false, kk, 0)
            KKT_ELIM_STEP(false, kk + 1, 1)
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int j = 0; j < NJ; ++j)
                if (fl_on[j]) *(gd2*)(fl_dst[j] + (size_t)(k0 + kk) * fl_rec[j]) = *(const d2*)fl_src[j];
            __builtin_amdgcn_wave_barrier();
        }
        const int ktail = kend < KCKF ? kend + 1 : kend;
        for (; kk < ktail; ++kk) KKT_ELIM_STEP(true, kk, -1)
#undef KKT_ELIM_STEP
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();           // the coefficient chunks are done with; AG / AY written by this group are read back by itself below
    KT(0);

    // ---- backward pass: spikes.  Lanes 5..9 carry X^R (starts as G of the last point), lanes 10..14 X^L (starts as Y of the last point)
    {
        double* spk = ovl + KO_SPK + g * 100;
        if (has) {
            const int m = lo_pt + L - 1;
            if (cl >= 5 && cl < 10) {
                if (cl > 5) AS[(size_t)m * KAS + 4 + (cl - 6)] = (RT)v[0];
#pragma unroll
                for (int r = 0; r < 5; ++r) spk[75 + r * 5 + (cl - 5)] = v[r];          // XR at the last point
            } else if (cl >= 10 && cl < 15) {
                if (cl > 10) AS[(size_t)m * KAS + (cl - 11)] = (RT)v[0];
#pragma unroll
                for (int r = 0; r < 5; ++r) spk[50 + r * 5 + (cl - 10)] = v[r];         // XL at the last point
            } else if (cl == 15 && fv) {
                fv[m] = v[0];
#pragma unroll
                for (int r = 0; r < 5; ++r) per[KP_X0 + g * 10 + 5 + r] = v[r];         // X0 at the last point
            }
        }
        // alpha row of a lane's column: the spikes' record (lanes 5..14) or the right-hand side vector itself (lane 15)
        // (lane 15's column goes to the fp64 vector fv, the spikes' rows to the record array: two typed pointers, one of them used)
        RG* const sp_rec = cl >= 10 ? AS + (cl - 11) : AS + 4 + (cl - 6);        // (columns 0 of both spikes -- lanes 5, 10 -- are not stored)
        const bool sp_on = (cl > 5 && cl < 10) || (cl > 10 && cl < 15) || (cl == 15 && fv != nullptr);
        double* chG = ovl + KO_CH + g * KS_CH2G;
        double* chY = ovl + KO_CH2 + g * KS_CH2Y;
        const int nq = (Lmax - 1 + KCK2 - 1) / KCK2;          // chunks over the steps 0 .. Lmax-2
        double up_prev[5] = {0.0, 0.0, 0.0, 0.0, 0.0};          // Lo of the waypoint processed one step earlier: starts with the segment's last one
        if (has) {
#pragma unroll
            for (int r = 0; r < 5; ++r) up_prev[r] = (double)AD[(size_t)(lo_pt + L - 1) * KAD + 15 + r];
        }
        // column 0 of the left spike from columns 1 and 2: the constants are lo3, lo4 of the segment's first waypoint
        const double l3f = has ? (double)AD[(size_t)lo_pt * KAD + 18] : 0.0, l4f = has ? (double)AD[(size_t)lo_pt * KAD + 19] : 0.0;
        KItem rg[(KCK2 * KAD / KRec<F32>::PER + 15) / 16], ry[(KCK2 * KAYR / KRec<F32>::PER + 15) / 16];
        if (nq > 0) {
            kkt_stage_issue<F32, KCK2 * KAD>(AD + (size_t)(lo_pt + (nq - 1) * KCK2) * KAD, cl, rg);
            kkt_stage_issue<F32, KCK2 * KAYR>(AY + (size_t)(lo_pt + (nq - 1) * KCK2) * KAYR, cl, ry);
        }
        for (int q = nq - 1; q >= 0; --q) {
            __builtin_amdgcn_wave_barrier();
            kkt_stage_commit<F32, KCK2 * KAD>(chG, cl, rg);
            kkt_stage_commit<F32, KCK2 * KAYR>(chY, cl, ry);
            __builtin_amdgcn_wave_barrier();
            if (q > 0) {
                kkt_stage_issue<F32, KCK2 * KAD>(AD + (size_t)(lo_pt + (q - 1) * KCK2) * KAD, cl, rg);
                kkt_stage_issue<F32, KCK2 * KAYR>(AY + (size_t)(lo_pt + (q - 1) * KCK2) * KAYR, cl, ry);
            }
            // G_k x = D~_k^-1 (Up_k x),  Up_k = Lo_(k+1)': the step reads D~^-1 and Lo of its own record and applies the Lo it read one step
            // earlier (waypoint k + 1)
            const int cy4 = cl >= 11 && cl < 15 ? cl - 11 : 0;
#define KKT_YREAD(b_, r_) ((b_)[cl == 15 ? 20 + (r_) : (r_) * 4 + cy4])                /* (lane 10 reads lane 11's column: its own recursion is not used, see below) */
            double g_c[15], y_c[5], lo_c[5];
#pragma unroll
            for (int e = 0; e < 15; ++e) g_c[e] = chG[(KCK2 - 1) * KAD + e];
#pragma unroll
            for (int r = 0; r < 5; ++r) { y_c[r] = KKT_YREAD(chY + (KCK2 - 1) * KAYR, r); lo_c[r] = chG[(KCK2 - 1) * KAD + 15 + r]; }
#pragma unroll
            for (int kk = KCK2 - 1; kk >= 0; --kk) {
                const int k = q * KCK2 + kk;
                const bool active = has && k < L - 1;
                double g_n[15], y_n[5], lo_n[5];
                if (kk > 0) {
#pragma unroll
                    for (int e = 0; e < 15; ++e) g_n[e] = chG[(kk - 1) * KAD + e];
#pragma unroll
                    for (int r = 0; r < 5; ++r) { y_n[r] = KKT_YREAD(chY + (kk - 1) * KAYR, r); lo_n[r] = chG[(kk - 1) * KAD + 15 + r]; }
                }
                double t[5], nx_[5];
                KKT_UP_APPLY(up_prev, v, t);
#pragma unroll
                for (int r = 0; r < 5; ++r) {
                    double acc = cl >= 10 ? y_c[r] : 0.0;
#pragma unroll
                    for (int j = 0; j < 5; ++j) acc = fma(-g_c[KTRI(r, j)], t[j], acc);
                    nx_[r] = acc;
                }
                // (lane 10 -- column 0 of the left spike -- does not run its own recursion, its y is not stored: every column obeys the same
                //  linear recursion, so column 0 stays  lo3 col1 + lo4 col2  all the way; it is rebuilt where the full block is needed, below)
                if (active) {
#pragma unroll
                    for (int r = 0; r < 5; ++r) { v[r] = nx_[r]; up_prev[r] = lo_c[r]; }
                    if (sp_on) {
                        if (cl == 15) fv[lo_pt + k] = v[0];
                        else sp_rec[(size_t)(lo_pt + k) * KAS] = (RT)v[0];
                    }
                }
                if (kk > 0) {
#pragma unroll
                    for (int e = 0; e < 15; ++e) g_c[e] = g_n[e];
#pragma unroll
                    for (int r = 0; r < 5; ++r) { y_c[r] = y_n[r]; lo_c[r] = lo_n[r]; }
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 5; ++r) {      // column 0 of the left spike at the first interior point, all five rows
            const double f = l3f * dpp_shl1(v[r]) + l4f * dpp_shl2(v[r]);
            if (cl == 10) v[r] = f;
        }
        if (has) {             // v now holds the spikes at the first interior point
            if (cl >= 5 && cl < 10) {
#pragma unroll
                for (int r = 0; r < 5; ++r) spk[25 + r * 5 + (cl - 5)] = v[r];          // XR at the first point
            } else if (cl >= 10 && cl < 15) {
#pragma unroll
                for (int r = 0; r < 5; ++r) spk[r * 5 + (cl - 10)] = v[r];              // XL at the first point
            } else if (cl == 15 && fv) {
#pragma unroll
                for (int r = 0; r < 5; ++r) per[KP_X0 + g * 10 + r] = v[r];             // X0 at the first point
            }
        }
    }
    __syncthreads();
    KT(1);

    // ---- the separators' blocks:  RD_j = Dg - Up XL0(j) - Lo XRl(j-1),  RU_j = -Up XR0(j),  RL_j = -Lo XLl(j-1) -------------------------
    for (int e = tid; e < nseg * 25; e += MCQ_NT) {
        const int j = e / 25, rc_ = e % 25, r = rc_ / 5, cc = rc_ % 5;
        const int jp = j > 0 ? j - 1 : nseg - 1;
        const double* rec = ovl + KO_SREC + j * KCOEF;
        const double* spj = ovl + KO_SPK + j * 100;
        const double* spp = ovl + KO_SPK + jp * 100;
        const double lo[5] = {rec[7], rec[8], rec[9], rec[10], rec[11]};
        const double up[5] = {rec[12], rec[13], rec[14], rec[15], rec[16]};
        double xl0[5], xr0[5], xll[5], xrl[5], t[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            xl0[q] = spj[q * 5 + cc];
            xr0[q] = spj[25 + q * 5 + cc];
            xll[q] = spp[50 + q * 5 + cc];
            xrl[q] = spp[75 + q * 5 + cc];
        }
        const double dg = rec[kkt_base_index(cc, r, false)];          // Dg[r][cc] (slot 18 of a record is the zero)
        // (t[r] with a runtime r would put t into scratch memory -- four round trips per entry: selected instead)
#define KKT_SEL5(t_, r_) ((r_) == 0 ? t_[0] : (r_) == 1 ? t_[1] : (r_) == 2 ? t_[2] : (r_) == 3 ? t_[3] : t_[4])
        KKT_UP_APPLY(up, xl0, t);
        const double u_xl0 = KKT_SEL5(t, r);
        KKT_UP_APPLY(up, xr0, t);
        const double u_xr0 = KKT_SEL5(t, r);
        if (c.chain && j == 0) {           // open chain: Lo_0 = 0 (KKT_LO_APPLY has the 1s of T built in: its operands are zeroed instead --
#pragma unroll                              //  a select on its result would stop the compiler from fusing the products into the differences below,
            for (int q = 0; q < 5; ++q) xll[q] = xrl[q] = 0.0;       //  and rings would round differently)
        }
        KKT_LO_APPLY(lo, xll, t);
        const double l_xll = KKT_SEL5(t, r);
        KKT_LO_APPLY(lo, xrl, t);
        const double l_xrl = KKT_SEL5(t, r);
#undef KKT_SEL5
        double* rb = ovl + KO_RB + j * 75;
        rb[rc_] = dg - u_xl0 - l_xrl;
        rb[25 + rc_] = -l_xll;
        rb[50 + rc_] = -u_xr0;
        if (j > 0) per[KP_STEP + (j - 1) * 100 + 50 + rc_] = -l_xll;        // RL_j: what a solve's forward chain multiplies by
    }
    __syncthreads();

    // ---- the separators' chain (wave 0; all four rows of the wave run it, row 0 stores) -------------------------------------------------
    if (wv == 0) {
        const bool st = lane < 16;
        bool badr = false;
        if (nseg == 1) {
            double w5[5];
#pragma unroll
            for (int r = 0; r < 5; ++r) {
                const int cc = cl < 5 ? cl : 0;
                w5[r] = ovl[KO_RB + r * 5 + cc] + ovl[KO_RB + 25 + r * 5 + cc] + ovl[KO_RB + 50 + r * 5 + cc];
                if (cl >= 5) w5[r] = (r == (cl % 5)) ? 1.0 : 0.0;
            }
            kkt_gj(w5, cl, badr);
            const int pos = kkt_col_of_lane(cl);
            if (st && cl < 5) {
#pragma unroll
                for (int r = 0; r < 5; ++r) per[KP_R0I + r * 5 + pos] = w5[r];
            }
        } else {
            const int LR = nseg - 1;
            double vr[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
            // Forward chain, one column per lane:  [ RD_k - RL_k G_(k-1) | RU_k | -RL_k Y_(k-1)  (RL_1 itself at the first step) ]  reduced by
            // Gauss-Jordan.  No branching by lane class inside the step: a lane reads ITS entry of the step's blocks through an index fixed
            // here, scaled by 1 or 0, and takes  - RL (its source column)  with the source column scaled by -1 or 0 -- the step had spent more
            // instructions on execution masks and on waiting for one LDS read at a time than on arithmetic.
            const int cc = cl % 5;
            const int rd_off = cl < 5 ? cc : cl < 10 ? 50 + cc : 25 + cc;                  // lanes 0..4: RD, 5..9: RU, 10..14: RL (first step only)
            const double cAF = cl < 15 ? 1.0 : 0.0, cAN = cl < 10 ? 1.0 : 0.0;
            const double nsc = (cl < 5 || (cl >= 10 && cl < 15)) ? -1.0 : 0.0;
            const int pos = kkt_col_of_lane(cl);
            // where the column goes: D^-1 (un-permuted), G of the step record; Y into the spike blocks' region (done with)
            const int st_lane = cl < 5 ? SM_S + KP_STEP + pos : cl < 10 ? SM_S + KP_STEP + 25 + (cl - 5) : SM_OVL + KO_SPK + (cl - 10);
            const int st_step = cl < 10 ? 100 : 25;
            const bool st_on = st && cl < 15;
            for (int k = 0; k < LR; ++k) {
                const double* rb = ovl + KO_RB + (k + 1) * 75;
                double rl[25], own[5], sn[5], w5[5];
#pragma unroll
                for (int e = 0; e < 25; ++e) rl[e] = rb[25 + e];
#pragma unroll
                for (int r = 0; r < 5; ++r) own[r] = rb[rd_off + r * 5];
                const double cA = k == 0 ? cAF : cAN;
#pragma unroll
                for (int r = 0; r < 5; ++r) sn[r] = nsc * dpp_shl5_low8(vr[r]);             // lanes 0..4: G of the previous step; 10..14: their own Y
#pragma unroll
                for (int r = 0; r < 5; ++r) {
                    double acc = cA * own[r];
#pragma unroll
                    for (int j = 0; j < 5; ++j) acc = fma(rl[r * 5 + j], sn[j], acc);
                    w5[r] = acc;
                }
                kkt_gj(w5, cl, badr);
                __builtin_amdgcn_wave_barrier();
                if (st_on) {
                    double* o = g_sm + st_lane + k * st_step;
#pragma unroll
                    for (int r = 0; r < 5; ++r) o[r * 5] = w5[r];
                }
#pragma unroll
                for (int r = 0; r < 5; ++r) vr[r] = w5[r];
            }
            // backward: lanes 5..9 X^R, lanes 10..14 X^L;  XS = X^L + X^R per step
            __builtin_amdgcn_wave_barrier();
            for (int k = LR - 1; k >= 0; --k) {
                if (k < LR - 1) {
                    const double* gk = per + KP_STEP + k * 100 + 25;
                    const double* ys = ovl + KO_SPK + k * 25;
                    const int cy = cl >= 10 && cl < 15 ? cl - 10 : 0;
                    double nx_[5];
#pragma unroll
                    for (int r = 0; r < 5; ++r) {
                        double acc = (cl >= 10 && cl < 15) ? ys[r * 5 + cy] : 0.0;
#pragma unroll
                        for (int j = 0; j < 5; ++j) acc = fma(-gk[r * 5 + j], vr[j], acc);
                        nx_[r] = acc;
                    }
#pragma unroll
                    for (int r = 0; r < 5; ++r) vr[r] = nx_[r];
                }
                double* ps = per + KP_STEP + k * 100;
#pragma unroll
                for (int r = 0; r < 5; ++r) {
                    const double xs = vr[r] + dpp_shl5(vr[r]);          // lanes 5..9: X^R + X^L
                    if (st && cl >= 5 && cl < 10) ps[75 + r * 5 + (cl - 5)] = xs;
                }
            }
            __builtin_amdgcn_wave_barrier();
            // separator 0:  R0 = RD_0 - RU_0 XS_0 - RL_0 XS_last
            {
                const double* rb = ovl + KO_RB;
                const double* x0 = per + KP_STEP + 75;
                const double* xl = per + KP_STEP + (LR - 1) * 100 + 75;
                const int cc = cl % 5;
                double w5[5];
#pragma unroll
                for (int r = 0; r < 5; ++r) {
                    double acc = rb[r * 5 + cc];
#pragma unroll
                    for (int j = 0; j < 5; ++j) acc -= rb[50 + r * 5 + j] * x0[j * 5 + cc] + rb[25 + r * 5 + j] * xl[j * 5 + cc];
                    w5[r] = cl < 5 ? acc : ((r == cc) ? 1.0 : 0.0);
                }
                kkt_gj(w5, cl, badr);
            const int pos = kkt_col_of_lane(cl);
                if (st && cl < 5) {
#pragma unroll
                    for (int r = 0; r < 5; ++r) {
                        per[KP_R0I + r * 5 + pos] = w5[r];
                        per[KP_RU0 + r * 5 + cl] = rb[50 + r * 5 + cl];
                        per[KP_RL0 + r * 5 + cl] = rb[25 + r * 5 + cl];
                    }
                }
            }
        }
#ifdef IPM_TRACE
        if (badr && lane == 0) printf("factor_kkt: bad pivot in the separators' chain\n");
#endif
        bad |= badr;
    }
    if (bad) ovl[KO_FLAG] = 1.0;
    __syncthreads();
    // A solve's forward chain over the separators,  y_k = D_k^-1 (r_(k+1) - RL_k y_(k-1)),  is the workgroup's longest serial stretch: the
    // step records take  M_k = D_k^-1 RL_k  in RL_k's place, so that the chain's step is ONE 5 x 5 product on the previous y (the part
    // D_k^-1 r_(k+1) does not depend on the chain and is formed for all k at once).  375 entries, all threads.
    if (nseg > 1) {
        double m_[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int e = tid + q * MCQ_NT;
            m_[q] = 0.0;
            if (e < (nseg - 1) * 25) {
                const double* ps = per + KP_STEP + (e / 25) * 100;
                const int r = (e % 25) / 5, cc = e % 5;
#pragma unroll
                for (int j = 0; j < 5; ++j) m_[q] = fma(ps[r * 5 + j], ps[50 + j * 5 + cc], m_[q]);
            }
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int e = tid + q * MCQ_NT;
            if (e < (nseg - 1) * 25) per[KP_STEP + (e / 25) * 100 + 50 + e % 25] = m_[q];
        }
    }
    KT(2);
    const bool fail = ovl[KO_FLAG] != 0.0;
    __syncthreads();
    return fail ? MCQ_NOT_PD : 0;
}

// ---- solve  M v = rhs  in place -------------------------------------------------------------------------------------
template <bool F32>
KKT_FN void solve_kkt(const LCtx& c, gdouble* vv, bool fwd_done)
{
    typedef typename KRec<F32>::G RG;
    typedef typename KRec<F32>::T RT;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int cl = lane & 15, g = 4 * wv + (lane >> 4);
    const int n = c.d.n;
    const KktGeom G = kkt_geom(n);
    const int nseg = G.nseg, Lmax = G.Lmax;
    double* per = g_sm + SM_S;
    double* ovl = g_sm + SM_OVL;
    const bool has = g < nseg;
    const int s0 = has ? KSEP(g, n, nseg) : 0;
    const int s1 = has ? (g + 1 < nseg ? KSEP(g + 1, n, nseg) : n) : 1;
    const int lo_pt = s0 + 1, L = s1 - s0 - 1;
    const RG* AD = (const RG*)K_AD(c);
    const RG* AS = (const RG*)K_AS(c);
    RG* YV = (RG*)K_YV(c);
    double* ch = ovl + KO_CH + g * KS_CH;
    double* aux = ovl + KO_AUX + g * KS_AUX;
    const int rr_ = cl < 5 ? cl : 4;              // the row of the block this lane computes (lanes 5..15 shadow row 4, never stored)
    int ro[5];                                    // row rr_ of the packed symmetric D~^-1
#pragma unroll
    for (int j = 0; j < 5; ++j) ro[j] = KTRI(rr_, j);
    const int nq = (Lmax + KCK - 1) / KCK;
    long long kt_last = KKT_TIMERS ? (long long)wall_clock64() : 0;
    __syncthreads();

    // ---- forward chain ---------------------------------------------------------------------------------------------------
    if (!fwd_done) {
        KItem rg[(KCK * KAD / KRec<F32>::PER + 15) / 16];
        double rv;
        kkt_stage_issue<F32, KCK * KAD>(AD + (size_t)lo_pt * KAD, cl, rg);
        { int m = lo_pt + cl; m = m < n ? m : n - 1; rv = vv[m]; }
        double y = 0.0;
        for (int q = 0; q < nq; ++q) {
            __builtin_amdgcn_wave_barrier();
            kkt_stage_commit<F32, KCK * KAD>(ch, cl, rg);
            aux[cl] = rv;
            __builtin_amdgcn_wave_barrier();
            if (q + 1 < nq) {
                kkt_stage_issue<F32, KCK * KAD>(AD + (size_t)(lo_pt + (q + 1) * KCK) * KAD, cl, rg);
                int m = lo_pt + (q + 1) * KCK + cl; m = m < n ? m : n - 1; rv = vv[m];
            }
            // operands of a step are read from LDS one step ahead of their use: only the broadcasts of y and 3 + 3 dependent operations
            // remain on the chain
            double lo_c[5], dr_c[5], rk_c;
#pragma unroll
            for (int j = 0; j < 5; ++j) { lo_c[j] = ch[15 + j]; dr_c[j] = ch[ro[j]]; }
            rk_c = aux[0];
#pragma unroll
            for (int kk = 0; kk < KCK; ++kk) {
                const int k = q * KCK + kk;
                const bool active = has && k < L;
                double lo_n[5], dr_n[5], rk_n = 0.0;
                if (kk + 1 < KCK) {
                    const double* rn = ch + (kk + 1) * KAD;
#pragma unroll
                    for (int j = 0; j < 5; ++j) { lo_n[j] = rn[15 + j]; dr_n[j] = rn[ro[j]]; }
                    rk_n = aux[kk + 1];
                }
                double yb[5], t[5];
                yb[0] = bcast_row16<0>(y); yb[1] = bcast_row16<1>(y); yb[2] = bcast_row16<2>(y); yb[3] = bcast_row16<3>(y); yb[4] = bcast_row16<4>(y);
                KKT_LO_APPLY(lo_c, yb, t);
                t[0] = rk_c - t[0];
                // t holds Lo y except t[0] = r - (Lo y)_0:  D~^-1 (r e_0 - Lo y)
                const double yn = (dr_c[0] * t[0] - dr_c[1] * t[1]) - (dr_c[2] * t[2] + dr_c[3] * t[3]) - dr_c[4] * t[4];
                if (active) {
                    y = yn;
                    if (cl < 5) YV[(size_t)(lo_pt + k) * 5 + cl] = (RT)yn;
                }
                if (kk + 1 < KCK) {
#pragma unroll
                    for (int j = 0; j < 5; ++j) { lo_c[j] = lo_n[j]; dr_c[j] = dr_n[j]; }
                    rk_c = rk_n;
                }
            }
        }
    }
    __syncthreads();
    KT(3);

    // ---- backward chain --------------------------------------------------------------------------------------------------
    if (!fwd_done) {
        // y of a chunk: KCK x 5 doubles, entry e = cl + 16 i of the chunk (waypoint e / 5, component e % 5)
#define KKT_Y_ISSUE(qq)                                                                                              \
    _Pragma("unroll") for (int i = 0; i < (KCK * 5 + 15) / 16; ++i) {                                                \
        const int e = cl + 16 * i;                                                                                   \
        int m = lo_pt + (qq) * KCK + e / 5;                                                                          \
        m = m < n ? m : n - 1;                                                                                       \
        ry[i] = (double)YV[(size_t)m * 5 + e % 5];                                                                         \
    }
        KItem rg[(KCK * KAD / KRec<F32>::PER + 15) / 16];
        double ry[(KCK * 5 + 15) / 16];
        kkt_stage_issue<F32, KCK * KAD>(AD + (size_t)(lo_pt + (nq - 1) * KCK) * KAD, cl, rg);
        KKT_Y_ISSUE(nq - 1)
        double x = 0.0;
        double up_prev[5] = {0.0, 0.0, 0.0, 0.0, 0.0};          // x_(L-1) = y_(L-1): whatever is applied to x = 0
        double* x0s = per + KP_X0 + g * 10;
        for (int q = nq - 1; q >= 0; --q) {
            __builtin_amdgcn_wave_barrier();
            kkt_stage_commit<F32, KCK * KAD>(ch, cl, rg);
#pragma unroll
            for (int i = 0; i < (KCK * 5 + 15) / 16; ++i)
                if (cl + 16 * i < KCK * 5) aux[cl + 16 * i] = ry[i];
            __builtin_amdgcn_wave_barrier();
            if (q > 0) {
                kkt_stage_issue<F32, KCK * KAD>(AD + (size_t)(lo_pt + (q - 1) * KCK) * KAD, cl, rg);
                KKT_Y_ISSUE(q - 1)
            }
            // x_k = y_k - D~_k^-1 (Up_k x_(k+1)),  Up_k = Lo_(k+1)' (the Lo read one step earlier)
            double gr_c[5], lo_c[5], yk_c;
#pragma unroll
            for (int j = 0; j < 5; ++j) { gr_c[j] = ch[(KCK - 1) * KAD + ro[j]]; lo_c[j] = ch[(KCK - 1) * KAD + 15 + j]; }
            yk_c = aux[(KCK - 1) * 5 + rr_];
#pragma unroll
            for (int kk = KCK - 1; kk >= 0; --kk) {
                const int k = q * KCK + kk;
                const bool active = has && k < L;
                double gr_n[5], lo_n[5], yk_n = 0.0;
                if (kk > 0) {
#pragma unroll
                    for (int j = 0; j < 5; ++j) { gr_n[j] = ch[(kk - 1) * KAD + ro[j]]; lo_n[j] = ch[(kk - 1) * KAD + 15 + j]; }
                    yk_n = aux[(kk - 1) * 5 + rr_];
                }
                double xb[5], t[5];
                xb[0] = bcast_row16<0>(x); xb[1] = bcast_row16<1>(x); xb[2] = bcast_row16<2>(x); xb[3] = bcast_row16<3>(x); xb[4] = bcast_row16<4>(x);
                KKT_UP_APPLY(up_prev, xb, t);
                const double xn = yk_c - ((gr_c[0] * t[0] + gr_c[1] * t[1]) + (gr_c[2] * t[2] + gr_c[3] * t[3]) + gr_c[4] * t[4]);
                if (active) {
                    x = xn;
#pragma unroll
                    for (int j = 0; j < 5; ++j) up_prev[j] = lo_c[j];
                    const int m = lo_pt + k;
                    if (cl == 0) vv[m] = xn;
                    if (cl < 5) {
                        if (k == L - 1) x0s[5 + cl] = xn;
                        if (k == 0) x0s[cl] = xn;
                    }
                }
                if (kk > 0) {
#pragma unroll
                    for (int j = 0; j < 5; ++j) { gr_c[j] = gr_n[j]; lo_c[j] = lo_n[j]; }
                    yk_c = yk_n;
                }
            }
        }
    }
    __syncthreads();
    KT(4);

    // ---- the separators ----------------------------------------------------------------------------------------------------
    if (wv == 0) {
        double* rr = ovl + KO_RR;
        double* yr = ovl + KO_YR;
        if (lane < nseg) {
            const int j = lane, jp = j > 0 ? j - 1 : nseg - 1;
            const double* sp = per + KP_SEP + j * 10;
            const double lo[5] = {sp[0], sp[1], sp[2], sp[3], sp[4]};
            const double up[5] = {sp[5], sp[6], sp[7], sp[8], sp[9]};
            double xf[5], xl[5], t[5], u[5];
#pragma unroll
            for (int q = 0; q < 5; ++q) { xf[q] = per[KP_X0 + j * 10 + q]; xl[q] = per[KP_X0 + jp * 10 + 5 + q]; }
            if (c.chain && j == 0) {                    // open chain: Lo_0 = 0 (zero operand, as in factor_kkt)
#pragma unroll
                for (int q = 0; q < 5; ++q) xl[q] = 0.0;
            }
            KKT_UP_APPLY(up, xf, u);
            KKT_LO_APPLY(lo, xl, t);
            rr[j * 5 + 0] = vv[KSEP(j, n, nseg)] - u[0] - t[0];
#pragma unroll
            for (int q = 1; q < 5; ++q) rr[j * 5 + q] = -u[q] - t[q];
        }
        __builtin_amdgcn_wave_barrier();
        const double* r0i = per + KP_R0I + rr_ * 5;
        if (nseg == 1) {
            const double x0 = (r0i[0] * rr[0] + r0i[1] * rr[1]) + (r0i[2] * rr[2] + r0i[3] * rr[3]) + r0i[4] * rr[4];
            __builtin_amdgcn_wave_barrier();
            if (lane < 5) rr[lane] = x0;
        } else {
            const int LR = nseg - 1;
            // c_k = D_k^-1 r_(k+1) for all k at once (75 entries over the wave's 64 lanes), then the chain  y_k = c_k - M_k y_(k-1)
            // with the M_k = D_k^-1 RL_k the factorisation left in the step records
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int e = lane + 64 * q;
                if (e < LR * 5) {
                    const double* dr = per + KP_STEP + (e / 5) * 100 + (e % 5) * 5;
                    const double* rk = rr + (e / 5 + 1) * 5;
                    yr[e] = (dr[0] * rk[0] + dr[1] * rk[1]) + (dr[2] * rk[2] + dr[3] * rk[3]) + dr[4] * rk[4];
                }
            }
            __builtin_amdgcn_wave_barrier();
            double y = 0.0;
            for (int k = 0; k < LR; ++k) {
                const double* mr = per + KP_STEP + k * 100 + 50 + rr_ * 5;
                const double ck = yr[k * 5 + rr_];
                double yb[5];
                yb[0] = bcast_row16<0>(y); yb[1] = bcast_row16<1>(y); yb[2] = bcast_row16<2>(y); yb[3] = bcast_row16<3>(y); yb[4] = bcast_row16<4>(y);
                y = ck - ((mr[0] * yb[0] + mr[1] * yb[1]) + (mr[2] * yb[2] + mr[3] * yb[3]) + mr[4] * yb[4]);
                __builtin_amdgcn_wave_barrier();
                if (lane < 5) yr[k * 5 + lane] = y;
            }
            __builtin_amdgcn_wave_barrier();
            double x = 0.0;
            for (int k = LR - 1; k >= 0; --k) {
                const double* gr = per + KP_STEP + k * 100 + 25 + rr_ * 5;
                double xb[5];
                xb[0] = bcast_row16<0>(x); xb[1] = bcast_row16<1>(x); xb[2] = bcast_row16<2>(x); xb[3] = bcast_row16<3>(x); xb[4] = bcast_row16<4>(x);
                x = yr[k * 5 + rr_] - ((gr[0] * xb[0] + gr[1] * xb[1]) + (gr[2] * xb[2] + gr[3] * xb[3]) + gr[4] * xb[4]);
                __builtin_amdgcn_wave_barrier();
                if (lane < 5) yr[k * 5 + lane] = x;           // X0 of the separator chain
            }
            __builtin_amdgcn_wave_barrier();
            // separator 0
            double r0[5];
#pragma unroll
            for (int r = 0; r < 5; ++r) {
                double acc = rr[r];
#pragma unroll
                for (int j = 0; j < 5; ++j) acc -= per[KP_RU0 + r * 5 + j] * yr[j] + per[KP_RL0 + r * 5 + j] * yr[(LR - 1) * 5 + j];
                r0[r] = acc;
            }
            const double x0 = (r0i[0] * r0[0] + r0i[1] * r0[1]) + (r0i[2] * r0[2] + r0i[3] * r0[3]) + r0i[4] * r0[4];
            double x0b[5];
            x0b[0] = bcast_row16<0>(x0); x0b[1] = bcast_row16<1>(x0); x0b[2] = bcast_row16<2>(x0); x0b[3] = bcast_row16<3>(x0); x0b[4] = bcast_row16<4>(x0);
            __builtin_amdgcn_wave_barrier();
            if (lane < 5) rr[lane] = x0;
            // x_k = x'_k - XS_k x_0: independent entries, the wave's 64 lanes over the 5 (nseg - 1) of them (it had been a loop over k)
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int e = lane + 64 * q;
                if (e < LR * 5) {
                    const double* xs = per + KP_STEP + (e / 5) * 100 + 75 + (e % 5) * 5;
                    rr[5 + e] = yr[e] - ((xs[0] * x0b[0] + xs[1] * x0b[1]) + (xs[2] * x0b[2] + xs[3] * x0b[3]) + xs[4] * x0b[4]);
                }
            }
        }
    }
    __syncthreads();
    KT(5);

    // ---- alpha_m -= X^L_m xs_j + X^R_m xs_(j+1) ------------------------------------------------------------------------------------
    if (has) {
        const double* rr = ovl + KO_RR;
        const int gn = g + 1 < nseg ? g + 1 : 0;
        double xa[5], xb[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) { xa[q] = rr[g * 5 + q]; xb[q] = rr[gn * 5 + q]; }
#ifdef MCQ_PERTURB_ULP
        // Robustness experiment (docs/NOTEBOOK.md R4.6, kept as a build switch since round 5; scripts/build_variants.sh, the `-m gpu` test
        // test_arithmetic_variants_on_the_stadium): every solve's separator values off by one unit in the last place.  Nothing the solver
        // returns may depend on it beyond rounding.
        for (int q = 0; q < 5; ++q) { xa[q] *= 1.0 + 0x1p-52; xb[q] *= 1.0 + 0x1p-52; }
#endif
        if (cl == 0) vv[s0] = xa[0];
        // the spikes' columns 0 ride on columns 1 and 2 (KAS): X^L with lo3, lo4 of the segment's first waypoint, X^R with lo0 / lo2, lo1 / lo2
        // of the separator to the right
        if (L > 0) {
            const RG* adf = (const RG*)K_AD(c) + (size_t)lo_pt * KAD;
            const double* sr = per + KP_SEP + gn * 10;
            xa[1] = fma((double)adf[18], xa[0], xa[1]);
            xa[2] = fma((double)adf[19], xa[0], xa[2]);
            // (open chain, last segment: the right separator is waypoint 0, whose Lo is 0 -- 0 / 0 here.  X^R of that segment is identically
            //  zero (Up_(n-1) = 0 starts its recursion), so there is nothing to fold)
            if (!(c.chain && gn == 0)) {
                xb[1] = fma(sr[0] / sr[2], xb[0], xb[1]);
                xb[2] = fma(sr[1] / sr[2], xb[0], xb[2]);
            }
        }
#if MCQ_KKT_CORR_BATCH
        // A lane's waypoints k, k + 16, ... KKT_CB at a time: every load of the batch is issued before the first value is used, then the
        // accumulations, then the stores -- one round trip to memory per batch.  (One waypoint per trip, the stores to vv keep the next trip's
        // loads behind them: a trip per round trip, eight of them at L = 124.)  A trip past L loads the lane's first waypoint of the batch
        // and stores nothing.
        constexpr int KKT_CB = F32 ? KKT_CORR_TRIPS_F32 : KKT_CORR_TRIPS_F64;
        for (int k0 = cl; k0 < L; k0 += 16 * KKT_CB) {
            int idx[KKT_CB];
            bool ok[KKT_CB];
#pragma unroll
            for (int u = 0; u < KKT_CB; ++u) {
                ok[u] = k0 + 16 * u < L;
                idx[u] = lo_pt + (ok[u] ? k0 + 16 * u : k0);
            }
            RT as[KKT_CB][KAS];
            double acc[KKT_CB];
#pragma unroll
            for (int u = 0; u < KKT_CB; ++u) {
                const RG* src = AS + (size_t)idx[u] * KAS;
#pragma unroll
                for (int q = 0; q < KAS; ++q) as[u][q] = src[q];
                acc[u] = vv[idx[u]];
            }
#pragma unroll
            for (int u = 0; u < KKT_CB; ++u) {
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[u] -= (double)as[u][q] * xa[1 + q] + (double)as[u][4 + q] * xb[1 + q];
            }
#pragma unroll
            for (int u = 0; u < KKT_CB; ++u)
                if (ok[u]) vv[idx[u]] = acc[u];
        }
#else
        for (int k = cl; k < L; k += 16) {
            const int m = lo_pt + k;
            const RG* as = AS + (size_t)m * KAS;
            double acc = vv[m];
#pragma unroll
            for (int q = 0; q < 4; ++q) acc -= (double)as[q] * xa[1 + q] + (double)as[4 + q] * xb[1 + q];
            vv[m] = acc;
        }
#endif
    }
    __syncthreads();
    KT(6);
}
