// mcq_mtstep.inc -- the regularised primal-dual Newton step of the minimum-time NLP from its resident blocks (mcq_mintime_step_device; contract:
// include/mcq.h).  Part of the one translation unit (mcq_kernels.hip includes it after mcq_mintime.inc, whose helpers it uses).
//
//     K = [ H + diag(dw)   J^T      ]      H the sum of the Hessian blocks (overlaps added, block 0's slots 29 .. 32 on U_N-1), J the Jacobian blocks'
//         [ J             -diag(dg) ]      row slots, the periodicity rows and the energy row -- mintime.kkt_matrix assembles the same matrix.
//
// ELIMINATION: a multifrontal LDL^T without pivoting in ONE static order, a front per interval.  Front k assembles block k of H and of J and
// eliminates what no later block touches, in this order:
//     U_k-1 (4), X_k (5), Xc_k,0..2 (15)     their diagonals dw enter here
//     the 13 path-row slots of interval k - 1  (rows at X_k with U_k-1: every variable they read is eliminated by now)
//     the 20 collocation and continuity rows of interval k
// and passes on a Schur complement of 37: [U_k (4), X_k+1 (5), the 13 path-row slots of interval k | the border: X_0 (5), U_N-1 (4), the 5
// periodicity rows, the energy row].  A row is never a pivot before the variables it reads have been pivots (a path row pivoted in its own
// interval's front would have the pivot -dg alone: 1e-8 on the roll-moment row).  Front 0 has no predecessor: X_0 and the wrap of block 0's slots
// 29 .. 32 (U_N-1) go to the border, its 22 first pivots are placeholders.  In the last front U_k IS the border's U_N-1; after its 57 pivots the
// remaining 37 are eliminated in place: X_N, the path rows of interval N - 1, X_0, U_N-1, the periodicity rows, the energy row.  N = 2 needs no case.
// A placeholder (front 0's predecessor, an absent actuator or safe slot, the energy row where disabled) is a pivot 1 with an empty column and is not
// counted.  The front is 94 x 94, lower triangle packed: 4465 doubles of LDS; one barrier per pivot; the trailing update is spread over the 256
// lanes by packed index (a lane's 18 entries are the same in every front and live in registers).
// FACTOR KEPT: per interval the 94 x 57 panel of L (unit diagonal replaced by D), row-major, and the last 37 x 37 -- 42.9 KB per interval.
// SOLVES: the panel of a front is staged in LDS once per sweep; each of the four waves carries ONE right-hand side in registers (a lane holds
// entries `lane` and `64 + lane` of the front's vector, the pivots' values travel by __shfl), so up to four right-hand sides share a sweep.
// REFINEMENT: r = rhs - K x in float64 from the blocks, a lane per unknown in one fixed order (fused multiply-adds), the dense energy row by a tree.
// Every sum's order depends on the problem's own N alone.
// THE NLP'S STRUCTURE is mcq_kernels.h's (mcq_mt_row_of, mcq_mt_slot_of, mcq_mt_holders, mcq_mt_slot_entry, mcq_mt_sizes): what is stated here is the
// front alone -- the positions (mts_var_pos, mts_row_pos), the unknowns behind them (mts_own_unknown, mts_fin_unknown), the diagonals (mts_diag).

#define MTS_OWN 57
#define MTS_F 94
#define MTS_TAIL 37
#define MTS_TRI (MTS_F * (MTS_F + 1) / 2)
#define MTS_ELEMS ((MTS_TRI + MCQ_NT - 1) / MCQ_NT)

// the problem's sizes, and where the multiplier part of this launch's [nwmax + ngmax] vectors begins
struct MtsDims : McqMtSizes {
    int nwmax;
};
// f(i) for every entry i of such a vector that is the problem's own: the w part, then the multiplier part, each spread over the lanes from 0
template <class F>
__device__ __forceinline__ void mts_each_own(const MtsDims& D, F f)
{
    for (int i = threadIdx.x; i < D.nw; i += MCQ_NT) f(i);
    for (int i = threadIdx.x; i < D.ng; i += MCQ_NT) f(D.nwmax + i);
}

__device__ __forceinline__ int mts_tri(int i) { return i * (i + 1) / 2; }
// the row of entry e of a packed lower triangle
__device__ __forceinline__ int mts_tri_row(int e)
{
    int i = (int)((sqrt(8.0 * e + 1.0) - 1.0) * 0.5);
    while (mts_tri(i + 1) <= e) ++i;
    while (mts_tri(i) > e) --i;
    return i;
}

// the entry of the solution vector behind row slot r of interval k, or -1 where the slot is absent
__device__ __forceinline__ int mts_row_unknown(const MtsDims& D, int k, int r)
{
    const int row = mcq_mt_row_of(k, D.safe, r);
    return row < 0 ? -1 : D.nwmax + row;
}
// the entry behind pivot p (0 .. 56) of front k, or -1 for a placeholder
__device__ __forceinline__ int mts_own_unknown(const MtsDims& D, int k, int p)
{
    if (p < 4) return k > 0 ? 24 * (k - 1) + 5 + p : -1;
    if (p < 9) return k > 0 ? 24 * k + (p - 4) : -1;
    if (p < 24) return 24 * k + p;
    if (p < 37) return k > 0 ? mts_row_unknown(D, k - 1, 20 + (p - 24)) : -1;
    return D.nwmax + mcq_mt_row0(k, D.safe) + (p - 37);
}
// the entry behind position p (57 .. 93) of the LAST front, or -1 for a placeholder
__device__ __forceinline__ int mts_fin_unknown(const MtsDims& D, int p)
{
    if (p < 61) return -1;
    if (p < 66) return 24 * D.N + (p - 61);
    if (p < 79) return mts_row_unknown(D, D.N - 1, 20 + (p - 66));
    if (p < 84) return p - 79;
    if (p < 88) return 24 * (D.N - 1) + 5 + (p - 84);
    if (p < 93) return D.nwmax + D.per + (p - 88);
    return D.energy ? D.nwmax + D.per + 5 : -1;
}
// the front position of column slot s (0 .. 32) of block k
__device__ __forceinline__ int mts_var_pos(const MtsDims& D, int k, int s)
{
    if (s < 5) return k > 0 ? 4 + s : 79 + s;
    if (s < 9) return k == D.N - 1 ? 84 + (s - 5) : 57 + (s - 5);
    if (s < 24) return s;
    if (s < 29) return 61 + (s - 24);
    return k > 0 ? s - 29 : 84 + (s - 29);
}
__device__ __forceinline__ int mts_row_pos(int r) { return r < 20 ? 37 + r : 66 + (r - 20); }

// what front k adds on the diagonal at position p beside the blocks' entries and what it inherits
__device__ __forceinline__ double mts_diag(const MtsDims& D, int k, int p, const double* dw, const double* dg)
{
    const bool last = k == D.N - 1;
    if (p < 24) { const int u = mts_own_unknown(D, k, p); return u < 0 ? 1.0 : dw[u]; }
    if (p < 37) return k == 0 ? 1.0 : 0.0;
    if (p < 57) return -dg[mcq_mt_row0(k, D.safe) + (p - 37)];
    if (p >= 66 && p < 79) { const int u = mts_row_unknown(D, k, 20 + (p - 66)); return u < 0 ? 1.0 : -dg[u - D.nwmax]; }
    if (!last) return 0.0;
    const int u = mts_fin_unknown(D, p);
    return u < 0 ? 1.0 : (u < D.nwmax ? dw[u] : -dg[u - D.nwmax]);
}
// the variable whose column of the energy row enters at position p of front k (where its dw enters), or -1
__device__ __forceinline__ int mts_energy_var(const MtsDims& D, int k, int p)
{
    if (p < 24) return mts_own_unknown(D, k, p);
    if (k == D.N - 1 && ((p >= 61 && p < 66) || (p >= 79 && p < 88))) return mts_fin_unknown(D, p);
    return -1;
}

struct MtsLane {
    int at[MTS_ELEMS];       // per packed entry of the lane: row's triangle offset | column << 16 (-1: none)
    int tc[MTS_ELEMS];       // the column's triangle offset
};

// pivots j0 .. j1 - 1 of the packed front F; counts the signs; false at a pivot that is zero or not finite (the same on every lane)
__device__ bool mts_eliminate(double* F, const MtsLane& L, const MtsDims& D, int k, int j0, int j1, int* inertia)
{
    const int tid = threadIdx.x;
    for (int j = j0; j < j1; ++j) {
        const double d = F[mts_tri(j) + j];
        if (!(d - d == 0.0) || d == 0.0) return false;
        const bool placeholder = j < MTS_OWN ? (j < 24 || j >= 37 ? mts_own_unknown(D, k, j) < 0 : (k == 0 || mts_row_unknown(D, k - 1, 20 + (j - 24)) < 0))
                                             : mts_fin_unknown(D, j) < 0;
        if (!placeholder) inertia[d > 0.0 ? 0 : 1] += 1;
        const double rinv = 1.0 / d;
#pragma unroll
        for (int q = 0; q < MTS_ELEMS; ++q) {
            const int a = L.at[q], c = a >> 16;
            if (a >= 0 && c > j) {
                const int e = tid + MCQ_NT * q;
                F[e] = fma(-F[(a & 0xffff) + j], F[L.tc[q] + j] * rinv, F[e]);
            }
        }
        __syncthreads();
    }
    return true;
}

struct MtsVec {
    double v0, v1;           // entries `lane` and `64 + lane` of the front's vector
};
__device__ __forceinline__ double mts_get(const MtsVec& V, int p)
{
    const double a = __shfl(V.v0, p & 63), b = __shfl(V.v1, p & 63);
    return p < 64 ? a : b;
}

// K x = b in place for the right-hand sides x[t], t = t0 + wave, from the factor in `work`; every lane of the workgroup takes part
__device__ void mts_solve(const McqMtStep& S, const MtsDims& D, const double* work, double* x, size_t stride, double* s_buf, double* s_fin)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, N = D.N;
    const int panel = MTS_F * MTS_OWN;
    const double* fin = work + (size_t)S.nmax * panel;
    for (int t0 = 0; t0 < S.nvec; t0 += MCQ_NT / 64) {
        const bool on = t0 + wave < S.nvec;
        double* xv = x + (size_t)(on ? t0 + wave : 0) * stride;
        MtsVec V;
        V.v0 = 0.0; V.v1 = 0.0;
        // forward: L y = b, front after front
        for (int k = 0; k < N; ++k) {
            __syncthreads();
            for (int e = tid; e < panel; e += MCQ_NT) s_buf[e] = work[(size_t)k * panel + e];
            if (k == N - 1)
                for (int e = tid; e < MTS_TAIL * MTS_TAIL; e += MCQ_NT) s_fin[e] = fin[e];
            __syncthreads();
            if (!on) continue;
            // what the previous front passed on moves to its place: U_k-1 / X_k, the path rows, the border
            const int sp = lane < 9 ? 57 + lane : (lane >= 24 && lane < 37 ? 66 + (lane - 24) : 0);
            const double moved = mts_get(V, sp);
            const int u = lane < MTS_OWN ? mts_own_unknown(D, k, lane) : -1;
            V.v0 = (k > 0 && (lane < 9 || (lane >= 24 && lane < 37)) ? moved : 0.0) + (u >= 0 ? xv[u] : 0.0);
            V.v1 = k > 0 && lane >= 15 ? V.v1 : 0.0;
            for (int j = 0; j < MTS_OWN; ++j) {
                const double vj = __shfl(V.v0, j);
                if (lane > j) V.v0 = fma(-s_buf[lane * MTS_OWN + j], vj, V.v0);
                if (lane < MTS_F - 64) V.v1 = fma(-s_buf[(64 + lane) * MTS_OWN + j], vj, V.v1);
            }
            if (u >= 0) xv[u] = V.v0;
        }
        if (on) {
            // the last 37: their right-hand sides, L y = b, D, L^T x = y
            const int p0 = lane, p1 = 64 + lane;
            const int u0 = p0 >= MTS_OWN ? mts_fin_unknown(D, p0) : -1, u1 = p1 < MTS_F ? mts_fin_unknown(D, p1) : -1;
            if (u0 >= 0) V.v0 += xv[u0];
            if (u1 >= 0) V.v1 += xv[u1];
            for (int j = MTS_OWN; j < MTS_F; ++j) {
                const double vj = mts_get(V, j);
                if (p0 > j) V.v0 = fma(-s_fin[(p0 - MTS_OWN) * MTS_TAIL + (j - MTS_OWN)], vj, V.v0);
                if (p1 > j && p1 < MTS_F) V.v1 = fma(-s_fin[(p1 - MTS_OWN) * MTS_TAIL + (j - MTS_OWN)], vj, V.v1);
            }
            if (p0 >= MTS_OWN) V.v0 = V.v0 / s_fin[(p0 - MTS_OWN) * (MTS_TAIL + 1)];
            if (p1 < MTS_F) V.v1 = V.v1 / s_fin[(p1 - MTS_OWN) * (MTS_TAIL + 1)];
            for (int i = MTS_F - 1; i > MTS_OWN; --i) {
                const double xi = mts_get(V, i);
                if (p0 >= MTS_OWN && p0 < i) V.v0 = fma(-s_fin[(i - MTS_OWN) * MTS_TAIL + (p0 - MTS_OWN)], xi, V.v0);
                if (p1 < i) V.v1 = fma(-s_fin[(i - MTS_OWN) * MTS_TAIL + (p1 - MTS_OWN)], xi, V.v1);
            }
            if (u0 >= 0) xv[u0] = V.v0;
            if (u1 >= 0) xv[u1] = V.v1;
        }
        // backward: D^-1, L^T x = y, the fronts in falling order (the last front's panel is still staged)
        for (int k = N - 1; k >= 0; --k) {
            if (k < N - 1) {
                __syncthreads();
                for (int e = tid; e < panel; e += MCQ_NT) s_buf[e] = work[(size_t)k * panel + e];
                __syncthreads();
            }
            if (!on) continue;
            const int u = lane < MTS_OWN ? mts_own_unknown(D, k, lane) : -1;
            double z = lane < MTS_OWN ? (u >= 0 ? xv[u] : 0.0) / s_buf[lane * (MTS_OWN + 1)] : 0.0;
            for (int i = MTS_OWN; i < MTS_F; ++i) {
                const double xi = mts_get(V, i);
                if (lane < MTS_OWN) z = fma(-s_buf[i * MTS_OWN + lane], xi, z);
            }
            for (int i = MTS_OWN - 1; i > 0; --i) {
                const double xi = __shfl(z, i);
                if (lane < i) z = fma(-s_buf[i * MTS_OWN + lane], xi, z);
            }
            if (u >= 0) xv[u] = z;
            // this front's U_k-1 / X_k and path rows are what front k - 1 passed on
            const int p1 = 64 + lane;
            const int from0 = lane - 57, from1 = p1 < 66 ? p1 - 57 : 24 + (p1 - 66);
            const double a0 = __shfl(z, from0 & 63), a1 = __shfl(z, from1 & 63);
            if (lane >= MTS_OWN) V.v0 = a0;
            if (lane < 15) V.v1 = a1;
        }
    }
    __syncthreads();
}

// r = b - K x for every right-hand side, float64, from the blocks; res[t] = max |r| (NaN kept).  r may be NULL (the norm alone).
__device__ void mts_residual(const McqMtStep& S, const MtsDims& D, int b, const double* x, const double* rhs, double* r, size_t stride, double* res,
                             double* s_red)
{
    const int tid = threadIdx.x, N = D.N, nmax = S.nmax, nn = MCQ_MT_BLOCK * MCQ_MT_BLOCK;
    const double* hb = S.hblocks + (size_t)b * nmax * nn;
    const double* jb = S.blocks + (size_t)b * nmax * nn;
    const double* dw = S.dw + (size_t)b * S.nwmax;
    const double* dg = S.dg + (size_t)b * S.ngmax;
    const double* ge = D.energy ? S.grad_energy + (size_t)b * S.nwmax : nullptr;
    for (int t = 0; t < S.nvec; ++t) {
        const double* xv = x + (size_t)t * stride;
        const double* lam = xv + D.nwmax;
        const double* bv = rhs + (size_t)t * stride;
        double* rv = r ? r + (size_t)t * stride : nullptr;
        double rmax = 0.0, esum = 0.0;
        for (int i = tid; i < D.nw; i += MCQ_NT) {
            const int k = i / 24, c = i - 24 * k;
            // up to two blocks hold the entry: (block of H, slot), (block of J, slot)
            int hk[2], hs[2], jk[2], js[2];
            mcq_mt_holders(N, i, true, hk, hs);
            mcq_mt_holders(N, i, false, jk, js);
            double acc = dw[i] * xv[i];
            for (int s = 0; s < 2; ++s) {
                if (hk[s] < 0) continue;
                const double* row = hb + (size_t)hk[s] * nn + hs[s] * MCQ_MT_BLOCK;
                const double* vk = xv + mcq_mt_slot_entry(N, hk[s], 0);
                const double* vu = xv + mcq_mt_slot_entry(N, hk[s], 29);
                for (int a = 0; a < 29; ++a) acc = fma(row[a], vk[a], acc);
                for (int a = 0; a < 4; ++a) acc = fma(row[29 + a], vu[a], acc);
            }
            for (int s = 0; s < 2; ++s) {
                if (jk[s] < 0) continue;
                const double* col = jb + (size_t)jk[s] * nn + js[s];
                const double* lk = lam + mcq_mt_row0(jk[s], D.safe);
                for (int rr = 0; rr < MCQ_MT_ROWS_ALWAYS; ++rr) acc = fma(col[rr * MCQ_MT_BLOCK], lk[rr], acc);
                for (int rr = MCQ_MT_ROWS_ALWAYS; rr < MCQ_MT_BLOCK; ++rr) {
                    const int off = mcq_mt_row_off(jk[s], D.safe, rr);
                    if (off >= 0) acc = fma(col[rr * MCQ_MT_BLOCK], lk[off], acc);
                }
            }
            if (c < 5 && k == 0) acc += lam[D.per + c];
            if (c < 5 && k == N) acc -= lam[D.per + c];
            if (ge) {
                acc = fma(ge[i], lam[D.per + 5], acc);
                esum = fma(ge[i], xv[i], esum);
            }
            const double ri = bv[i] - acc;
            if (rv) rv[i] = ri;
            rmax = mt_nanmax(rmax, fabs(ri));
        }
        for (int i = tid; i < D.per + 5; i += MCQ_NT) {
            double acc = -(dg[i] * lam[i]);
            if (i >= D.per) {
                acc += xv[i - D.per] - xv[24 * (size_t)N + (i - D.per)];
            } else {
                int k, s;
                mcq_mt_slot_of(i, D.safe, &k, &s);
                const double* row = jb + (size_t)k * nn + s * MCQ_MT_BLOCK;
                const double* vk = xv + mcq_mt_slot_entry(N, k, 0);
                const double* vu = xv + mcq_mt_slot_entry(N, k, 29);
                for (int a = 0; a < 29; ++a) acc = fma(row[a], vk[a], acc);
                if (k > 0)      // (the Jacobian's block 0 has no slots 29 .. 32)
                    for (int a = 0; a < 4; ++a) acc = fma(row[29 + a], vu[a], acc);
            }
            const double ri = bv[D.nwmax + i] - acc;
            if (rv) rv[D.nwmax + i] = ri;
            rmax = mt_nanmax(rmax, fabs(ri));
        }
        if (ge) {
            // the dense row: lane t adds its entries in rising order, then the tree
            const double e = mt_tree<mt_add>(esum, s_red);
            if (tid == 0) {
                const int i = D.per + 5;
                const double ri = bv[D.nwmax + i] - (e - dg[i] * lam[i]);
                if (rv) rv[D.nwmax + i] = ri;
                rmax = mt_nanmax(rmax, fabs(ri));
            }
        }
        rmax = mt_tree<mt_nanmax>(rmax, s_red);
        if (tid == 0) res[t] = rmax;
    }
    __syncthreads();
}

// this problem gets no solution (refused, or a pivot failed): NaN in all of its sol and res
__device__ void mts_no_solution(const McqMtStep& S, double* sol, double* res, size_t stride)
{
    for (size_t e = threadIdx.x; e < S.nvec * stride; e += MCQ_NT) sol[e] = NAN;
    for (int t = threadIdx.x; t < S.nvec; t += MCQ_NT) res[t] = NAN;
}

// ---- a workgroup per problem: check, factor, solve, refine ----
__global__ void __launch_bounds__(MCQ_NT) mcq_mintime_step_kernel(McqMtStep S)
{
    __shared__ double s_buf[MTS_F * MTS_OWN];      // the packed front while factoring (4465), a front's panel while solving
    __shared__ double s_aux[MTS_TAIL * MTS_TAIL];  // the Schur complement passed on (703 packed), the last 37 x 37 while solving
    __shared__ double s_red[MCQ_NT];
    const int b = blockIdx.x, tid = threadIdx.x, nmax = S.nmax, nn = MCQ_MT_BLOCK * MCQ_MT_BLOCK;
    const MtsDims D = {mcq_mt_sizes(S.n_list, nmax, b, S.safe, S.energy), S.nwmax};
    const int N = D.N;
    const size_t stride = (size_t)S.nwmax + S.ngmax;
    const double* hb = S.hblocks + (size_t)b * nmax * nn;
    const double* jb = S.blocks + (size_t)b * nmax * nn;
    const double* dw = S.dw + (size_t)b * S.nwmax;
    const double* dg = S.dg + (size_t)b * S.ngmax;
    const double* ge = S.energy ? S.grad_energy + (size_t)b * S.nwmax : nullptr;
    const double* rhs = S.rhs + (size_t)b * S.nvec * stride;
    double* sol = S.sol + (size_t)b * S.nvec * stride;
    double* res = S.res + (size_t)b * S.nvec;
    double* work = S.work + (size_t)b * S.work_per;
    double* rbuf = work + (size_t)nmax * (MTS_F * MTS_OWN) + MTS_TAIL * MTS_TAIL;
    // every input inside the problem's own extent is finite
    double chk = 0.0;
    for (size_t e = tid; e < (size_t)N * nn; e += MCQ_NT) chk += mt_chk(hb[e]) + mt_chk(jb[e]);
    for (int i = tid; i < D.nw; i += MCQ_NT) chk += mt_chk(dw[i]) + (ge ? mt_chk(ge[i]) : 0.0);
    for (int i = tid; i < D.ng; i += MCQ_NT) chk += mt_chk(dg[i]);
    for (int t = 0; t < S.nvec; ++t) mts_each_own(D, [&](int i) { chk += mt_chk(rhs[t * stride + i]); });
    chk = mt_tree<mt_add>(chk, s_red);
    const bool ok = N && chk == 0.0;
    // NaN past the problem's own entries (everywhere for a refused problem); inside them the solution starts as the right-hand side
    mts_no_solution(S, sol, res, stride);
    if (!ok) {
        if (tid < 3) S.inertia[3 * (size_t)b + tid] = -1;
        if (tid == 0) S.status[b] = MCQ_BAD_INPUT;
        return;
    }
    __syncthreads();
    for (int t = 0; t < S.nvec; ++t) mts_each_own(D, [&](int i) { sol[t * stride + i] = rhs[t * stride + i]; });
    // ---- the factorisation ----
    MtsLane L;
#pragma unroll
    for (int q = 0; q < MTS_ELEMS; ++q) {
        const int e = tid + MCQ_NT * q, i = mts_tri_row(e), c = e - mts_tri(i);
        L.at[q] = e < MTS_TRI ? (mts_tri(i) | (c << 16)) : -1;
        L.tc[q] = mts_tri(c);
    }
    int inertia[2] = {0, 0};
    bool regular = true;
    for (int k = 0; k < N && regular; ++k) {
        const bool last = k == N - 1;
        // what the front inherits, its diagonals, the energy row's columns, the periodicity rows' constants
        for (int e = tid; e < MTS_TRI; e += MCQ_NT) {
            const int i = mts_tri_row(e), c = e - mts_tri(i);
            const int qi = i < 9 ? i : (i >= 24 && i < 37 ? 9 + (i - 24) : (i >= 79 ? 22 + (i - 79) : -1));
            const int qc = c < 9 ? c : (c >= 24 && c < 37 ? 9 + (c - 24) : (c >= 79 ? 22 + (c - 79) : -1));
            double v = k > 0 && qi >= 0 && qc >= 0 ? s_aux[mts_tri(qi) + qc] : 0.0;
            if (i == c) v += mts_diag(D, k, i, dw, dg);
            if (i == MTS_F - 1 && ge && c != i) { const int u = mts_energy_var(D, k, c); if (u >= 0) v += ge[u]; }
            if (last && i >= 88 && i < 93) v += c == 79 + (i - 88) ? 1.0 : (c == 61 + (i - 88) ? -1.0 : 0.0);
            s_buf[e] = v;
        }
        __syncthreads();
        // block k of H: the lower triangle in the front's order
        for (int e = tid; e < nn; e += MCQ_NT) {
            const int r = e / MCQ_MT_BLOCK, c = e - MCQ_MT_BLOCK * r, pr = mts_var_pos(D, k, r), pc = mts_var_pos(D, k, c);
            if (pr > pc || r == c) s_buf[mts_tri(pr) + pc] += hb[(size_t)k * nn + e];
        }
        __syncthreads();
        // block k of J: the row slots that exist against the column slots that exist
        for (int e = tid; e < nn; e += MCQ_NT) {
            const int r = e / MCQ_MT_BLOCK, c = e - MCQ_MT_BLOCK * r;
            if (mcq_mt_row_off(k, D.safe, r) < 0 || (k == 0 && c >= 29)) continue;
            const int pr = mts_row_pos(r), pc = mts_var_pos(D, k, c), hi = pr > pc ? pr : pc, lo = pr > pc ? pc : pr;
            s_buf[mts_tri(hi) + lo] += jb[(size_t)k * nn + e];
        }
        __syncthreads();
        regular = mts_eliminate(s_buf, L, D, k, 0, last ? MTS_F : MTS_OWN, inertia);
        if (!regular) break;
        // keep the panel: L below D, row-major [94][57]; then the last 37 x 37, or pass the Schur complement on
        double* pk = work + (size_t)k * (MTS_F * MTS_OWN);
        for (int e = tid; e < MTS_F * MTS_OWN; e += MCQ_NT) {
            const int i = e / MTS_OWN, j = e - MTS_OWN * i;
            pk[e] = i > j ? s_buf[mts_tri(i) + j] * (1.0 / s_buf[mts_tri(j) + j]) : (i == j ? s_buf[mts_tri(j) + j] : 0.0);
        }
        if (last) {
            double* fin = work + (size_t)nmax * (MTS_F * MTS_OWN);
            for (int e = tid; e < MTS_TAIL * MTS_TAIL; e += MCQ_NT) {
                const int i = MTS_OWN + e / MTS_TAIL, j = MTS_OWN + e % MTS_TAIL;
                fin[e] = i > j ? s_buf[mts_tri(i) + j] * (1.0 / s_buf[mts_tri(j) + j]) : (i == j ? s_buf[mts_tri(j) + j] : 0.0);
            }
        } else {
            for (int e = tid; e < MTS_TAIL * (MTS_TAIL + 1) / 2; e += MCQ_NT) {
                const int i = mts_tri_row(e);
                s_aux[e] = s_buf[mts_tri(MTS_OWN + i) + MTS_OWN + (e - mts_tri(i))];
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        S.inertia[3 * (size_t)b] = inertia[0];
        S.inertia[3 * (size_t)b + 1] = inertia[1];
        S.inertia[3 * (size_t)b + 2] = regular ? 0 : 1;
        S.status[b] = regular ? MCQ_OK : MCQ_SINGULAR;
    }
    if (!regular) {
        __syncthreads();
        mts_no_solution(S, sol, res, stride);
        return;
    }
    // ---- solve, refine ----
    mts_solve(S, D, work, sol, stride, s_buf, s_aux);
    for (int it = 0; it < S.refine; ++it) {
        mts_residual(S, D, b, sol, rhs, rbuf, stride, res, s_red);
        mts_solve(S, D, work, rbuf, stride, s_buf, s_aux);
        for (int t = 0; t < S.nvec; ++t) mts_each_own(D, [&](int i) { sol[t * stride + i] += rbuf[t * stride + i]; });
        __syncthreads();
    }
    mts_residual(S, D, b, sol, rhs, nullptr, stride, res, s_red);
}
