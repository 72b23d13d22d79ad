// mcq_mintime.inc -- the minimum-time optimal-control problem as functions of a decision vector (mcq_mintime_*_device; layouts and edges:
// include/mcq.h) [REF opt_mintime_traj/src/opt_mintime.py:143-861].  Part of the one translation unit (mcq_kernels.hip includes it).
//
// THE MODEL, ONCE: mt_model is the reference's double-track model (:284-441) as a function template over a scalar type T, instantiated with double
// (mcq_mintime_eval_kernel), with MtDual, a dual number of a value and ONE tangent (mcq_mintime_jac_kernel), and with MtHyper, a hyper-dual number
// of a value, two tangents and their mixed term (mcq_mintime_hess_kernel).  Statement order follows the
// reference's expressions from left to right; the compiler may contract a * b + c.
//
// LANE MAPPINGS.  Evaluation: one lane per (interval k, evaluation point p): p = 0 .. 2 the collocation points (f_dyn at Xc_k,p with U_k), p = 3 the
// path point (tire forces and accelerations at X_k+1 with U_k) -- four adjacent lanes of one wave, which exchange the three quadrature terms by
// __shfl.  Jacobian: one lane per (k, p, direction d): d = 0 .. 4 a state of the point, d = 5 .. 8 a control -- 36 lanes per interval, each one model
// evaluation with a single tangent, the value part recomputed.  A dual number that carried all 9 tangents in one lane would hold 10 doubles per live
// intermediate (the model has about 40 of them live at the slip angles: 400 doubles against 512 registers of 32 bits, i.e. 256 doubles); one tangent
// keeps the live set at twice the scalar model's, and a block's column slots become adjacent lanes' stores.  docs/NOTEBOOK.md "Mintime evaluation"
// records the registers the compiler reports.
//
// Hessian of the Lagrangian (mcq_mintime_hess_kernel): one workgroup of 192 lanes per interval, one lane per (evaluation point p, unordered pair
// of directions a <= b): 4 x 45 = 180 lanes, each ONE model evaluation with MtHyper, a hyper-dual number (value, two tangents, the mixed term).  Per
// point only one scalar needs second derivatives -- the multiplier-weighted sum of the point's rows plus its quadrature share -- so a lane reduces
// its rows' mixed terms to one double in LDS; after a barrier the 192 lanes store the block's 1089 entries in row-major order, each entry a pure
// function of its unordered slot pair (so (r, c) and (c, r) carry the same bits), one writer each, no zero-fill pass.  docs/NOTEBOOK.md "Mintime
// Hessian" records the mappings compiled and their registers.
//
// THE STRUCTURE, ONCE: which row of g a row slot of an interval is (and back), which blocks and column slots hold an entry of w, which entry is behind
// a column slot, and a problem's own sizes are mcq_kernels.h's mcq_mt_row_off / mcq_mt_row_of, mcq_mt_slot_of, mcq_mt_holders, mcq_mt_slot_entry and
// mcq_mt_sizes (mt_sizes here; mt_intervals for N alone).  A walk over an interval's rows takes the slots in rising order and skips the absent ones
// (evaluation); the certificate takes the MCQ_MT_ROWS_ALWAYS slots every interval has in a loop of their own and asks the map once per group behind
// them, which is what keeps it at 128 VGPRs (docs/NOTEBOOK.md "Mintime kernels: the NLP's row, slot and block maps").  The Jacobian and Hessian
// kernels sit at the end of the register file: they take N from mt_intervals and keep their bodies; the Hessian kernel's k > 0 / safe tests stay by
// hand.  The kernels share these indices, not their sums: every dot product stays where it is, spelled as it is (acc += a * b here).
//
// CasADi's interpolant is NOT pinned bit for bit: curvature at collocation point j is kappa_cl[k] + tau_j * (kappa_cl[k + 1] - kappa_cl[k]).

#define MT_VS 50.0
#define MT_BETAS 0.5
#define MT_NS 5.0
#define MT_DELTAS 0.5
#define MT_FDS 7500.0
#define MT_FBS 20000.0
#define MT_GYS 5000.0

struct MtDual {
    double v, d;
};
__device__ __forceinline__ MtDual mt_dual(double v, double d) { MtDual r; r.v = v; r.d = d; return r; }
__device__ __forceinline__ MtDual operator+(MtDual a, MtDual b) { return mt_dual(a.v + b.v, a.d + b.d); }
__device__ __forceinline__ MtDual operator-(MtDual a, MtDual b) { return mt_dual(a.v - b.v, a.d - b.d); }
__device__ __forceinline__ MtDual operator*(MtDual a, MtDual b) { return mt_dual(a.v * b.v, a.d * b.v + a.v * b.d); }
__device__ __forceinline__ MtDual operator/(MtDual a, MtDual b) { const double q = a.v / b.v; return mt_dual(q, (a.d - q * b.d) / b.v); }
__device__ __forceinline__ MtDual operator+(MtDual a, double b) { return mt_dual(a.v + b, a.d); }
__device__ __forceinline__ MtDual operator+(double a, MtDual b) { return mt_dual(a + b.v, b.d); }
__device__ __forceinline__ MtDual operator-(MtDual a, double b) { return mt_dual(a.v - b, a.d); }
__device__ __forceinline__ MtDual operator-(double a, MtDual b) { return mt_dual(a - b.v, -b.d); }
__device__ __forceinline__ MtDual operator*(MtDual a, double b) { return mt_dual(a.v * b, a.d * b); }
__device__ __forceinline__ MtDual operator*(double a, MtDual b) { return mt_dual(a * b.v, a * b.d); }
__device__ __forceinline__ MtDual operator/(MtDual a, double b) { return mt_dual(a.v / b, a.d / b); }
__device__ __forceinline__ MtDual operator-(MtDual a) { return mt_dual(-a.v, -a.d); }
__device__ __forceinline__ double mt_sin(double x) { return sin(x); }
__device__ __forceinline__ double mt_cos(double x) { return cos(x); }
__device__ __forceinline__ double mt_atan(double x) { return atan(x); }
__device__ __forceinline__ double mt_exp(double x) { return exp(x); }
__device__ __forceinline__ double mt_pos(double x) { return fmax(x, 0.0); }
__device__ __forceinline__ double mt_neg(double x) { return fmin(x, 0.0); }
__device__ __forceinline__ MtDual mt_sin(MtDual x) { return mt_dual(sin(x.v), cos(x.v) * x.d); }
__device__ __forceinline__ MtDual mt_cos(MtDual x) { return mt_dual(cos(x.v), -sin(x.v) * x.d); }
__device__ __forceinline__ MtDual mt_atan(MtDual x) { return mt_dual(atan(x.v), x.d / (1.0 + x.v * x.v)); }
__device__ __forceinline__ MtDual mt_exp(MtDual x) { const double e = exp(x.v); return mt_dual(e, e * x.d); }
__device__ __forceinline__ MtDual mt_pos(MtDual x) { return x.v > 0.0 ? x : mt_dual(x.v != x.v ? x.v : 0.0, x.v != x.v ? x.v : 0.0); }
__device__ __forceinline__ MtDual mt_neg(MtDual x) { return x.v < 0.0 ? x : mt_dual(x.v != x.v ? x.v : 0.0, x.v != x.v ? x.v : 0.0); }
__device__ __forceinline__ double mt_val(double x) { return x; }
__device__ __forceinline__ double mt_val(MtDual x) { return x.v; }
__device__ __forceinline__ double mt_tan(double) { return 0.0; }
__device__ __forceinline__ double mt_tan(MtDual x) { return x.d; }

// a hyper-dual number: value, the tangents along two directions a and b, and the mixed second derivative
struct MtHyper {
    double v, a, b, ab;
};
__device__ __forceinline__ MtHyper mt_hyper(double v, double a, double b, double ab) { MtHyper r; r.v = v; r.a = a; r.b = b; r.ab = ab; return r; }
__device__ __forceinline__ MtHyper operator+(MtHyper x, MtHyper y) { return mt_hyper(x.v + y.v, x.a + y.a, x.b + y.b, x.ab + y.ab); }
__device__ __forceinline__ MtHyper operator-(MtHyper x, MtHyper y) { return mt_hyper(x.v - y.v, x.a - y.a, x.b - y.b, x.ab - y.ab); }
__device__ __forceinline__ MtHyper operator*(MtHyper x, MtHyper y)
{
    return mt_hyper(x.v * y.v, x.a * y.v + x.v * y.a, x.b * y.v + x.v * y.b, x.ab * y.v + x.a * y.b + x.b * y.a + x.v * y.ab);
}
__device__ __forceinline__ MtHyper operator/(MtHyper x, MtHyper y)
{
    const double q = x.v / y.v, qa = (x.a - q * y.a) / y.v, qb = (x.b - q * y.b) / y.v;
    return mt_hyper(q, qa, qb, (x.ab - qa * y.b - qb * y.a - q * y.ab) / y.v);
}
__device__ __forceinline__ MtHyper operator+(MtHyper x, double y) { return mt_hyper(x.v + y, x.a, x.b, x.ab); }
__device__ __forceinline__ MtHyper operator+(double x, MtHyper y) { return mt_hyper(x + y.v, y.a, y.b, y.ab); }
__device__ __forceinline__ MtHyper operator-(MtHyper x, double y) { return mt_hyper(x.v - y, x.a, x.b, x.ab); }
__device__ __forceinline__ MtHyper operator-(double x, MtHyper y) { return mt_hyper(x - y.v, -y.a, -y.b, -y.ab); }
__device__ __forceinline__ MtHyper operator*(MtHyper x, double y) { return mt_hyper(x.v * y, x.a * y, x.b * y, x.ab * y); }
__device__ __forceinline__ MtHyper operator*(double x, MtHyper y) { return mt_hyper(x * y.v, x * y.a, x * y.b, x * y.ab); }
__device__ __forceinline__ MtHyper operator/(MtHyper x, double y) { return mt_hyper(x.v / y, x.a / y, x.b / y, x.ab / y); }
__device__ __forceinline__ MtHyper operator-(MtHyper x) { return mt_hyper(-x.v, -x.a, -x.b, -x.ab); }
// f(x) from f, f' and f'' at the value
__device__ __forceinline__ MtHyper mt_chain(MtHyper x, double f, double f1, double f2) { return mt_hyper(f, f1 * x.a, f1 * x.b, f1 * x.ab + f2 * (x.a * x.b)); }
__device__ __forceinline__ MtHyper mt_sin(MtHyper x) { const double s = sin(x.v), c = cos(x.v); return mt_chain(x, s, c, -s); }
__device__ __forceinline__ MtHyper mt_cos(MtHyper x) { const double s = sin(x.v), c = cos(x.v); return mt_chain(x, c, -s, -c); }
__device__ __forceinline__ MtHyper mt_atan(MtHyper x) { const double r = 1.0 / (1.0 + x.v * x.v); return mt_chain(x, atan(x.v), r, -2.0 * x.v * (r * r)); }
__device__ __forceinline__ MtHyper mt_exp(MtHyper x) { const double e = exp(x.v); return mt_chain(x, e, e, e); }
// the second derivative of the branch taken (zero on the other; a NaN stays one)
__device__ __forceinline__ MtHyper mt_pos(MtHyper x) { const double z = x.v != x.v ? x.v : 0.0; return x.v > 0.0 ? x : mt_hyper(z, z, z, z); }
__device__ __forceinline__ MtHyper mt_neg(MtHyper x) { const double z = x.v != x.v ? x.v : 0.0; return x.v < 0.0 ? x : mt_hyper(z, z, z, z); }
__device__ __forceinline__ double mt_val(MtHyper x) { return x.v; }

template <class T>
struct MtModel {
    T dx[5], sf;         // the five derivatives divided by x_s, the time-distance scaling factor
    T fx[4], fy[4], fz[4];   // fl, fr, rl, rr
    T ax, ay;
};

// the time-distance scaling factor alone (the quadrature's integrand; it reads no control)
template <class T>
__device__ __forceinline__ T mt_sf(const T* xn, double kappa)
{
    const T v = xn[0] * MT_VS, beta = xn[1] * MT_BETAS, n = xn[3] * MT_NS, xi = xn[4];
    return (1.0 - n * kappa) / (v * mt_cos(xi + beta));
}

template <class T>
__device__ __forceinline__ void mt_model(const T* xn, const T* un, double kappa, const mcq_mintime_pars& P, MtModel<T>& o)
{
    const T v = xn[0] * MT_VS, beta = xn[1] * MT_BETAS, omega = xn[2], n = xn[3] * MT_NS, xi = xn[4];
    const T delta = un[0] * MT_DELTAS, f_drive = un[1] * MT_FDS, f_brake = un[2] * MT_FBS, gamma_y = un[3] * MT_GYS;
    const double mass = P.mass, g = P.g, wb = P.wheelbase_front + P.wheelbase_rear;
    const T v2 = v * v;
    const T f_xdrag = P.dragcoeff * v2;
    const double f_xroll_f = 0.5 * P.c_roll * mass * g * P.wheelbase_rear / wb, f_xroll_r = 0.5 * P.c_roll * mass * g * P.wheelbase_front / wb;
    const double f_xroll = P.c_roll * mass * g;
    const double f_zstat_f = 0.5 * mass * g * P.wheelbase_rear / wb, f_zstat_r = 0.5 * mass * g * P.wheelbase_front / wb;
    const T f_zlift_f = 0.5 * P.liftcoeff_front * v2, f_zlift_r = 0.5 * P.liftcoeff_rear * v2;
    const T f_long = f_drive + f_brake - f_xdrag - f_xroll;
    const double cz = 0.5 * P.cog_z / wb;
    o.fz[0] = f_zstat_f + f_zlift_f + (-cz * f_long - P.k_roll * gamma_y);
    o.fz[1] = f_zstat_f + f_zlift_f + (-cz * f_long + P.k_roll * gamma_y);
    o.fz[2] = f_zstat_r + f_zlift_r + (cz * f_long - (1.0 - P.k_roll) * gamma_y);
    o.fz[3] = f_zstat_r + f_zlift_r + (cz * f_long + (1.0 - P.k_roll) * gamma_y);
    const T vs = v * mt_sin(beta), vc = v * mt_cos(beta);
    const T num_f = vs + P.wheelbase_front * omega, num_r = -vs + P.wheelbase_rear * omega;
    const T twf = 0.5 * P.track_width_front * omega, twr = 0.5 * P.track_width_rear * omega;
    T alpha[4];
    alpha[0] = delta - mt_atan(num_f / (vc - twf));
    alpha[1] = delta - mt_atan(num_f / (vc + twf));
    alpha[2] = mt_atan(num_r / (vc - twr));
    alpha[3] = mt_atan(num_r / (vc + twr));
    for (int q = 0; q < 4; ++q) {
        const double B = q < 2 ? P.B_front : P.B_rear, C = q < 2 ? P.C_front : P.C_rear, E = q < 2 ? P.E_front : P.E_rear;
        const double eps = q < 2 ? P.eps_front : P.eps_rear;
        const T ba = B * alpha[q];
        o.fy[q] = P.mue * o.fz[q] * (1.0 + eps * o.fz[q] / P.f_z0) * mt_sin(C * mt_atan(ba - E * (ba - mt_atan(ba))));
    }
    o.fx[0] = 0.5 * f_drive * P.k_drive_front + 0.5 * f_brake * P.k_brake_front - f_xroll_f;
    o.fx[1] = o.fx[0];
    o.fx[2] = 0.5 * f_drive * (1.0 - P.k_drive_front) + 0.5 * f_brake * (1.0 - P.k_brake_front) - f_xroll_r;
    o.fx[3] = o.fx[2];
    const T sd = mt_sin(delta), cd = mt_cos(delta);
    const T fxf = o.fx[0] + o.fx[1], fxr = o.fx[2] + o.fx[3], fyf = o.fy[0] + o.fy[1], fyr = o.fy[2] + o.fy[3];
    o.ax = (fxr + fxf * cd - fyf * sd - P.dragcoeff * v2) / mass;
    o.ay = (fxf * sd + o.fy[2] + o.fy[3] + fyf * cd) / mass;
    const T sf = (1.0 - n * kappa) / (v * mt_cos(xi + beta));
    o.sf = sf;
    const T sb = mt_sin(beta), cb = mt_cos(beta), sdb = mt_sin(delta - beta), cdb = mt_cos(delta - beta);
    const T dv = (sf / mass) * (fxr * cb + fxf * cdb + fyr * sb - fyf * sdb - f_xdrag * cb);
    const T dbeta = sf * (-omega + (-fxr * sb + fxf * sdb + fyr * cb + fyf * cdb + f_xdrag * sb) / (mass * v));
    const T domega = (sf / P.I_z) * ((o.fx[3] - o.fx[2]) * P.track_width_rear / 2.0 - fyr * P.wheelbase_rear +
                                     ((o.fx[1] - o.fx[0]) * cd + (o.fy[0] - o.fy[1]) * sd) * P.track_width_front / 2.0 +
                                     (fyf * cd + fxf * sd) * P.track_width_front);
    const T dn = sf * v * mt_sin(xi + beta);
    const T dxi = sf * omega - kappa;
    o.dx[0] = dv / MT_VS;
    o.dx[1] = dbeta / MT_BETAS;
    o.dx[2] = domega;
    o.dx[3] = dn / MT_NS;
    o.dx[4] = dxi;
}

// the friction coefficient of wheel q at row `row` (k + 1) and lateral position n [m]: the constant, the line, or the Gaussian bumps the reference
// evaluates (:717-747): centres (i - n_gauss) * center_dist, sigma = 2 center_dist, the sum in rising order, then the intercept
template <class T>
__device__ __forceinline__ T mt_mue(const McqMintime& M, const mcq_mintime_pars& P, int b, int q, int row, T n)
{
    if (M.o.friction < 0) return 0.0 * n + P.mue;
    const double* wr = M.d.w_mue + (((size_t)b * 4 + q) * ((size_t)M.d.nmax + 1) + row) * M.P;
    if (M.o.friction == MCQ_FRIC_LINEAR) return wr[0] * n + wr[1];
    const double cdist = M.d.center_dist[(size_t)b * ((size_t)M.d.nmax + 1) + row], sigma = 2.0 * cdist;
    const int ng = M.o.n_gauss;
    T acc = 0.0 * n;
    for (int i = 0; i < 2 * ng + 1; ++i) {
        const T dq = n - (double)(i - ng) * cdist;
        acc = acc + wr[i] * mt_exp(-(dq * dq) / (2.0 * (sigma * sigma)));
    }
    return acc + wr[2 * ng + 1];
}

// the 13 path rows of an interval at X_k+1 with U_k (:704-786): power, Kamm x 4, roll moment, pedal, actuator x 4 (k > 0), safe x 2 (where enabled)
template <class T>
__device__ __forceinline__ void mt_path_rows(const McqMintime& M, const mcq_mintime_pars& P, int b, int k, const T* x1, const T* u, const double* u_prev,
                                             double kappa_k, double h_prev, const MtModel<T>& m, T* rows)
{
    rows[0] = x1[0] * u[1];
    const T n = x1[3] * MT_NS;
    for (int q = 0; q < 4; ++q) {
        const T den = mt_mue(M, P, b, q, k + 1, n) * m.fz[q];
        const T a = m.fx[q] / den, c = m.fy[q] / den;
        rows[1 + q] = a * a + c * c;
    }
    const T delta = u[0] * MT_DELTAS;
    rows[5] = ((m.fy[0] + m.fy[1]) * mt_cos(delta) + m.fy[2] + m.fy[3] + (m.fx[0] + m.fx[1]) * mt_sin(delta)) * P.cog_z /
                  ((P.track_width_front + P.track_width_rear) / 2.0) - u[3] * MT_GYS;
    rows[6] = u[1] * u[2];
    if (k > 0) {
        const T sigma = (1.0 - kappa_k * x1[3] * MT_NS) / (x1[0] * MT_VS);
        for (int i = 0; i < 4; ++i) rows[7 + i] = (u[i] - u_prev[i]) / (h_prev * sigma);
    } else {
        for (int i = 0; i < 4; ++i) rows[7 + i] = 0.0 * u[i];
    }
    if (M.o.safe_traj) {
        const T ap = mt_pos(m.ax) / P.ax_pos_safe, an = mt_neg(m.ax) / P.ax_neg_safe, al = m.ay / P.ay_safe;
        rows[11] = ap * ap + al * al;
        rows[12] = an * an + al * al;
    } else {
        rows[11] = 0.0 * u[0];
        rows[12] = 0.0 * u[0];
    }
}

__device__ __forceinline__ int mt_intervals(const McqMintime& M, int b) { return mcq_mt_intervals(M.d.n_list, M.d.nmax, b); }
__device__ __forceinline__ McqMtSizes mt_sizes(const McqMintime& M, int b) { return mcq_mt_sizes(M.d.n_list, M.d.nmax, b, M.o.safe_traj, M.o.limit_energy); }

// x - x: 0 for a finite x, NaN for every other
__device__ __forceinline__ double mt_chk(double x) { return x - x; }

// ---- bounds and the flat guess (:482-507, :563-819): a workgroup per problem ----
__global__ void __launch_bounds__(MCQ_NT) mcq_mintime_bounds_kernel(McqMintime M)
{
    const int b = blockIdx.x, tid = threadIdx.x;
    const McqMtSizes Z = mt_sizes(M, b);
    const mcq_mintime_pars P = M.d.pars[b];
    const size_t n1 = (size_t)M.d.nmax + 1;
    double* w0 = M.w0 + (size_t)b * M.nwmax;
    double* lbw = M.lbw + (size_t)b * M.nwmax;
    double* ubw = M.ubw + (size_t)b * M.nwmax;
    double* lbg = M.lbg + (size_t)b * M.ngmax;
    double* ubg = M.ubg + (size_t)b * M.ngmax;
    const double half_pi = 0.5 * 3.141592653589793, inf = INFINITY;
    const double delta_min = -P.delta_max / MT_DELTAS, delta_max = P.delta_max / MT_DELTAS, f_drive_max = P.f_drive_max / MT_FDS,
                 f_brake_min = -P.f_brake_max / MT_FBS;
    for (int i = tid; i < M.nwmax; i += MCQ_NT) {
        double g0 = NAN, lo = NAN, hi = NAN;
        if (i < Z.nw) {
            const int k = i / 24, c = i - 24 * k;
            if (c < 5) {
                const double wr = M.d.w_tr_right_cl[b * n1 + k], wl = M.d.w_tr_left_cl[b * n1 + k];
                g0 = c == 0 ? 20.0 / MT_VS : 0.0;
                lo = c == 0 ? 1.0 / MT_VS : (c == 1 ? -half_pi / MT_BETAS : (c == 3 ? (-wr + P.width_opt / 2.0) / MT_NS : -half_pi));
                hi = c == 0 ? P.v_max / MT_VS : (c == 1 ? half_pi / MT_BETAS : (c == 3 ? (wl - P.width_opt / 2.0) / MT_NS : half_pi));
            } else if (c < 9) {
                g0 = 0.0;
                lo = c == 5 ? delta_min : (c == 6 ? 0.0 : (c == 7 ? f_brake_min : -inf));
                hi = c == 5 ? delta_max : (c == 6 ? f_drive_max : (c == 7 ? 0.0 : inf));
            } else {
                g0 = (c - 9) % 5 == 0 ? 20.0 / MT_VS : 0.0;
                lo = -inf;
                hi = inf;
            }
        }
        w0[i] = g0; lbw[i] = lo; ubw[i] = hi;
    }
    for (int i = tid; i < M.ngmax; i += MCQ_NT) {
        double lo = NAN, hi = NAN;
        if (i < Z.ng) {
            lo = 0.0; hi = 0.0;       // collocation, continuity, roll moment, periodicity
            if (i >= Z.per) {
                if (i == Z.per + 5) hi = P.energy_limit;
            } else {
                int k, r;
                mcq_mt_slot_of(i, Z.safe, &k, &r);
                if (r == 20) { lo = -inf; hi = P.power_max / (MT_FDS * MT_VS); }
                else if (r >= 21 && r < 25) hi = 1.0;
                else if (r == 26) lo = -20000.0 / (MT_FDS * MT_FBS);
                else if (r == 27) { lo = delta_min / P.t_delta; hi = delta_max / P.t_delta; }
                else if (r == 28) { lo = -inf; hi = f_drive_max / P.t_drive; }
                else if (r == 29) { lo = f_brake_min / P.t_brake; hi = inf; }
                else if (r == 30) { lo = -inf; hi = inf; }
                else if (r >= 31) hi = 1.0;
            }
        }
        lbg[i] = lo; ubg[i] = hi;
    }
}

// ---- g, the f_sol outputs and the per-interval quadrature: 64 intervals per workgroup, four lanes each ----
__global__ void __launch_bounds__(MCQ_NT) mcq_mintime_eval_kernel(McqMintime M)
{
    const int b = blockIdx.y, tid = threadIdx.x, N = mt_intervals(M, b), safe = M.o.safe_traj ? 1 : 0;
    const int k = blockIdx.x * (MCQ_NT / MCQ_MT_EVAL_LANES) + tid / MCQ_MT_EVAL_LANES, p = tid % MCQ_MT_EVAL_LANES;
    const bool live = k < N;
    const int kk = live ? k : 0;       // (a lane without an interval computes interval 0's numbers and stores nothing: the shuffles below take every lane)
    const size_t n1 = (size_t)M.d.nmax + 1;
    const double* w = M.d.w + (size_t)b * M.nwmax + 24 * (size_t)kk;
    double q = 0.0;
    if (N == 0) return;                // (the whole workgroup: mcq_mintime_sum_kernel fills a refused problem's outputs)
    const mcq_mintime_pars P = M.d.pars[b];
    const double hk = M.d.h[(size_t)b * M.d.nmax + kk], ka = M.d.kappa_cl[b * n1 + kk], kb = M.d.kappa_cl[b * n1 + kk + 1];
    double* g = M.g + (size_t)b * M.ngmax + mcq_mt_row0(kk, safe);
    double u[4], chk = mt_chk(hk);
    for (int i = 0; i < 4; ++i) { u[i] = w[5 + i]; chk += mt_chk(u[i]); }
    MtModel<double> m;
    if (p < 3) {
        const int j = p + 1;
        double xc[5], xp[5];
        for (int i = 0; i < 5; ++i) {
            xc[i] = w[9 + 5 * p + i];
            xp[i] = M.c.C[0][j] * w[i];
            for (int r = 0; r < 3; ++r) xp[i] = xp[i] + M.c.C[r + 1][j] * w[9 + 5 * r + i];
            chk += mt_chk(xp[i]);
        }
        const double kappa = ka + M.c.tau[j] * (kb - ka);
        mt_model(xc, u, kappa, P, m);
        chk += mt_chk(kappa);
        q = M.c.B[j] * m.sf * hk;
        if (live)
            for (int i = 0; i < 5; ++i) g[5 * p + i] = chk == 0.0 ? hk * m.dx[i] - xp[i] : NAN;
    }
    // the interval's time: sf_opt[0] + sf_opt[1] + sf_opt[2], on every lane of the four
    const int base = (tid & 63) & ~3;
    const double q0 = __shfl(q, base), q1 = __shfl(q, base + 1), q2 = __shfl(q, base + 2);
    if (p == 3) {
        const double dt = q0 + q1 + q2;
        double x1[5], xe[5], up[4] = {0.0, 0.0, 0.0, 0.0};
        for (int i = 0; i < 5; ++i) {
            x1[i] = w[24 + i];
            xe[i] = M.c.D[0] * w[i];
            for (int r = 0; r < 3; ++r) xe[i] = xe[i] + M.c.D[r + 1] * w[9 + 5 * r + i];
            chk += mt_chk(x1[i]) + mt_chk(xe[i]);
        }
        double hp = 1.0;
        if (kk > 0) {
            hp = M.d.h[(size_t)b * M.d.nmax + kk - 1];
            for (int i = 0; i < 4; ++i) { up[i] = w[5 + i - 24]; chk += mt_chk(up[i]); }
            chk += mt_chk(hp) + mt_chk(ka);
        }
        mt_model(x1, u, ka, P, m);
        double rows[13];
        mt_path_rows(M, P, b, kk, x1, u, up, ka, hp, m, rows);
        if (!live) return;
        const bool ok = chk == 0.0;
        for (int i = 0; i < 5; ++i) g[15 + i] = ok ? xe[i] - x1[i] : NAN;
        for (int i = 0; i < 13; ++i) {
            const int off = mcq_mt_row_off(kk, safe, 20 + i);
            if (off >= 0) g[off] = ok ? rows[i] : NAN;
        }
        const size_t bk = (size_t)b * M.d.nmax + kk;
        const double xs[5] = {MT_VS, MT_BETAS, 1.0, MT_NS, 1.0}, us[4] = {MT_DELTAS, MT_FDS, MT_FBS, MT_GYS};
        // the interval's START state carries the energy (:674); a start state that is not finite spoils it alone
        const double ec = w[0] * MT_VS * u[1] * MT_FDS * dt;
        M.dt_own[bk] = ok ? dt : NAN;
        M.ec_own[bk] = ok ? ec : NAN;
        if (M.x_opt) {
            double* xo = M.x_opt + ((size_t)b * n1 + kk + 1) * 5;
            for (int i = 0; i < 5; ++i) xo[i] = x1[i] * xs[i];
            if (kk == 0)
                for (int i = 0; i < 5; ++i) xo[i - 5] = w[i] * xs[i];
        }
        if (M.u_opt)
            for (int i = 0; i < 4; ++i) M.u_opt[bk * 4 + i] = u[i] * us[i];
        if (M.tf_opt)
            for (int qw = 0; qw < 4; ++qw) {
                M.tf_opt[bk * 12 + 3 * qw] = ok ? m.fx[qw] : NAN;
                M.tf_opt[bk * 12 + 3 * qw + 1] = ok ? m.fy[qw] : NAN;
                M.tf_opt[bk * 12 + 3 * qw + 2] = ok ? m.fz[qw] : NAN;
            }
        if (M.ax_opt) M.ax_opt[bk] = ok ? m.ax : NAN;
        if (M.ay_opt) M.ay_opt[bk] = ok ? m.ay : NAN;
    }
}

__device__ __forceinline__ double mt_add(double a, double b) { return a + b; }
// a maximum that keeps a NaN
__device__ __forceinline__ double mt_nanmax(double a, double b) { return (a != a || b != b) ? NAN : fmax(a, b); }
// the workgroup's 256 partial values combined by OP (mt_add, mt_nanmax) in one fixed order: a binary tree in LDS
template <double (*OP)(double, double)>
__device__ double mt_tree(double v, double* s)
{
    const int tid = threadIdx.x;
    __syncthreads();
    s[tid] = v;
    __syncthreads();
    for (int half = MCQ_NT / 2; half > 0; half >>= 1) {
        if (tid < half) s[tid] = OP(s[tid], s[tid + half]);
        __syncthreads();
    }
    return s[0];
}

// ---- the ordered sums, the rows after the last interval, the tails: a workgroup per problem ----
__global__ void __launch_bounds__(MCQ_NT) mcq_mintime_sum_kernel(McqMintime M)
{
    __shared__ double s_red[MCQ_NT];
    const int b = blockIdx.x, tid = threadIdx.x, nmax = M.d.nmax;
    const McqMtSizes Z = mt_sizes(M, b);
    const int N = Z.N, ng = Z.ng, per = Z.per;
    const size_t n1 = (size_t)nmax + 1;
    const mcq_mintime_pars P = M.d.pars[b];
    const double* w = M.d.w + (size_t)b * M.nwmax;
    double* g = M.g + (size_t)b * M.ngmax;
    double* dt = M.dt_own + (size_t)b * nmax;
    double* ec = M.ec_own + (size_t)b * nmax;
    double lap = 0.0, en = 0.0, rd = 0.0, rf = 0.0, chk = 0.0;
    for (int k = tid; k < N; k += MCQ_NT) {
        const int kn = k + 1 < N ? k + 1 : 0;
        const double* uk = w + 24 * (size_t)k + 5;
        const double* un = w + 24 * (size_t)kn + 5;
        const double dd = uk[0] * MT_DELTAS - un[0] * MT_DELTAS;
        const double df = (uk[1] * MT_FDS / 10000.0 + uk[2] * MT_FBS / 10000.0) - (un[1] * MT_FDS / 10000.0 + un[2] * MT_FBS / 10000.0);
        lap += dt[k];
        en += ec[k];
        rd += dd * dd;
        rf += df * df;
        for (int i = 0; i < 24; ++i) chk += mt_chk(w[24 * (size_t)k + i]);
        chk += mt_chk(M.d.h[(size_t)b * nmax + k]) + mt_chk(M.d.kappa_cl[b * n1 + k]);
    }
    if (tid < 5 && N) chk += mt_chk(w[24 * (size_t)N + tid]);
    if (tid == 5 && N) chk += mt_chk(M.d.kappa_cl[b * n1 + N]);
    lap = mt_tree<mt_add>(lap, s_red);
    en = mt_tree<mt_add>(en, s_red);
    rd = mt_tree<mt_add>(rd, s_red);
    rf = mt_tree<mt_add>(rf, s_red);
    chk = mt_tree<mt_add>(chk, s_red);
    const bool ok = N && chk == 0.0;
    if (tid == 0) {
        M.J[b] = ok ? lap + P.penalty_F * rf + P.penalty_delta * rd : NAN;
        if (M.lap) M.lap[b] = ok ? lap : NAN;
        if (M.energy) M.energy[b] = ok ? en / 3600000.0 : NAN;
        M.status[b] = ok && lap == lap && en == en ? MCQ_OK : MCQ_BAD_INPUT;
        if (N && M.o.limit_energy) g[per + 5] = ok ? en / 3600000.0 : NAN;
    }
    if (tid < 5 && N) g[per + tid] = w[tid] - w[24 * (size_t)N + tid] + (mt_chk(w[tid]) + mt_chk(w[24 * (size_t)N + tid]));
    for (int i = ng + tid; i < M.ngmax; i += MCQ_NT) g[i] = NAN;
    // the tails of the per-interval outputs (a refused problem: all of them)
    for (int k = N + tid; k < nmax; k += MCQ_NT) {
        const size_t bk = (size_t)b * nmax + k;
        if (M.dt_opt) M.dt_opt[bk] = NAN;
        if (M.ec_opt) M.ec_opt[bk] = NAN;
        if (M.ax_opt) M.ax_opt[bk] = NAN;
        if (M.ay_opt) M.ay_opt[bk] = NAN;
        if (M.u_opt) for (int i = 0; i < 4; ++i) M.u_opt[bk * 4 + i] = NAN;
        if (M.tf_opt) for (int i = 0; i < 12; ++i) M.tf_opt[bk * 12 + i] = NAN;
    }
    if (M.x_opt)
        for (int k = (N ? N + 1 : 0) + tid; k <= nmax; k += MCQ_NT)
            for (int i = 0; i < 5; ++i) M.x_opt[((size_t)b * n1 + k) * 5 + i] = NAN;
}

// ---- the Jacobian in interval blocks, grad J, grad energy: 36 lanes per interval, one dual evaluation each ----
__global__ void __launch_bounds__(MCQ_NT) mcq_mintime_jac_kernel(McqMintime M)
{
    const int b = blockIdx.y, N = mt_intervals(M, b), nmax = M.d.nmax;
    const long long gl = (long long)blockIdx.x * MCQ_NT + threadIdx.x;
    const int k = (int)(gl / MCQ_MT_JAC_LANES), s = (int)(gl - (long long)k * MCQ_MT_JAC_LANES), p = s / 9, d = s - 9 * p;
    if (k >= nmax) return;
    const size_t n1 = (size_t)nmax + 1;
    double* blk = M.blocks + ((size_t)b * nmax + k) * (MCQ_MT_BLOCK * MCQ_MT_BLOCK);
    double* gJ = M.grad_J + (size_t)b * M.nwmax + 24 * (size_t)k;
    double* gE = M.grad_E ? M.grad_E + (size_t)b * M.nwmax + 24 * (size_t)k : nullptr;
    // the column slots this lane owns: its own, and for the path point's lanes X_k (d < 5) or U_k-1 (d >= 5) as well
    const int col = p < 3 ? (d < 5 ? 9 + 5 * p + d : d) : (d < 5 ? 24 + d : d);
    const int col2 = p < 3 ? -1 : (d < 5 ? d : 24 + d);
    const int r0 = p < 3 && d >= 5 ? 5 * p : (p == 3 && d >= 5 ? 15 : 0), r1 = p < 3 && d >= 5 ? 5 * p + 5 : MCQ_MT_BLOCK;
    if (k >= N) {
        for (int r = r0; r < r1; ++r) blk[r * MCQ_MT_BLOCK + col] = NAN;
        if (col2 >= 0)
            for (int r = 0; r < MCQ_MT_BLOCK; ++r) blk[r * MCQ_MT_BLOCK + col2] = NAN;
        // grad entries 24 k + c past the problem's own nw = 24 N + 5 (X_N itself belongs to interval N - 1's lanes)
        if (p < 3 && d < 5) { gJ[col] = NAN; if (gE) gE[col] = NAN; }
        if (p == 3) {
            if (d >= 5 || k > N || N == 0) { gJ[d] = NAN; if (gE) gE[d] = NAN; }
            if (d < 5 && k == nmax - 1) { gJ[24 + d] = NAN; if (gE) gE[24 + d] = NAN; }
        }
        return;
    }
    const mcq_mintime_pars P = M.d.pars[b];
    const double* w = M.d.w + (size_t)b * M.nwmax + 24 * (size_t)k;
    const double hk = M.d.h[(size_t)b * nmax + k], ka = M.d.kappa_cl[b * n1 + k], kb = M.d.kappa_cl[b * n1 + k + 1];
    MtDual u[4];
    double chk = mt_chk(hk);
    for (int i = 0; i < 4; ++i) { u[i] = mt_dual(w[5 + i], d == 5 + i ? 1.0 : 0.0); chk += mt_chk(u[i].v); }
    MtModel<MtDual> m;
    const double escale = MT_VS * MT_FDS / 3600000.0;
    if (p < 3) {
        const int j = p + 1;
        MtDual xc[5];
        for (int i = 0; i < 5; ++i) { xc[i] = mt_dual(w[9 + 5 * p + i], d == i ? 1.0 : 0.0); chk += mt_chk(xc[i].v); }
        const double kappa = ka + M.c.tau[j] * (kb - ka);
        chk += mt_chk(kappa);
        mt_model(xc, u, kappa, P, m);
        const bool ok = chk == 0.0;
        if (d >= 5) {
            for (int i = 0; i < 5; ++i) blk[(5 * p + i) * MCQ_MT_BLOCK + col] = ok ? hk * m.dx[i].d : NAN;
            return;
        }
        for (int qq = 0; qq < 3; ++qq)
            for (int i = 0; i < 5; ++i) {
                const double own = qq == p ? hk * m.dx[i].d : 0.0;
                blk[(5 * qq + i) * MCQ_MT_BLOCK + col] = ok ? own - (i == d ? M.c.C[j][qq + 1] : 0.0) : NAN;
            }
        for (int i = 0; i < 5; ++i) blk[(15 + i) * MCQ_MT_BLOCK + col] = ok ? (i == d ? M.c.D[j] : 0.0) : NAN;
        for (int r = 20; r < MCQ_MT_BLOCK; ++r) blk[r * MCQ_MT_BLOCK + col] = ok ? 0.0 : NAN;
        const double dq = M.c.B[j] * m.sf.d * hk;
        gJ[col] = ok ? dq : NAN;
        if (gE) gE[col] = ok ? w[0] * w[6] * escale * dq + mt_chk(w[0]) : NAN;
        return;
    }
    MtDual x1[5];
    double up[4] = {0.0, 0.0, 0.0, 0.0}, hp = 1.0;
    for (int i = 0; i < 5; ++i) { x1[i] = mt_dual(w[24 + i], d == i ? 1.0 : 0.0); chk += mt_chk(x1[i].v); }
    if (k > 0) {
        hp = M.d.h[(size_t)b * nmax + k - 1];
        for (int i = 0; i < 4; ++i) { up[i] = w[5 + i - 24]; chk += mt_chk(up[i]); }
        chk += mt_chk(hp) + mt_chk(ka);
    }
    mt_model(x1, u, ka, P, m);
    MtDual rows[13];
    mt_path_rows(M, P, b, k, x1, u, up, ka, hp, m, rows);
    const bool ok = chk == 0.0;
    // the interval's time, for the energy's gradient: the three quadrature terms again (values only)
    double dt = 0.0;
    for (int j = 1; j <= 3; ++j) dt += M.c.B[j] * mt_sf(w + 9 + 5 * (j - 1), ka + M.c.tau[j] * (kb - ka)) * hk;
    if (d < 5) {
        for (int r = 0; r < 15; ++r) blk[r * MCQ_MT_BLOCK + col] = ok ? 0.0 : NAN;
        for (int i = 0; i < 5; ++i) blk[(15 + i) * MCQ_MT_BLOCK + col] = ok ? (i == d ? -1.0 : 0.0) : NAN;
        for (int i = 0; i < 13; ++i) blk[(20 + i) * MCQ_MT_BLOCK + col] = ok ? rows[i].d : NAN;
        // column X_k: constants of the collocation and continuity rows
        const double fin = mt_chk(w[d]);
        for (int qq = 0; qq < 3; ++qq)
            for (int i = 0; i < 5; ++i) blk[(5 * qq + i) * MCQ_MT_BLOCK + col2] = (i == d ? -M.c.C[0][qq + 1] : 0.0) + fin;
        for (int i = 0; i < 5; ++i) blk[(15 + i) * MCQ_MT_BLOCK + col2] = (i == d ? M.c.D[0] : 0.0) + fin;
        for (int r = 20; r < MCQ_MT_BLOCK; ++r) blk[r * MCQ_MT_BLOCK + col2] = 0.0 + fin;
        gJ[d] = 0.0 + fin;
        if (gE) gE[d] = (d == 0 ? w[6] * escale * dt : 0.0) + fin + mt_chk(w[6]);
        if (k == N - 1) {
            gJ[24 + d] = ok ? 0.0 : NAN;
            if (gE) gE[24 + d] = ok ? 0.0 : NAN;
        }
        return;
    }
    for (int r = 15; r < 20; ++r) blk[r * MCQ_MT_BLOCK + col] = ok ? 0.0 : NAN;
    for (int i = 0; i < 13; ++i) blk[(20 + i) * MCQ_MT_BLOCK + col] = ok ? rows[i].d : NAN;
    // column U_k-1: the actuator row of this control alone
    const int c = d - 5;
    const double sigma = (1.0 - ka * x1[3].v * MT_NS) / (x1[0].v * MT_VS);
    for (int r = 0; r < MCQ_MT_BLOCK; ++r) blk[r * MCQ_MT_BLOCK + col2] = ok ? (k > 0 && r == 27 + c ? -1.0 / (hp * sigma) : 0.0) : NAN;
    // grad J on a control: the cyclic regularisation alone (the quadrature's integrand reads no control)
    const int kn = k + 1 < N ? k + 1 : 0, kp = k > 0 ? k - 1 : N - 1;
    const double* wb = M.d.w + (size_t)b * M.nwmax;
    const double* un = wb + 24 * (size_t)kn + 5;
    const double* uq = wb + 24 * (size_t)kp + 5;
    double gj = 0.0;
    if (c == 0) {
        const double pk = w[5] * MT_DELTAS, pn = un[0] * MT_DELTAS, pp = uq[0] * MT_DELTAS;
        gj = P.penalty_delta * 2.0 * ((pk - pn) - (pp - pk)) * MT_DELTAS;
    } else if (c < 3) {
        const double pk = w[6] * MT_FDS / 10000.0 + w[7] * MT_FBS / 10000.0, pn = un[1] * MT_FDS / 10000.0 + un[2] * MT_FBS / 10000.0,
                     pp = uq[1] * MT_FDS / 10000.0 + uq[2] * MT_FBS / 10000.0;
        gj = P.penalty_F * 2.0 * ((pk - pn) - (pp - pk)) * (c == 1 ? MT_FDS / 10000.0 : MT_FBS / 10000.0);
    } else {
        gj = mt_chk(w[8]);
    }
    gJ[d] = gj;
    if (gE) gE[d] = (c == 1 ? w[0] * escale * dt : 0.0) + mt_chk(w[0]) + mt_chk(w[5 + c]);
}

// ---- the certificate: r = grad J + J_g^T lam_g + lam_x and the three maxima, a workgroup per problem ----
__global__ void __launch_bounds__(MCQ_NT) mcq_mintime_kkt_kernel(McqMintime M)
{
    __shared__ double s_red[MCQ_NT];
    const int b = blockIdx.x, tid = threadIdx.x, nmax = M.d.nmax;
    const McqMtSizes Z = mt_sizes(M, b);
    const int N = Z.N, per = Z.per;
    const size_t ow = (size_t)b * M.nwmax, og = (size_t)b * M.ngmax;
    const double* blocks = M.blocks_in + (size_t)b * nmax * (MCQ_MT_BLOCK * MCQ_MT_BLOCK);
    const double* lam_g = M.lam_g + og;
    double rmax = 0.0, viol = 0.0, comp = 0.0;
    for (int i = tid; i < M.nwmax; i += MCQ_NT) {
        if (i >= Z.nw) { M.r[ow + i] = NAN; continue; }
        const int k = i / 24, c = i - 24 * k;
        double acc = 0.0;
        int kb[2], cb[2];
        mcq_mt_holders(N, i, false, kb, cb);
        for (int t = 0; t < 2; ++t) {
            if (kb[t] < 0) continue;
            const double* blk = blocks + (size_t)kb[t] * (MCQ_MT_BLOCK * MCQ_MT_BLOCK) + cb[t];
            const double* lk = lam_g + mcq_mt_row0(kb[t], Z.safe);
            for (int r = 0; r < MCQ_MT_ROWS_ALWAYS; ++r) acc += blk[r * MCQ_MT_BLOCK] * lk[r];
            // (the actuator rows 27 .. 30 are there together or not at all, the safe pair 31, 32 is adjacent: asked once per group -- one loop over
            // the six slots compiles to 132 VGPRs and 3 waves per SIMD, this to the 128 and 4 it had)
            if (mcq_mt_row_off(kb[t], Z.safe, 27) >= 0)
                for (int r = 27; r < 31; ++r) acc += blk[r * MCQ_MT_BLOCK] * lk[r];
            const int pair = mcq_mt_row_off(kb[t], Z.safe, 31);
            if (pair >= 0)
                for (int r = 0; r < 2; ++r) acc += blk[(31 + r) * MCQ_MT_BLOCK] * lk[pair + r];
        }
        if (c < 5 && k == 0) acc += lam_g[per + c];
        if (c < 5 && k == N) acc -= lam_g[per + c];
        if (Z.energy) acc += M.grad_E_in[ow + i] * lam_g[per + 5];
        const double lx = M.lam_x[ow + i], wi = M.d.w[ow + i], lo = M.lbw_in[ow + i], hi = M.ubw_in[ow + i];
        const double r = M.grad_J_in[ow + i] + acc + lx;
        M.r[ow + i] = r;
        rmax = mt_nanmax(rmax, fabs(r));
        viol = mt_nanmax(viol, mt_nanmax(lo - wi, wi - hi));
        if (lx > 0.0 && hi < INFINITY) comp = mt_nanmax(comp, fabs(lx * (hi - wi)));
        if (lx < 0.0 && lo > -INFINITY) comp = mt_nanmax(comp, fabs(lx * (wi - lo)));
        if (lx != lx) comp = NAN;
    }
    for (int i = tid; i < Z.ng; i += MCQ_NT) {
        const double lg = lam_g[i], gi = M.g_in[og + i], lo = M.lbg_in[og + i], hi = M.ubg_in[og + i];
        viol = mt_nanmax(viol, mt_nanmax(lo - gi, gi - hi));
        if (lg > 0.0 && hi < INFINITY) comp = mt_nanmax(comp, fabs(lg * (hi - gi)));
        if (lg < 0.0 && lo > -INFINITY) comp = mt_nanmax(comp, fabs(lg * (gi - lo)));
        if (lg != lg) comp = NAN;
    }
    rmax = mt_tree<mt_nanmax>(rmax, s_red);
    viol = mt_tree<mt_nanmax>(viol, s_red);
    comp = mt_tree<mt_nanmax>(comp, s_red);
    if (tid == 0) {
        M.kkt[3 * (size_t)b] = N ? rmax : NAN;
        M.kkt[3 * (size_t)b + 1] = N ? viol : NAN;
        M.kkt[3 * (size_t)b + 2] = N ? comp : NAN;
    }
}

// ---- the Hessian of the Lagrangian in interval blocks: a workgroup per interval, one lane per (evaluation point, pair of directions) ----
// the index of the unordered pair a <= b of 9 directions among the 45
__device__ __forceinline__ int mt_pair(int a, int b) { return a * 9 - a * (a - 1) / 2 + (b - a); }
// the regularisation's second derivative between controls i and j of one interval (the same between the two intervals' controls, negated)
__device__ __forceinline__ double mt_reg2(const mcq_mintime_pars& P, int i, int j)
{
    const double cf[4] = {0.0, MT_FDS / 10000.0, MT_FBS / 10000.0, 0.0};
    return i == 0 && j == 0 ? P.penalty_delta * (2.0 * MT_DELTAS * MT_DELTAS) : P.penalty_F * (2.0 * cf[i] * cf[j]);
}

__global__ void __launch_bounds__(MCQ_MT_HESS_NT) mcq_mintime_hess_kernel(McqMintime M)
{
    __shared__ double s_h[4][MCQ_MT_HESS_PAIRS];   // per point: the weighted scalar's second derivative along every pair of its 9 directions
    __shared__ double s_dq[3][5], s_q[3];          // per collocation point: the quadrature term's gradient on its state, and the term
    __shared__ int s_bad;
    const int b = blockIdx.y, k = blockIdx.x, tid = threadIdx.x, N = mt_intervals(M, b), nmax = M.d.nmax, safe = M.o.safe_traj ? 1 : 0;
    const int nn = MCQ_MT_BLOCK * MCQ_MT_BLOCK;
    double* blk = M.hblocks + ((size_t)b * nmax + k) * nn;
    if (k >= N) {                      // (the whole workgroup)
        for (int e = tid; e < nn; e += MCQ_MT_HESS_NT) blk[e] = NAN;
        return;
    }
    const size_t n1 = (size_t)nmax + 1;
    const mcq_mintime_pars P = M.d.pars[b];
    const double* w = M.d.w + (size_t)b * M.nwmax + 24 * (size_t)k;
    // slots 29 .. 32: U_k-1, at k = 0 U_N-1 (the regularisation's wrapped term)
    const double* wu = M.d.w + (size_t)b * M.nwmax + 24 * (size_t)(k > 0 ? k - 1 : N - 1) + 5;
    // (this kernel's register allocation is at its limit: its walks over the row slots stay as they were measured, the safe pair's offset from the map)
    const int row0 = mcq_mt_row0(k, safe), at = mcq_mt_row_off(k, 1, 31);
    const double* lam = M.lam_g + (size_t)b * M.ngmax + row0;
    const double sg = M.sigma ? M.sigma[b] : 1.0;
    const double lam_e = M.o.limit_energy ? M.lam_g[(size_t)b * M.ngmax + mcq_mt_row0(N, safe) + 5] : 0.0;
    const double hk = M.d.h[(size_t)b * nmax + k], hp = k > 0 ? M.d.h[(size_t)b * nmax + k - 1] : 1.0;
    const double ka = M.d.kappa_cl[b * n1 + k], kb = M.d.kappa_cl[b * n1 + k + 1];
    const double ce = lam_e * (MT_VS * MT_FDS / 3600000.0);
    // every input of the interval is finite, or the whole block is NaN: an input per lane
    if (tid == 0) s_bad = 0;
    __syncthreads();
    double chk = 0.0;
    if (tid < 29) chk = mt_chk(w[tid]);
    else if (tid < 33) chk = mt_chk(wu[tid - 29]);
    else if (tid < 60) chk = mt_chk(lam[tid - 33]);
    else if (tid < 64) chk = k > 0 ? mt_chk(lam[27 + tid - 60]) : 0.0;
    else if (tid < 66) chk = safe ? mt_chk(lam[at + tid - 64]) : 0.0;
    else if (tid == 66) chk = mt_chk(hk) + mt_chk(hp) + mt_chk(ka) + mt_chk(kb) + mt_chk(sg) + mt_chk(lam_e);
    if (chk != 0.0) s_bad = 1;
    if (tid < 4 * MCQ_MT_HESS_PAIRS) {
        const int p = tid / MCQ_MT_HESS_PAIRS, q = tid - MCQ_MT_HESS_PAIRS * p;
        int da = 0, db = q;
        while (db >= 9 - da) { db -= 9 - da; ++da; }
        db += da;
        // directions 0 .. 4: a state of the point (Xc_k,p, or X_k+1 at the path point), 5 .. 8: a control of U_k
        const int xo = p < 3 ? 9 + 5 * p : 24, j = p < 3 ? p + 1 : 0;
        const double kappa = p < 3 ? ka + M.c.tau[j] * (kb - ka) : ka;
        MtHyper x[5], u[4];
        for (int i = 0; i < 5; ++i) x[i] = mt_hyper(w[xo + i], da == i ? 1.0 : 0.0, db == i ? 1.0 : 0.0, 0.0);
        for (int i = 0; i < 4; ++i) u[i] = mt_hyper(w[5 + i], da == 5 + i ? 1.0 : 0.0, db == 5 + i ? 1.0 : 0.0, 0.0);
        MtModel<MtHyper> m;
        mt_model(x, u, kappa, P, m);
        double acc = 0.0;
        if (p < 3) {
            // the collocation rows' multipliers, and on the quadrature term sigma (the objective) and the energy row's share at the START state
            for (int i = 0; i < 5; ++i) acc += lam[5 * p + i] * (hk * m.dx[i].ab);
            acc += (sg + ce * (w[0] * w[6])) * (M.c.B[j] * m.sf.ab * hk);
            if (q == 0) s_q[p] = M.c.B[j] * m.sf.v * hk;
            if (da == db && da < 5) s_dq[p][da] = M.c.B[j] * m.sf.a * hk;
        } else {
            double up[4];
            for (int i = 0; i < 4; ++i) up[i] = k > 0 ? wu[i] : 0.0;
            MtHyper rows[13];
            mt_path_rows(M, P, b, k, x, u, up, ka, hp, m, rows);
            for (int i = 0; i < 7; ++i) acc += lam[20 + i] * rows[i].ab;
            if (k > 0)
                for (int i = 0; i < 4; ++i) acc += lam[27 + i] * rows[7 + i].ab;
            if (safe)
                for (int i = 0; i < 2; ++i) acc += lam[at + i] * rows[11 + i].ab;
        }
        s_h[p][q] = acc;
    }
    __syncthreads();
    const bool bad = s_bad != 0;
    const double dt = s_q[0] + s_q[1] + s_q[2];
    // the actuator rows against U_k-1 in closed form: row i is (U_k[i] - U_k-1[i]) G, G = v_k+1 / (h[k - 1] (1 - kappa_cl[k] n_k+1))
    const double den = 1.0 - ka * (w[27] * MT_NS);
    const double g0 = MT_VS / (hp * den), g3 = (w[24] * MT_VS) * (ka * MT_NS) / (hp * (den * den));
    for (int e = tid; e < nn; e += MCQ_MT_HESS_NT) {
        const int er = e / MCQ_MT_BLOCK, ec = e - MCQ_MT_BLOCK * er, r = er < ec ? er : ec, c = er < ec ? ec : er;
        // the groups of the slots: 0 X_k, 1 U_k, 2 .. 4 Xc_k,0..2, 5 X_k+1, 6 U_k-1, and the index inside
        const int gr = r < 5 ? 0 : (r < 9 ? 1 : (r < 24 ? 2 + (r - 9) / 5 : (r < 29 ? 5 : 6)));
        const int gc = c < 5 ? 0 : (c < 9 ? 1 : (c < 24 ? 2 + (c - 9) / 5 : (c < 29 ? 5 : 6)));
        const int ir = r - (gr == 0 ? 0 : (gr == 1 ? 5 : (gr < 5 ? 9 + 5 * (gr - 2) : (gr == 5 ? 24 : 29))));
        const int ic = c - (gc == 0 ? 0 : (gc == 1 ? 5 : (gc < 5 ? 9 + 5 * (gc - 2) : (gc == 5 ? 24 : 29))));
        double v = 0.0;
        if (gr == 0) {
            // the energy's cross terms of the START state's speed: with f_drive, with the quadrature's states
            if (r == 0 && c == 6) v = ce * dt;
            else if (r == 0 && gc >= 2 && gc < 5) v = ce * w[6] * s_dq[gc - 2][ic];
        } else if (gr == 1) {
            if (gc == 1) {
                const int pq = mt_pair(5 + ir, 5 + ic);
                v = s_h[0][pq] + s_h[1][pq] + s_h[2][pq] + s_h[3][pq] + sg * mt_reg2(P, ir, ic);
            } else if (gc < 5) {
                v = s_h[gc - 2][mt_pair(ic, 5 + ir)] + (ir == 1 ? ce * w[0] * s_dq[gc - 2][ic] : 0.0);
            } else if (gc == 5) {
                v = s_h[3][mt_pair(ic, 5 + ir)];
            } else {
                v = -(sg * mt_reg2(P, ir, ic));
            }
        } else if (gr < 5) {
            if (gc == gr) v = s_h[gr - 2][mt_pair(ir, ic)];
        } else if (gr == 5) {
            if (gc == 5) v = s_h[3][mt_pair(ir, ic)];
            else if (k > 0 && ir == 0) v = -(lam[27 + ic] * g0);
            else if (k > 0 && ir == 3) v = -(lam[27 + ic] * g3);
        } else {
            v = sg * mt_reg2(P, ir, ic);
        }
        blk[e] = bad ? NAN : v;
    }
}

// ---- y = H v from the blocks: a lane per entry of w, the block that holds the entry at 24 k + slot first, then the other, slots rising ----
__global__ void __launch_bounds__(MCQ_NT) mcq_mintime_hessvec_kernel(McqMintime M)
{
    const int b = blockIdx.y, nmax = M.d.nmax;
    const McqMtSizes Z = mt_sizes(M, b);
    const int i = blockIdx.x * MCQ_NT + threadIdx.x;
    if (i >= M.nwmax) return;
    const int nn = MCQ_MT_BLOCK * MCQ_MT_BLOCK;
    const double* blocks = M.hblocks_in + (size_t)b * nmax * nn;
    int kb[2], cb[2];
    mcq_mt_holders(Z.N, i, true, kb, cb);       // (past the problem's own entries: none, nothing is read)
    for (int t = 0; t < M.nvec; ++t) {
        const double* v = M.v + ((size_t)b * M.nvec + t) * M.nwmax;
        double acc = 0.0;
        for (int s = 0; s < 2; ++s) {
            if (kb[s] < 0) continue;
            const double* row = blocks + (size_t)kb[s] * nn + cb[s] * MCQ_MT_BLOCK;       // (a block is symmetric: the slot's row is its column)
            const double* vk = v + mcq_mt_slot_entry(Z.N, kb[s], 0);
            const double* vu = v + mcq_mt_slot_entry(Z.N, kb[s], 29);
            for (int a = 0; a < 29; ++a) acc += row[a] * vk[a];
            for (int a = 0; a < 4; ++a) acc += row[29 + a] * vu[a];
        }
        M.y[((size_t)b * M.nvec + t) * M.nwmax + i] = i < Z.nw ? acc : NAN;
    }
}
