// TEST INFRASTRUCTURE ONLY (tests/test_host_layout.py builds and runs it; no GPU, no kernel launch, nothing loaded into an interpreter).
// csrc/mcq_api.hip is compiled INTO this program against the SIMT interpreter's headers, so that its static host functions can be called:
//   1. the scratch layouts (*_layout) against the formulas the entries carried before the arena -- written out below as they stood, the
//      record of the layout the kernels were validated with: total bytes, every region's offset, every region's alignment (the IQP driver's
//      buffers were allocations of their own before: the regions the driver indexes, back to back on 8-byte boundaries);
//   2. the structural scan behind mcq_les_scalings / mcq_les_scalings_open on small systems with one corrupted entry, on 1 and on 3 threads:
//      return code and mcq_last_error text.
// -DSCAN_ONLY leaves part 1 out (the scan alone also compiles against sources that have no layout functions).
#include "../global_racetrajectory_optimization_amd/csrc/mcq_api.hip"

static int failures = 0;
#define EXPECT(cond, ...)                                                       \
    do {                                                                        \
        if (!(cond)) {                                                          \
            if (++failures <= 20) { printf("FAILED %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } \
        }                                                                       \
    } while (0)

#ifndef SCAN_ONLY
static size_t old_up8(size_t bytes) { return (bytes + 7) & ~(size_t)7; }

static void expect_layout(const char* what, const Arena& a, size_t total, std::initializer_list<size_t> offsets, std::initializer_list<size_t> aligns)
{
    EXPECT(a.bytes == total, "%s: %zu bytes, %zu before", what, a.bytes, total);
    EXPECT(a.n == offsets.size() && a.n == aligns.size(), "%s: %zu regions", what, a.n);
    size_t i = 0;
    for (size_t off : offsets) { EXPECT(a.off[i] == off, "%s: region %zu at %zu, before at %zu", what, i, a.off[i], off); ++i; }
    i = 0;
    for (size_t al : aligns) {
        EXPECT(a.align[i] == al && a.off[i] % al == 0, "%s: region %zu at %zu for an alignment of %zu (recorded %zu)", what, i, a.off[i], al, a.align[i]);
        ++i;
    }
    for (i = 0; i + 1 < a.n; ++i) EXPECT(a.off[i] <= a.off[i + 1] && a.off[i + 1] <= a.bytes, "%s: regions out of order", what);
}

static void check_layouts()
{
    const size_t D = sizeof(double), I = sizeof(int), AD = alignof(double), AI = alignof(int);
    for (size_t tracks : {1, 2, 3, 5, 4097, 32767}) {
        for (size_t nmax : {3, 4, 5, 7, 33, 1001}) {
            // mcq_bound_dists_device
            for (size_t nbmax : {0, 1, 2, 7, 4096}) {
                const size_t sides = 2 * tracks;
                const size_t fixed = sides * nmax * 2 + sides * (nmax + 1) + tracks;
                const size_t need = (sides * nbmax * 2 + fixed) * D;
                const size_t pts = sides * nbmax * 2 * D, cum = pts + sides * nmax * 2 * D, side_status = cum + sides * (nmax + 1) * D;
                expect_layout("bound", bound_layout(tracks, nmax, nbmax), need, {0, pts, cum, side_status}, {AD, AD, AD, AI});
            }
            // mcq_spline_fit_device
            for (size_t k = 1; k <= 5; ++k) {
                for (size_t nk : {2 * k + 2, 2 * k + 3, (size_t)57}) {
                    for (size_t mm : {2, 3, 17, 100}) {
                        const size_t nm = nmax;
                        const size_t work_per = mm * (k + 2) + 2 * (size_t)(2 * k + 5) * nk + 2 * nk + nk * (k + 2) + nk + 2 + (2 * mm + nk + 2 + 1) / 2 + 1 + mm * (k + 3);
                        const size_t per = nm + 1 + 3 * mm + work_per;
                        const size_t pts = tracks * (nm + 1) * D, u = pts + tracks * mm * 2 * D, work = u + tracks * mm * D;
                        EXPECT(fit_work_per(mm, k, nk) == work_per, "fit: %zu doubles of work per track, %zu before", fit_work_per(mm, k, nk), work_per);
                        expect_layout("fit", fit_layout(tracks, nmax, mm, k, nk), tracks * per * D, {0, pts, u, work}, {AD, AD, AD, AD});
                    }
                }
            }
            // mcq_spline_approx_device
            {
                const size_t per = tracks * (nmax + 1);
                const size_t need = (4 * per + tracks) * D;
                expect_layout("spline", spl_layout(tracks, nmax), need, {0, per * D, 2 * per * D, 3 * per * D, 4 * per * D}, {AD, AD, AD, AD, AI});
            }
            // mcq_friction_gen_device: the buffer of the boundaries' launch
            {
                const size_t tn = tracks * nmax, t2 = tracks * 2;
                const size_t b_poly = tn * 8 * D, b_cont = tn * 16 * D, b_rad = t2 * D, b_flag = old_up8(tn * 4 * I);
                const size_t b_cnt = old_up8(t2 * I);
                const size_t flag = 2 * b_poly + b_cont + b_rad, pcount = flag + b_flag;
                expect_layout("fgen", fgen_layout(tracks, nmax), 2 * b_poly + b_cont + b_rad + b_flag + 3 * b_cnt,
                              {0, b_poly, 2 * b_poly, 2 * b_poly + b_cont, flag, pcount, pcount + b_cnt, pcount + 2 * b_cnt}, {AD, AD, AD, AD, AI, AI, AI, AI});
            }
        }
        // ... and the one sized after the read-back
        for (size_t maxblk : {(size_t)0, (size_t)1, (size_t)3, (size_t)1000, (size_t)1 << 21}) {
            const size_t b_bits = old_up8(tracks * maxblk * 256);
            expect_layout("fgen_pts", fgen_pts_layout(tracks, maxblk), b_bits + tracks * std::max<size_t>(maxblk, 1) * I, {0, b_bits}, {alignof(unsigned char), AI});
        }
    }
    // mcq_iqp_device / mcq_iqp_batch (allocations of their own before the arena): [batch] per region, the live count [1], each on an 8-byte boundary
    for (size_t batch : {1, 2, 3, 4, 11, 1024, 4097}) {
        const size_t bi = old_up8(batch * I), lc = 5 * bi, pc = lc + 8, tr = pc + batch * D, buf = tr + batch * MCQ_IQP_TRACE * D;
        expect_layout("iqp", iqp_layout(batch), buf + 2 * bi, {0, bi, 2 * bi, 3 * bi, 4 * bi, lc, pc, tr, buf, buf + bi}, {AI, AI, AI, AI, AI, AI, AD, AD, AI, AI});
        for (size_t nmax : {3, 7, 128, 2128}) {
            const size_t e = batch * nmax;
            expect_layout("iqp_set", iqp_set_layout(e), e * 6 * D, {0, e * 4 * D}, {AD, AD});
            expect_layout("iqp_pin", iqp_pin_layout(e, batch), e * 6 * D + bi, {0, e * 4 * D, e * 6 * D}, {AD, AD, AI});
        }
    }
    // mcq_points_in_path_device
    for (size_t paths : {1, 2, 3, 7, 65535}) {
        for (size_t vmax : {1, 2, 3, 7, 2002}) {
            for (int given = 0; given < 2; ++given) {       // contour_out given: no region of the scratch for the contours
                const size_t pv = paths * vmax;
                const size_t b_kept = pv * 2 * D, b_cont = given ? 0 : pv * 4 * D, b_flag = old_up8(pv * I);
                expect_layout("path", path_layout(paths, vmax, !given), b_kept + b_cont + b_flag + old_up8(paths * I),
                              {0, b_kept, b_kept + b_cont, b_kept + b_cont + b_flag}, {AD, AD, AI, AI});
            }
        }
    }
}
#endif

// calc_splines' system through n waypoints, closed ([4n][4n]) or open ([4(n-1)][4(n-1)]), with the scalings s
static std::vector<double> les_system(int n, bool closed, const std::vector<double>& s)
{
    const int ns = closed ? n : n - 1;
    const size_t m = (size_t)4 * ns;
    std::vector<double> A(m * m, 0.0);
    for (int i = 0; i < ns; ++i) {
        const size_t j = (size_t)4 * i;
        const bool last = i == ns - 1;
        A[j * m + j] = 1.0;
        for (int c = 0; c < 4; ++c) A[(j + 1) * m + j + c] = 1.0;
        if (!last) {
            A[(j + 2) * m + j + 1] = 1.0; A[(j + 2) * m + j + 2] = 2.0; A[(j + 2) * m + j + 3] = 3.0; A[(j + 2) * m + j + 5] = -s[i];
            A[(j + 3) * m + j + 2] = 2.0; A[(j + 3) * m + j + 3] = 6.0; A[(j + 3) * m + j + 6] = -2.0 * s[i] * s[i];
        } else if (closed) {
            A[(j + 2) * m + j + 1] = -1.0; A[(j + 2) * m + j + 2] = -2.0; A[(j + 2) * m + j + 3] = -3.0; A[(j + 2) * m + 1] = s[i];
            A[(j + 3) * m + j + 2] = -2.0; A[(j + 3) * m + j + 3] = -6.0; A[(j + 3) * m + 2] = 2.0 * s[i] * s[i];
        } else {
            A[(j + 2) * m + 1] = 1.0;
            A[(j + 3) * m + j + 1] = 1.0; A[(j + 3) * m + j + 2] = 2.0; A[(j + 3) * m + j + 3] = 3.0;
        }
    }
    return A;
}

static void expect_scan(bool closed, int n, const std::vector<double>& A, long long bad_row, const char* what)
{
    std::vector<double> s_out((size_t)n, -7.0);
    const int rc = (closed ? mcq_les_scalings : mcq_les_scalings_open)(A.data(), n, s_out.data(), 1);
    char want[200] = "";
    if (bad_row >= 0)       // the text as it stood before the two exports shared their implementation
        snprintf(want, sizeof want, closed ? "mcq_les_scalings: row %lld of A does not have the structure of calc_splines' closed-spline system"
                                           : "mcq_les_scalings_open: row %lld of A does not have the structure of calc_splines' open-spline system", bad_row);
    EXPECT(rc == (bad_row >= 0 ? MCQ_E_ARG : 0), "%s n %d %s: return code %d", closed ? "closed" : "open", n, what, rc);
    if (bad_row >= 0) EXPECT(!strcmp(mcq_last_error(), want), "%s n %d %s: '%s', not '%s'", closed ? "closed" : "open", n, what, mcq_last_error(), want);
}

static void check_scan()
{
    for (const char* threads : {"1", "3"}) {
        setenv("MCQ_PACK_THREADS", threads, 1);
        for (int closed = 1; closed >= 0; --closed) {
            for (int n : {3, 4, 7}) {
                const int ns = closed ? n : n - 1;
                const size_t m = (size_t)4 * ns;
                std::vector<double> s((size_t)n);
                for (int i = 0; i < n; ++i) s[i] = 0.75 + 0.125 * i;
                const std::vector<double> good = les_system(n, closed, s);
                expect_scan(closed, n, good, -1, "as built");
                {       // the scalings read back: the closed system's n, the open system's n - 2 and two ones
                    std::vector<double> got((size_t)n, -7.0);
                    (closed ? mcq_les_scalings : mcq_les_scalings_open)(good.data(), n, got.data(), 0);
                    for (int i = 0; i < n; ++i) EXPECT(got[i] == (closed || i < n - 2 ? s[i] : 1.0), "scaling %d of %d: %g", i, n, got[i]);
                }
                for (int i = 0; i < ns; ++i) {
                    for (int r = 0; r < 4; ++r) {
                        const size_t row = (size_t)4 * i + r;
                        // the first entry the row has: another value
                        std::vector<double> A = good;
                        size_t c = (size_t)4 * i;       // (not the wrap-around entries in front of the block: the closed system's last scaling is one)
                        while (c < m && A[row * m + c] == 0.0) ++c;
                        if (c == m) for (c = 0; A[row * m + c] == 0.0;) ++c;
                        A[row * m + c] += 0.5;
                        expect_scan(closed, n, A, (long long)row, "an entry changed");
                        // an entry the row does not have
                        A = good;
                        c = m - 1;
                        while (A[row * m + c] != 0.0) --c;
                        A[row * m + c] = 1e-300;
                        expect_scan(closed, n, A, (long long)row, "an entry added");
                    }
                    if (closed || i < ns - 1) {     // a scaling that is not positive: reported at the row it is read from
                        std::vector<double> A = good;
                        const size_t col = i == ns - 1 ? 1 : (size_t)4 * i + 5;
                        A[((size_t)4 * i + 2) * m + col] = -A[((size_t)4 * i + 2) * m + col];
                        expect_scan(closed, n, A, (long long)(4 * i + 2), "a negative scaling");
                    }
                }
                // two offenders in two threads' blocks: the lower one is reported
                std::vector<double> A = good;
                A[(m - 3) * m + m - 1] = 2.0;
                A[1 * m + 0] = 2.0;
                expect_scan(closed, n, A, 1, "two offenders");
            }
        }
        for (int closed = 1; closed >= 0; --closed) {
            double a = 0.0;
            const int rc = (closed ? mcq_les_scalings : mcq_les_scalings_open)(&a, 2, &a, 1);
            EXPECT(rc == MCQ_E_ARG && !strcmp(mcq_last_error(), closed ? "mcq_les_scalings: bad argument" : "mcq_les_scalings_open: bad argument"),
                   "n = 2: %d '%s'", rc, mcq_last_error());
        }
    }
}

#ifndef SCAN_ONLY
// the minimum-time NLP's maps (csrc/mcq_kernels.h: mcq_mt_row_of, mcq_mt_slot_of, mcq_mt_holders, mcq_mt_slot_entry, mcq_mt_sizes) against a
// brute-force statement of the structure: every row slot and every column slot of every block visited
static void check_mintime_maps()
{
    const int nmax = 6;
    for (int N = 2; N <= nmax; ++N) for (int safe = 0; safe < 2; ++safe) for (int energy = 0; energy < 2; ++energy) {
        const int nw = 5 + 24 * N, per = mcq_mt_row0(N, safe);
        // (a) the present row slots in order are the rows 0 .. per - 1; (b) mcq_mt_slot_of inverts
        int next = 0;
        for (int k = 0; k < N; ++k)
            for (int s = 0; s < MCQ_MT_BLOCK; ++s) {
                const int row = mcq_mt_row_of(k, safe, s);
                const bool absent = (s >= 27 && s < 31 && k == 0) || (s >= 31 && !safe);
                EXPECT((row < 0) == absent, "N %d safe %d: slot %d of interval %d gives row %d", N, safe, s, k, row);
                if (row < 0) continue;
                EXPECT(row == next, "N %d safe %d: slot %d of interval %d is row %d, not %d", N, safe, s, k, row, next);
                EXPECT(row == mcq_mt_row0(k, safe) + mcq_mt_row_off(k, safe, s), "N %d safe %d: offset of slot %d of interval %d", N, safe, s, k);
                // what the kernels' group-wise walks rely on: slots 0 .. 30 at their own number, the actuator rows together, the safe pair adjacent
                EXPECT(s >= 31 || mcq_mt_row_off(k, safe, s) == s, "N %d safe %d: slot %d of interval %d is not at its own number", N, safe, s, k);
                EXPECT(s < MCQ_MT_ROWS_ALWAYS || s >= 31 || mcq_mt_row_off(k, safe, 27) >= 0, "N %d safe %d: actuator slot %d without slot 27", N, safe, s);
                EXPECT(s != 32 || mcq_mt_row_off(k, safe, 31) == mcq_mt_row_off(k, safe, 32) - 1, "N %d safe %d: the safe pair of interval %d", N, safe, k);
                ++next;
                int k2 = -1, s2 = -1;
                mcq_mt_slot_of(row, safe, &k2, &s2);
                EXPECT(k2 == k && s2 == s, "N %d safe %d: row %d is (%d, %d), not (%d, %d)", N, safe, row, k, s, k2, s2);
            }
        EXPECT(next == per && mcq_mt_ng(N, safe, energy) == per + 5 + energy, "N %d safe %d energy %d: %d rows in the intervals, row0(N) = %d", N, safe, energy, next, per);
        // (c) the holders of every entry of w, by a scan over all (block, slot) with the slot-to-entry map written out here
        for (int wrap = 0; wrap < 2; ++wrap)
            for (int i = 0; i < 5 + 24 * nmax; ++i) {
                int want_k[2] = {-1, -1}, want_c[2] = {-1, -1}, found = 0;
                for (int k = 0; k < N && i < nw; ++k)
                    for (int s = 0; s < (wrap || k > 0 ? 33 : 29); ++s) {
                        const int entry = s < 29 ? 24 * k + s : 24 * ((k - 1 + N) % N) + 5 + (s - 29);
                        if (entry != i) continue;
                        const int t = k == i / 24 && s == i % 24 ? 0 : 1;      // the block at i = 24 k + slot first
                        EXPECT(want_k[t] < 0, "N %d: entry %d is twice in place %d", N, i, t);
                        want_k[t] = k; want_c[t] = s; ++found;
                        if (wrap) EXPECT(mcq_mt_slot_entry(N, k, s) == i, "N %d: slot %d of block %d is entry %d, not %d", N, s, k, mcq_mt_slot_entry(N, k, s), i);
                    }
                int kb[2] = {7, 7}, cb[2] = {7, 7};
                mcq_mt_holders(N, i, wrap != 0, kb, cb);
                EXPECT(found <= 2 && (i >= nw) == (found == 0), "N %d wrap %d: entry %d has %d holders", N, wrap, i, found);
                for (int t = 0; t < 2; ++t)
                    EXPECT(kb[t] == want_k[t] && cb[t] == want_c[t], "N %d wrap %d: entry %d holder %d is (%d, %d), not (%d, %d)", N, wrap, i, t, kb[t], cb[t],
                           want_k[t], want_c[t]);
            }
        // (d) the sizes: from the list or from nmax, nothing for an N out of range
        const int list[5] = {N, 1, nmax + 1, 0, -3};
        for (int b = 0; b < 5; ++b) {
            const McqMtSizes Z = mcq_mt_sizes(list, nmax, b, safe, energy);
            const bool in = b == 0;
            EXPECT(Z.N == (in ? N : 0) && Z.nw == (in ? nw : 0) && Z.ng == (in ? per + 5 + energy : 0) && Z.per == (in ? per : 0) && Z.safe == safe &&
                       Z.energy == energy, "sizes of N = %d: N %d nw %d ng %d per %d", list[b], Z.N, Z.nw, Z.ng, Z.per);
        }
        const McqMtSizes Z = mcq_mt_sizes(nullptr, N, 3, safe, energy);
        EXPECT(Z.N == N && Z.nw == nw && Z.per == per, "sizes without a list: N %d nw %d per %d", Z.N, Z.nw, Z.per);
    }
}
#endif

int main()
{
#ifndef SCAN_ONLY
    check_layouts();
    check_mintime_maps();
#endif
    check_scan();
    printf(failures ? "%d checks FAILED\n" : "layout_check: all checks passed\n", failures);
    return failures ? 1 : 0;
}
