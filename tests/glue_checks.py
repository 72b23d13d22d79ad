"""The bodies of tests/test_emu_glue.py (SIMT interpreter) and tests/test_gpu_glue.py (MI355X): the same launches of tests/glue_cases.py through
the same entry points, against tests/glue_ref.py in longdouble (oracle/vel_ref.py for the velocity profiles) under the guards of
tests/glue_guard.py.  Every function takes the engine and a ring_guard.Worst that collects, per family and quantity, the worst deviation next
to the guard it was held to.  Point counts, statuses and crossing verdicts are compared exactly; every launch is run a second time in reversed
order (or case by case) and must return the same bits."""
import numpy as np

import glue_cases as gc
import glue_guard as gg
import glue_ref
from global_racetrajectory_optimization_amd import engine

LD = np.longdouble
OK, BAD_INPUT = 0, engine.STATUS_BAD_INPUT


def _hold(worst, family, quantity, dev, spread, what):
    g = gg.guard(quantity, spread)
    worst.add("%s.%s" % (family, quantity), dev, g)
    assert dev <= g, "%s: %s deviates by %.3e, guard %.3e" % (what, quantity, dev, g)


def _rings(family, sizes):
    r = [gc.ring(family, n) for n in sizes]
    return [x[0] for x in r], [x[1] for x in r], [x[2] for x in r]


# ---- mcq_raceline_device ---------------------------------------------------------------------------------------------------------------------
def _raceline_rows_equal(a, b, ka, kb):
    if a["status"][ka] != b["status"][kb] or a["m"][ka] != b["m"][kb]:
        return False
    m = int(a["m"][ka]) if a["status"][ka] == OK else 0
    return all(np.array_equal(a[q][ka, :m], b[q][kb, :m]) for q in ("xy", "psi", "kappa", "el_lengths"))


def check_raceline_launch(eng, family, launch, worst):
    name, sizes, stepsize, mmax = launch
    refs, nvs, als = _rings(family, sizes)
    out = eng.raceline_batch(refs, nvs, als, stepsize, mmax=mmax)
    S = gg.spread("raceline/%s/%s" % (family, name))
    for k, n in enumerate(sizes):
        what = "raceline %s/%s n=%d" % (family, name, n)
        r = gg.raceline_ref(family, n, stepsize)
        if r["m"] < 2 or r["m"] > mmax:
            assert out["status"][k] == BAD_INPUT, what
            continue
        assert out["status"][k] == OK and out["m"][k] == r["m"], "%s: status %d, m %d for %d" % (what, out["status"][k], out["m"][k], r["m"])
        m = r["m"]
        _hold(worst, family, "xy", gg.dmax(out["xy"][k, :m], r["xy"]), S[k, 0], what)
        _hold(worst, family, "psi", gg.dpsi(out["psi"][k, :m], r["psi"]), S[k, 1], what)
        _hold(worst, family, "kappa", gg.dmax(out["kappa"][k, :m], r["kappa"]), S[k, 2], what)
        _hold(worst, family, "el", gg.dmax(out["el_lengths"][k, :m], r["el_lengths"]), S[k, 3], what)
        assert np.all(out["psi"][k, :m] >= -np.pi) and np.all(out["psi"][k, :m] < np.pi), what
    rev = eng.raceline_batch(refs[::-1], nvs[::-1], als[::-1], stepsize, mmax=mmax)
    for k in range(len(sizes)):
        assert _raceline_rows_equal(out, rev, k, len(sizes) - 1 - k), "raceline %s/%s n=%d: the reversed launch returns other bits" % (family, name, sizes[k])
    return out


# ---- mcq_relinearise_device ------------------------------------------------------------------------------------------------------------------
NAN_PATTERN = np.frombuffer(np.array([0x7FF8DEADBEEF0001], dtype=np.uint64).tobytes(), dtype=np.float64)[0]


def relin_device(eng, refs, nvs, alphas, alpha_scale, stepsize, nmax, live=None, same_buffers=False):
    """mcq_relinearise_device through Engine.alloc / upload / download.  The output buffers are filled with a NaN pattern first.  Returns
    (ref_out [B, nmax, 4], nv_out [B, nmax, 2], n_out [B], status [B]); status / n_out start from -1 / -7."""
    bsz = len(refs)
    n_in = np.array([r.shape[0] for r in refs], dtype=np.int32)
    ref_in = np.zeros((bsz, nmax, 4))
    nv_in = np.zeros((bsz, nmax, 2))
    al = np.zeros((bsz, nmax))
    for k in range(bsz):
        ref_in[k, :n_in[k]] = refs[k]
        nv_in[k, :n_in[k]] = nvs[k]
        al[k, :n_in[k]] = alphas[k]
    with eng.scope() as dev:
        up = dev.up
        d_n, d_ref, d_nv, d_al = up(n_in), up(ref_in), up(nv_in), up(al)
        d_live = up(np.ascontiguousarray(live, dtype=np.int32)) if live is not None else None
        d_ro, d_no = up(np.full((bsz, nmax, 4), NAN_PATTERN)), up(np.full((bsz, nmax, 2), NAN_PATTERN))
        d_m, d_st = up(np.full(bsz, -7, dtype=np.int32)), up(np.full(bsz, -1, dtype=np.int32))
        if same_buffers:
            d_ro, d_no = d_ref, d_nv
        eng.relinearise_device(bsz, nmax, d_n, d_ref, d_nv, d_al, d_live, alpha_scale, stepsize, d_ro, d_no, d_m, d_st)
        eng.sync()
        return (eng.download(d_ro, (bsz, nmax, 4), np.float64), eng.download(d_no, (bsz, nmax, 2), np.float64),
                eng.download(d_m, (bsz,), np.int32), eng.download(d_st, (bsz,), np.int32))


def _untouched(a):
    return bool(np.all(a.view(np.uint64) == np.array([NAN_PATTERN]).view(np.uint64)[0]))


def check_relin_launch(eng, family, launch, worst):
    name, sizes, alpha_scale, stepsize, nmax = launch
    refs, nvs, als = _rings(family, sizes)
    ro, no, m_out, st = relin_device(eng, refs, nvs, als, alpha_scale, stepsize, nmax)
    S = gg.spread("relin/%s/%s" % (family, name))
    for k, n in enumerate(sizes):
        what = "relinearise %s/%s n=%d" % (family, name, n)
        r = gg.relin_ref(family, n, alpha_scale, stepsize)
        if r["m"] < 3 or r["m"] > nmax:
            assert st[k] == BAD_INPUT and m_out[k] == n, "%s: status %d, n_out %d (m = %d)" % (what, st[k], m_out[k], r["m"])
            continue
        assert st[k] == OK and m_out[k] == r["m"], "%s: status %d, n_out %d for %d" % (what, st[k], m_out[k], r["m"])
        m = r["m"]
        _hold(worst, family, "relin_rows", gg.dmax(ro[k, :m], r["rows"]), S[k, 0], what)
        _hold(worst, family, "relin_normals", gg.dmax(no[k, :m], r["normals"]), S[k, 1], what)
        assert _untouched(ro[k, m:]) and _untouched(no[k, m:]), what + ": rows beyond n_out written"
    ro2, no2, m2, st2 = relin_device(eng, refs[::-1], nvs[::-1], als[::-1], alpha_scale, stepsize, nmax)
    for a, b in ((ro, ro2), (no, no2), (m_out, m2), (st, st2)):
        assert np.array_equal(a.view(np.uint8), b[::-1].copy().view(np.uint8)), "relinearise %s/%s: the reversed launch returns other bits" % (family, name)


def check_relin_mask_and_arguments(eng, family):
    """A `live` mask leaves a masked-out track's outputs bitwise as they were; input == output buffers is MCQ_E_ARG."""
    sizes = (5, 97, 48, 257)
    refs, nvs, als = _rings(family, sizes)
    step = gc.relin_launches(family)[0][3]
    full = relin_device(eng, refs, nvs, als, 1.0, step, 400)
    live = [1, 0, 1, 0]
    ro, no, m_out, st = relin_device(eng, refs, nvs, als, 1.0, step, 400, live=live)
    for k in range(4):
        if live[k]:
            assert st[k] == OK and all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for a, b in zip(full, (ro, no, m_out, st)))
        else:
            assert _untouched(ro[k]) and _untouched(no[k]) and m_out[k] == -7 and st[k] == -1
    try:
        relin_device(eng, refs, nvs, als, 1.0, step, 400, same_buffers=True)
    except engine.EngineError as e:
        assert "(-1)" in str(e), str(e)           # MCQ_E_ARG
    else:
        raise AssertionError("mcq_relinearise_device accepted input == output buffers")


# ---- mcq_prep_device -------------------------------------------------------------------------------------------------------------------------
def check_prep(eng, family, worst):
    refs = [gc.ring(family, n)[0] for n in gc.SIZES]
    nvs, scs = eng.prep_batch(refs)
    S = gg.spread("prep/%s" % family)
    for k, n in enumerate(gc.SIZES):
        nv0, s0 = gg.prep_ref(family, n)
        what = "prep %s n=%d" % (family, n)
        _hold(worst, family, "prep_normals", gg.dmax(nvs[k], nv0), S[k, 0], what)
        _hold(worst, family, "prep_scalings", gg.dmax(scs[k], s0), S[k, 1], what)
    for lo in range(0, len(refs), 7):                   # in smaller launches (other strides): the same bits
        sub = eng.prep_batch(refs[lo:lo + 7][::-1])
        for j, k in enumerate(range(lo, min(lo + 7, len(refs)))[::-1]):
            assert np.array_equal(sub[0][j], nvs[k]) and np.array_equal(sub[1][j], scs[k]), "prep %s n=%d: other bits in another launch" % (family, gc.SIZES[k])


# ---- mcq_vel_profile_device / _ragged / _opts --------------------------------------------------------------------------------------------------
def _vel_run(eng, L, order=None):
    o = np.arange(L["ggv"].shape[0]) if order is None else np.asarray(order)
    return eng.vel_profile_batch(L["kappa"], L["el"], L["ggv"][o], L["axm"][o], L["drag"][o], L["mass"][o], L["vmax"][o],
                                 dyn_model_exp=L["exp"], track_of=L["track_of"][o], n_of_track=L["n_of_track"], mu=L["mu"],
                                 filt_window=L["filt_window"])


def check_vel_launch(eng, L, worst, reference=None):
    """reference: {variant: (vx, lap)} computed beforehand (the caller may spread the oracle's Python loops over processes)."""
    vx, lt = _vel_run(eng, L)
    S = gg.spread("vel/%s" % L["name"])
    nmax = L["kappa"].shape[1]
    for v in range(L["ggv"].shape[0]):
        what = "velocity profile %s variant %d" % (L["name"], v)
        r = reference[v] if reference is not None else gg.vel_ref_case(L, v)
        if r is None:                                   # n < 2 or n > nmax: the documented NaN lap time and NaN row
            assert np.isnan(lt[v]) and np.all(np.isnan(vx[v])), what
            continue
        n = r[0].size
        _hold(worst, "vel", "vx", gg.dmax(vx[v, :n], r[0]), S[v, 0], what)
        _hold(worst, "vel", "lap", abs(float(lt[v]) - r[1]), S[v, 1], what)
    order = np.arange(L["ggv"].shape[0])[::-1]
    vx2, lt2 = _vel_run(eng, L, order)
    for v in range(L["ggv"].shape[0]):
        n = gg.vel_row(L, v)[1]
        n = n if 2 <= n <= nmax else nmax
        assert np.array_equal(vx[v, :n], vx2[len(order) - 1 - v, :n], equal_nan=True) and \
            np.array_equal(lt[v], lt2[len(order) - 1 - v], equal_nan=True), "velocity profile %s variant %d: other bits in the reversed launch" % (L["name"], v)


VEL_GUARD_CAP = 1e-7


def check_raceline_into_vel(eng, family, worst):
    """The kernel's own padded kappa / el_lengths rows (strided by mmax, m as n_of_track) straight into the ragged profile entry.  The oracle
    runs on the SAME rows -- the kernel's kappa, already held to its guard against the reference by check_raceline_launch -- so the vx guard
    needs no widening by the profile's sensitivity to kappa; its spread is vel_ref's movement under the usual draws, computed here on what the
    device returned, so the cap of the stored velocity guards (1e-7: tests/test_glue_ref.py) is asserted here, case by case."""
    launch = [L for L in gc.raceline_launches(family) if L[0] == "m==mmax@97"][0]
    sizes = launch[1]
    refs, nvs, als = _rings(family, sizes)
    out = eng.raceline_batch(refs, nvs, als, launch[2], mmax=launch[3])
    rows = [k for k in range(len(sizes)) if out["status"][k] == OK]
    assert len(rows) >= 10
    nt = np.where(out["status"] == OK, out["m"], 0).astype(np.int32)
    base = gc.vel_launches()[3]
    bsz = 2 * len(rows)
    L = dict(name="chain/" + family, kappa=out["kappa"], el=out["el_lengths"], mu=None, n_of_track=nt,
             track_of=np.array(rows + rows[::-1], dtype=np.int32), exp=1.0, filt_window=None,
             **{q: base[q][:bsz] for q in ("ggv", "axm", "drag", "mass", "vmax")})
    vx, lt = _vel_run(eng, L)
    for v in range(bsz):
        r = gg.vel_ref_case(L, v)
        s = gg.compute_vel_spread(L, only=[v])[v]
        what = "raceline into velocity profile %s variant %d" % (family, v)
        assert gg.guard("vx", s[0]) <= VEL_GUARD_CAP and gg.guard("lap", s[1]) <= VEL_GUARD_CAP, what + ": the oracle itself is undecided here"
        _hold(worst, "chain", "vx", gg.dmax(vx[v, :r[0].size], r[0]), s[0], what)
        _hold(worst, "chain", "lap", abs(float(lt[v]) - r[1]), s[1], what)
    vx2, lt2 = _vel_run(eng, L, np.arange(bsz)[::-1])
    assert np.array_equal(vx, vx2[::-1]) and np.array_equal(lt, lt2[::-1]), "raceline into velocity profile %s: other bits in the reversed launch" % family


# ---- mcq_normals_crossing_device ---------------------------------------------------------------------------------------------------------------
def check_crossing(eng):
    cases = gc.crossing_cases()
    trks, nvs = [c[1] for c in cases], [c[2] for c in cases]
    seen = set()
    for hz in gc.crossing_horizons():
        want = [glue_ref.normals_crossing(t, nv, hz, LD)[0] for t, nv in zip(trks, nvs)]
        got = eng.normals_crossing_batch(trks, nvs, horizon=hz)
        assert list(got) == want, "horizon %d: %s" % (hz, [(c[0], int(g), w) for c, g, w in zip(cases, got, want) if g != w])
        rev = eng.normals_crossing_batch(trks[::-1], nvs[::-1], horizon=hz)
        assert list(rev[::-1]) == want
        seen |= set(want)
    assert seen == {-1, 0, 1}


# ---- the fp32 boundary -------------------------------------------------------------------------------------------------------------------------
def _solve64(eng, rows, nvs=None, scs=None):
    bsz = rows.shape[0]
    al, curv, st, _ = eng.solve_batch([dict(reftrack=rows[k], normvec=None if nvs is None else nvs[k], scaling=None if scs is None else scs[k],
                                            kappa_bound=gc.F32_KAPPA_BOUND, w_veh=gc.F32_W_VEH) for k in range(bsz)])
    return np.stack(al), curv, st


F32_ALL = ("abs", "abs_origin", "uni", "uni_nv_sc", "uni_nv", "inc", "inc_origin", "open", "open_origin")
F32_LIGHT = ("abs_origin", "uni_nv_sc", "inc_origin", "open")          # one variant of each comparison
F32_ONE = ("uni_nv_sc", "open")                                        # mcq_widen_kernel's tail and mcq_widen_rows_kernel's slices, once each
CURV_FLOOR, ALPHA_FLOOR = 1e-10, 1e-9       # the suite's assertions for the same comparison (tests/test_emu_kernels.py: fp32 increment rows)
F32_GUARD_CAP = 100.0                       # x floor: a twin spread beyond that would hide the kernel


def check_f32(eng, batch, n, worst, variants=F32_ALL, reversed_too=True):
    """Absolute rows (mcq_widen_rows_kernel layout 0, mcq_widen_kernel on rows / normals / scalings, mcq_narrow_kernel on alpha): the float alpha
    is BITWISE float32 of the fp64 engine's alpha on the widened inputs, curv_err bitwise the twin's.

    Increment rows (mcq_widen_rows_kernel's running sum with the closure defect spread evenly): the rebuilt rows live inside the handle, so they
    are seen through the solve.  The fp64 twin gets the rows glue_ref rebuilds in longdouble; how far the twin's own answer is determined is
    its movement when the rows are rebuilt in float64 instead (the two rebuilds differ by rounding alone, far below 1e-12 of the extent), and
        |curv_err - twin's| <= max(1e-10, 4 x that movement),   |alpha32 - twin's alpha| <= 2^-24 |alpha| + max(1e-9, 4 x that movement),
    both guards capped at 100 x their floors.  curv_err stays fp64 on the way out, so it resolves a rebuild that is off by 1e-10 of the extent
    (6e-8 against 2e-12 measured); the float alpha alone would not.  The second set of increments does not close by 0.3 m.
    variants: which comparisons run (the interpreter's solver takes minutes for long rings); reversed_too: every fp32 entry once more with the
    tracks in reversed order, same bits."""
    kb, wv = gc.F32_KAPPA_BOUND, gc.F32_W_VEH
    ref = gc.f32_tracks(batch, n)
    org = np.ascontiguousarray(ref[:, 0, :2]) + np.array([0.25, -0.5])
    rel32 = (ref - np.concatenate((org, np.zeros((batch, 2))), axis=1)[:, None, :]).astype(np.float32)

    def same_bits_reversed(fn, first, *arrays):
        if not reversed_too or batch == 1:
            return
        again = fn(*[None if a is None else np.ascontiguousarray(a[::-1]) for a in arrays])
        for x, y in zip(first[:3], again[:3]):
            assert np.array_equal(np.asarray(x), np.asarray(y)[::-1]), "fp32 (%d, %d): other bits with the tracks in reversed order" % (batch, n)

    # absolute layout, through both entries
    for tag, origin in (("abs", None), ("abs_origin", org)):
        if tag not in variants:
            continue
        fn = lambda r, o: eng.solve_batch_f32(r, o, kb, wv, layout=engine.F32_ABSOLUTE)
        got = fn(rel32, origin)
        a32, curv, st = got[:3]
        rows = rel32.astype(np.float64)
        if origin is not None:
            rows[:, :, :2] = origin[:, None, :] + rows[:, :, :2]
        a64, curv64, st64 = _solve64(eng, rows)
        assert np.array_equal(st, st64) and np.all(st == OK), (batch, n, list(st), list(st64))
        assert a32.dtype == np.float32 and np.array_equal(a32, a64.astype(np.float32)), "absolute rows (%d, %d): alpha is not float32 of the fp64 solve" % (batch, n)
        assert np.array_equal(curv, curv64)
        same_bits_reversed(fn, got, rel32, origin)
    pr = [glue_ref.prep(ref[k, :, :2], np.float64) for k in range(batch)]
    nv32, sc32 = np.stack([q[0] for q in pr]).astype(np.float32), np.stack([q[1] for q in pr]).astype(np.float32)
    for tag, nv, sc in (("uni", None, None), ("uni_nv_sc", nv32, sc32), ("uni_nv", nv32, None)):
        if tag not in variants:
            continue
        fn = lambda r, a, b: eng.solve_uniform_f32(r, a, b, kb, wv)
        got = fn(rel32, nv, sc)
        a32, curv, st = got[:3]
        a64, curv64, st64 = _solve64(eng, rel32.astype(np.float64), None if nv is None else nv.astype(np.float64),
                                     None if sc is None else sc.astype(np.float64))
        assert np.array_equal(st, st64) and np.all(st == OK), (batch, n, list(st), list(st64))
        assert np.array_equal(a32, a64.astype(np.float32)), "float rows (%s) (%d, %d): alpha is not float32 of the fp64 solve" % (tag, batch, n)
        assert np.array_equal(curv, curv64)
        same_bits_reversed(fn, got, rel32, nv, sc)
    # increment layout
    inc32, org0 = engine.rows_to_increments(ref)
    open32 = inc32.copy()
    open32[:, n // 2, 0] += np.float32(0.3)
    for tag, r32, origin in (("inc", inc32, None), ("inc_origin", inc32, org0), ("open", open32, None), ("open_origin", open32, org0)):
        if tag not in variants:
            continue
        fn = lambda r, o: eng.solve_batch_f32(r, o, kb, wv, layout=engine.F32_INCREMENTS)
        got = fn(r32, origin)
        a32, curv, st = got[:3]
        a64, curv64, st64 = _solve64(eng, glue_ref.rows_increments(r32, origin, LD).astype(np.float64))
        b64, curvb, stb = _solve64(eng, glue_ref.rows_increments(r32, origin, np.float64))
        assert np.array_equal(st, st64) and np.array_equal(st, stb) and np.all(st == OK), (tag, batch, n, list(st), list(st64))
        g_curv = max(CURV_FLOOR, 4.0 * gg.dmax(curvb, curv64))
        g_alpha = max(ALPHA_FLOOR, 4.0 * gg.dmax(b64, a64))
        assert g_curv <= F32_GUARD_CAP * CURV_FLOOR and g_alpha <= F32_GUARD_CAP * ALPHA_FLOOR, (tag, batch, n, g_curv, g_alpha)
        fam = "f32.%s" % tag.split("_")[0]
        d_curv = gg.dmax(curv, curv64)
        worst.add(fam + ".curv_err", d_curv, g_curv)
        assert d_curv <= g_curv, "%s rows (%d, %d): curv_err differs from the fp64 twin's by %.3e (guard %.3e)" % (tag, batch, n, d_curv, g_curv)
        excess = float(np.max(np.abs(a32.astype(np.float64) - a64) - np.abs(a64) * 2.0 ** -24))
        worst.add(fam + ".alpha_beyond_rounding", max(excess, 0.0), g_alpha)
        assert excess <= g_alpha, "%s rows (%d, %d): alpha differs from the fp64 twin by %.3e beyond its float rounding (guard %.3e)" % (tag, batch, n, excess, g_alpha)
        same_bits_reversed(fn, got, r32, origin)
