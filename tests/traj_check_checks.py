"""The shared bodies of tests/test_emu_traj_check.py (SIMT interpreter) and tests/test_gpu_traj_check.py (MI355X): mcq_trajectory_device and
mcq_bound_dists_device through Engine.trajectory_batch / Engine.bound_dists_batch (and the device-pointer variants for the argument errors)
on the cases of tests/traj_check_cases.py, against the longdouble reference of tests/traj_check_ref.py, every quantity held to
max(floor, 4 x spread) of tests/traj_check_guard.py.  Counts, statuses, flags and the copied columns are exact; every launch is repeated in
reversed order and must return the same bits."""
import numpy as np

import glue_cases as gc
import traj_check_cases as tc
import traj_check_guard as tg
import traj_check_ref as tcr
from global_racetrajectory_optimization_amd import engine
from ring_guard import SPREAD_DRAWS, draw_rng

LD = np.longdouble
OK, BAD_INPUT = 0, tc.BAD_INPUT
GGV_BITS = engine.CHK_AY | engine.CHK_AX_POS | engine.CHK_AX_NEG | engine.CHK_A_TOT


def _hold(worst, family, q, dev, spread, what):
    g = tg.guard(q, spread)
    worst.add("%s.%s" % (family, q), dev, g)
    assert dev <= g, "%s: %s deviates by %.3e, guard %.3e" % (what, q, dev, g)


def _same_bits(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


# ---- boundary distances ----------------------------------------------------------------------------------------------------------------
def run_bound(eng, launch, order=None, scalars_of=None):
    """Engine.bound_dists_batch of a launch; order: a permutation of its rows; scalars_of: one row alone with its dimensions as scalars."""
    idx = list(range(len(launch["rows"]))) if order is None else list(order)
    if scalars_of is not None:
        idx = [scalars_of]
    refs, nvs = zip(*[tc.bound_track(launch, k) for k in idx])
    race = tc.pack_race([launch["rows"][k] for k in idx])
    dims = [tc.bound_dims(launch, k) for k in idx]
    if isinstance(launch["length"], list) and scalars_of is None:
        ln, wd = np.array([d[0] for d in dims]), np.array([d[1] for d in dims])
    else:
        ln, wd = dims[0]
    return eng.bound_dists_batch(list(refs), list(nvs), race, ln, wd, stepsize_bound=launch["step"], first_row_only=launch["first_row"])


def check_bound_launch(eng, family, launch, worst):
    name = launch["name"]
    out = run_bound(eng, launch)
    S = tg.spread("%s/bound/%s" % (family, name))
    for k, (_, n, m) in enumerate(launch["rows"]):
        what = "%s/%s row %d (n=%d, m=%d)" % (family, name, k, n, m)
        r0 = tc.bound_ref_cached(family, name, k)
        assert out["status"][k] == OK, what + ": status %d" % out["status"][k]
        assert tuple(out["nb"][k]) == tuple(r0["nb"]), what + ": samples %s, reference %s" % (tuple(out["nb"][k]), r0["nb"])
        _hold(worst, family, "dist", tg.dmax(out["min_dists"][k, :m], r0["min_dists"]), S[k, 0], what + ", per station")
        _hold(worst, family, "dist", tg.dmax(out["min_dist"][k], r0["min_dist"]), S[k, 1], what + ", per track")
        assert out["min_dist"][k] == np.min(out["min_dists"][k, :m]), what + ": min_dist is not the minimum of min_dists"
        dev = max(tg.dmax(out["bound_r"][k, :n], r0["bound_r"]), tg.dmax(out["bound_l"][k, :n], r0["bound_l"]))
        _hold(worst, family, "bound", dev, S[k, 2], what + ", raw boundaries")
        assert np.all(np.isnan(out["min_dists"][k, m:])) and np.all(np.isnan(out["bound_r"][k, n:])) and np.all(np.isnan(out["bound_l"][k, n:])), \
            what + ": entries behind m / n are not NaN"
    order = list(range(len(launch["rows"])))[::-1]
    rev = run_bound(eng, launch, order)
    for k, kr in enumerate(order):
        n, m = launch["rows"][k][1], launch["rows"][k][2]
        for q, cnt in (("min_dists", m), ("bound_r", n), ("bound_l", n)):
            assert _same_bits(out[q][k, :cnt], rev[q][kr, :cnt]), "%s/%s: the reversed launch returns other bits (%s)" % (family, name, q)
        assert _same_bits(out["min_dist"][k], rev["min_dist"][kr]) and tuple(out["nb"][k]) == tuple(rev["nb"][kr])
    if isinstance(launch["length"], list):      # a per-track list next to the scalar: the same bits
        for k, (_, n, m) in enumerate(launch["rows"]):
            one = run_bound(eng, launch, scalars_of=k)
            assert _same_bits(out["min_dists"][k, :m], one["min_dists"][0, :m]) and _same_bits(out["min_dist"][k], one["min_dist"][0]), \
                "%s/%s row %d: the list entry and the scalar give other bits" % (family, name, k)


def check_bound_status_and_arguments(eng, family):
    """MCQ_BAD_INPUT rows between good ones (n < 3, m < 1, a NaN coordinate, a NaN heading, a boundary element of length 0, more samples than the
    scratch holds) leave their neighbours' bits alone and return NaN distances; argument errors are MCQ_E_ARG."""
    rows = [(family, 48, 47), (family, 47, 96), (family, 96, 95)]
    tracks = [gc.ring(f, n)[:2] for f, n, _ in rows]
    race = tc.pack_race(rows)
    refs, nvs = [np.array(t[0]) for t in tracks], [np.array(t[1]) for t in tracks]
    clean = eng.bound_dists_batch(refs, nvs, race, tc.LENGTH_VEH, tc.WIDTH_VEH)
    assert list(clean["status"]) == [OK, OK, OK]

    def bad_middle(refs2, nvs2, race2, what, step=1.0):
        out = eng.bound_dists_batch(refs2, nvs2, race2, tc.LENGTH_VEH, tc.WIDTH_VEH, stepsize_bound=step)
        assert list(out["status"]) == [OK, BAD_INPUT, OK], "%s: statuses %s" % (what, list(out["status"]))
        assert np.all(np.isnan(out["min_dists"][1])) and np.isnan(out["min_dist"][1]), what + ": a MCQ_BAD_INPUT row holds distances"
        for k in (0, 2):
            m = rows[k][2]
            assert _same_bits(out["min_dists"][k, :m], clean["min_dists"][k, :m]) and _same_bits(out["min_dist"][k], clean["min_dist"][k]), \
                what + ": a MCQ_BAD_INPUT row disturbed its neighbours"
        return out
    bad_middle([refs[0], refs[1][:2], refs[2]], [nvs[0], nvs[1][:2], nvs[2]], race, "n = 2")
    r2 = dict(race, m=np.array([47, 0, 95], dtype=np.int32))
    bad_middle(refs, nvs, r2, "m = 0")
    nanref = refs[1].copy()
    nanref[5, 0] = np.nan
    bad_middle([refs[0], nanref, refs[2]], nvs, race, "a NaN coordinate")
    infw = refs[1].copy()
    infw[7, 3] = np.inf
    bad_middle([refs[0], infw, refs[2]], nvs, race, "an infinite width")
    r3 = dict(race, psi=race["psi"].copy())
    r3["psi"][1, 11] = np.nan
    bad_middle(refs, nvs, r3, "a NaN heading")
    dup_ref, dup_nv = refs[1].copy(), nvs[1].copy()
    dup_ref[9], dup_nv[9] = dup_ref[8], dup_nv[8]
    bad_middle([refs[0], dup_ref, refs[2]], [nvs[0], dup_nv, nvs[2]], race, "a boundary element of length 0")
    # more samples than a boundary's scratch holds: every track is refused and reports the samples it would need
    tiny = eng.bound_dists_batch(refs, nvs, race, tc.LENGTH_VEH, tc.WIDTH_VEH, stepsize_bound=1e-4)
    assert list(tiny["status"]) == [BAD_INPUT] * 3 and np.all(tiny["nb"] > 65536) and np.all(np.isnan(tiny["min_dist"]))
    # argument errors through the device-pointer entry
    buf = eng.alloc(1 << 16)
    try:
        good = dict(tracks=1, nmax=8, d_n=None, d_ref=buf, d_nv=buf, mmax=8, d_m=None, d_xy=buf, d_psi=buf, length_veh=4.7, width_veh=2.0,
                    d_length_list=None, d_width_list=None, stepsize_bound=1.0, mode=0, d_min_dists=buf, d_min_dist=buf, d_nb=buf, d_bound=None,
                    d_status=buf)
        for key, val in (("tracks", 0), ("nmax", 2), ("mmax", 0), ("d_ref", None), ("d_nv", None), ("d_xy", None), ("d_psi", None),
                         ("stepsize_bound", 0.0), ("stepsize_bound", float("nan")), ("mode", 2), ("length_veh", float("nan")),
                         ("width_veh", -1.0), ("d_min_dists", None), ("d_min_dist", None), ("d_nb", None), ("d_status", None)):
            try:
                eng.bound_dists_device(**dict(good, **{key: val}))
            except engine.EngineError as e:
                assert "(-1)" in str(e), str(e)           # MCQ_E_ARG
            else:
                raise AssertionError("mcq_bound_dists_device accepted %s = %r" % (key, val))
    finally:
        eng.sync()
        eng.free(buf)


# ---- trajectories ----------------------------------------------------------------------------------------------------------------------
def run_traj(eng, L, order=None, ggv=True, axm=True):
    o = np.arange(len(L["track_of"])) if order is None else np.asarray(order)
    return eng.trajectory_batch(L["race"], L["vx"][o], L["ggv"][o] if ggv else None, L["axm"][o] if axm else None, L["drag"][o], L["mass"][o],
                                L["vmax"][o], L["curvlim"], track_of=L["track_of"][o], closed=L["closed"])


def hold_variant(worst, family, out, v, ref, S, what, inputs):
    """One variant of a result against (trajectory dict, limits, flags) of the reference; inputs: (xy, psi, kappa, vx) rows it copies."""
    T, lim, flags = ref
    m = T["traj"].shape[0]
    ne = T["t"].shape[0] - 1
    row = out["traj"][v]
    _hold(worst, family, "s", tg.dmax(row[:m, 0], T["traj"][:, 0]), S[0], what)
    _hold(worst, family, "ax", tg.dmax(row[:m, 6], T["traj"][:, 6]), S[1], what)
    _hold(worst, family, "t", tg.dmax(out["t"][v, :ne + 1], T["t"]), S[2], what)
    _hold(worst, family, "length", tg.dmax(out["length"][v], T["length"]), S[3], what)
    for q in range(6):
        _hold(worst, family, tg.TRAJ_Q[4 + q], tg.dmax(out["limits"][v, q], lim[q]), S[4 + q], what + ", limit %s" % tcr.LIMITS[q])
    xy, psi, kappa, vx = inputs
    assert _same_bits(row[:m, 1:3], xy[:m]) and _same_bits(row[:m, 3], psi[:m]) and _same_bits(row[:m, 4], kappa[:m]) and \
        _same_bits(row[:m, 5], vx[:m]), what + ": a copied column differs from its input"
    assert out["t"][v, 0] == 0.0 and row[0, 0] == 0.0
    assert np.all(np.isnan(row[m:])) and np.all(np.isnan(out["t"][v, ne + 1:])), what + ": entries behind the last row / time are not NaN"
    assert out["flags"][v] == flags, what + ": flags %d, reference %d" % (out["flags"][v], flags)


def check_traj_launch(eng, family, name, L, worst, expected_flags=None):
    out = run_traj(eng, L)
    S = tg.spread("%s/traj/%s" % (family, name))
    for v, t in enumerate(L["track_of"]):
        T, lim, flags, _ = tc.traj_reference(L, v)
        if expected_flags is not None:
            assert flags == expected_flags
        hold_variant(worst, family, out, v, (T, lim, flags), S[v], "%s/%s variant %d" % (family, name, v),
                     (L["race"]["xy"][t], L["race"]["psi"][t], L["race"]["kappa"][t], L["vx"][v]))
    order = np.arange(len(L["track_of"]))[::-1]
    rev = run_traj(eng, L, order)
    for q in ("traj", "t", "length", "limits", "flags"):
        assert _same_bits(out[q], rev[q][::-1]), "%s/%s: the reversed launch returns other bits (%s)" % (family, name, q)
    return out


def check_null_tables(eng, family):
    """ggv == NULL leaves the four ggv bits 0, ax_max_machines == NULL the machine bit; everything else keeps its bits."""
    for name, L, bit in tc.flag_launches(family):
        full = run_traj(eng, L)
        assert full["flags"][0] == bit, "%s/%s: flags %d" % (family, name, full["flags"][0])
        for ggv, axm, mask in ((False, True, GGV_BITS), (True, False, engine.CHK_MACHINES), (False, False, GGV_BITS | engine.CHK_MACHINES)):
            part = run_traj(eng, L, ggv=ggv, axm=axm)
            assert part["flags"][0] == bit & ~mask, "%s/%s without %s: flags %d" % (family, name, "ggv" if not ggv else "machines", part["flags"][0])
            for q in ("traj", "t", "length", "limits"):
                assert _same_bits(part[q], full[q])


def check_lap_time_bitwise(eng, family, closed):
    """t_out[m] (closed) / t_out[m - 1] (unclosed) IS the lap_time_out of the velocity kernel on the same arrays, bit for bit; vx too."""
    L = tc.traj_launch(family, closed)
    race = L["race"]
    bsz = len(L["track_of"])
    v_start = 5.0 + np.arange(bsz)
    vx, lap = eng.vel_profile_batch(race["kappa"], race["el_lengths"], L["ggv"], L["axm"], L["drag"], L["mass"], L["vmax"], dyn_model_exp=1.0,
                                    track_of=L["track_of"], n_of_track=race["m"], closed=closed, v_start=None if closed else v_start)
    out = eng.trajectory_batch(race, vx, L["ggv"], L["axm"], L["drag"], L["mass"], L["vmax"], L["curvlim"], track_of=L["track_of"], closed=closed)
    for v, t in enumerate(L["track_of"]):
        m = int(race["m"][t])
        last = out["t"][v, m if closed else m - 1]
        assert np.isfinite(lap[v]) and _same_bits(last, lap[v]), "%s variant %d (m=%d): t_out %r, lap_time_out %r" % (family, v, m, last, lap[v])
        assert _same_bits(out["traj"][v, :m, 5], vx[v, :m])


def check_traj_nan_and_status(eng, family):
    """A row length outside [2, mmax] or a NaN in a vx row: NaN rows, times, length and limits, flags -1; the neighbours keep their bits."""
    L = tc.traj_launch(family, True)
    clean = run_traj(eng, L)
    assert np.all(clean["flags"] >= 0)
    mmax = L["race"]["xy"].shape[1]
    for what, m_bad, nan_at in (("m = 1", 1, None), ("m = mmax + 1", mmax + 1, None), ("m = 0", 0, None), ("a NaN in vx", None, 200)):
        race = dict(L["race"], m=L["race"]["m"].copy())
        vx = L["vx"].copy()
        t_bad = 4                                # the row of 257 stations
        hit = [v for v, t in enumerate(L["track_of"]) if t == t_bad]
        if m_bad is not None:
            race["m"][t_bad] = m_bad
        else:
            vx[hit[0], nan_at] = np.nan
            hit = hit[:1]
        out = eng.trajectory_batch(race, vx, L["ggv"], L["axm"], L["drag"], L["mass"], L["vmax"], L["curvlim"], track_of=L["track_of"], closed=True)
        for v in range(len(L["track_of"])):
            if v in hit:
                assert out["flags"][v] == -1 and np.all(np.isnan(out["traj"][v])) and np.all(np.isnan(out["t"][v])) and \
                    np.isnan(out["length"][v]) and np.all(np.isnan(out["limits"][v])), "%s: variant %d is not flagged" % (what, v)
            else:
                assert all(_same_bits(out[q][v], clean[q][v]) for q in ("traj", "t", "length", "limits", "flags")), \
                    "%s: a flagged variant disturbed variant %d" % (what, v)


def check_traj_arguments(eng):
    buf = eng.alloc(1 << 16)
    try:
        good = dict(batch=1, m=8, mmax=8, d_m_of_track=None, d_track_of=None, d_xy=buf, d_psi=buf, d_kappa=buf, d_el=buf, d_vx=buf, closed=True,
                    d_drag=buf, d_mass=buf, d_vmax=buf, d_ggv=None, n_ggv=0, d_axm=None, n_machines=0, curvlim=0.12, d_traj=None, d_t=None,
                    d_length=buf, d_limits=buf, d_flags=buf)
        eng.trajectory_device(**good)            # (zero-filled buffers: a legal call)
        for key, val in (("batch", 0), ("mmax", 1), ("m", 1), ("m", 9), ("d_xy", None), ("d_psi", None), ("d_kappa", None), ("d_el", None),
                         ("d_vx", None), ("d_drag", None), ("d_mass", None), ("d_vmax", None), ("curvlim", float("nan")), ("d_length", None),
                         ("d_limits", None), ("d_flags", None)):
            try:
                eng.trajectory_device(**dict(good, **{key: val}))
            except engine.EngineError as e:
                assert "(-1)" in str(e), str(e)           # MCQ_E_ARG
            else:
                raise AssertionError("mcq_trajectory_device accepted %s = %r" % (key, val))
        for key, val in (("d_ggv", buf), ("d_axm", buf)):   # a table without rows
            try:
                eng.trajectory_device(**dict(good, **{key: val}))
            except engine.EngineError as e:
                assert "(-1)" in str(e), str(e)
            else:
                raise AssertionError("mcq_trajectory_device accepted a table of 0 rows")
    finally:
        eng.sync()
        eng.free(buf)


# ---- end to end: solve -> raceline -> profile -> trajectory -> check -----------------------------------------------------------------------
ALPHA_CONTRACT = 1e-6
E2E_STEP, E2E_BOUND_STEP = 6.0, 4.0         # m: stations of the raceline, samples of the boundaries (below tc.MAX_PAIRS on the interpreter)


def check_end_to_end(eng, golden, worst):
    """The Berlin golden: solve_batch, its alpha held to the golden; raceline_batch on that alpha; vel_profile_batch on the kernel's own rows;
    trajectory_batch and bound_dists_batch on all of it, held to the reference ON THE SAME ARRAYS under the guards (spreads computed live: no stored
    entry can know the engine's own rows); the last time is the profile's lap time bit for bit; the flags are the reference's."""
    g = golden
    ref, nv = g["reftrack"], g["normvec"]
    al, _, st, _ = eng.solve_batch([dict(reftrack=ref, normvec=nv, scaling=g["scaling"], kappa_bound=float(g["kappa_bound"]), w_veh=float(g["w_veh"]))])
    d = float(np.max(np.abs(al[0] - g["alpha"])))
    assert st[0] == OK and d < ALPHA_CONTRACT, (st[0], d)
    race = eng.raceline_batch([ref], [nv], al, E2E_STEP)
    assert race["status"][0] == OK
    m = int(race["m"][0])
    rng = gc._seed("traj", "e2e")
    ggv, axm, drag, mass, vmax = gc._vehicle(rng, 19, on_grid=False)
    vx, lap = eng.vel_profile_batch(race["kappa"], race["el_lengths"], ggv[None], axm[None], drag, mass, vmax, n_of_track=race["m"])
    curvlim = float(g["kappa_bound"])
    out = eng.trajectory_batch(race, vx, ggv[None], axm[None], drag, mass, vmax, curvlim)
    assert _same_bits(out["t"][0, m], lap[0]), "the last time %r is not the profile's lap time %r" % (out["t"][0, m], lap[0])
    L = dict(rows=None, race=race, track_of=np.zeros(1, dtype=np.int32), vx=vx, ggv=ggv[None], axm=axm[None], drag=np.array([drag]),
             mass=np.array([mass]), vmax=np.array([vmax]), curvlim=curvlim, closed=True)

    def traj_ref(dtype=LD, p=None):
        p = p or (lambda a: a)
        T = tcr.trajectory(p(race["xy"][0, :m]), p(race["psi"][0, :m]), p(race["kappa"][0, :m]), p(race["el_lengths"][0, :m]), p(vx[0, :m]), True, dtype)
        lim = tcr.limits(T["traj"], p(L["drag"])[0], p(L["mass"])[0], dtype)
        return T, lim
    T0, lim0 = traj_ref()
    flags, gaps = tcr.verdicts(lim0, ggv, axm, vmax, curvlim, LD)
    assert min(gaps.values()) >= tc.DECISION_GAP
    S = np.asarray(tg.traj_deviations(traj_ref(np.float64), (T0, lim0)))
    for dr in range(SPREAD_DRAWS):
        S = np.maximum(S, tg.traj_deviations(traj_ref(LD, tg._perturber(draw_rng("traj_check/e2e", "traj", 0, dr))), (T0, lim0)))
    hold_variant(worst, "e2e", out, 0, (T0, lim0, flags), S, "end to end: trajectory", (race["xy"][0], race["psi"][0], race["kappa"][0], vx[0]))

    def bound_ref(dtype=LD, p=None):
        p = p or (lambda a: a)
        return tcr.bound_dists(p(ref), p(nv), p(race["xy"][0, :m]), p(race["psi"][0, :m]), tc.LENGTH_VEH, tc.WIDTH_VEH, E2E_BOUND_STEP, False, dtype)
    b0 = bound_ref()
    assert min(tc.gap_to_integer(q) for q in b0["ratios"]) >= tc.INTEGER_GAP
    bd = eng.bound_dists_batch([ref], [nv], race, tc.LENGTH_VEH, tc.WIDTH_VEH, stepsize_bound=E2E_BOUND_STEP)
    assert bd["status"][0] == OK and tuple(bd["nb"][0]) == tuple(b0["nb"])
    SB = np.asarray(tg.bound_deviations(bound_ref(np.float64), b0))
    for dr in range(SPREAD_DRAWS):
        SB = np.maximum(SB, tg.bound_deviations(bound_ref(LD, tg._perturber(draw_rng("traj_check/e2e", "bound", 0, dr))), b0))
    _hold(worst, "e2e", "dist", tg.dmax(bd["min_dists"][0, :m], b0["min_dists"]), SB[0], "end to end: distances per station")
    _hold(worst, "e2e", "dist", tg.dmax(bd["min_dist"][0], b0["min_dist"]), SB[1], "end to end: the track's distance")
    n = ref.shape[0]
    _hold(worst, "e2e", "bound", max(tg.dmax(bd["bound_r"][0, :n], b0["bound_r"]), tg.dmax(bd["bound_l"][0, :n], b0["bound_l"])), SB[2],
          "end to end: raw boundaries")
    assert bd["min_dist"][0] > 0.0
