"""The bodies of tests/test_emu_vel_forms.py (SIMT interpreter) and tests/test_gpu_vel_forms.py (MI355X): the launches of tests/vel_forms_cases.py
through Engine.vel_profile_batch(closed=, loc_gg=, v_start=, v_end=) -- mcq_vel_profile_device_forms -- against oracle/vel_ref.py under the
guards of tests/vel_forms_guard.py, the NaN / +inf / MCQ_E_ARG rules of the entry, and the closed / ggv form through the new entry against the
three old ones, bit for bit.  Every function takes the engine and a ring_guard.Worst.  Every launch is run a second time in reversed variant
order and must return the same bits."""
import ctypes

import numpy as np
import pytest

import glue_cases as gc
import vel_forms_cases as fc
import vel_forms_guard as fg
from global_racetrajectory_optimization_amd import engine

E_ARG = -1                  # MCQ_E_ARG
STALE = 123.0               # what the output buffers of forms_call hold before the launch


def _take(a, o):
    return None if a is None else a[o]


def run(eng, F, order=None, **over):
    """One forms launch through the Python interface; order: the variants in another order; over: keywords that replace the launch's."""
    o = np.arange(F["axm"].shape[0]) if order is None else np.asarray(order)
    kw = dict(dyn_model_exp=F["exp"], track_of=F["track_of"][o], n_of_track=F["n_of_track"], mu=F["mu"], filt_window=F["filt_window"],
              closed=F["closed"], loc_gg=F["loc_gg"], v_start=_take(F["v_start"], o), v_end=_take(F["v_end"], o))
    kw.update(over)
    ggv = None if kw["loc_gg"] is not None else F["ggv"][o]
    return eng.vel_profile_batch(F["kappa"], F["el"], ggv, F["axm"][o], F["drag"][o], F["mass"][o], F["vmax"][o], **kw)


def lateral_limit(F, v):
    """sqrt(ay_max_i R_i) of variant v's row (local limits), cut at v_max: what no point of the profile may exceed."""
    t, n = fc.row(F, v)
    kap = F["kappa"][t, :n]
    with np.errstate(divide="ignore"):
        rad = np.where(kap != 0.0, np.abs(1.0 / np.where(kap != 0.0, kap, 1.0)), np.inf)
    return np.minimum(np.sqrt(F["loc_gg"][t, :n, 1] * rad), F["vmax"][v])


def check_launch(eng, F, worst):
    kind, name = F["kind"], F["name"]
    vx, lt = run(eng, F)
    bsz, nmax = F["axm"].shape[0], F["kappa"].shape[1]
    if F["parity"]:
        S = fg.spread(fg.key(F))
        for v in range(bsz):
            what = "velocity profile %s/%s variant %d" % (kind, name, v)
            r = fg.ref_case(F, v)
            n = r[0].size
            for qi, (q, dev) in enumerate((("vx", fg.dmax(vx[v, :n], r[0])), ("lap", fg._dlap(float(lt[v]), r[1])))):
                g = fg.guard(q, S[v, qi])
                worst.add("%s.%s" % (kind, q), dev, g)
                assert dev <= g, "%s: %s deviates by %.3e, guard %.3e" % (what, q, dev, g)
    else:
        # the reference has no answer to the floor here (vel_forms_cases.py): what is decided
        for v in range(bsz):
            what = "velocity profile %s/%s variant %d" % (kind, name, v)
            n = fc.row(F, v)[1]
            p = vx[v, :n]
            assert not np.any(np.isnan(p)) and not np.isnan(lt[v]), what
            # a moving average of fw speeds <= v_max, summed as fw products v_i (1 / fw) in floating point, is <= v_max to the roundings of
            # 1 / fw, of every product and of every addition: (fw + 1) 2^-53 relative; without a filter the bound is exact
            fw = F["filt_window"] if (F["filt_window"] or 0) > 1 else 0
            over = float(np.max(p / F["vmax"][v] - 1.0))
            worst.add("%s.above_v_max_rel" % kind, max(over, 0.0), (fw + 1) * 2.0 ** -53 if fw else 0.0)
            assert over <= ((fw + 1) * 2.0 ** -53 if fw else 0.0), what + ": above v_max by %.3e (relative)" % over
            if not fw:
                lim = lateral_limit(F, v)
                assert np.all(p <= lim * (1.0 + 2.0 ** -52)), what + ": above the local lateral limit"
            moving = np.all(p[:-1] + p[1:] > 0.0) and (not F["closed"] or p[-1] + p[0] > 0.0)
            assert np.isfinite(lt[v]) == bool(moving) and lt[v] > 0.0, what + ": time %r" % lt[v]
    order = np.arange(bsz)[::-1]
    vx2, lt2 = run(eng, F, order)
    for v in range(bsz):
        n = fc.row(F, v)[1]
        n = n if 2 <= n <= nmax else nmax
        assert np.array_equal(vx[v, :n], vx2[bsz - 1 - v, :n], equal_nan=True) and np.array_equal(lt[v], lt2[bsz - 1 - v], equal_nan=True), \
            "velocity profile %s/%s variant %d: other bits in the reversed launch" % (kind, name, v)


# ---- the entry itself, below the Python interface ----------------------------------------------------------------------------------------
def forms_call(eng, L, closed=True, loc_gg=None, v_start=None, v_end=None, ggv="launch", mu="launch", filt_window="launch", n_ggv=None, order=None,
               forms_null=False):
    """mcq_vel_profile_device_forms on the arrays of a launch through Engine.alloc / upload / download.  Returns (rc, vx [batch, nmax], time
    [batch]); the output buffers hold STALE before the launch."""
    o = np.arange(L["axm"].shape[0]) if order is None else np.asarray(order)
    bsz, nmax = o.size, L["kappa"].shape[1]
    ggv = L["ggv"][o] if isinstance(ggv, str) else ggv
    mu = L["mu"] if isinstance(mu, str) else mu
    fw = L["filt_window"] if isinstance(filt_window, str) else filt_window
    with eng.scope() as dev:
        def up(a, dtype=np.float64):
            return dev.up(None if a is None else np.asarray(a, dtype=dtype))
        d_vx, d_lt = up(np.full((bsz, nmax), STALE)), up(np.full(bsz, STALE))
        vf = engine.McqVelForms(float(L["exp"]), int(fw or 0), 1 if closed else 0, up(mu), up(loc_gg),
                                up(None if v_start is None else np.broadcast_to(np.asarray(v_start, dtype=np.float64), (bsz,))),
                                up(None if v_end is None else np.broadcast_to(np.asarray(v_end, dtype=np.float64), (bsz,))))
        rc = eng.lib.mcq_vel_profile_device_forms(eng.h, bsz, nmax, nmax, up(L["n_of_track"], np.int32), up(L["track_of"][o], np.int32), up(L["kappa"]),
                                                  up(L["el"]), up(ggv), (0 if ggv is None else ggv.shape[1]) if n_ggv is None else n_ggv,
                                                  up(L["axm"][o]), L["axm"].shape[1], up(L["drag"][o]), up(L["mass"][o]), up(L["vmax"][o]),
                                                  None if forms_null else ctypes.byref(vf), d_vx, d_lt)
        if rc != 0:
            return rc, None, None
        eng.sync()
        return rc, eng.download(d_vx, (bsz, nmax), np.float64), eng.download(d_lt, (bsz,), np.float64)


def _rows_equal(L, a, b, flip=False):
    bsz, nmax = L["axm"].shape[0], L["kappa"].shape[1]
    for v in range(bsz):
        n = fc.row(L, v)[1]
        n = n if 2 <= n <= nmax else nmax
        w = bsz - 1 - v if flip else v
        if not (np.array_equal(a[0][v, :n], b[0][w, :n], equal_nan=True) and np.array_equal(a[1][v], b[1][w], equal_nan=True)):
            return False
    return True


def check_existing_form_untouched(eng, L):
    """closed = 1, a ggv and no loc_gg through the new entry: BITWISE what vel_profile_batch returns through the three old entries."""
    old = eng.vel_profile_batch(L["kappa"], L["el"], L["ggv"], L["axm"], L["drag"], L["mass"], L["vmax"], dyn_model_exp=L["exp"],
                                track_of=L["track_of"], n_of_track=L["n_of_track"], mu=L["mu"], filt_window=L["filt_window"])
    rc, vx, lt = forms_call(eng, L, closed=True, v_start=np.nan, v_end=np.nan)       # (closed: v_start / v_end are not read)
    assert rc == 0
    assert _rows_equal(L, old, (vx, lt)), "launch %s: the closed / ggv form through mcq_vel_profile_device_forms returns other bits" % L["name"]


def _launch(kind, name):
    return [F for F in fc.launches(kind) if F["name"] == name][0]


def check_filter_ends(eng):
    """tph.conv_filt(closed=False) on unclosed rows, fw in {none, 1, 3, 7, n}: the w = (fw - 1) / 2 entries at both ends are the unfiltered
    profile's bit for bit (fw <= 1: the whole row), the entries between are not (fw >= 3: parity with the oracle is check_launch's, on the
    launches that carry a window)."""
    for kind, name in (("open", "n17"), ("open", "n65"), ("open_locgg", "n17"), ("open_locgg_flat", "n257")):
        F = _launch(kind, name)
        n = F["kappa"].shape[1]
        plain = run(eng, F, filt_window=None)
        for fw in (1, 3, 7, n if n % 2 else n - 1):
            vx, lt = run(eng, F, filt_window=fw)
            w = (fw - 1) // 2
            what = "%s/%s fw=%d" % (kind, name, fw)
            assert np.array_equal(vx[:, :w], plain[0][:, :w]) and np.array_equal(vx[:, n - w:], plain[0][:, n - w:]), what + ": the ends moved"
            if fw == 1:
                assert np.array_equal(vx, plain[0]) and np.array_equal(lt, plain[1]), what
            else:
                assert not np.array_equal(vx[:, w:n - w], plain[0][:, w:n - w]), what + ": nothing filtered"
                from oracle import vel_ref
                for v in range(0, vx.shape[0], 5):
                    assert fg.dmax(vx[v], vel_ref.conv_filt(plain[0][v], fw, False)) <= fg.FLOOR["vx"], what


def check_standing_two_points(eng):
    """Two points, v_start = v_end = 0: vx = (0, 0) and the time of the one element is 2 l / 0 = +inf -- not an error, not a NaN.  The other
    variants of the launch are what they are without that neighbour."""
    F = _launch("open", "n2")
    F2 = _launch("open_locgg", "n2")
    for G in (F, F2):
        vx, lt = run(eng, G, v_start=0.0, v_end=0.0)
        assert np.array_equal(vx, np.zeros_like(vx)) and np.all(np.isposinf(lt)), (vx, lt)
        r = fg.ref_case(dict(G, v_start=np.zeros(1), v_end=np.zeros(1)), 0)
        assert np.array_equal(r[0], np.zeros(2)) and np.isposinf(r[1])
    G = _launch("open", "ragged_plain")                 # rows of 2 .. 65 points side by side: only the standing two-point rows are +inf
    vx, lt = run(eng, G, v_start=0.0, v_end=0.0)
    two = np.array([fc.row(G, v)[1] == 2 for v in range(lt.size)])
    assert two.any() and np.all(np.isposinf(lt[two])) and np.all(np.isfinite(lt[~two])) and not np.any(np.isnan(vx[~two, :2]))


def check_negative_speeds(eng):
    """Negative v_start / v_end count as 0, as upstream: the same bits."""
    for kind, name in (("open", "n17"), ("open_locgg", "ragged_plain")):
        F = _launch(kind, name)
        bsz = F["axm"].shape[0]
        zero = run(eng, F, v_start=np.zeros(bsz), v_end=np.zeros(bsz))
        neg = run(eng, F, v_start=-np.linspace(0.5, 40.0, bsz), v_end=np.full(bsz, -1e-300))
        assert np.array_equal(zero[0], neg[0]) and np.array_equal(zero[1], neg[1]), (kind, name)
        some = F["v_start"].copy()
        some[::3] = -7.0
        ref = F["v_start"].copy()
        ref[::3] = 0.0
        a, b = run(eng, F, v_start=some), run(eng, F, v_start=ref)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (kind, name)


def check_v_end_forms(eng):
    """v_end NULL == an array of NaNs; a NaN for some variants of a launch only leaves exactly those without an end speed; v_end above every
    limit changes nothing."""
    for kind, name in (("open", "n64"), ("open_locgg_flat", "n17")):
        F = _launch(kind, name)
        bsz = F["axm"].shape[0]
        none = run(eng, F, v_end=None)
        nans = run(eng, F, v_end=np.full(bsz, np.nan))
        high = run(eng, F, v_end=np.full(bsz, 1e9))
        assert np.array_equal(none[0], nans[0]) and np.array_equal(none[1], nans[1]) and np.array_equal(none[0], high[0]), (kind, name)
        stop = run(eng, F, v_end=np.zeros(bsz))
        mixed_ve = np.where(np.arange(bsz) % 2 == 0, np.nan, 0.0)
        mixed = run(eng, F, v_end=mixed_ve)
        ev = np.arange(bsz) % 2 == 0
        assert np.array_equal(mixed[0][ev], none[0][ev]) and np.array_equal(mixed[0][~ev], stop[0][~ev]), (kind, name)
        assert np.array_equal(mixed[1][ev], none[1][ev]) and np.array_equal(mixed[1][~ev], stop[1][~ev]), (kind, name)
        n = F["kappa"].shape[1]
        assert np.all(stop[0][:, n - 1] == 0.0) and np.all(none[0][:, n - 1] > 0.0)


def check_start_against_the_lateral_limit(eng):
    """The first point never exceeds v_start, nor what it is without a start speed; the case tables hold start speeds on both sides of that
    (counted here on what the device returns)."""
    below = above = 0
    for kind in ("open", "open_locgg"):
        F = _launch(kind, "n130")
        vx, _ = run(eng, F, filt_window=None)
        free, _ = run(eng, F, filt_window=None, v_start=np.full(vx.shape[0], 1e9), v_end=None)
        for v in range(vx.shape[0]):
            vs = F["v_start"][v]
            below += vs < free[v, 0]
            above += vs > free[v, 0]
            assert vx[v, 0] <= min(vs, free[v, 0]), (kind, v)      # (the backward sweep may still lower it: parity is check_launch's)
    assert below >= 4 and above >= 2


def check_timed(eng):
    """timed=True adds the device time of the launch and changes nothing else, for the old entries and the new one."""
    for kind, name in (("open", "n65"), ("locgg", "n17")):
        F = _launch(kind, name)
        a, b = run(eng, F), run(eng, F, timed=True)
        assert len(b) == 3 and b[2] >= 0.0 and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    L = [x for x in gc.vel_launches() if x["name"] == "n17"][0]
    arg = (L["kappa"], L["el"], L["ggv"], L["axm"], L["drag"], L["mass"], L["vmax"])
    a, b = eng.vel_profile_batch(*arg, track_of=L["track_of"]), eng.vel_profile_batch(*arg, track_of=L["track_of"], timed=True)
    assert len(b) == 3 and b[2] >= 0.0 and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def check_nan_rules(eng):
    """Everything that flags a variant: lap_time NaN and a NaN row (never STALE buffer contents), per variant -- the neighbours are computed."""
    base = [L for L in gc.vel_launches() if L["name"] == "nan_rows"][0]
    bsz, nmax = base["axm"].shape[0], base["kappa"].shape[1]
    T = base["kappa"].shape[0]
    lg = np.stack([fc.loc_gg_row("open_locgg", "nan_rows", t, nmax) for t in range(T)])
    vs0 = np.full(bsz, 5.0)
    for closed, loc in ((False, None), (True, lg), (False, lg)):
        kw = dict(closed=closed, loc_gg=loc, v_start=None if closed else vs0)
        if loc is not None:
            kw.update(ggv=None, mu=None)
        # bad row lengths (n = 1, n = 66 > nmax)
        rc, vx, lt = forms_call(eng, base, **kw)
        assert rc == 0
        for v in range(bsz):
            n = fc.row(base, v)[1]
            if n < 2 or n > nmax:
                assert np.isnan(lt[v]) and np.all(np.isnan(vx[v])), (closed, v)
            else:
                assert np.isfinite(lt[v]) and np.all(np.isfinite(vx[v, :n])) and np.all(vx[v, n:] == STALE), (closed, v)
        good = np.isfinite(lt)
        # a machine table that ends below v_max; a ggv that does (only where there is one)
        L = dict(base, vmax=base["vmax"].copy())
        L["vmax"][::4] = 80.0
        rc, vx2, lt2 = forms_call(eng, L, **kw)
        hit = np.arange(bsz) % 4 == 0
        assert rc == 0 and np.all(np.isnan(lt2[hit])) and np.array_equal(lt2[~hit], lt[~hit], equal_nan=True)
        assert all(np.all(np.isnan(vx2[v, :max(2, min(fc.row(base, v)[1], nmax))])) for v in np.nonzero(hit)[0])
        if loc is None:
            L = dict(base, axm=base["axm"].copy(), vmax=base["vmax"].copy())
            L["axm"][:, -1, 0] = 90.0
            L["vmax"][1::4] = 80.0                  # the machine table reaches, the diagram (72 m/s) does not
            rc, _, lt3 = forms_call(eng, L, **kw)
            assert rc == 0 and np.all(np.isnan(lt3[1::4])) and np.all(np.isfinite(lt3[good & (np.arange(bsz) % 4 != 1)]))
        else:                                       # local limits: ONLY the machine table is range-checked
            L = dict(base, axm=base["axm"].copy(), vmax=base["vmax"].copy())
            L["axm"][:, -1, 0] = 90.0
            L["vmax"][1::4] = 80.0
            rc, _, lt3 = forms_call(eng, L, **kw)
            assert rc == 0 and np.array_equal(np.isfinite(lt3), good)
        # an even filter window, one wider than the row (rows of 5, 17, 64 entries: fw = 7 flags the rows of 5)
        rc, _, lt4 = forms_call(eng, base, filt_window=4, **kw)
        assert rc == 0 and np.all(np.isnan(lt4))
        rc, vx5, lt5 = forms_call(eng, base, filt_window=7, **kw)
        ns = np.array([fc.row(base, v)[1] for v in range(bsz)])
        assert rc == 0 and np.all(np.isnan(lt5[ns < 7])) and np.array_equal(np.isfinite(lt5), good & (ns >= 7))
        # a start speed that is not finite
        if not closed:
            for bad in (np.nan, np.inf, -np.inf):
                vs = vs0.copy()
                vs[2::5] = bad
                rc, vx6, lt6 = forms_call(eng, base, **dict(kw, v_start=vs))
                hit = np.arange(bsz) % 5 == 2
                assert rc == 0 and np.all(np.isnan(lt6[hit])) and np.array_equal(lt6[~hit], lt[~hit], equal_nan=True), bad
                assert all(np.all(np.isnan(vx6[v, :max(2, min(ns[v], nmax))])) for v in np.nonzero(hit)[0]) and np.array_equal(vx6[~hit], vx[~hit], equal_nan=True)


def check_argument_errors(eng):
    """Every MCQ_E_ARG of the entry, and every argument error of tph.calc_vel_profile in upstream's words through the Python interface."""
    L = [x for x in gc.vel_launches() if x["name"] == "n17"][0]
    T, n = L["kappa"].shape
    lg = np.stack([fc.loc_gg_row("locgg", "n17", t, n) for t in range(T)])
    assert L["mu"] is not None
    ok = dict(ggv=None, mu=None)
    assert forms_call(eng, L, loc_gg=lg, **ok)[0] == 0
    assert forms_call(eng, L, loc_gg=lg, mu=None)[0] == E_ARG                            # loc_gg and a ggv
    assert forms_call(eng, L, loc_gg=lg, ggv=None)[0] == E_ARG                           # loc_gg and mu
    assert forms_call(eng, L, loc_gg=lg, n_ggv=2, **ok)[0] == E_ARG                      # loc_gg and n_ggv != 0
    assert forms_call(eng, L, ggv=None, mu=None)[0] == E_ARG                             # neither
    assert forms_call(eng, L, ggv=None)[0] == E_ARG
    assert forms_call(eng, L, n_ggv=0)[0] == E_ARG                                       # a ggv of no rows
    assert forms_call(eng, L, closed=False)[0] == E_ARG                                  # unclosed without v_start
    assert forms_call(eng, L, closed=False, loc_gg=lg, **ok)[0] == E_ARG
    assert forms_call(eng, L, closed=False, v_start=1.0)[0] == 0
    assert forms_call(eng, L, forms_null=True)[0] == E_ARG
    assert forms_call(eng, L, filt_window=-3)[0] == E_ARG
    assert b"mcq_vel_profile" in eng.lib.mcq_last_error()

    def call(**kw):
        a = dict(kappa=L["kappa"], el_lengths=L["el"], ggv=L["ggv"], ax_max_machines=L["axm"], drag_coeff=L["drag"], m_veh=L["mass"],
                 v_max=L["vmax"], track_of=L["track_of"])
        a.update(kw)
        return eng.vel_profile_batch(**a)
    with pytest.raises(RuntimeError, match=r"Either ggv and optionally mu OR loc_gg must be supplied, not both \(or all\) of them!"):
        call(loc_gg=lg)
    with pytest.raises(RuntimeError, match=r"Either ggv and optionally mu OR loc_gg must be supplied, not both \(or all\) of them!"):
        call(ggv=None, loc_gg=lg, mu=L["mu"])
    with pytest.raises(RuntimeError, match="Either ggv or loc_gg must be supplied!"):
        call(ggv=None)
    with pytest.raises(RuntimeError, match="v_max must be supplied if loc_gg is used!"):
        call(ggv=None, loc_gg=lg, v_max=None)
    for bad in (lg[:, :-1], lg[:, :, :1], lg[0], np.zeros((T, n, 3))):
        with pytest.raises(RuntimeError, match=r"loc_gg must have the shape \[no_points, 2\]!"):
            call(ggv=None, loc_gg=bad)
    with pytest.raises(RuntimeError, match="v_start must be provided for the unclosed case!"):
        call(closed=False)
    with pytest.raises(RuntimeError, match="v_start must be provided for the unclosed case!"):
        call(ggv=None, loc_gg=lg, closed=False, v_end=3.0)
    with pytest.raises(RuntimeError, match="ax_max_machines has to cover the entire velocity range"):
        call(ggv=None, loc_gg=lg, v_max=80.0)
    with pytest.raises(RuntimeError, match="Window width of moving average filter must be odd!"):
        call(closed=False, v_start=0.0, filt_window=4)
    vx, lt = call(ggv=None, loc_gg=lg, closed=False, v_start=2.0, v_end=1.0)              # scalars for v_start / v_end
    assert vx.shape == (L["axm"].shape[0], n) and np.all(vx[:, 0] <= 2.0) and np.all(vx[:, -1] <= 1.0) and np.all(np.isfinite(lt))
