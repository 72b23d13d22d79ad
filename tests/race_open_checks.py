"""The bodies of tests/test_emu_race_open.py (SIMT interpreter) and tests/test_gpu_race_open.py (MI355X): the launches of tests/race_open_cases.py
through Engine.raceline_batch(ends=...) / mcq_raceline_device_ends against tests/race_open_ref.py in longdouble under the guards of
tests/race_open_guard.py.  Point counts and statuses are compared exactly; every launch is run a second time in reversed order and must return
the same bits.  Every function takes the engine and a ring_guard.Worst that collects the worst deviation next to the guard it was held to."""
import numpy as np

import glue_cases as gc
import glue_checks as gck
import race_open_cases as oc
import race_open_guard as og
import race_open_ref as ror
import vel_forms_guard as vg
from global_racetrajectory_optimization_amd import engine
from ring_guard import SPREAD_DRAWS, SPREAD_REL, draw_rng

LD = np.longdouble
OK, BAD_INPUT = 0, engine.STATUS_BAD_INPUT
QUANTITIES = ("xy", "psi", "kappa", "el_lengths")


def _hold(worst, family, quantity, dev, spread, what):
    g = og.guard(quantity, spread)
    worst.add("%s.%s" % (family, quantity), dev, g)
    assert dev <= g, "%s: %s deviates by %.3e, guard %.3e" % (what, quantity, dev, g)


def _arcs(family, sizes):
    a = [oc.arc(family, n) for n in sizes]
    return [x[0] for x in a], [x[1] for x in a], [x[2] for x in a], oc.ends_of(family, sizes)


def rows_equal(a, b, ka, kb):
    """Row ka of result a and row kb of result b: same status, same m, same bits in the m valid entries."""
    if a["status"][ka] != b["status"][kb] or a["m"][ka] != b["m"][kb]:
        return False
    m = int(a["m"][ka]) if a["status"][ka] == OK else 0
    return all(np.array_equal(a[q][ka, :m], b[q][kb, :m]) for q in QUANTITIES)


def hold_row(worst, family, out, k, r, S, what):
    """One status-0 row of an engine result against the reference r under the spreads S [4]."""
    m = r["m"]
    assert out["status"][k] == OK and out["m"][k] == m, "%s: status %d, m %d for %d" % (what, out["status"][k], out["m"][k], m)
    _hold(worst, family, "xy", og.dmax(out["xy"][k, :m], r["xy"]), S[0], what)
    _hold(worst, family, "psi", og.dpsi(out["psi"][k, :m], r["psi"]), S[1], what)
    _hold(worst, family, "kappa", og.dmax(out["kappa"][k, :m], r["kappa"]), S[2], what)
    _hold(worst, family, "el", og.dmax(out["el_lengths"][k, :m - 1], r["el_lengths"][:m - 1]), S[3], what)
    assert np.all(out["psi"][k, :m] >= -np.pi) and np.all(out["psi"][k, :m] < np.pi), what
    # the last station IS the last raceline point, and nothing follows it
    d_last = og.dmax(out["xy"][k, m - 1], r["last"])
    assert d_last <= og.guard("xy", S[0]), "%s: the last station is %.3e off the last raceline point" % (what, d_last)
    assert out["el_lengths"][k, m - 1] == 0.0, what + ": el_lengths[m - 1] is not the written 0"


def check_launch(eng, family, launch, worst):
    name, sizes, stepsize, mmax = launch
    refs, nvs, als, ends = _arcs(family, sizes)
    out = eng.raceline_batch(refs, nvs, als, stepsize, mmax=mmax, ends=ends)
    S = og.spread(og.key(family, launch))
    for k, n in enumerate(sizes):
        what = "open raceline %s/%s n=%d" % (family, name, n)
        r = og.reference(family, n, stepsize)
        if r["m"] > mmax:       # reports the m it needs, as rings do
            assert out["status"][k] == BAD_INPUT and out["m"][k] == r["m"], "%s: status %d, m_out %d for %d" % (what, out["status"][k], out["m"][k], r["m"])
            continue
        hold_row(worst, family, out, k, r, S[k], what)
    if oc.aimed(name):
        what, K = oc.aimed(name)
        mK = int(out["m"][sizes.index(K)])
        assert mK == {"m==mmax": mmax, "m==mmax+1": mmax + 1, "m==3": 3, "m==2": 2}[what], (name, mK)
    rev = eng.raceline_batch(refs[::-1], nvs[::-1], als[::-1], stepsize, mmax=mmax, ends=ends[::-1])
    for k in range(len(sizes)):
        assert rows_equal(out, rev, k, len(sizes) - 1 - k), "open raceline %s/%s n=%d: the reversed launch returns other bits" % (family, name, sizes[k])
    return out


def check_mixed(eng, family):
    """ring, chain, ring, chain, ... of different sizes in one launch: the ring rows are mcq_raceline_device's bits on those rings, the chain rows
    the chain-only launch's."""
    step = oc.launches(family)[0][2]
    refs, nvs, als, ends = [], [], [], []
    for kind, n in oc.MIXED:
        if kind == "ring":
            r = gc.ring(family, n)
            ends.append(None if n != 3 else dict(closed=True))
        else:
            a = oc.arc(family, n)
            r = a[:3]
            ends.append(dict(psi_s=a[3], psi_e=a[4], fix_s=True))          # (fix_s / fix_e are ignored)
        refs.append(r[0]); nvs.append(r[1]); als.append(r[2])
    mmax = 2 + int(max(float(gc.ring_total(family, n)) if kind == "ring" else float(oc.arc_total(family, n)) for kind, n in oc.MIXED) / step) + 2
    mixed = eng.raceline_batch(refs, nvs, als, step, mmax=mmax, ends=ends)
    assert np.all(mixed["status"] == OK), list(mixed["status"])
    ri = [k for k, (kind, _) in enumerate(oc.MIXED) if kind == "ring"]
    ci = [k for k, (kind, _) in enumerate(oc.MIXED) if kind == "chain"]
    rings = eng.raceline_batch([refs[k] for k in ri], [nvs[k] for k in ri], [als[k] for k in ri], step, mmax=mmax)
    chains = eng.raceline_batch([refs[k] for k in ci], [nvs[k] for k in ci], [als[k] for k in ci], step, mmax=mmax, ends=[ends[k] for k in ci])
    for j, k in enumerate(ri):
        assert rows_equal(mixed, rings, k, j), "mixed launch %s: ring row %d (n=%d) differs from mcq_raceline_device's bits" % (family, k, oc.MIXED[k][1])
    for j, k in enumerate(ci):
        assert rows_equal(mixed, chains, k, j), "mixed launch %s: chain row %d (n=%d) differs from the chain-only launch" % (family, k, oc.MIXED[k][1])
    # every row flagged a ring: the bits of mcq_raceline_device once more, with psi == NULL allowed
    allr = eng.raceline_batch([refs[k] for k in ri], [nvs[k] for k in ri], [als[k] for k in ri], step, mmax=mmax, ends=[None] * len(ri))
    for j in range(len(ri)):
        assert rows_equal(allr, rings, j, j)


def _device_call(eng, refs, nvs, als, closed, psi, stepsize, mmax):
    """mcq_raceline_device_ends on device pointers; closed / psi: arrays or None (NULL).  Returns the result dict of raceline_batch."""
    bsz = len(refs)
    ns = np.array([r.shape[0] for r in refs], dtype=np.int32)
    nmax = max(2, int(ns.max()))
    ref, nv, al = np.zeros((bsz, nmax, 4)), np.zeros((bsz, nmax, 2)), np.zeros((bsz, nmax))
    for k in range(bsz):
        ref[k, :ns[k]], nv[k, :ns[k]], al[k, :ns[k]] = refs[k], nvs[k], als[k]
    with eng.scope() as dev:
        up = dev.up
        d = [up(a) for a in (ns, ref, nv, al)]
        d_c = up(np.ascontiguousarray(closed, dtype=np.int32)) if closed is not None else None
        d_p = up(np.ascontiguousarray(psi, dtype=np.float64)) if psi is not None else None
        d_xy, d_ps, d_k, d_el = (up(np.full((bsz, mmax) + s, gck.NAN_PATTERN)) for s in ((2,), (), (), ()))
        d_m, d_st = up(np.full(bsz, -7, dtype=np.int32)), up(np.full(bsz, -1, dtype=np.int32))
        eng.raceline_device_ends(bsz, nmax, d[0], d[1], d[2], d[3], d_c, d_p, stepsize, mmax, d_xy, d_ps, d_k, d_el, d_m, d_st)
        eng.sync()
        return dict(xy=eng.download(d_xy, (bsz, mmax, 2), np.float64), psi=eng.download(d_ps, (bsz, mmax), np.float64),
                    kappa=eng.download(d_k, (bsz, mmax), np.float64), el_lengths=eng.download(d_el, (bsz, mmax), np.float64),
                    m=eng.download(d_m, (bsz,), np.int32), status=eng.download(d_st, (bsz,), np.int32))


def check_arguments_and_status(eng, family):
    """MCQ_E_ARG: psi == NULL with a chain row.  MCQ_BAD_INPUT for that row only: n = 1, a NaN psi_s; rows beyond m stay untouched."""
    sizes = (50, 5, 257, 3)
    refs, nvs, als, ends = _arcs(family, sizes)
    step = oc.launches(family)[0][2]
    mmax = max(og.reference(family, n, step)["m"] for n in sizes) + 3
    psi = np.array([[e["psi_s"], e["psi_e"]] for e in ends])
    for closed in (None, [1, 0, 1, 1]):
        try:
            _device_call(eng, refs, nvs, als, closed, None, step, mmax)
        except engine.EngineError as e:
            assert "(-1)" in str(e), str(e)           # MCQ_E_ARG
        else:
            raise AssertionError("mcq_raceline_device_ends accepted psi == NULL with a chain row")
    clean = _device_call(eng, refs, nvs, als, None, psi, step, mmax)
    assert np.all(clean["status"] == OK)
    for k in range(len(sizes)):
        m = int(clean["m"][k])
        assert all(gck._untouched(clean[q][k, m:]) for q in QUANTITIES), "n=%d: entries beyond m written" % sizes[k]
    byflag = _device_call(eng, refs, nvs, als, [0, 0, 0, 0], psi, step, mmax)
    assert all(rows_equal(clean, byflag, k, k) for k in range(len(sizes)))
    # a row of one waypoint and a row with a NaN heading between good rows
    one = (refs[1][:1], nvs[1][:1], als[1][:1])
    refs2, nvs2, als2 = [refs[0], one[0], refs[2], refs[3]], [nvs[0], one[1], nvs[2], nvs[3]], [als[0], one[2], als[2], als[3]]
    psi2 = psi.copy()
    psi2[2, 0] = np.nan
    bad = _device_call(eng, refs2, nvs2, als2, None, psi2, step, mmax)
    assert list(bad["status"]) == [OK, BAD_INPUT, BAD_INPUT, OK] and bad["m"][1] == 0 and bad["m"][2] == 0, (list(bad["status"]), list(bad["m"]))
    assert rows_equal(bad, clean, 0, 0) and rows_equal(bad, clean, 3, 3), "a MCQ_BAD_INPUT row disturbed its neighbours"
    for k in (1, 2):
        assert all(gck._untouched(bad[q][k]) for q in QUANTITIES)
    # the same two through raceline_batch(ends=...), and a NaN psi_e
    e2 = [ends[0], dict(psi_s=0.1, psi_e=0.2), dict(psi_s=ends[2]["psi_s"], psi_e=float("nan")), ends[3]]
    out = eng.raceline_batch(refs2, nvs2, als2, step, mmax=mmax, ends=e2)
    assert list(out["status"]) == [OK, BAD_INPUT, BAD_INPUT, OK]
    assert rows_equal(out, clean, 0, 0) and rows_equal(out, clean, 3, 3)


# ---- end to end: chain solve -> open raceline -> unclosed velocity profile -------------------------------------------------------------------
ALPHA_CONTRACT, ALPHA_GUARD = 1e-6, 1e-8        # tests/test_gpu_open.py: the parity contract and the guard on the open goldens
VEL_GUARD_CAP = gck.VEL_GUARD_CAP
E2E_STEP = 1.7                                  # m


def _live_spread(ref, nv, al, psi_s, psi_e, stepsize, r0):
    """race_open_guard's spread of one row, computed live (the row is the engine's own alpha: no stored entry can know it)."""
    out = np.maximum(0.0, og.deviations(ror.raceline(ref, nv, al, psi_s, psi_e, stepsize, np.float64), r0))
    for d in range(SPREAD_DRAWS):
        rng = draw_rng("race_open/e2e", "arc", ref.shape[0], d)
        p = og._perturb(np.array([psi_s, psi_e]), rng)
        r = ror.raceline(og._perturb(ref, rng), og._perturb(nv, rng), og._perturb(al, rng), p[0], p[1], stepsize, LD)
        assert r["m"] == r0["m"]
        out = np.maximum(out, og.deviations(r, r0))
    return out


def _vel_ref(kap, el, veh, v, v_start, rng=None):
    from oracle import vel_ref
    if rng is not None:
        kap = kap * (1.0 + SPREAD_REL * rng.standard_normal(kap.size))
        el = el * (1.0 + SPREAD_REL * rng.standard_normal(el.size))
    vx = vel_ref.calc_vel_profile(ax_max_machines=veh["axm"][v], kappa=kap, el_lengths=el, closed=False, drag_coeff=float(veh["drag"][v]),
                                  m_veh=float(veh["mass"][v]), ggv=veh["ggv"][v], v_max=float(veh["vmax"][v]), dyn_model_exp=1.0,
                                  v_start=float(v_start[v]))
    return vx, vg.lap_time_open(vx, el)


def check_end_to_end(eng, golden, worst):
    """solve_batch(ends=...) on the handling arc, its alpha held to the golden; raceline_batch(ends=...) on THAT alpha, held to the reference under
    the guards; vel_profile_batch(closed=False, v_start=...) on the kernel's own kappa / el_lengths rows, held to oracle/vel_ref.py on those same
    rows under vel_forms_guard's rule (spread: the oracle's movement under the usual draws on kappa and el_lengths, capped)."""
    g = golden
    ends = [dict(psi_s=float(g["psi_s"]), psi_e=float(g["psi_e"]), fix_s=bool(g["fix_s"]), fix_e=bool(g["fix_e"]))]
    al, _, st, _ = eng.solve_batch([dict(reftrack=g["reftrack"], normvec=g["normvec"], scaling=g["scaling"], kappa_bound=float(g["kappa_bound"]),
                                         w_veh=float(g["w_veh"]))], ends=ends)
    d = float(np.max(np.abs(al[0] - g["alpha"])))
    assert st[0] == OK and d < ALPHA_CONTRACT and d < ALPHA_GUARD, (st[0], d)
    r0 = ror.raceline(g["reftrack"], g["normvec"], al[0], ends[0]["psi_s"], ends[0]["psi_e"], E2E_STEP, LD)
    assert abs(r0["ratio"] - np.rint(r0["ratio"])) >= oc.INTEGER_GAP
    out = eng.raceline_batch([g["reftrack"]], [g["normvec"]], al, E2E_STEP, ends=ends)
    S = _live_spread(g["reftrack"], g["normvec"], al[0], ends[0]["psi_s"], ends[0]["psi_e"], E2E_STEP, r0)
    hold_row(worst, "e2e", out, 0, r0, S, "end to end: open raceline")
    m = r0["m"]
    base = gc.vel_launches()[3]
    bsz = 6
    veh = {q: base[q][:bsz] for q in ("ggv", "axm", "drag", "mass", "vmax")}
    v_start = np.linspace(3.0, 25.0, bsz)
    kap, el = np.ascontiguousarray(out["kappa"][:, :m]), np.ascontiguousarray(out["el_lengths"][:, :m])
    vx, lt = eng.vel_profile_batch(kap, el, veh["ggv"], veh["axm"], veh["drag"], veh["mass"], veh["vmax"], dyn_model_exp=1.0,
                                   track_of=np.zeros(bsz, dtype=np.int32), closed=False, v_start=v_start)
    for v in range(bsz):
        what = "end to end: unclosed profile, variant %d" % v
        r = _vel_ref(kap[0], el[0, :m - 1], veh, v, v_start)
        s = np.zeros(2)
        for dr in range(SPREAD_DRAWS):
            p = _vel_ref(kap[0], el[0, :m - 1], veh, v, v_start, draw_rng("race_open/e2e", "vx", v, dr))
            s = np.maximum(s, [vg.dmax(p[0], r[0]), vg._dlap(p[1], r[1])])
        assert vg.guard("vx", s[0]) <= VEL_GUARD_CAP and vg.guard("lap", s[1]) <= VEL_GUARD_CAP, what + ": the oracle itself is undecided here"
        for q, dev, sp in (("vx", vg.dmax(vx[v, :m], r[0]), s[0]), ("lap", vg._dlap(float(lt[v]), r[1]), s[1])):
            gd = vg.guard(q, sp)
            worst.add("e2e." + q, dev, gd)
            assert dev <= gd, "%s: %s deviates by %.3e, guard %.3e" % (what, q, dev, gd)
