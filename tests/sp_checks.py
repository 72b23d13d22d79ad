"""The bodies of tests/test_emu_sp.py (SIMT interpreter) and tests/test_gpu_sp.py (MI355X): the launches of tests/sp_cases.py with the shortest-path
objective, against tests/sp_ref.py in longdouble under the guard of tests/sp_guard.py (the 1e-9 m floor on every case).  Every function takes the
engine; those that compare alphas take a ring_guard.Worst that collects, per family, the worst |d alpha| next to its guard.  Working sets, bounds,
statuses and counts are compared exactly; launches are repeated in other orders and through the other entry points and must return the same bits."""
import ctypes

import numpy as np

import sp_cases as sc
import sp_guard as sg
import sp_ref
from global_racetrajectory_optimization_amd import engine

LD = np.longdouble
SP = engine.OBJ_SHORTEST_PATH
OK, BAD_INPUT = 0, engine.STATUS_BAD_INPUT
INFO_EXACT = ("ipm_iters", "as_iters", "n_active_box", "n_active_kappa", "refine_rounds", "second_attempt", "f32_factorisations", "gi_iters")


def _dev(a, b):
    return float(np.max(np.abs(np.asarray(a, dtype=LD) - np.asarray(b, dtype=LD))))


def check_row(what, alpha, curv, status, info, r, lo, hi, guard, worst, family):
    """One good row against the reference r (sp_ref.solve's dict) and the float64 bounds lo, hi (sp_ref.bounds: the kernel's bits)."""
    assert status == OK and curv == 0.0, "%s: status %d, curv_err %r" % (what, status, curv)
    d = _dev(alpha, r["alpha"])
    print("%s: |d alpha| %.3e (guard %.1e)" % (what, d, guard))
    worst.add(family, d, guard)
    assert d < guard, "%s: alpha is %.3e m from the reference, guard %.3e" % (what, d, guard)
    assert np.all(alpha >= lo) and np.all(alpha <= hi), "%s: outside the box by %.3e" % (what, max(np.max(lo - alpha), np.max(alpha - hi)))
    st = r["state"]
    on_lo, on_hi = alpha == lo, alpha == hi
    assert np.array_equal(on_lo, st == sp_ref.AT_LO) and np.array_equal(on_hi, st == sp_ref.AT_HI), \
        "%s: rows on a bound differ from the reference's working set at %s" % (what, np.flatnonzero((on_lo != (st == sp_ref.AT_LO)) | (on_hi != (st == sp_ref.AT_HI)))[:8])
    if info is not None:
        assert info["n_active_box"] == int(np.sum(st != sp_ref.FREE)) and info["gi_iters"] == 0, (what, info["n_active_box"], int(np.sum(st != 0)), info["gi_iters"])


def _same_row(a, b, ka, kb):
    """Row ka of one solve_batch result and row kb of another: the same bits (alpha, curv_err, status) and the same counts."""
    return (np.array_equal(a[0][ka].view(np.uint64), b[0][kb].view(np.uint64)) and a[1][ka].tobytes() == b[1][kb].tobytes() and a[2][ka] == b[2][kb]
            and all(a[3][ka][q] == b[3][kb][q] for q in INFO_EXACT))


def check_launch(eng, lname, rows, opts, worst):
    """A ragged launch with its bad rows: every good row against the reference, every bad row refused, and the good rows bitwise those of the
    launch without the bad rows.  Returns the launch's result."""
    out = eng.solve_batch(sc.launch_problems(rows), objective=SP, **opts)
    al, curv, st, info = out
    assert len(rows) <= sc.MAX_LAUNCH
    for k, name in enumerate(rows):
        what = "%s[%d] %s" % (lname, k, name)
        if name.startswith("bad/"):
            assert st[k] == BAD_INPUT and not np.any(al[k]) and curv[k] == 0.0, "%s: status %d" % (what, st[k])
            continue
        ref, _, w_veh = sc.case(name)
        lo, hi = sp_ref.bounds(ref, w_veh)
        check_row(what, al[k], curv[k], st[k], info[k], sg.reference(name), lo, hi, sg.guard(name), worst, name.split("/")[0])
    good = [k for k, name in enumerate(rows) if not name.startswith("bad/")]
    if len(good) < len(rows):
        clean = eng.solve_batch(sc.launch_problems([rows[k] for k in good]), objective=SP, **opts)
        for j, k in enumerate(good):
            assert _same_row(out, clean, k, j), "%s: %s has other bits without the bad rows in the launch" % (lname, rows[k])
    return out


def check_order_and_neighbours(eng, lname, rows, opts, out=None):
    """The launch reversed, and split into single-problem calls: bitwise the same rows."""
    probs = sc.launch_problems(rows)
    if out is None:
        out = eng.solve_batch(probs, objective=SP, **opts)
    rev = eng.solve_batch(probs[::-1], objective=SP, **opts)
    for k, name in enumerate(rows):
        assert _same_row(out, rev, k, len(rows) - 1 - k), "%s: %s has other bits in the reversed launch" % (lname, name)
        one = eng.solve_batch([probs[k]], objective=SP, **opts)
        assert _same_row(out, one, k, 0), "%s: %s has other bits in a launch of its own" % (lname, name)


def check_last_resort(lname, rows, out):
    """max_as_iter = 1: the solver kernel's 8 n + 200 round continuation has to run for at least one case (check_launch has already held every
    row to the reference); with one interior-point iteration as well (last_resort_cold) for every case -- nothing else can settle a problem
    whose interior point ran out of its budget.  Returns the sizes at which it ran."""
    good = [k for k, name in enumerate(rows) if not name.startswith("bad/")]
    ran = [sc.size(rows[k]) for k in good if out[3][k]["second_attempt"] & 4]
    assert ran, "%s: the last resort ran for no case" % lname
    if lname == "last_resort_cold":
        assert len(ran) == len(good), "%s: the last resort ran at %s only" % (lname, ran)
    return ran


# ---- the other entry points ---------------------------------------------------------------------------------------------------------------------
def _stack(names):
    return np.stack([sc.case(x)[0] for x in names]), np.stack([sc.case(x)[1] for x in names])


def _info_rows(raw, bsz):
    infos = (engine.McqInfo * bsz).from_buffer_copy(np.asarray(raw).tobytes())
    return [{q: getattr(i, q) for q in INFO_EXACT} for i in infos]


def _expect(what, base, al, curv, st, info=None, order=None):
    """A uniform entry's [B, n] / [B] outputs against solve_batch's result `base` (rows in `order`): the same bits."""
    bsz = len(base[0])
    order = range(bsz) if order is None else order
    for j, k in enumerate(order):
        assert np.array_equal(np.asarray(al[j]).view(np.uint64), base[0][k].view(np.uint64)), "%s: alpha of row %d is not solve_batch's" % (what, j)
        assert np.asarray(curv[j]).tobytes() == base[1][k].tobytes() and st[j] == base[2][k], "%s: row %d status %d" % (what, j, st[j])
        if info is not None:
            assert all(info[j][q] == base[3][k][q] for q in INFO_EXACT), "%s: info of row %d" % (what, j)


def check_entry_points(eng, n, worst):
    """The same uniform problems through every entry point that takes this objective: bitwise solve_batch's rows, which are held to the
    reference here.  mcq_solve_device_stream and mcq_solve_host_pipelined run three steps (the problems rotated by one from step to step), so
    that steps land on both workspaces of the handle."""
    names = sc.uniform_names(n)
    bsz = len(names)
    refs, nvs = _stack(names)
    steps = 3
    rot = [[(j + s) % bsz for j in range(bsz)] for s in range(steps)]
    base = eng.solve_batch([sc.problem(x) for x in names], objective=SP)
    for k, name in enumerate(names):
        lo, hi = sp_ref.bounds(refs[k], sc.W_VEH)
        check_row("solve_batch %s" % name, base[0][k], base[1][k], base[2][k], base[3][k], sg.reference(name), lo, hi, sg.guard(name), worst, "entries")
    isz = ctypes.sizeof(engine.McqInfo)
    # mcq_solve_host
    al, curv, st, info = eng.solve_host(refs, nvs, None, 1.0, sc.W_VEH, objective=SP)
    _expect("solve_host n=%d" % n, base, al, curv, st, [{q: getattr(i, q) for q in INFO_EXACT} for i in info])
    with eng.scope() as D:
        d_ref, d_nv = D.up(refs), D.up(nvs)
        d_n = D.up(np.full(bsz, n, dtype=np.int32))

        def outs():
            return (D.up(np.full((bsz, n), np.nan)), D.up(np.full(bsz, np.nan)), D.up(np.full(bsz, -1, dtype=np.int32)),
                    D.up(np.full(bsz * isz, 0xFF, dtype=np.uint8)))

        def fetch(o):
            eng.sync()
            return (eng.download(o[0], (bsz, n), np.float64), eng.download(o[1], (bsz,), np.float64), eng.download(o[2], (bsz,), np.int32),
                    _info_rows(eng.download(o[3], (bsz * isz,), np.uint8), bsz))
        # mcq_solve_device, mcq_solve_device_ragged
        o = outs()
        eng.solve_device(bsz, n, d_ref, d_nv, None, 1.0, sc.W_VEH, o[0], o[1], o[2], o[3], objective=SP)
        _expect("solve_device n=%d" % n, base, *fetch(o))
        o = outs()
        eng.solve_device_ragged(bsz, n, d_n, d_ref, d_nv, None, 1.0, sc.W_VEH, o[0], o[1], o[2], o[3], objective=SP)
        _expect("solve_device_ragged n=%d" % n, base, *fetch(o))
        # mcq_solve_device_ragged_params: a vehicle width per problem, two of them wide enough to clip rows to +-0.001 m
        w_list = np.array(sc.W_VEH_SWEEP)
        per = eng.solve_batch([dict(sc.problem(x), w_veh=float(w)) for x, w in zip(names, w_list)], objective=SP)
        clipped = 0
        for k, name in enumerate(names):
            derived = "w_veh/%d/%d" % (n, k)             # (a case of its own in the spread table)
            lo, hi = sp_ref.bounds(refs[k], float(w_list[k]))
            clipped += int(np.sum(hi == sp_ref.CLIP) + np.sum(lo == -sp_ref.CLIP))
            d = _dev(per[0][k], sg.reference(derived)["alpha"])
            worst.add("entries", d, sg.guard(derived))
            assert per[2][k] == OK and d < sg.guard(derived) and np.all(per[0][k] >= lo) and np.all(per[0][k] <= hi), (name, per[2][k], d)
        assert clipped > n
        o = outs()
        eng.solve_device_ragged_params(bsz, n, d_n, d_ref, d_nv, None, 1.0, 77.0, None, D.up(w_list), o[0], o[1], o[2], o[3], objective=SP)
        _expect("solve_device_ragged_params n=%d" % n, per, *fetch(o))
        # mcq_solve_device_stream: three steps
        d_refs, d_nvs = [D.up(refs[r]) for r in rot], [D.up(nvs[r]) for r in rot]
        os_ = [outs() for _ in range(steps)]
        eng.solve_device_stream(bsz, n, d_refs, d_nvs, None, 1.0, sc.W_VEH, [o[0] for o in os_], [o[1] for o in os_], [o[2] for o in os_], objective=SP)
        for s in range(steps):
            got = fetch(os_[s])
            _expect("solve_device_stream n=%d step %d" % (n, s), base, got[0], got[1], got[2], None, rot[s])
    # mcq_solve_host_pipelined: three steps
    alphas = [np.full((bsz, n), np.nan) for _ in range(steps)]
    curv, st = eng.solve_host_pipelined([refs[r] for r in rot], [nvs[r] for r in rot], None, 1.0, sc.W_VEH, alphas, objective=SP)
    for s in range(steps):
        _expect("solve_host_pipelined n=%d step %d" % (n, s), base, alphas[s], curv[s], st[s], None, rot[s])


HOST_BATCH, HOST_N = sc.HOST_BATCH, sc.HOST_N


def check_solve_host_large_batch(eng, worst):
    """mcq_solve_host with a batch above MCQ_HOST_SLICE_MIN (512): the minimum-curvature objective goes in slices on two streams there, this one
    stays one launch (slices_for() in csrc/mcq_api.hip) -- and has to come back right: bitwise solve_batch's rows, every row on the reference.
    The rings are the host/<k> entries of the spread table."""
    rings = [sc.case("host/%d" % k) for k in range(HOST_BATCH)]
    refs, nvs = np.stack([r[0] for r in rings]), np.stack([r[1] for r in rings])
    al, curv, st, _ = eng.solve_host(refs, nvs, None, 1.0, sc.W_VEH, objective=SP)
    base = eng.solve_batch([dict(reftrack=refs[k], normvec=nvs[k], scaling=None, kappa_bound=1.0, w_veh=sc.W_VEH) for k in range(HOST_BATCH)], objective=SP)
    _expect("solve_host %d x %d" % (HOST_BATCH, HOST_N), base, al, curv, st)
    for k in range(HOST_BATCH):
        d = _dev(al[k], sg.reference("host/%d" % k)["alpha"])
        worst.add("host520", d, sg.guard("host/%d" % k))
        assert st[k] == OK and d < sg.guard("host/%d" % k), (k, st[k], d)


# ---- the fp32 entries -------------------------------------------------------------------------------------------------------------------------
def check_f32(eng, n, worst):
    """include/mcq.h: mcq_solve_device_f32 with normals solves this objective on the widened rows and normals; without normals, and through the
    _rows entries (which derive their normals), the objective is refused with MCQ_E_ARG.  Where it solves: float32 of the fp64 engine's alpha on
    the widened inputs bit for bit, which in turn is held to the reference on those inputs -- together, one float rounding of alpha."""
    names = sc.uniform_names(n)
    refs, nvs = _stack(names)
    ref32, nv32 = refs.astype(np.float32), nvs.astype(np.float32)
    a32, curv, st, _ = eng.solve_uniform_f32(ref32, nv32, None, 1.0, sc.W_VEH, objective=SP)
    r64, n64 = ref32.astype(np.float64), nv32.astype(np.float64)
    twin = eng.solve_batch([dict(reftrack=r64[k], normvec=n64[k], scaling=None, kappa_bound=1.0, w_veh=sc.W_VEH) for k in range(len(names))], objective=SP)
    for k, name in enumerate(names):
        assert st[k] == OK and twin[2][k] == OK and curv[k] == 0.0, (name, st[k], twin[2][k])
        assert a32.dtype == np.float32 and np.array_equal(a32[k], twin[0][k].astype(np.float32)), "%s: the float alpha is not float32 of the fp64 solve" % name
        derived = "f32/%d/%d" % (n, k)                   # (the rounded inputs: a case of their own in the spread table)
        assert np.array_equal(sc.case(derived)[0], r64[k]) and np.array_equal(sc.case(derived)[1], n64[k])
        r, g = sg.reference(derived), sg.guard(derived)
        d = _dev(twin[0][k], r["alpha"])
        worst.add("f32", d, g)
        assert d < g, "%s on the rounded inputs: %.3e m from the reference" % (name, d)
        beyond = float(np.max(np.abs(a32[k].astype(LD) - r["alpha"]) - np.abs(r["alpha"]) * LD(2.0) ** -24))
        assert beyond < g, "%s: the float alpha is %.3e m beyond one float rounding of the reference" % (name, beyond)
    for call in (lambda: eng.solve_uniform_f32(ref32, None, None, 1.0, sc.W_VEH, objective=SP),
                 lambda: eng.solve_batch_f32(ref32, None, 1.0, sc.W_VEH, layout=engine.F32_ABSOLUTE, objective=SP),
                 lambda: eng.solve_batch_f32(engine.rows_to_increments(refs)[0], None, 1.0, sc.W_VEH, layout=engine.F32_INCREMENTS, objective=SP)):
        try:
            call()
        except engine.EngineError as e:
            assert "(-1)" in str(e) and "normvec is required" in str(e), str(e)          # MCQ_E_ARG
        else:
            raise AssertionError("a float entry without normals accepted the shortest-path objective")
    # the refusals left nothing behind: the next solve on the handle is the twin's again
    again = eng.solve_batch([dict(reftrack=r64[0], normvec=n64[0], scaling=None, kappa_bound=1.0, w_veh=sc.W_VEH)], objective=SP)
    assert _same_row(twin, again, 0, 0)


# ---- handle history -----------------------------------------------------------------------------------------------------------------------------
HISTORY_BIG = ("ladder/6", "corner/2053/separators", "all_free/300", "ladder/2053")          # nmax = 2053: workspace vectors
HISTORY_SMALL = ("ladder/257", "corner/257/second", "ladder/3")                             # nmax = 257


def check_handle_history(eng_factory, golden_track):
    """One fresh engine: shortest path at nmax = 2053, minimum curvature, shortest path at nmax = 257, the first launch again.  The shortest-path
    vectors alias the minimum-curvature path's (V_SPD .. V_SPC on V_XP, V_YP, V_IDL, V_XPP, V_YPP, V_TUC), and the workspace is reallocated and
    reused on the way.  Every result: bitwise that of a fresh engine given that launch alone."""
    mc = [dict(reftrack=golden_track["reftrack"], normvec=golden_track["normvec"], scaling=golden_track["scaling"], kappa_bound=0.12, w_veh=3.4)]
    launches = [(sc.launch_problems(HISTORY_BIG), dict(objective=SP)), (mc, {}), (sc.launch_problems(HISTORY_SMALL), dict(objective=SP)),
                (sc.launch_problems(HISTORY_BIG), dict(objective=SP))]
    eng = eng_factory()
    try:
        got = [eng.solve_batch(p, **kw) for p, kw in launches]
    finally:
        eng.close()
    for k, (p, kw) in enumerate(launches[:3]):
        fresh = eng_factory()
        try:
            alone = fresh.solve_batch(p, **kw)
        finally:
            fresh.close()
        for who in ([k, 3] if k == 0 else [k]):
            for j in range(len(p)):
                assert alone[2][j] == OK and _same_row(got[who], alone, j, j), "launch %d of the history, row %d: not a fresh engine's bits" % (who + 1, j)
