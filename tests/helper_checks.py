"""The shared bodies of tests/test_emu_helpers.py (SIMT interpreter) and tests/test_gpu_helpers.py (MI355X): the plumbing behind the helper
entries -- Engine.scope and _pad_rows in engine.py, the ABI table load_library declares, the handle's seven grow-only Scratch buffers in
csrc/mcq_api.hip.  No reference and no tolerance: pointers are counted, results are compared bit for bit with those of a fresh engine.

The shapes are the smallest legal ones (one or two tracks of 8 to 12 waypoints, a 3-row ggv, a 2-row ax_max_machines); the launch that makes a
scratch grow has 3 tracks of 33 to 40.  The friction map has 36 cells, the generated one about sixty; the Gaussian fit has one bump a side."""
import collections
import contextlib
import ctypes
import os
import re

import numpy as np

import open_ref
from global_racetrajectory_optimization_amd import engine, parallel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL, LARGE = (10,), (40, 37, 33)
GGV = np.array([[0.0, 10.0, 10.0], [30.0, 8.0, 9.0], [70.0, 5.0, 8.0]])
AXM = np.array([[0.0, 6.0], [70.0, 2.0]])
DRAG, MASS, VMAX = 0.85, 1000.0, 60.0


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------
def ring(n, seed=0):
    """An ellipse of n waypoints as rows [x, y, w_r, w_l], and its unit normals (to the right of the driving direction, as tph's)."""
    t = 2.0 * np.pi * (np.arange(n) + 0.25 * seed) / n
    ref = np.column_stack(((30.0 + 2.0 * seed) * np.cos(t), 18.0 * np.sin(t), 3.0 + 0.5 * np.sin(3.0 * t), np.full(n, 3.5)))
    d = np.roll(ref[:, :2], -1, axis=0) - np.roll(ref[:, :2], 1, axis=0)
    return ref, np.column_stack((d[:, 1], -d[:, 0])) / np.hypot(d[:, 0], d[:, 1])[:, None]


def rings(sizes):
    refs, nvs = zip(*[ring(n, k) for k, n in enumerate(sizes)])
    return list(refs), list(nvs)


def tck_of(seed, knots=12, k=3):
    """A periodic cubic B-spline (t, c, k) around ring(., seed) in the layout scipy.interpolate.splprep(per=1) returns."""
    c = ring(knots, seed)[0][:, :2]
    c = np.vstack((c, c[:k]))
    return np.arange(-k, knots + k + 1) / float(knots), (c[:, 0], c[:, 1]), k


def race_of(refs):
    """The reference lines themselves as raceline_batch's dict (xy, psi, kappa, el_lengths, m)."""
    ns, xy = engine._pad_rows([r[:, :2] for r in refs], 2)
    out = dict(xy=xy, m=ns, psi=np.zeros(xy.shape[:2]), kappa=np.zeros(xy.shape[:2]), el_lengths=np.zeros(xy.shape[:2]))
    for b, r in enumerate(refs):
        d = np.roll(r[:, :2], -1, axis=0) - r[:, :2]
        out["psi"][b, :ns[b]] = np.arctan2(d[:, 1], d[:, 0]) - np.pi / 2
        out["el_lengths"][b, :ns[b]] = np.hypot(d[:, 0], d[:, 1])
        out["kappa"][b, :ns[b]] = 0.03 + 0.01 * np.sin(np.arange(ns[b]))
    return out


def traj_of(race):
    """race_of's rows as trajectory_batch's padded table [rows, mmax, 7] = s, x, y, psi, kappa, vx, ax (NaN behind a row's m)."""
    tj = np.full(race["xy"].shape[:2] + (engine.TRAJ_COLS,), np.nan)
    for b, m in enumerate(race["m"]):
        tj[b, :m, 0] = np.concatenate(([0.0], np.cumsum(race["el_lengths"][b, :m - 1])))
        tj[b, :m, 1:3], tj[b, :m, 3], tj[b, :m, 4], tj[b, :m, 5], tj[b, :m, 6] = race["xy"][b, :m], race["psi"][b, :m], race["kappa"][b, :m], 20.0, 0.0
    return tj


def vel_tables(bsz):
    return np.tile(GGV, (bsz, 1, 1)), np.tile(AXM, (bsz, 1, 1))


# ---- 1. every pointer freed exactly once ------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def ledger(eng):
    """Records what eng.alloc returns and eng.free takes while it is open: .left() is the multiset of pointers allocated and not freed (a
    pointer freed more often than allocated counts negative and is an error too)."""
    led = collections.namedtuple("Ledger", "allocs frees left")([], [], None)
    alloc, free = eng.alloc, eng.free

    def rec_alloc(nbytes):
        led.allocs.append(alloc(nbytes))
        return led.allocs[-1]

    def rec_free(ptr):
        led.frees.append(ptr)
        free(ptr)
    eng.alloc, eng.free = rec_alloc, rec_free

    def left():
        c = collections.Counter(led.allocs)
        c.subtract(led.frees)
        return sorted(p for p, k in c.items() for _ in range(abs(k)))
    try:
        yield led._replace(left=left)
    finally:
        del eng.alloc, eng.free


def batch_calls(eng):
    """(name, call, failing call) per method rewritten on Engine.scope, at its smallest shapes.  The failing calls are refused on the host
    behind the uploads (MCQ_E_ARG from the entry's argument check); prep_batch, normals_crossing_batch, friction_query_batch,
    contains_points_batch and track_boundaries_batch have no argument an entry refuses: there the first download raises in the host's place.
    Nothing faults on the device.  The friction map made here is the engine's to free (Engine.close)."""
    refs, nvs = rings((8, 11))
    tracks, tcks = refs, [tck_of(0), tck_of(1)]
    race = race_of(refs)
    ggv, axm = vel_tables(2)
    kap, el = race["kappa"] + 0.0, np.where(race["el_lengths"] > 0.0, race["el_lengths"], 1.0)
    alphas = [0.3 * np.sin(np.arange(r.shape[0])) for r in refs]
    chain = open_ref.seeded_chain(9, 1)
    u_ref, u_nv = [np.stack(a) for a in rings((12, 12))]
    ends = [None, dict(psi_s=chain[3], psi_e=chain[4])]
    traj = traj_of(race)
    gx, gy = np.meshgrid(np.linspace(-36.0, 36.0, 6), np.linspace(-24.0, 24.0, 6))
    fmap = eng.friction_map(np.column_stack((gx.ravel(), gy.ravel())), 0.8 + 0.01 * np.arange(36))
    fq = np.linspace(-1.0, 1.0, 3) * np.ones((2, 12, 1))
    fw = np.stack((np.full((2, 4, 12), 0.01), np.full((2, 4, 12), 0.9)), axis=3)

    def no_download(call):
        def failing():
            def refuse(*a, **kw):
                raise engine.EngineError("download refused by the test")
            eng.download = refuse
            try:
                call()
            finally:
                del eng.download
        return failing
    vel = lambda **kw: eng.vel_profile_batch(kap, el, ggv, axm, DRAG, MASS, VMAX, n_of_track=race["m"], **kw)      # noqa: E731
    prep = lambda: eng.prep_batch(refs)      # noqa: E731
    cross = lambda: eng.normals_crossing_batch(refs, nvs)      # noqa: E731
    query = lambda: eng.friction_query_batch(fmap, refs[0][:, :2], want_idx=True, want_dist=True)      # noqa: E731
    grid = lambda dn=1.0, **kw: eng.friction_grid_batch(fmap, refs, nvs, 2.0, 1.5, 1.4, dn, jmax=5, **kw)      # noqa: E731
    inside = lambda: eng.contains_points_batch([r[:, :2] for r in refs], refs[1][:5, :2], radius=0.5, want_contours=True)      # noqa: E731
    bounds = lambda: eng.track_boundaries_batch(refs)      # noqa: E731
    return [
        ("prep_batch", prep, no_download(prep)),
        ("vel_profile_batch", vel, lambda: vel(dyn_model_exp=0.0)),
        ("vel_profile_batch, unclosed", lambda: vel(closed=False, v_start=5.0, v_end=4.0), lambda: vel(closed=False, v_start=5.0, dyn_model_exp=0.0)),
        ("normals_crossing_batch", cross, no_download(cross)),
        ("spline_approx_batch", lambda: eng.spline_approx_batch(tracks, tcks, 3.0), lambda: eng.spline_approx_batch(tracks, tcks, 3.0, mmax=2)),
        ("min_width_batch", lambda: eng.min_width_batch(refs, 7.5), lambda: eng.min_width_batch(refs, float("nan"))),
        ("prep_track_batch", lambda: eng.prep_track_batch(tracks, tcks=tcks, min_width=7.5),
         lambda: eng.prep_track_batch(tracks, tcks=tcks, min_width=float("nan"))),
        ("raceline_batch", lambda: eng.raceline_batch(refs, nvs, alphas, 2.0), lambda: eng.raceline_batch(refs, nvs, alphas, 0.0, mmax=16)),
        ("raceline_batch, ends", lambda: eng.raceline_batch([refs[0], chain[0]], [nvs[0], chain[1]], [alphas[0], alphas[1][:9]], 2.0, ends=ends),
         lambda: eng.raceline_batch([refs[0], chain[0]], [nvs[0], chain[1]], [alphas[0], alphas[1][:9]], 0.0, mmax=16, ends=ends)),
        ("trajectory_batch", lambda: eng.trajectory_batch(race, kap * 0.0 + 20.0, ggv, axm, DRAG, MASS, VMAX, 0.12),
         lambda: eng.trajectory_batch(race, kap * 0.0 + 20.0, ggv, axm, DRAG, MASS, VMAX, float("nan"))),
        ("bound_dists_batch", lambda: eng.bound_dists_batch(refs, nvs, race, 4.7, 2.0), lambda: eng.bound_dists_batch(refs, nvs, race, 4.7, 2.0, stepsize_bound=0.0)),
        ("solve_uniform_f32", lambda: eng.solve_uniform_f32(u_ref, u_nv, None, 0.5, 2.0),
         lambda: eng.solve_uniform_f32(u_ref, None, None, 0.5, 2.0, objective=engine.OBJ_SHORTEST_PATH)),
        ("export_batch", lambda: eng.export_batch(refs, nvs, alphas, traj), lambda: eng.export_batch(refs, nvs, alphas, traj[:, :1])),
        ("spline_fit_batch", lambda: eng.spline_fit_batch(tracks, stepsize_prep=8.0, points=True), lambda: eng.spline_fit_batch(tracks, s=-1.0, stepsize_prep=8.0)),
        ("friction_query_batch", query, no_download(query)),
        ("friction_grid_batch", lambda: grid(want_idx=True), lambda: grid(dn=0.0)),
        ("friction_grid_batch, gauss", lambda: grid(fit="gauss", n_gauss=1), lambda: grid(fit="gauss", n_gauss=1, rcond=float("nan"))),
        ("friction_model_batch", lambda: eng.friction_model_batch(fq, fw), lambda: eng.friction_model_batch(fq, fw, model=7)),
        ("contains_points_batch", inside, no_download(inside)),
        ("track_boundaries_batch", bounds, no_download(bounds)),
        ("friction_gen_batch", lambda: eng.friction_gen_batch(refs, 4.0), lambda: eng.friction_gen_batch(refs, 0.0)),
        ("parallel.solve_sharded", lambda: parallel.solve_sharded([dict(reftrack=u_ref[0], normvec=u_nv[0], scaling=None, kappa_bound=0.5, w_veh=2.0)], eng),
         None),
    ]


def check_freed_once(eng):
    for name, call, failing in batch_calls(eng):
        with ledger(eng) as led:
            call()
        assert led.allocs and led.left() == [], "%s: %d allocations, %d frees, unbalanced: %s" % (name, len(led.allocs), len(led.frees), led.left())
        if failing is None:
            continue
        with ledger(eng) as led:
            try:
                failing()
            except engine.EngineError:
                pass
            else:
                raise AssertionError("%s: the failing call did not raise EngineError" % name)
        assert led.allocs and led.left() == [], "%s, failing: %d allocations, %d frees, unbalanced: %s" % (name, len(led.allocs), len(led.frees), led.left())
    # keep: exactly the two returned pointers stay, and they are the caller's
    refs, _ = rings((8, 11))
    with ledger(eng) as led:
        keep = []
        eng.spline_approx_batch(refs, [tck_of(0), tck_of(1)], 3.0, keep=keep)
        assert len(keep) == 3 and led.left() == sorted(keep[:2]), "spline_approx_batch(keep=[]): outstanding %s, returned %s" % (led.left(), keep[:2])
        eng.free(keep[0])
        eng.free(keep[1])
        assert led.left() == []


# ---- 2. a scratch that grew returns the bits of a fresh handle --------------------------------------------------------------------------------
# stage_*(eng, dev, sizes): uploads a launch's inputs and allocates its (zero-filled) outputs in the scope `dev`; returns go(), which enqueues
# the launch -- asynchronous: nothing waits for it -- and returns fetch(), which downloads the outputs.
def stage_vel(eng, dev, sizes):
    race = race_of(rings(sizes)[0])
    bsz, nmax = race["xy"].shape[:2]
    ggv, axm = vel_tables(bsz)
    d_in = [dev.up(a) for a in (race["m"], race["kappa"], np.where(race["el_lengths"] > 0.0, race["el_lengths"], 1.0), ggv, axm, np.full(bsz, DRAG),
                                np.full(bsz, MASS), np.full(bsz, VMAX))]
    d_vx, d_lt = dev.new(bsz * nmax * 8), dev.new(bsz * 8)

    def go():
        rc = eng.lib.mcq_vel_profile_device_ragged(eng.h, bsz, nmax, d_in[0], None, d_in[1], d_in[2], d_in[3], 3, d_in[4], 2, d_in[5], d_in[6], d_in[7],
                                                   1.0, d_vx, d_lt)
        eng._check(rc, "mcq_vel_profile_device_ragged")
        return lambda: (eng.download(d_vx, (bsz, nmax), np.float64), eng.download(d_lt, (bsz,), np.float64))
    return go


def stage_bound(eng, dev, sizes):
    refs, nvs = rings(sizes)
    race = race_of(refs)
    ns, ref = engine._pad_rows(refs, 4, nmin=3)
    nv = engine._pad_like(nvs, ns, (2,), nmin=3)
    bsz, nmax = ref.shape[:2]
    d_ref, d_nv, d_n, d_xy, d_psi = [dev.up(a) for a in (ref, nv, ns, race["xy"], race["psi"])]
    d_md, d_mn, d_nb, d_bd, d_st = dev.new(bsz * nmax * 8), dev.new(bsz * 8), dev.new(bsz * 8), dev.new(bsz * 2 * nmax * 16), dev.new(bsz * 4)

    def go():
        eng.bound_dists_device(bsz, nmax, d_n, d_ref, d_nv, nmax, d_n, d_xy, d_psi, 4.7, 2.0, None, None, 1.0, engine.BOUNDS_ALL, d_md, d_mn, d_nb, d_bd, d_st)
        return lambda: (eng.download(d_md, (bsz, nmax), np.float64), eng.download(d_mn, (bsz,), np.float64), eng.download(d_nb, (bsz, 2), np.int32),
                        eng.download(d_bd, (bsz, 2, nmax, 2), np.float64), eng.download(d_st, (bsz,), np.int32))
    return go


def stage_spline(eng, dev, sizes, mmax=64):
    ns, trk = engine._pad_rows(rings(sizes)[0], 4, nmin=3)
    bsz, nmax = trk.shape[:2]
    k, nk, knots, coef = eng.pack_tcks([tck_of(b) for b in range(bsz)])
    d_trk, d_n, d_nk, d_kn, d_cf = [dev.up(a) for a in (trk, ns, nk, knots, coef)]
    d_m, d_ct, d_ds, d_dev, d_nm, d_st = (dev.new(bsz * 4), dev.new(bsz * (nmax + 1) * 8), dev.new(bsz * (nmax + 1) * 8), dev.new(bsz * 16),
                                          dev.new(bsz * 4), dev.new(bsz * 4))
    d_ref = dev.new(bsz * mmax * 32)

    def go():
        eng.spline_approx_device(bsz, nmax, d_n, d_trk, k, knots.shape[1], d_nk, d_kn, d_cf, 3.0, mmax, d_ref, d_m, d_ct, d_ds, d_dev, d_nm, d_st)
        return lambda: (eng.download(d_ref, (bsz, mmax, 4), np.float64), eng.download(d_m, (bsz,), np.int32), eng.download(d_ct, (bsz, nmax + 1), np.float64),
                        eng.download(d_ds, (bsz, nmax + 1), np.float64), eng.download(d_dev, (bsz, 2), np.float64), eng.download(d_nm, (bsz,), np.int32),
                        eng.download(d_st, (bsz,), np.int32))
    return go


STAGES = dict(vel=stage_vel, bound=stage_bound, spline=stage_spline)


def _bits(outs):
    return [np.ascontiguousarray(a).tobytes() for a in outs]


def check_scratch_regrowth(eng_factory, which):
    """Small launch, a larger one that makes the scratch grow while the small one may still be queued, the small one again: all three enqueued on
    one engine before anything is waited for.  Each returns the bits of the same launch alone on a fresh engine."""
    stage = STAGES[which]
    order = (SMALL, LARGE, SMALL)
    eng = eng_factory()
    try:
        with eng.scope() as dev:
            staged = [stage(eng, dev, sizes) for sizes in order]
            fetch = [go() for go in staged]
            eng.sync()
            got = [_bits(f()) for f in fetch]
    finally:
        eng.close()
    for sizes in (SMALL, LARGE):
        fresh = eng_factory()
        try:
            with fresh.scope() as dev:
                alone = stage(fresh, dev, sizes)()()
        finally:
            fresh.close()
        good = np.all(np.isfinite(alone[-1])) if which == "vel" else not np.any(alone[-1])      # (lap times; statuses)
        assert good, "%s %s: the launch alone reports %s" % (which, sizes, alone[-1])
        for j in [j for j, s in enumerate(order) if s == sizes]:
            assert got[j] == _bits(alone), "%s: launch %d (%s) on the grown scratch differs from the launch alone on a fresh engine" % (which, j, sizes)


def ends_launch(sizes):
    """Rings and chains alternating, as solve_batch(ends=...) takes them."""
    probs, ends = [], []
    for k, n in enumerate(sizes):
        if k % 2 == 0:
            ref, nv = ring(n, k)
            probs.append(dict(reftrack=ref, normvec=nv, scaling=None, kappa_bound=0.5, w_veh=2.0))
            ends.append(None)
        else:
            ref, nv, _, ps, pe = open_ref.seeded_chain(n, k)
            probs.append(dict(reftrack=ref, normvec=nv, scaling=open_ref.open_scalings(ref), kappa_bound=1e3, w_veh=2.0))
            ends.append(dict(psi_s=ps, psi_e=pe))
    return probs, ends


def check_ends_regrowth(eng_factory):
    """The device copy of the mcq_ends records through solve_batch(ends=...): 2 problems, 4 (the records' buffer grows), 2 again; a ring and a chain
    in each.  Bitwise the launch alone on a fresh engine."""
    launches = [ends_launch(s) for s in ((10, 9), (40, 37, 33, 12), (10, 9))]

    def run(eng, launch):
        al, curv, st, _ = eng.solve_batch(launch[0], ends=launch[1])
        assert not np.any(st), "solve_batch(ends=...): statuses %s" % list(st)
        return _bits(al) + _bits((curv, st))
    eng = eng_factory()
    try:
        got = [run(eng, launch) for launch in launches]
    finally:
        eng.close()
    for j in (0, 1):
        fresh = eng_factory()
        try:
            alone = run(fresh, launches[j])
        finally:
            fresh.close()
        for i in ((0, 2) if j == 0 else (1,)):
            assert got[i] == alone, "solve_batch(ends=...): launch %d differs from the launch alone on a fresh engine" % i


# ---- 3. include/mcq.h and the ABI table -------------------------------------------------------------------------------------------------------
def header_prototypes():
    """{name: (return type, number of parameters)} of every function include/mcq.h declares (comments stripped; (void) is 0)."""
    hdr = open(os.path.join(ROOT, "include", "mcq.h")).read()
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    hdr = re.sub(r"//[^\n]*", " ", hdr)
    out = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w \*]*?)\s*\b(mcq_[a-z0-9_]+)\s*\(([^;{}()]*)\)\s*;", hdr):
        params = params.strip()
        out[name] = (ret.strip(), 0 if params in ("", "void") else params.count(",") + 1)
    return out


def check_abi_table():
    protos = header_prototypes()
    assert len(protos) >= 52 and set(protos) == set(engine._ABI) == set(engine.EXPORTED_SYMBOLS)
    assert engine.EXPORTED_SYMBOLS == tuple(engine._ABI)
    simple = (type(ctypes.c_int), type(ctypes.POINTER(ctypes.c_int)), type(engine.IQP_ROUND_CB))
    for name, entry in engine._ABI.items():
        assert len(entry) == 2, name
        restype, argtypes = entry
        assert isinstance(restype, simple) if protos[name][0] != "void" else restype is None, "%s: restype %r for '%s'" % (name, restype, protos[name][0])
        assert len(argtypes) == protos[name][1], "%s: %d argtypes, %d parameters in include/mcq.h" % (name, len(argtypes), protos[name][1])
        assert all(isinstance(a, simple) for a in argtypes), name


# ---- 4. the packer's two modes ----------------------------------------------------------------------------------------------------------------
def check_packer_modes(eng):
    """A reftrack of 2 columns: numpy's ValueError before anything is allocated where the rows are taken whole; accepted, its widths zero, by
    prep_batch and raceline_batch."""
    refs, nvs = rings((9, 12))
    two = [r[:, :2].copy() for r in refs]
    zeros = [np.column_stack((r, np.zeros((r.shape[0], 2)))) for r in two]
    race = race_of(refs)
    tcks = [tck_of(0), tck_of(1)]
    for name, call in (("bound_dists_batch", lambda: eng.bound_dists_batch(two, nvs, race, 4.7, 2.0)),
                       ("normals_crossing_batch", lambda: eng.normals_crossing_batch(two, nvs)),
                       ("min_width_batch", lambda: eng.min_width_batch(two, 7.5)),
                       ("spline_approx_batch", lambda: eng.spline_approx_batch(two, tcks, 3.0))):
        with ledger(eng) as led:
            try:
                call()
            except ValueError:
                pass
            else:
                raise AssertionError("%s took a reftrack of 2 columns" % name)
        assert led.allocs == [], "%s allocated before it refused a reftrack of 2 columns" % name
    a, b = eng.prep_batch(two), eng.prep_batch(zeros)
    assert _bits(a[0] + a[1]) == _bits(b[0] + b[1]), "prep_batch: 2 columns and 2 + 2 zero columns give other bits"
    alphas = [0.3 * np.sin(np.arange(r.shape[0])) for r in refs]
    a, b = eng.raceline_batch(two, nvs, alphas, 2.0), eng.raceline_batch(zeros, nvs, alphas, 2.0)
    assert not np.any(a["status"]) and sorted(a) == sorted(b) and all(_bits([a[q]]) == _bits([b[q]]) for q in a), "raceline_batch: other bits"
    # the packer itself: lengths, floor, zero fill
    ns, out = engine._pad_rows(refs, 4, nmin=3)
    assert ns.dtype == np.int32 and list(ns) == [9, 12] and out.shape == (2, 12, 4) and out.dtype == np.float64
    assert np.array_equal(out[0, :9], refs[0]) and not np.any(out[0, 9:]) and np.array_equal(out[1], refs[1])
    assert engine._pad_rows([refs[0][:2]], 4, nmin=3)[1].shape == (1, 3, 4)
    assert np.array_equal(engine._pad_rows(two, 4, strict=False)[1], engine._pad_rows(zeros, 4)[1])
