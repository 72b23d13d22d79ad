"""tests/race_open_ref.py, tests/race_open_cases.py and tests/race_open_guard.py on their own (no engine, no GPU): the reference satisfies the
conditions it was written from and agrees with the host shims of the open spline; the case table meets the condition that makes exact comparisons
of point counts legitimate; the stored spreads are what tests/race_open_guard.py computes."""
import numpy as np
import pytest

import race_open_cases as oc
import race_open_guard as og
import race_open_ref as ror
from global_racetrajectory_optimization_amd import trajectory_planning_helpers as tph

LD = np.longdouble


@pytest.fixture(scope="module", autouse=True)
def the_entry_exists():
    """This file is the reference OF mcq_raceline_device_ends / raceline_batch(ends=...): without the entry it has nothing to stand for."""
    import inspect
    import os
    from conftest import ROOT
    from global_racetrajectory_optimization_amd import engine
    assert "mcq_raceline_device_ends" in engine.EXPORTED_SYMBOLS and "ends" in inspect.signature(engine.Engine.raceline_batch).parameters
    with open(os.path.join(ROOT, "include", "mcq.h")) as f:
        assert "int mcq_raceline_device_ends(" in f.read()


@pytest.mark.parametrize("family", tuple(oc.FAMILIES))
@pytest.mark.parametrize("dtype", [np.float64, LD])
def test_reference_satisfies_its_own_conditions(family, dtype):
    """tph's joint conditions to rounding, b_0 = h_s, the last spline's derivative at t = 1 = h_e, the last station = the last raceline point."""
    for n in oc.SIZES:
        ref, nv, al, psi_s, psi_e = oc.arc(family, n)
        fr = ror.front(ref, nv, al, psi_s, psi_e, dtype)
        a, b, c, d = fr["coef"]
        scale = float(np.max(np.abs(fr["P"][1:] - fr["P"][:-1])))
        tol = 1e-13 * max(1.0, scale) * (1.0 if dtype is LD else 100.0)
        assert og.dmax(b[:-1] + 2 * c[:-1] + 3 * d[:-1], b[1:]) < tol, n
        assert og.dmax(2 * c[:-1] + 6 * d[:-1], 2 * c[1:]) < tol, n
        assert og.dmax(a + b + c + d, fr["P"][1:]) < tol * max(1.0, float(np.max(np.abs(fr["P"])))), n
        assert og.dmax(b[0], ror.heading_vector(psi_s, dtype)) < tol, n
        assert og.dmax(b[-1] + 2 * c[-1] + 3 * d[-1], ror.heading_vector(psi_e, dtype)) < tol, n
        assert abs(float(np.hypot(*ror.heading_vector(psi_s, dtype))) - ror.HEADING_SCALE) < 1e-15


@pytest.mark.parametrize("family", tuple(oc.FAMILIES))
def test_reference_matches_the_host_shims(family):
    """calc_splines(psi_s, psi_e, use_dist_scaling=False) + calc_spline_lengths + interp_splines(incl_last_point=True) + calc_head_curv_an: the host
    composition the device entry stands for, to 1e-12 (relative to the coordinates' size) on the sizes up to 257."""
    for n in (s for s in oc.SIZES if s <= 257):
        ref, nv, al, psi_s, psi_e = oc.arc(family, n)
        P = ref[:, :2] + al[:, None] * nv
        scale = max(1.0, float(np.max(np.abs(P))))
        cx, cy, _, _ = tph.calc_splines.calc_splines(P, psi_s=psi_s, psi_e=psi_e, use_dist_scaling=False)
        fr = ror.front(ref, nv, al, psi_s, psi_e, np.float64)
        C = np.stack(fr["coef"], axis=2)
        assert og.dmax(C[:, 0, :], cx) < 1e-12 * scale and og.dmax(C[:, 1, :], cy) < 1e-12 * scale, n
        lengths = tph.calc_spline_lengths.calc_spline_lengths(cx, cy)
        assert og.dmax(fr["lengths"], lengths) < 1e-12 * scale
        for step in (oc.launches(family)[0][2], oc.launches(family)[2][2]):
            r = ror.stations(fr, step)
            xy, inds, tv, dists = tph.interp_splines.interp_splines(cx, cy, spline_lengths=lengths, incl_last_point=True, stepsize_approx=step)
            assert r["m"] == xy.shape[0], (n, step)
            assert og.dmax(r["xy"], xy) < 1e-12 * scale and og.dmax(np.cumsum(r["el_lengths"][:-1]), dists[1:]) < 1e-12 * scale
            psi, kappa = tph.calc_head_curv_an.calc_head_curv_an(cx, cy, inds, tv)
            assert og.dpsi(r["psi"], psi) < 1e-12 and og.dmax(r["kappa"], kappa) < 1e-12 * max(1.0, float(np.max(np.abs(kappa))))


@pytest.mark.parametrize("family", tuple(oc.FAMILIES))
def test_point_counts_are_decided(family):
    """total / stepsize of every row of every launch is at least INTEGER_GAP away from every integer in the longdouble reference; the aimed launches
    hit their counts; every generous launch has an arc AT mmax."""
    names = set()
    for name, sizes, step, mmax in oc.launches(family):
        ms = []
        for n in sizes:
            r = og.reference(family, n, step)
            assert abs(r["ratio"] - np.rint(r["ratio"])) >= oc.INTEGER_GAP, (name, n)
            assert r["m"] >= 2 and r["xy"].shape == (r["m"], 2) and r["el_lengths"].shape == (r["m"],) and r["el_lengths"][-1] == 0
            ms.append(r["m"])
        if oc.aimed(name):
            what, K = oc.aimed(name)
            assert ms[sizes.index(K)] == {"m==mmax": mmax, "m==mmax+1": mmax + 1, "m==3": 3, "m==2": 2}[what], (name, ms)
        else:
            assert max(ms) == mmax
        names.add(name.split("@")[0])
    assert names == {"1.37h", "0.61h", "2.0", "3.0", "m==mmax", "m==mmax+1", "m==3", "m==2"}
    assert oc.SIZES == (2, 3, 4, 5, 49, 50, 51, 97, 255, 256, 257, 2048, 2049, 2050, 4097)


def test_two_points_when_the_stepsize_exceeds_the_arc():
    for family in oc.FAMILIES:
        L = [x for x in oc.launches(family) if x[0] == "m==2@4097"][0]
        r = og.reference(family, 4097, L[2])
        fr = og.front(family, 4097, 0)
        assert r["m"] == 2 and og.dmax(r["xy"][0], fr["P"][0]) == 0.0 and og.dmax(r["xy"][1], fr["P"][-1]) < 1e-12
        assert r["el_lengths"][0] == r["total"]


def test_stored_spreads_are_complete_and_reproducible():
    ent = og.entries()
    z = np.load(og.PATH)
    assert sorted(z.files) == sorted(ent)
    for key in ("stadium/1.37h", "trefoil/m==mmax@97", "peanut/m==2@2", "stadium/m==mmax+1@2049"):
        new, old = ent[key](), og.spread(key)
        assert new.shape == old.shape
        assert np.allclose(np.maximum(4 * new, 1e-13), np.maximum(4 * old, 1e-13), rtol=1e-3, atol=0.0), key
