"""The reference side of the trajectory / check_traj tests, on the CPU alone: tests/traj_check_ref.py (the restatement) is held to the arrays
recorded from the reference's OWN interp_track, calc_min_bound_dists and check_traj (tests/golden/traj_check/reference_calls.npz, written by
scripts/make_golden_traj_check.py), the package's interp_track shim agrees with it, and the conditions the device tests rely on hold on every
case of tests/traj_check_cases.py: sample counts and flag decisions far from flipping, no case left out, every launch small, floors derived from
the measured values, stored spreads reproducible."""
import os

import numpy as np
import pytest

import traj_check_cases as tc
import traj_check_guard as tg
import traj_check_ref as tcr
from global_racetrajectory_optimization_amd import engine
from global_racetrajectory_optimization_amd.trajectory_planning_helpers import interp_track as shim
from oracle import vel_ref

LD = np.longdouble
RECORDED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "traj_check", "reference_calls.npz")
RECORD_TOL = 1e-12          # m: the float64 restatement against the reference's own float64 arrays
LEFT_OUT_MAX = 0            # cases left out of a comparison


@pytest.fixture(scope="module")
def rec():
    z = np.load(RECORDED)
    return {k: z[k] for k in z.files}


@pytest.mark.parametrize("track", ("berlin_2018", "handling_track"))
def test_restatement_reproduces_the_recorded_calls(rec, track):
    P = dict(zip([str(k) for k in rec["param_names"]], rec["params"]))
    ref, nv, traj = rec[track + "/reftrack"], rec[track + "/normvec"], rec[track + "/trajectory"]
    br, bl = tcr.boundaries(ref, nv, np.float64)
    assert tg.dmax(br, rec[track + "/bound_r"]) <= RECORD_TOL and tg.dmax(bl, rec[track + "/bound_l"]) <= RECORD_TOL
    sr, sl = tcr.interp_track(br, 1.0, np.float64), tcr.interp_track(bl, 1.0, np.float64)
    assert sr.shape == rec[track + "/interp_r"].shape and sl.shape == rec[track + "/interp_l"].shape
    assert tg.dmax(sr, rec[track + "/interp_r"]) <= RECORD_TOL and tg.dmax(sl, rec[track + "/interp_l"]) <= RECORD_TOL
    # the package's own shim of tph.interp_track is the same function
    assert tg.dmax(shim.interp_track(br, 1.0), sr) <= RECORD_TOL
    for mode, key in ((False, "/min_dists_all"), (True, "/min_dists_first")):
        r = tcr.bound_dists(ref, nv, traj[:, 1:3], traj[:, 3], P["length"], P["width"], 1.0, mode, np.float64)
        d = tg.dmax(r["min_dists"], rec[track + key])
        assert d <= RECORD_TOL, "%s, first_row_only=%s: %.3e m" % (track, mode, d)
        if mode:    # check_traj's own call measures against the first rows: the minimum it prints
            assert "%.2f" % float(r["min_dist"]) == "%.2f" % float(rec[track + "/printed_min_dist"])
    # the quirk is one: against the whole boundaries the vehicle is far closer than the printed figure
    assert rec[track + "/min_dists_all"].min() < rec[track + "/min_dists_first"].min() - 1.0


def test_profile_restatement_is_the_oracle(rec):
    """calc_ax_profile and the stable lap time of oracle/vel_ref.py, on the recorded Berlin profile taken as a ring of its own."""
    traj = rec["berlin_2018/trajectory"]
    vx = traj[:, 5]
    el = np.append(np.diff(traj[:, 0]), 2.0)
    T = tcr.trajectory(traj[:, 1:3], traj[:, 3], traj[:, 4], el, vx, True, np.float64)
    ax = vel_ref.calc_ax_profile(np.append(vx, vx[0]), el, False)
    assert tg.dmax(T["traj"][:, 6], ax) <= 1e-12
    assert abs(float(T["t"][-1]) - vel_ref.lap_time_stable(vx, el)) <= 1e-11
    To = tcr.trajectory(traj[:, 1:3], traj[:, 3], traj[:, 4], el, vx, False, np.float64)
    assert tg.dmax(To["traj"][:, 6], vel_ref.calc_ax_profile(vx, el[:-1], True)) <= 1e-12 and To["traj"][-1, 6] == 0.0
    assert To["t"].shape[0] == vx.shape[0] and T["t"].shape[0] == vx.shape[0] + 1


def test_constants_are_the_headers():
    assert tcr.ACC_MARGIN == engine.CHECK_ACC_MARGIN
    assert [tcr.CHK[k] for k in ("kappa", "ay", "ax_pos", "ax_neg", "a_tot", "machines", "v_max")] == \
        [engine.CHK_KAPPA, engine.CHK_AY, engine.CHK_AX_POS, engine.CHK_AX_NEG, engine.CHK_A_TOT, engine.CHK_MACHINES, engine.CHK_V_MAX]
    assert len(tcr.LIMITS) == engine.TRAJ_NLIM == len(engine.LIMIT_NAMES)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "mcq.h")).read()
    for line in ("#define MCQ_CHECK_ACC_MARGIN 0.1", "#define MCQ_CHECK_DIST_WARN 1.0", "#define MCQ_TRAJ_NLIM 6", "#define MCQ_BOUNDS_ALL 0",
                 "#define MCQ_BOUNDS_FIRST_ROW 1", "#define MCQ_CHK_V_MAX 64"):
        assert line in header, line
    kernels = open(os.path.join(root, "global_racetrajectory_optimization_amd", "csrc", "mcq_kernels.h")).read()
    assert "#define MCQ_BD_TILE %d" % tc.TILE in kernels and "#define MCQ_BD_S %d" % (tc.BLOCK // 256) in kernels


@pytest.mark.parametrize("family", tuple(tc.FAMILIES))
def test_conditions_of_the_boundary_cases(family):
    """Every sample count sits INTEGER_GAP from flipping, every launch stays below MAX_PAIRS, no case is left out, and the targeted sample counts
    are the ones the launches' names promise."""
    left_out, smallest = 0, 1.0
    names = [L["name"] for L in tc.bound_launches(family)]
    assert names == ["sizes", "blocks", "nb1", "tile-1", "tile", "tile+1", "2tiles+1", "large", "first_row", "zero_width", "lists"]
    for L in tc.bound_launches(family):
        assert tc.bound_pairs(L) <= tc.MAX_PAIRS, (family, L["name"], tc.bound_pairs(L))
        for k in range(len(L["rows"])):
            r = tc.bound_ref_cached(family, L["name"], k)
            gap = min(tc.gap_to_integer(q) for q in r["ratios"])
            smallest = min(smallest, gap)
            if gap < tc.INTEGER_GAP or not r["el_min"] > 0.0:
                left_out += 1
            assert np.all(np.isfinite(r["min_dists"].astype(np.float64))) and r["min_dist"] >= 0
    want = {"nb1": 1, "tile-1": tc.TILE - 1, "tile": tc.TILE, "tile+1": tc.TILE + 1, "2tiles+1": 2 * tc.TILE + 1}
    for name, nb in want.items():
        assert tc.bound_ref_cached(family, name, 0)["nb"][0] == nb
    assert left_out <= LEFT_OUT_MAX
    print("%s: total / stepsize_bound stays %.3g from an integer" % (family, smallest))
    # the zero-width waypoint: the two boundaries touch there
    r = tc.bound_ref_cached(family, "zero_width", 0)
    assert np.min(np.sum(np.abs(r["bound_r"] - r["bound_l"]), axis=1)) == 0.0


@pytest.mark.parametrize("family", tuple(tc.FAMILIES))
def test_conditions_of_the_trajectory_cases(family):
    """Every flag decision sits DECISION_GAP of its threshold away from it, in longdouble and in float64 alike; the flag cases set exactly
    their bit; the station counts are the chunk's edges."""
    left_out = 0
    for name, L in tg.traj_named_launches(family):
        for v in range(len(L["track_of"])):
            _, _, flags, gaps = tc.traj_reference(L, v)
            _, _, flags64, _ = tc.traj_reference(L, v, np.float64)
            if min(gaps.values()) < tc.DECISION_GAP:
                left_out += 1
            assert flags == flags64
    assert left_out <= LEFT_OUT_MAX
    for name, L, bit in tc.flag_launches(family):
        assert tc.traj_reference(L, 0)[2] == bit, name
    assert sorted(m for _, _, m in tc.traj_launch(family, True)["rows"]) == [2, 3, 255, 256, 257, 600]
    assert sorted(set(tc.traj_launch(family, True)["track_of"])) == list(range(6))      # every raceline shared by two variants


def test_floors_come_from_the_measured_deviation():
    """ax, t, ay, a_tot: floor = the next power of ten above four times the largest float64-against-longdouble deviation of the reference."""
    now = tg.measure_f64_deviation()
    for q, m in tg.MEASURED.items():
        assert now[q] <= m * 1.01 and now[q] >= m * 0.99, "%s: measured %.3e, the guard module says %.3e" % (q, now[q], m)
        assert tg.FLOOR[q] == tc.next_power_of_ten(4.0 * m), q
    assert tg.FLOOR["dist"] == tg.FLOOR["bound"] == tg.FLOOR["s"] == 1e-9


def test_stored_spreads_are_complete_reproducible_and_small():
    entries = tg.entries()
    z = np.load(tg.PATH)
    assert sorted(z.files) == sorted(entries)
    for key in ("peanut/bound/nb1", "trefoil/bound/zero_width", "stadium/bound/tile", "peanut/traj/closed", "stadium/traj/unclosed",
                "trefoil/traj/flag_a_tot"):
        new, old = entries[key](), z[key]
        assert new.shape == old.shape
        assert np.allclose(np.maximum(4 * new, 1e-15), np.maximum(4 * old, 1e-15), rtol=1e-3, atol=0.0), key
    # caps: no guard grows beyond a hundred floors -- the reference is determined everywhere the kernels are held to it
    for key in z.files:
        Q = tg.BOUND_Q if "/bound/" in key else tg.TRAJ_Q
        for qi, q in enumerate(Q):
            assert tg.guard(q, z[key][:, qi].max()) <= 100.0 * tg.FLOOR[q], (key, q, z[key][:, qi].max())
