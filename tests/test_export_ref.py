"""The export tests' own ground, on the CPU: the restatement tests/export_ref.py against what the reference's export_traj_race / export_traj_ltpl
wrote (tests/golden/export/reference_files.npz, scripts/make_golden_export.py); the package's writers against those bytes; the cap on undecided
waypoints for every case, on the reference alone; the hand-made tables' expected indices by numpy's argmin; the stored spreads; the host pieces of
Engine.export_batch."""
import os

import numpy as np
import pytest

import export_cases as xc
import export_guard as xg
import export_ref as xr
import glue_cases as gc
from global_racetrajectory_optimization_amd import engine, export

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "export", "reference_files.npz")
TRACKS = ("rounded_rectangle", "handling_track")


@pytest.fixture(scope="module")
def recorded():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def _lines(raw):
    return bytes(raw).decode("ascii").splitlines()


def _rows(lines):
    return np.array([[float(c) for c in ln.split("; ")] for ln in lines[3:]])


@pytest.mark.parametrize("name", TRACKS)
def test_the_restatement_against_the_reference_files(recorded, name):
    g = {k.split("/")[1]: v for k, v in recorded.items() if k.startswith(name + "/")}
    n = g["reftrack"].shape[0]
    for dtype in (np.longdouble, np.float64):
        R = xr.table(g["reftrack"], g["normvec"], g["alpha"], g["trajectory"], dtype)
        assert xg.dmax(R["lengths"], g["spline_lengths"]) <= xg.FLOOR and xg.dmax(R["race_cl"], g["traj_race_cl"]) <= xg.FLOOR
        rows = _rows(_lines(g["ltpl_file"]))
        assert rows.shape == (n, 12) and R["ltpl"].shape == (n + 1, 12)
        assert np.max(np.abs(rows - R["ltpl"][:n])) <= 0.5000001e-7
        # the indices the reference's loop took, read back from its file: at decided waypoints the station's values identify it
        und = xg.undecided(R["margin"], xg.FLOOR)
        assert np.mean(und) <= xc.UNDECIDED_CAP
        assert np.max(np.abs(rows[~und, 8:12] - g["trajectory"][R["idx"][~und], 3:7])) <= 0.5000001e-7
    assert [xr.rule(g["trajectory"][:, 0], s) for s in np.float64(R["s_ref"][:-1])] == list(xr.lookup(g["trajectory"][:, 0], np.float64(R["s_ref"][:-1]))[0])


@pytest.mark.parametrize("name", TRACKS)
def test_the_writers_against_the_reference_bytes(recorded, name, tmp_path):
    """From line 2 on (line 1 is a random UUID): the digest of the ggv file, the header, every row."""
    g = {k.split("/")[1]: v for k, v in recorded.items() if k.startswith(name + "/")}
    ggv = tmp_path / "ggv.csv"
    ggv.write_bytes(bytes(recorded["ggv_file"]))
    R = xr.table(g["reftrack"], g["normvec"], g["alpha"], g["trajectory"])
    export.write_traj_ltpl(tmp_path / "ltpl.csv", R["ltpl"], ggv_file=str(ggv))
    export.write_traj_race(tmp_path / "race.csv", R["race_cl"], ggv_file=str(ggv))
    for mine, theirs in (("ltpl.csv", "ltpl_file"), ("race.csv", "race_file")):
        a, b = (tmp_path / mine).read_bytes().split(b"\n"), bytes(g[theirs]).split(b"\n")
        assert len(a[0]) == len(b[0]) == 2 + 36 and a[0] != b[0] and a[1:] == b[1:], "%s differs from the reference's file" % mine
    export.write_traj_race(tmp_path / "race0.csv", R["race_cl"])
    uid, digest, names, rows = export.read_table(tmp_path / "race0.csv")
    assert digest == "da39a3ee5e6b4b0d3255bfef95601890afd80709" and names == export.RACE_COLUMNS and rows.shape == R["race_cl"].shape and len(uid) == 36
    with pytest.raises(ValueError):
        export.write_traj_ltpl(tmp_path / "bad.csv", R["race_cl"])


@pytest.mark.parametrize("family", xc.FAMILIES)
def test_the_cap_on_undecided_waypoints_holds_on_the_reference_alone(family):
    for L in xc.launches(family):
        name = L["name"].split("/")[1]
        for v, t in enumerate(L["track_of"]):
            n = L["tracks"][t][0].shape[0]
            R = xc.reference(family, name, v)
            und = xg.undecided(R["margin"], xg.guards("%s/%d" % (family, n))[0])
            assert np.mean(und) <= xc.UNDECIDED_CAP, "%s variant %d: %d of %d waypoints undecided" % (L["name"], v, int(np.sum(und)), n)
            assert np.array_equal(R["idx"][~und], [xr.rule(L["trajs"][v][:, 0], s) for s in np.float64(R["s_ref"][:-1])[~und]])


def test_the_ties_case_is_one():
    track, traj = xc.ties()
    R = xr.table(*track, traj)
    und = xg.undecided(R["margin"], xg.guards("ties")[0])
    assert np.sum(und) >= track[0].shape[0] // 4


def test_the_hand_made_tables_by_argmin():
    q = np.float64(xr.front(*gc.ring(*xc.HAND_RING), np.float64)["s_ref"][:-1])
    for name, col, expected in xc.handmade(q):
        col = np.array(col)
        assert np.all(np.diff(col) >= 0.0)
        assert [int(np.abs(col - s).argmin()) for s in q] == expected == [xr.rule(col, s) for s in q], name
    col = np.array([0.0, 1e-17, 2e-17, 1.0])
    assert int(np.abs(col - 0.5).argmin()) == 0 == xr.rule(col, 0.5)


def test_the_stored_spreads():
    rings = xg.rings()
    assert set(np.load(xg.PATH).files) == set(rings)
    for key in ("peanut/7", "trefoil/257", "peanut/2049", "ties"):
        assert np.array_equal(xg.compute_spread(rings[key]), xg.spread(key)), key


def test_the_host_pieces_of_export_batch():
    """engine.export_result: the padded outputs cut to lists, the closed race tables, refused variants."""
    ns, ms, tr = np.array([3, 5], dtype=np.int32), np.array([4, 2], dtype=np.int32), np.array([1, 0, 1], dtype=np.int32)
    rng = np.random.default_rng(5)
    tab, idx = rng.standard_normal((3, 6, 12)), rng.integers(0, 4, (3, 5)).astype(np.int32)
    lens, s_ref, total = rng.random((2, 5)), rng.random((2, 6)), np.array([11.0, 22.0])
    tj = rng.standard_normal((3, 4, 7))
    status = np.array([0, 4, 0], dtype=np.int32)
    out = engine.export_result(tab, idx, lens, s_ref, total, status, ns, ms, tr, tj)
    assert [a.shape for a in out["ltpl"]] == [(6, 12), (4, 12), (6, 12)] and [a.shape for a in out["idx"]] == [(5,), (3,), (5,)]
    assert [a.shape for a in out["spline_lengths"]] == [(3,), (5,)] and [a.shape for a in out["s_ref"]] == [(4,), (6,)]
    assert [a.shape for a in out["race_cl"]] == [(3, 7), (5, 7), (3, 7)]
    assert out["race_cl"][0][-1, 0] == 22.0 and np.array_equal(out["race_cl"][0][-1, 1:], tj[0, 0, 1:]) and np.array_equal(out["race_cl"][0][:2], tj[0, :2])
    assert np.isnan(out["race_cl"][1][-1, 0]) and np.array_equal(out["ltpl"][1], tab[1, :4])
    assert engine.LTPL_COLS == 12 == len(export.LTPL_COLUMNS) and engine.TRAJ_COLS == len(export.RACE_COLUMNS)
