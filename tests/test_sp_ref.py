"""tests/sp_ref.py, tests/sp_cases.py and tests/sp_guard.py on their own (no engine, no GPU): the reference agrees with the dense oracle the project
already trusts wherever that one is affordable, certifies itself on every case, and is determined far below the floor the kernels are held to; the case
tables meet the conditions that make comparing working sets row by row legitimate; the stored spreads are what tests/sp_guard.py computes."""
import numpy as np
import pytest

import sp_cases as sc
import sp_guard as sg
import sp_ref
from oracle import tph_ref

LD = np.longdouble
ORACLE_NMAX, ORACLE_TOL = 300, 1e-12


@pytest.mark.parametrize("name", [n for n in sc.all_names() if sc.size(n) <= ORACLE_NMAX])
def test_reference_against_the_dense_oracle(name):
    ref, nv, w_veh = sc.case(name)
    d = float(np.max(np.abs(sg.reference(name)["alpha"] - tph_ref.opt_shortest_path(ref, nv, w_veh).astype(LD))))
    print("%s: %.2e m" % (name, d))
    assert d < ORACLE_TOL, "%s: %.3e m from oracle/tph_ref.opt_shortest_path" % (name, d)


def test_the_reseeded_case_is_the_oracles_miss():
    """corner/257/row0 has another seed (sp_cases.SEEDS) because the dense oracle cannot make the 1e-12 m comparison on the first one.  That this
    is the oracle's defect and not the reference's is held here, on the FIRST seed: the reference certifies itself there as everywhere (sp_ref.solve
    raises otherwise), with both margins; the oracle's own point has rows of the reference's working set -- rows it has active itself, they are
    within 1e-11 m of their bounds -- more than half the comparison's tolerance off those bounds, so it cannot decide that comparison; and the two
    still agree to ten times that defect."""
    name = "corner/257/row0"
    assert name in sc.SEEDS and sc.SEEDS[name] != sc.default_seed(name)
    ref, nv = sc.ring(257, sc.default_seed(name))
    ref[sc.corner_rows(257, "row0"), 2:4] = sc.CLIPPED_WIDTH
    r = sp_ref.solve(ref, nv, sc.W_VEH)
    assert r["cert"] is not None and r["margin_x"] >= sg.MARGIN_MIN and r["margin_g"] >= sg.MARGIN_MIN
    xo = tph_ref.opt_shortest_path(ref, nv, sc.W_VEH).astype(LD)
    st = r["state"]
    off = np.where(st == sp_ref.AT_LO, np.abs(xo - r["lo"]), np.where(st == sp_ref.AT_HI, np.abs(xo - r["hi"]), 0))
    d = float(np.max(np.abs(r["alpha"] - xo)))
    print("first seed: the oracle's active rows are up to %.2e m off their bounds; reference - oracle %.2e m" % (float(np.max(off)), d))
    assert 0.5 * ORACLE_TOL < float(np.max(off)) < 1e-11
    assert d < 10.0 * float(np.max(off))


@pytest.mark.parametrize("family", sc.BASE_FAMILIES)
def test_certificate_and_margins(family):
    """sp_ref.solve asserts its certificate itself (exact rational arithmetic on the longdouble data); here: it ran, the float64 run ends on the same
    working set, and the optimum is MARGIN_MIN away from every change of the working set, in metres and in gradient units."""
    for name in sc.names(family):
        r = sg.reference(name)
        assert r["cert"] is not None and r["cert"] <= sp_ref.CERT_FACTOR * float(np.finfo(LD).eps), name
        assert r["margin_x"] >= sg.MARGIN_MIN and r["margin_g"] >= sg.MARGIN_MIN, (name, r["margin_x"], r["margin_g"])
        r64 = sp_ref.solve(*sc.case(name), dt=np.float64)
        assert np.array_equal(r64["state"], r["state"]), name
        lo, hi = sp_ref.bounds(sc.case(name)[0], sc.case(name)[2])
        assert np.array_equal(lo, r64["lo"]) and np.array_equal(hi, r64["hi"]) and np.all(hi - lo >= 2 * sp_ref.CLIP)
    if family == "all_free":
        assert all(not np.any(sg.reference(n)["state"]) and np.max(np.abs(sg.reference(n)["alpha"])) > 10.0 for n in sc.names(family))
    if family == "corner":
        for n in sc.EDGE_SIZES:
            for p in sc.CORNER_PATTERNS:
                st, rows = sg.reference("corner/%d/%s" % (n, p))["state"], sc.corner_rows(n, p)
                # the clipped rows are in the working set: row 0 / row n - 1 / every separator without exception (what the pattern is for)
                assert np.all(st[rows] != 0) if p in ("row0", "last", "both", "separators") else np.mean(st[rows] != 0) > 0.95, (n, p)


def test_every_guard_is_the_floor():
    names = sc.spread_names()
    z = np.load(sg.PATH)
    assert list(z["name"]) == names
    worst = max(names, key=sg.spread)
    print("largest spread %.2e m (%s)" % (sg.spread(worst), worst))
    assert all(4.0 * sg.spread(n) <= sg.FLOOR and sg.guard(n) == sg.FLOOR for n in names), (worst, sg.spread(worst))


@pytest.mark.parametrize("name", ["ladder/6", "ladder/257", "corner/514/separators", "all_free/777", "nonunit/2053", "ladder/4097",
                                  "w_veh/2053/3", "f32/257/4", "host/0", "host/519"])
def test_stored_spreads_are_reproducible(name):
    new, old = sg.compute_spread(name), sg.spread(name)
    assert np.isclose(max(4 * new, 1e-16), max(4 * old, 1e-16), rtol=1e-3, atol=0.0), (name, new, old)


def test_reference_under_the_single_pivot_rule():
    """The fallback of sp_ref.solve (Murty's rule once the full exchange cycles) is a route of its own to the same certified point: forced from
    the first round on, it ends on the same working set."""
    for name in ("ladder/64", "corner/257/second", "nonunit/257"):
        ref, nv, w_veh = sc.case(name)
        r = sp_ref.solve(ref, nv, w_veh, single_from_start=True)
        assert r["murty"] > 0 and np.array_equal(r["state"], sg.reference(name)["state"]) and np.array_equal(r["alpha"], sg.reference(name)["alpha"]), name


def test_launch_tables():
    seen = set()
    for lname, (rows, opts) in sc.launches().items():
        good = [r for r in rows if not r.startswith("bad/")]
        sizes = [sc.size(r) for r in good]
        assert len(rows) <= sc.MAX_LAUNCH and min(sizes) <= 6 and min(sizes) >= 3 and max(sizes) > sc.TRI_MAXN and any(s <= sc.TRI_MAXN for s in sizes), lname
        bad = [k for k, r in enumerate(rows) if r.startswith("bad/")]
        assert sorted(rows[k][4:] for k in bad) == sorted(sc.BAD) and bad[0] > 0 and bad[-1] < len(rows) - 1, lname
        assert all(sc.options(r) == opts for r in good)
        seen |= set(good)
    assert seen >= set(n for f in sc.FAMILIES for n in sc.names(f))          # every case of every family is in a launch
    assert sc.launch_problems(["bad/n2"])[0]["reftrack"].shape[0] == 2
    assert np.isnan(sc.bad("nan_normal")["normvec"]).sum() == 1 and np.isinf(sc.bad("inf_width")["reftrack"]).sum() == 1
    for n in (257, 514, 769, 2053):          # a last block of a single row
        m = sc.block_rows(n)
        assert m > 1 and n % m == 1
