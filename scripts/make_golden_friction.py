#!/usr/bin/env python3
"""Records what the reference's OWN FrictionMapInterface.get_friction_singlepos, extract_friction_coeffs and approx_friction_map("linear") return,
once, into tests/golden/friction/reference.npz (data only: maps, inputs and outputs of the calls), so that tests/test_fric_ref.py can hold the
plain restatement tests/fric_ref.py to them, and the device tests the engine, without the reference tree.

Run where the reference tree is at hand:   python scripts/make_golden_friction.py --reference /path/to/reference

Tracks: rounded_rectangle with its own data file (constant 1.0) and berlin_2018 with the varmue08-12 data; reftrack and normvec are those of
tests/golden/<track>.npz, the vehicle the ini's (width_opt 3.4, wheelbase_front 1.6, wheelbase_rear 1.4), dn 0.25.  Per track T:
  T/cells_hm int16 [c, 2], T/mue_c uint8 [c]    the map in half-metres and hundredths (asserted here to reproduce the parsed files exactly)
  T/q [2000, 2], T/q_idx, T/q_mue               seeded queries in and around the box, cKDTree's indices, get_friction_singlepos' values
  T/cnt [rows], T/n [rows, jmax]                extract_friction_coeffs' rows (NaN behind a row's count)
  T/mue_c4 uint8 [4, rows, jmax]                its four grids in hundredths (255 behind a row's count; asserted exact)
  T/w [4, rows, 2]                              approx_friction_map's lines (numpy.polyfit's)
  T/decided                                     packed bits [4, rows, jmax]: the query's gap to its runner-up exceeds 1e-9 m (longdouble, among
                                                cKDTree's five nearest)
w_floor: the largest difference between tests/fric_ref.line (longdouble) and numpy's polyfit over the recorded rows AND the grid cases of
tests/fric_cases.py; w_spread: the largest tests/fric_ref.line_spread over the same rows (tests/fric_guard.py: guard = max(floor, 4 x spread))."""
import argparse
import json
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
TRACKS = (("rounded_rectangle", "rounded_rectangle_tpamap.csv", "rounded_rectangle_tpadata.json"),
          ("berlin_2018", "berlin_2018_tpamap.csv", "berlin_2018_varmue08-12_tpadata.json"))
PARS = dict(optim_opts=dict(width_opt=3.4, var_friction="linear"), vehicle_params_mintime=dict(wheelbase_front=1.6, wheelbase_rear=1.4))
DN = 0.25
LD = np.longdouble


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "friction", "reference.npz"))
    a = ap.parse_args()
    from scipy.spatial import cKDTree
    import fric_cases as fc
    import fric_ref as fr
    from global_racetrajectory_optimization_amd import harness, trajectory_planning_helpers as tph
    sys.modules.setdefault("trajectory_planning_helpers", tph)          # the reference package imports it by that name
    sys.modules.setdefault("casadi", harness._stub_casadi())
    sys.path.insert(0, a.reference)
    import opt_mintime_traj
    src = opt_mintime_traj.src
    out = dict(tracks=np.array([t[0] for t in TRACKS]), params=np.array([3.4, 1.6, 1.4, DN]))
    floor = spread = 0.0
    for name, f_map, f_data in TRACKS:
        p_map, p_data = (os.path.join(a.reference, "inputs", "frictionmaps", f) for f in (f_map, f_data))
        iface = src.friction_map_interface.FrictionMapInterface(tpamap_path=p_map, tpadata_path=p_data)
        cells = np.loadtxt(p_map, comments='#', delimiter=';')
        with open(p_data) as fh:
            data = {int(k): v for k, v in json.load(fh).items()}
        mue = np.array([data[i][0] for i in range(cells.shape[0])])
        hm, mc = np.round(cells * 2.0).astype(np.int16), np.round(mue * 100.0).astype(np.uint8)
        assert np.array_equal(hm / 2.0, cells) and np.array_equal(mc / 100.0, mue), "%s: half-metres / hundredths do not reproduce the files" % name
        lo, hi = cells.min(axis=0), cells.max(axis=0)
        q = np.random.default_rng(sum(map(ord, name))).uniform(lo - 0.1 * (hi - lo), hi + 0.1 * (hi - lo), (2000, 2))
        q_mue = iface.get_friction_singlepos(q)
        assert q_mue.shape == (2000, 1)
        tree = cKDTree(cells)
        q_idx = tree.query(q)[1]
        z = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
        ref, nv = z["reftrack"], z["normvec"]
        n, *grids = src.extract_friction_coeffs.extract_friction_coeffs(reftrack=ref, normvectors=nv, tpamap_path=p_map, tpadata_path=p_data,
                                                                        pars=PARS, dn=DN, print_debug=False, plot_debug=False)
        w = src.approx_friction_map.approx_friction_map(reftrack=ref, normvectors=nv, tpamap_path=p_map, tpadata_path=p_data, pars=PARS, dn=DN,
                                                        n_gauss=5, print_debug=False, plot_debug=False)
        rows, cnt = len(n), np.array([len(r) for r in n], dtype=np.int32)
        jmax = int(cnt.max())
        n_pad, m4 = np.full((rows, jmax), np.nan), np.full((4, rows, jmax), 255, dtype=np.uint8)
        decided = np.zeros((4, rows, jmax), dtype=bool)
        R = fr.grid(ref, nv, 3.4, 1.6, 1.4, DN)
        cl = cells.astype(LD)
        for i in range(rows):
            n_pad[i, :cnt[i]] = n[i]
            for k in range(4):
                g = grids[k][i][:, 0]
                m4[k, i, :cnt[i]] = np.round(g * 100.0).astype(np.uint8)
                assert np.array_equal(m4[k, i, :cnt[i]] / 100.0, g)
                cand = tree.query(R[i]["xy"][k], k=5)[1]
                qq = R[i]["xy"][k].astype(LD)
                d = np.sort(np.hypot(cl[cand, 0] - qq[:, None, 0], cl[cand, 1] - qq[:, None, 1]), axis=1)
                decided[k, i, :cnt[i]] = (d[:, 1] - d[:, 0]) > 1e-9
                s, c = fr.line(n[i], g)
                floor = max(floor, float(abs(s - w[k][i, 0])), float(abs(c - w[k][i, 1])))
                spread = max(spread, fr.line_spread(n[i], g))
        print("%-18s %6d cells, %d rows, %d .. %d positions, %d queries, %d undecided" % (name, cells.shape[0], rows, cnt.min(), cnt.max(),
                                                                                         4 * cnt.sum(), 4 * cnt.sum() - decided.sum()))
        out.update({name + "/cells_hm": hm, name + "/mue_c": mc, name + "/q": q, name + "/q_idx": q_idx.astype(np.int32), name + "/q_mue": q_mue[:, 0],
                    name + "/cnt": cnt, name + "/n": n_pad, name + "/mue_c4": m4, name + "/w": np.stack(w[:4]),
                    name + "/decided": np.packbits(decided)})
    # the hand-made grids: numpy's polyfit on the restatement's rows
    cells, mue = fc.grid_map()
    for cname, case in fc.grid_cases().items():
        for (ref, nv), width in zip(case["tracks"], fc.widths_of(case)):
            if not np.all(np.isfinite(ref)):
                continue
            for r in fr.grid(ref, nv, width, fc.WB_F, fc.WB_R, case["dn"]):
                if r["cnt"] < 2:
                    continue
                for k in range(4):
                    g = mue[fr.nearest(cells, r["xy"][k])[0]]
                    with warnings.catch_warnings():
                        warnings.simplefilter("error")
                        pf = np.polyfit(r["n"], g, 1)
                    s, c = fr.line(r["n"], g)
                    floor = max(floor, float(abs(s - pf[0])), float(abs(c - pf[1])))
                    spread = max(spread, fr.line_spread(r["n"], g))
    out.update(w_floor=np.array(floor), w_spread=np.array(spread))
    print("w_mue: floor %.3e (longdouble against numpy.polyfit), spread %.3e -> guard %.3e" % (floor, spread, max(floor, 4 * spread)))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    np.savez_compressed(a.out, **out)
    print("-> %s (%d bytes)" % (a.out, os.path.getsize(a.out)))


if __name__ == "__main__":
    main()
