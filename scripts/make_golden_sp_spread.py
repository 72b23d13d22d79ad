#!/usr/bin/env python
"""Writes tests/golden/sp_edges/sp_spread.npz: how far tests/sp_ref.py's answer is determined on every case of tests/sp_cases.py (tests/sp_guard.py says
how: its float64 run against its longdouble run, and its movement under four draws of a relative 1e-15 on rows and normals).  Names and spreads
only; the expected alphas are computed live.  Python loops over the rows of every ring: about a minute, over a pool.

  python scripts/make_golden_sp_spread.py [--jobs 8]
"""
import argparse
import multiprocessing as mp
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sp_cases as sc           # noqa: E402
import sp_guard as sg           # noqa: E402


def _one(name):
    r = sg.reference(name)
    return name, sg.compute_spread(name), r["margin_x"], r["margin_g"], r["rounds"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=8)
    args = ap.parse_args()
    names = sc.spread_names()
    with mp.Pool(args.jobs) as pool:
        rows = {r[0]: r[1:] for r in pool.imap_unordered(_one, names)}
    os.makedirs(os.path.dirname(sg.PATH), exist_ok=True)
    np.savez_compressed(sg.PATH, name=np.array(names), spread=np.array([rows[n][0] for n in names]))
    w = max(names, key=lambda n: rows[n][0])
    print("%d cases; largest spread %.2e m (%s), allowed %.2e; most rounds %d" % (len(names), rows[w][0], w, sg.FLOOR / 4.0, max(r[3] for r in rows.values())))
    cases = sc.all_names()          # (the derived inputs are compared by alpha alone: no margin is asked of them)
    for what, k in (("metres", 1), ("gradient units", 2)):
        m = min(cases, key=lambda n: rows[n][k])
        print("smallest margin in %s: %.2e (%s), required %.1e" % (what, rows[m][k], m, sg.MARGIN_MIN))
    for n in names:
        if 4.0 * rows[n][0] > sg.FLOOR or (n in cases and min(rows[n][1:3]) < sg.MARGIN_MIN):
            print("  NEEDS ANOTHER SEED (sp_cases.SEEDS): %s spread %.2e margins %.2e %.2e" % ((n,) + rows[n][:3]))


if __name__ == "__main__":
    main()
