"""
Generates tests/golden/open_edges.npz, tests/golden/open_kappa_fuzz.npz and tests/golden/SUMMARY_open_edges.json: open chains at the
structural edges of the chain code paths, through the dense oracle of tests/open_ref.py (tph's open calc_splines / opt_min_curv restated
densely, all 4N rows to the dense Goldfarb-Idnani of oracle.qp_ref.solve_qp_gi).

open_edges.npz -- the length ladder and the special chains:
  ladder     n in LADDER, seeded chains (open_ref.seeded_chain); case a: box only, b: fix_s + fix_e, c: a curvature bound at 0.8 x the
             curvature maximum of the box optimum with fix_e (n < 2040 only).  n = 47/48/49 and 255/256/257 straddle the segment-count
             switch of the saddle-point elimination, 63..73 the sweep window / halo, 2040..2048 the LDS capacity MCQ_CHAIN_MAXN.
  ragged     element lengths alternating 1 : 3, n = 49 and 257, cases a / c
  narrow     the last waypoint narrower than w_veh: with fix_e (solvable) and without (status_ref MCQ_INFEASIBLE, no alpha)
  stadium    the first 360 / 720 points of stadium rings of 400 / 800 (widths 4 m, w_veh 2 m, kappa 0.0223, headings the line's own):
             about MCQ_KMAX = 120 active curvature rows, and about twice that
open_kappa_fuzz.npz -- 120 chains, n in [20, 600], headings the line's own perturbed by up to +-0.1, curvature bound 0.6 .. 1.0 x the
  interior curvature maximum of the box optimum, random fix flags and widths; every tenth has its bound below the end rows' curvature
  (mostly the dense GI's "constraints are inconsistent": status_ref 5).

Layout (both files): chains are ragged rows [chain_offsets[c], chain_offsets[c+1]) of reftrack / normvec / scaling with psi_s / psi_e per
chain; problems refer to a chain and carry fix_s / fix_e / kappa_bound / w_veh, their alpha rows [offsets[k], offsets[k+1]) (zeros where
status_ref != 0), curv_error_max, n_active_kappa (positive multipliers of the curvature rows), status_ref and the KKT certificate.
alpha_spread: the largest |delta alpha| of the oracle over four draws of a relative 1e-15 random perturbation of H (symmetrised) and f --
the fixture's own determinacy, from which the tests derive their guard.  rev_gap / rev_curv_gap: the oracle's own gap between alpha and
-alpha'[::-1] of the mirrored chain (open_ref.mirror), asserted here for every ladder member with n >= 4.

PARITY UNPINNED by the reference: these are OUR oracle's outputs.  Deterministic (seeded, single-threaded BLAS per worker process);
several minutes of CPU (the dense oracle at n = 2048 inverts 8188 x 8188 matrices).  Never run by a test.
"""
import os

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[_v] = "1"              # bitwise-reproducible BLAS: one thread in every worker

import json  # noqa: E402
import math  # noqa: E402
import multiprocessing  # noqa: E402
import sys  # noqa: E402
import time  # noqa: E402

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import open_ref  # noqa: E402
from oracle import qp_ref  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
LADDER = (3, 4, 5, 8, 9, 15, 16, 17, 47, 48, 49, 63, 64, 65, 71, 72, 73, 255, 256, 257, 1023, 1024, 1025, 2040, 2047, 2048)
W_VEH = 2.0
W_STEP = 0.05
SPREAD_REL = 1e-15
SPREAD_DRAWS = 4
STATUS_INFEASIBLE, STATUS_KAPPA_INFEASIBLE = 1, 5
FAMILIES = ("ladder", "ragged", "narrow", "stadium", "fuzz")


def stadium_line(n, ls=120.0, r=40.0):
    """Two straights and two semicircles, n points equidistant in arclength (counter-clockwise), as the ring tests' stadium."""
    per = 2 * ls + 2 * np.pi * r
    xy = np.zeros((n, 2))
    for k, sk in enumerate(np.linspace(0.0, per, n, endpoint=False)):
        if sk < ls:
            xy[k] = (sk - ls / 2, -r)
        elif sk < ls + np.pi * r:
            th = (sk - ls) / r - np.pi / 2
            xy[k] = (ls / 2 + r * np.cos(th), r * np.sin(th))
        elif sk < 2 * ls + np.pi * r:
            xy[k] = (ls / 2 - (sk - ls - np.pi * r), r)
        else:
            th = (sk - 2 * ls - np.pi * r) / r + np.pi / 2
            xy[k] = (-ls / 2 + r * np.cos(th), r * np.sin(th))
    return xy


class Dense:
    """The dense QP of one chain (open_ref.assemble_open), solved for several bounds / fix flags."""

    def __init__(self, ref, nv, A, ps, pe):
        self.ref, self.n = ref, ref.shape[0]
        self.H, self.f, self.E, self.k_ref, self.aux = open_ref.assemble_open(ref, nv, A, ps, pe)

    def gh(self, kb, w_veh, fs, fe):
        hi, lo = open_ref.bounds_open(self.ref, w_veh, fs, fe)
        n = self.n
        return np.vstack((np.eye(n), -np.eye(n), self.E, -self.E)), np.concatenate((hi, lo, kb - self.k_ref, kb + self.k_ref))

    def solve(self, kb, w_veh, fs, fe, H=None, f=None):
        """dict(status, alpha, ...): status 0, MCQ_INFEASIBLE (bounds_open's "too small"), 5 (the GI's "inconsistent")."""
        n = self.n
        try:
            G, h = self.gh(kb, w_veh, fs, fe)
        except RuntimeError as e:
            assert "too small" in str(e)
            return dict(status=STATUS_INFEASIBLE, alpha=np.zeros(n))
        info = {}
        try:
            alpha = qp_ref.solve_qp_gi(self.H if H is None else H, self.f if f is None else f, G, h, info)
        except ValueError as e:
            assert "inconsistent" in str(e)
            return dict(status=STATUS_KAPPA_INFEASIBLE, alpha=np.zeros(n))
        if H is not None:
            return dict(status=0, alpha=alpha)
        kkt = qp_ref.kkt_residuals(self.H, self.f, G, h, alpha)
        return dict(status=0, alpha=alpha, curv_err=open_ref.curv_error(alpha, self.aux), nk=int(np.sum(info["lagr"][2 * n:] > 0)),
                    kkt_stationarity=float(kkt["stationarity"]), kkt_primal=float(kkt["primal"]))

    def spread(self, kb, w_veh, fs, fe, alpha, seed):
        rng = np.random.default_rng(seed)
        worst = 0.0
        for _ in range(SPREAD_DRAWS):
            R = rng.standard_normal((self.n, self.n))
            Hp = self.H * (1.0 + SPREAD_REL * 0.5 * (R + R.T))
            fp = self.f * (1.0 + SPREAD_REL * rng.standard_normal(self.n))
            r = self.solve(kb, w_veh, fs, fe, H=Hp, f=fp)
            worst = max(worst, float(np.max(np.abs(r["alpha"] - alpha))) if r["status"] == 0 else math.inf)
        return worst

    def kappa_max(self, alpha, interior=False):
        k = np.abs(self.k_ref + self.E @ alpha)
        return float(np.max(k[1:-1] if interior else k))


def solve_cases(D, cases, seed, mirror_of=None):
    """cases: (case, kb, w_veh, fs, fe) -> problem records (with spread and, given the mirrored chain's Dense, the reversal gap)."""
    out = []
    for j, (case, kb, wv, fs, fe) in enumerate(cases):
        r = D.solve(kb, wv, fs, fe)
        rec = dict(case=case, kappa_bound=float(kb), w_veh=wv, fix_s=fs, fix_e=fe, status=r["status"], alpha=r["alpha"],
                   curv_err=r.get("curv_err", 0.0), nk=r.get("nk", 0), kkt_stationarity=r.get("kkt_stationarity", 0.0),
                   kkt_primal=r.get("kkt_primal", 0.0), spread=0.0, rev_gap=-1.0, rev_curv_gap=-1.0)
        if r["status"] == 0:
            rec["spread"] = D.spread(kb, wv, fs, fe, r["alpha"], seed * 16 + j)
        if mirror_of is not None:
            rr = mirror_of.solve(kb, wv, fe, fs)
            assert rr["status"] == r["status"], (D.n, case, rr["status"], r["status"])
            if r["status"] == 0:
                rec["rev_gap"] = float(np.max(np.abs(-rr["alpha"][::-1] - r["alpha"])))
                rec["rev_curv_gap"] = abs(rr["curv_err"] - r["curv_err"])
        out.append(rec)
    return out


def chain_job(spec):
    """One chain and its problems.  spec: (family, n, seed)."""
    fam, n, seed = spec
    t0 = time.perf_counter()
    mirror = False
    if fam == "ladder":
        ref, nv, A, ps, pe = open_ref.seeded_chain(n, n, w_step=W_STEP)
        mirror = n >= 4
    elif fam == "ragged":
        ref, nv, A, ps, pe = open_ref.seeded_chain(n, n + 7, ragged=True, w_step=W_STEP)
    elif fam == "narrow":
        ref, nv, A, ps, pe = open_ref.seeded_chain(n, 4, w_step=W_STEP)
        ref[-1, 2:] = 0.75                       # w_r + w_l = 1.5 < w_veh = 2 at the last waypoint
    elif fam == "stadium":
        xy = stadium_line(n * 10 // 9)[:n]
        ps, pe = open_ref.own_headings(xy)
        ref, nv, A = open_ref.chain_from_line(xy, ps, pe, np.full((n, 2), 4.0))
    else:
        rng = np.random.default_rng(seed)
        xy = open_ref.seeded_path(n, seed, step=float(rng.uniform(1.0, 3.0)))
        ps, pe = open_ref.own_headings(xy)
        ps, pe = ps + float(rng.uniform(-0.1, 0.1)), pe + float(rng.uniform(-0.1, 0.1))
        w = np.round(rng.uniform(2.0, 4.0, size=(n, 2)) / W_STEP) * W_STEP
        ref, nv, A = open_ref.chain_from_line(xy, ps, pe, w)
    D = Dense(ref, nv, A, ps, pe)
    Dm = None
    if mirror:
        mref, mnv, mps, mpe, _, _ = open_ref.mirror(ref, nv, ps, pe)
        _, _, mA, _ = open_ref.calc_splines_open(mref[:, :2], psi_s=mps, psi_e=mpe)
        assert np.array_equal(open_ref.scalings_of(mA), open_ref.open_scalings(mref))
        Dm = Dense(mref, mnv, mA, mps, mpe)
    if fam in ("ladder", "ragged"):
        box = D.solve(1e3, W_VEH, False, False)
        cases = [("a", 1e3, W_VEH, False, False)]
        if fam == "ladder":
            cases.append(("b", 1e3, W_VEH, True, True))
        if n < 2040:
            cases.append(("c", 0.8 * D.kappa_max(box["alpha"]), W_VEH, False, fam == "ladder"))
    elif fam == "narrow":
        cases = [("fix_e", 1e3, W_VEH, False, True), ("free", 1e3, W_VEH, False, False)]
    elif fam == "stadium":
        cases = [("kappa", 0.0223, W_VEH, False, False)]
    else:
        fs, fe = bool(rng.integers(2)), bool(rng.integers(2))
        box = D.solve(1e3, W_VEH, fs, fe)
        if seed % 10 == 9:
            # far below the end rows' curvature with both ends pinned: mostly the dense GI's "constraints are inconsistent"
            fs = fe = True
            box = D.solve(1e3, W_VEH, fs, fe)
            kb = 0.05 * float(np.min(np.abs(D.k_ref[[0, -1]] + (D.E @ box["alpha"])[[0, -1]])))
        else:
            kb = float(rng.uniform(0.6, 1.0)) * D.kappa_max(box["alpha"], interior=True)
        cases = [("fuzz", kb, W_VEH, fs, fe)]
    probs = solve_cases(D, cases, seed, Dm)
    print("%-8s n=%4d  %s  %.1f s" % (fam, n, " ".join("%s:st%d,k%d,spread %.1e,rev %.1e" % (p["case"], p["status"], p["nk"], p["spread"], p["rev_gap"])
                                                       for p in probs), time.perf_counter() - t0), flush=True)
    return dict(family=fam, ref=ref, nv=nv, scaling=open_ref.scalings_of(A), psi_s=ps, psi_e=pe, probs=probs)


def save(path, chains):
    probs = [(c, p) for c, ch in enumerate(chains) for p in ch["probs"]]
    coff = np.concatenate(([0], np.cumsum([ch["ref"].shape[0] for ch in chains]))).astype(np.int64)
    off = np.concatenate(([0], np.cumsum([chains[c]["ref"].shape[0] for c, _ in probs]))).astype(np.int64)
    arr = dict(chain_offsets=coff, reftrack=np.concatenate([ch["ref"] for ch in chains]), normvec=np.concatenate([ch["nv"] for ch in chains]),
               scaling=np.concatenate([ch["scaling"] for ch in chains]), psi_s=np.array([ch["psi_s"] for ch in chains]),
               psi_e=np.array([ch["psi_e"] for ch in chains]),
               chain_family=np.array([FAMILIES.index(ch["family"]) for ch in chains], dtype=np.int32),
               offsets=off, chain=np.array([c for c, _ in probs], dtype=np.int32),
               case=np.array([p["case"] for _, p in probs]), alpha=np.concatenate([p["alpha"] for _, p in probs]))
    for key, src, dt in (("fix_s", "fix_s", np.bool_), ("fix_e", "fix_e", np.bool_), ("kappa_bound", "kappa_bound", np.float64),
                         ("w_veh", "w_veh", np.float64), ("status_ref", "status", np.int32), ("curv_error_max", "curv_err", np.float64),
                         ("n_active_kappa", "nk", np.int32), ("kkt_stationarity", "kkt_stationarity", np.float64),
                         ("kkt_primal", "kkt_primal", np.float64), ("alpha_spread", "spread", np.float64), ("rev_gap", "rev_gap", np.float64),
                         ("rev_curv_gap", "rev_curv_gap", np.float64)):
        arr[key] = np.array([p[src] for _, p in probs], dtype=dt)
    arr["family_names"] = np.array(FAMILIES)
    np.savez_compressed(path, **arr)
    return [dict(family=chains[c]["family"], n=int(chains[c]["ref"].shape[0]), case=p["case"], fix_s=p["fix_s"], fix_e=p["fix_e"],
                 kappa_bound=p["kappa_bound"], status_ref=p["status"], n_active_kappa=p["nk"], alpha_spread=p["spread"], rev_gap=p["rev_gap"],
                 kkt_stationarity=p["kkt_stationarity"], kkt_primal=p["kkt_primal"]) for c, p in probs]


def main():
    edges = [("ladder", n, n) for n in LADDER] + [("ragged", 49, 0), ("ragged", 257, 0), ("narrow", 33, 0), ("stadium", 360, 0),
                                                 ("stadium", 720, 0)]
    frng = np.random.default_rng(20261016)
    fuzz = [("fuzz", int(20 + 580 * frng.uniform() ** 3), 5000 + k) for k in range(120)]
    jobs = edges + fuzz
    order = sorted(range(len(jobs)), key=lambda j: -jobs[j][1])          # the largest first
    t0 = time.perf_counter()
    with multiprocessing.get_context("fork").Pool(min(8, os.cpu_count() or 1)) as pool:
        done = dict(zip(order, pool.map(chain_job, [jobs[j] for j in order], chunksize=1)))
    res = [done[j] for j in range(len(jobs))]
    # the oracle's own reversal symmetry (fails the run, after every job has reported)
    bad = [(ch["ref"].shape[0], p["case"], p["rev_gap"], p["spread"]) for ch in res for p in ch["probs"]
           if p["rev_gap"] >= 0 and p["rev_gap"] > max(1e-8, 4 * p["spread"])]
    assert not bad, "reversal identity broken in the oracle: %s" % bad
    summary = dict(edges=save(os.path.join(OUT, "open_edges.npz"), res[:len(edges)]),
                   fuzz=save(os.path.join(OUT, "open_kappa_fuzz.npz"), res[len(edges):]))
    with open(os.path.join(OUT, "SUMMARY_open_edges.json"), "w") as fh:
        json.dump(summary, fh, indent=1, sort_keys=True)
    print("done in %.0f s" % (time.perf_counter() - t0))


if __name__ == "__main__":
    main()
