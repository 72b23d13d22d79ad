"""The tight check on closed-ring (ring) results, on top of the 1e-6 m contract: guard(name, k, what) = max(1e-8, 4 x spread), by the rule
of tests/open_ref.py's OpenFixture.guard.

spread: how far the committed oracle answer `what` of fixture `name` (problem k of a batched fixture) is determined.  The larger of
  - the oracle's own movement under four draws of a relative 1e-15 perturbation of H (symmetrised) and f (perturbed below), measured
    against the stored golden value, and
  - every inter-route difference on record for that fixture (tests/golden/CHECK_r6.json, SUMMARY*.json second_route / bvls).
Written by scripts/make_golden_ring_spread.py into tests/golden/ring_spread.npz; a guard widens only through a recomputed spread there.

Comparisons without a stored fixture (the live dense oracle, CPU-B, two GPU paths at the same vertex) use FIXED."""
import os

import numpy as np

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PATH = os.path.join(GOLDEN_DIR, "ring_spread.npz")
FIXED = 1e-8
SPREAD_REL = 1e-15          # the constants of scripts/make_golden_open_edges.py
SPREAD_DRAWS = 4

# every ring fixture and the golden keys whose spread is on record (batched fixtures: one entry per status-0 problem)
FIRST_PASS = ("rounded_rectangle", "handling_track", "modena_2019", "berlin_2018", "berlin_2018_n333",
              "oval_n2000", "oval_n2000_w1", "oval_n2000_w2", "oval_n2000_w3", "oval_n2000_w7", "oval_n2000_w11",
              "oval_n2000_c5", "oval_n2000_c9", "oval_n2000_c13", "oval_n2000_c21", "oval_n2000_kappa",
              "oval_n2100", "oval_n2600", "oval_n2600_kappa")
UNIT_SCALING = ("iqp_pass2_oval5", "iqp_pass3_oval3", "iqp_pass3_oval629", "iqp_pass3_oval9")
IQP_CHAINS = ("rounded_rectangle", "handling_track", "berlin_2018_iqp", "modena_2019_iqp", "oval_n2000")
SHORTEST = ("rounded_rectangle", "handling_track", "modena_2019", "berlin_2018")
HARNESS = ("mincurv_oracle_alpha", "iqp_oracle_alpha", "iqp_oracle_reftrack", "shortest_oracle_alpha", "reopt_oracle_alpha")


def expected_entries():
    """(name, what, k) of every entry ring_spread.npz must hold (k = -1: not batched)."""
    out = [(n, "alpha", -1) for n in FIRST_PASS + UNIT_SCALING]
    out += [(n, w, -1) for n in IQP_CHAINS for w in ("iqp_alpha", "iqp_reftrack")]
    out += [("shortest_path", t + "_alpha", -1) for t in SHORTEST] + [("shortest_path_n2100", "alpha", -1)]
    out += [("harness_calls_berlin", w, -1) for w in HARNESS]
    z = np.load(os.path.join(GOLDEN_DIR, "kappa_tight_fuzz.npz"))
    out += [("kappa_tight_fuzz", "alpha", k) for k in range(len(z["status_ref"])) if int(z["status_ref"][k]) == 0]
    return out


def perturbed(H, f, rng, rel=SPREAD_REL):
    """One draw: H (1 + rel (R + R')/2) elementwise, f (1 + rel r), R and r standard normal."""
    n = f.shape[0]
    R = rng.standard_normal((n, n))
    return H * (1.0 + rel * 0.5 * (R + R.T)), f * (1.0 + rel * rng.standard_normal(n))


def perturbed_solver(rng):
    """A solver(H, f, G, h) for oracle.tph_ref's opt_min_curv / iqp_handler that perturbs H and f before the dense GI solve."""
    from oracle import qp_ref

    def solver(H, f, G, h):
        Hp, fp = perturbed(H, f, rng)
        return qp_ref.solve_qp_gi(Hp, fp, G, h)
    return solver


def draw_rng(name, what, k, draw):
    """The generator of one draw: seeded by the entry and the draw index alone (a pool may run draws in any order)."""
    key = "%s/%s/%d" % (name, what, k)
    return np.random.default_rng([sum((i + 1) * ord(c) for i, c in enumerate(key)), len(key), k + 1, draw])


_Z = None


def _table():
    global _Z
    if _Z is None:
        z = np.load(PATH)
        _Z = {(str(n), str(w), int(k)): (float(s), float(p), float(r))
              for n, w, k, s, p, r in zip(z["name"], z["what"], z["k"], z["spread"], z["perturb_spread"], z["route_gap"])}
    return _Z


def spread(name, k=None, what="alpha"):
    return _table()[(name, what, -1 if k is None else int(k))][0]


def guard(name, k=None, what="alpha"):
    """max(1e-8, 4 x spread) of the stored entry; a KeyError if the fixture has none."""
    return max(FIXED, 4.0 * spread(name, k, what))


class Worst:
    """The worst |d alpha| per family next to its guard, for the log (open_ref.worst_report's form)."""

    def __init__(self):
        self.w = {}

    def add(self, family, d, g):
        w = self.w.get(family)
        if w is None or d > w[0]:
            self.w[family] = [float(d), float(g)]
        return d

    def report(self, title, what="|d alpha|"):
        return "%s: worst %s per family (guard): %s" % (title, what, ", ".join(
            "%s %.1e (%.1e)" % (f, *w) for f, w in sorted(self.w.items())))


def print_uncaptured(config, line):
    """Print past pytest's capture (the GPU log records what the engine achieves next to its guards)."""
    cm = config.pluginmanager.getplugin("capturemanager")
    if cm is None:
        print(line)
        return
    with cm.global_and_fixture_disabled():
        print(line)


def dmax(a, b):
    return float(np.max(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64))))
