"""The case table of the Goldfarb-Idnani edges suite (tests/test_gi_ref.py on the CPU, tests/test_emu_gi_edges.py on the SIMT interpreter,
tests/test_gpu_gi_edges.py on the MI355X): problems chosen for the edges of csrc/mcq_gi.inc's OWN code -- the 64-column blocks of gi_backsub, the
four-columns-per-wave tail of gi_dots, deletions at l = 0 / l = q - 1 / q = 1 / 65 -> 64, the pass-by-pass shift beyond 1024 constraints, a working
set of exactly n rows, a small slot that ends at qcap - 1 / qcap / qcap + 1, the polish's curvature lists in the slot --, each with what the dense
restatement tests/gi_ref.py expects the engine to do STEP FOR STEP: adds, drops, the largest working set on the way, the final codes.

SPECS names the families and what each case is there for; scripts/make_golden_gi_edges.py searches seeds until a candidate reaches its edges AND is
decided (gi_ref.decided: every decision of the trace at least 1000 x the engine's resolution clear, no violation near the entry threshold) and writes
inputs and expectations into tests/golden/gi_edges.npz -- data only.  The runners read that file alone: no case is built, searched or skipped at run
time.  A case is the smallest shape found that reaches its edge; only ring/all1200 is large (the shift beyond 1024 constraints needs a constraint
to leave from under 1025 others: 850 ... 870 lie above the deepest one at 1100 waypoints, 1058 at 1200)."""
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gi_edges.npz")
W_VEH = 2.0
KB_OFF = 100.0                      # box-only cases: a curvature bound no row comes near
MAX_CANDIDATES = 40                 # seeds tried per case before the generator gives up on it

# name: family, parameters, the edges (gi_ref.EDGES) the case is there for, emu: the SIMT interpreter finishes it in about a minute
SPECS = {
    # alternating rings, every row active at the end: q walks up to n through hundreds of deletions
    "ring/all64": dict(family="ring", n=64, amp=0.3, half=0.1, want=("backsub/q63", "set/exactly_n", "delete/l0", "delete/last"), emu=True),
    "ring/all130": dict(family="ring", n=130, amp=0.3, half=0.1, emu=True,
                        want=("backsub/q64", "backsub/q65", "backsub/q128", "backsub/q129", "backsub/tail_block_of_one",
                              "dots/every_q_mod_16", "slot/grown", "set/exactly_n")),
    "ring/all160": dict(family="ring", n=160, amp=0.3, half=0.1, want=("slot/grown", "slot/deletion_after_the_move"), emu=True),
    "ring/all300": dict(family="ring", n=300, amp=0.3, half=0.1, want=("slot/grown", "slot/deletion_after_the_move", "set/exactly_n", "delete/65_to_64"), emu=False),
    "ring/all1200": dict(family="ring", n=1200, amp=0.3, half=0.1, want=("delete/shift_beyond_1024", "sub/beyond_1024_rows", "slot/grown"), emu=False),
    # ... all rows but `wide` of them (50 m of room there): the small slot of 128 constraints ends one short, full, one over
    "ring/slot127": dict(family="ring", n=129, amp=0.3, half=0.1, wide=2, want=("slot/qcap-1",), emu=True),
    "ring/slot128": dict(family="ring", n=129, amp=0.3, half=0.1, wide=1, want=("slot/qcap",), emu=True),
    "ring/slot129": dict(family="ring", n=130, amp=0.3, half=0.1, wide=1, want=("slot/qcap+1", "slot/grown"), emu=True),     # (the move is its LAST step: nothing reads
    # R afterwards -- 40 candidates with two wide rows at n = 131 never took a step at q = 129 either; ring/all130 and the larger ones do)
    # ... a dozen or two rows active: q stays small, alpha is off its bounds nearly everywhere (what the guard compares)
    "ring/part130": dict(family="ring", n=130, amp=0.1, half=0.3, want=(), emu=True),
    "ring/part300": dict(family="ring", n=300, amp=0.1, half=0.3, want=(), emu=False),
    "ring/n5": dict(family="ring", n=5, amp=0.3, half=0.1, want=(), emu=True),
    "uneven/q1": dict(family="uneven", n=16, skew=0.4, want=("delete/q1",), emu=True),
    # curvature rows: the stadium's plateaus (centreline and widths jittered: its symmetry would tie every decision), star-shaped rings
    "stadium/360": dict(family="stadium", n=360, kb=0.0223, want=("polish/kappa_lists_in_slot", "slot/grown"), emu=False),
    "star/mixed": dict(family="star", n=40, kb_rel=0.8, want=("mixed/box_and_kappa",), emu=True),
    "star/inconsistent": dict(family="star", n=40, kb_rel=0.2, want=("inconsistent/nonempty",), emu=True),
}
RAGGED = ("ring/all130", "ring/all300", "ring/n5")          # one launch: nmax = 300, so Q's column stride is not the ring's length for two of them
ALL_ACTIVE = ("ring/all130", "ring/all160", "ring/all300", "ring/all1200")  # the grown route must have run against the full-slot route for these at least
SLOT_EDGE = {"ring/slot127": -1, "ring/slot128": 0, "ring/slot129": 1}
LARGE = "ring/all1200"


def _scalings(A, n):
    idx = np.arange(n - 1)
    sc = np.empty(n)
    sc[:-1] = -A[4 * idx + 2, 4 * idx + 5]
    sc[-1] = A[4 * n - 2, 1]
    return sc


def build(name, seed):
    """Candidate `seed` of a case: dict(reftrack, normvec, scaling, kappa_bound, w_veh).  Generator-side (needs the dense oracle)."""
    from oracle import tph_ref
    s = SPECS[name]
    n = s["n"]
    rng = np.random.default_rng([seed, n, sum(ord(c) for c in name)])
    if s["family"] == "ring":
        # the centreline alternates +-amp about a circle with 3 m between waypoints; amp jittered by 30 %, the widths 1 + half raised by up to 20 % per side
        th = 2 * np.pi * np.arange(n) / n
        r = 3.0 * n / (2 * np.pi) + s["amp"] * (1 + 0.3 * rng.uniform(-1, 1, n)) * (-1.0) ** np.arange(n)
        xy = np.column_stack((r * np.cos(th), r * np.sin(th)))
        w = (1 + s["half"]) * (1 + 0.2 * rng.uniform(0, 1, (n, 2)))
        if s.get("wide"):
            w[rng.choice(n, s["wide"], replace=False)] = 50.0
        kb = KB_OFF
    elif s["family"] == "uneven":
        # a smooth ring with uneven spacing: neighbouring box normals nearly parallel and of different lengths, so a row can enter first and leave at once
        th = 2 * np.pi * (np.arange(n) + s["skew"] * rng.uniform(-1, 1, n)) / n
        r = 3.0 * n / (2 * np.pi) * (1 + 0.03 * np.sin(3 * th + rng.uniform(0, 6)))
        xy = np.column_stack((r * np.cos(th), r * np.sin(th)))
        # 50 m of room everywhere but at two neighbours i, j whose lower bounds the unconstrained line violates: i by more metres (it enters first), j
        # with the normal that takes i's violation along ((H^-1)_ij > (H^-1)_jj x viol_i / viol_j) -- i leaves when j enters, at q = 1
        w = np.full((n, 2), 50.0)
        _, _, A0, nv0 = tph_ref.calc_splines(np.vstack((xy, xy[0])))
        H, f, _, _, _ = tph_ref.assemble_dense(np.column_stack((xy, w)), nv0, A0)
        Hi = np.linalg.inv(H)
        x0 = -Hi @ f
        rho = np.array([Hi[k, (k + 1) % n] / Hi[(k + 1) % n, (k + 1) % n] for k in range(n)])
        i = int(np.argmax(rho))
        j = (i + 1) % n
        vj = 0.05
        vi = vj * (1.0 + 0.5 * (rho[i] - 1.0))
        w[i, 1] = W_VEH / 2 - (x0[i] + vi)
        w[j, 1] = W_VEH / 2 - (x0[j] + vj)
        kb = KB_OFF
    elif s["family"] == "stadium":
        from test_emu_kernels import _stadium
        xy = _stadium(n) + s.get("jit", 1e-3) * rng.uniform(-1, 1, (n, 2))
        w = s.get("w", 4.0) * (1 + 0.1 * rng.uniform(0, 1, (n, 2)))
        kb = s["kb"]
    else:
        from test_emu_kernels import _small_track
        ref, _, _, _ = _small_track(n, seed=9000 + seed)
        xy, w = ref[:, :2], ref[:, 2:]
        kb = None
        if "half" in s:             # a narrow corridor on the smooth ring: neighbouring rows want the same side
            w = (1 + s["half"]) * (1 + 0.2 * rng.uniform(0, 1, (n, 2)))
            kb = KB_OFF
    _, _, A, nv = tph_ref.calc_splines(np.vstack((xy, xy[0])))
    ref = np.column_stack((xy, w))
    if kb is None:
        # the bound relative to the curvature maximum of the box optimum
        from oracle import qp_ref
        H, f, E, k_ref, _ = tph_ref.assemble_dense(ref, nv, A)
        G, h = tph_ref.constraints_dense(ref, E, k_ref, KB_OFF, W_VEH)
        kb = float(s["kb_rel"] * np.max(np.abs(k_ref + E @ qp_ref.solve_qp_gi(H, f, G, h))))
    return dict(reftrack=ref, normvec=nv, scaling=_scalings(A, n), kappa_bound=float(kb), w_veh=W_VEH)


# ---- the committed table ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _table():
    z = np.load(GOLDEN)
    out = {}
    for key in z.files:
        name, field = key.split("|")
        out.setdefault(name, {})[field] = z[key]
    for c in out.values():
        for v in c.values():
            v.setflags(write=False)
    return out


def names():
    return tuple(n for n in SPECS if n in _table())


def case(name):
    """The stored case: inputs (reftrack, normvec, scaling, kappa_bound, w_veh) and the reference's expectations (status, adds, drops, steps, q_max,
    codes, n_active_box, n_active_kappa, events, alpha, curv_error, edges, margin, spread, seed, candidates)."""
    return _table()[name]


def problem(name):
    c = case(name)
    return dict(reftrack=np.array(c["reftrack"]), normvec=np.array(c["normvec"]), scaling=np.array(c["scaling"]),
                kappa_bound=float(c["kappa_bound"]), w_veh=float(c["w_veh"]))


def edges(name):
    return tuple(str(e) for e in case(name)["edges"])


def guard(name):
    """The rule of tests/ring_guard.py on the case's own spread (four draws of ring_guard.perturbed through the dense oracle)."""
    return max(1e-8, 4.0 * float(case(name)["spread"]))


EMU = tuple(n for n, s in SPECS.items() if s["emu"])
