"""The reference of the IQP edges suite (tests/test_emu_iqp.py, tests/test_gpu_iqp.py): tph.iqp_handler's loop as oracle/tph_ref.iqp_handler
states it -- the same calls in the same order: tph_ref.opt_min_curv's pieces, create_raceline, interp_track_widths, calc_splines -- with every round
kept and a round cap.  Nothing of the glue is restated here.

run(...) returns the list of rounds; the last entry is the end state.  A round holds
  iter, n, reftrack [n, 4], normvec [n, 2]   the ring the pass linearised on
  alpha [n]                                  UNDAMPED, as the QP returned it (the damping belongs to the step into the next ring)
  curv_error_max
  kappa_active                               rows of [E; -E] on their bound at alpha (the reference's own rows)
  length, ratio                              arclength of the raceline that create_raceline re-samples and length / stepsize_interp, the number
                                             whose ceiling is the next ring's waypoint count; None for a round without a step behind it
  stopped                                    True: iqp_handler's own break; False in the last entry: the round cap ended the run

Routes.  "gi": the dense Goldfarb-Idnani oracle (oracle/gi_dense.c), what tph_ref.iqp_handler runs -- THE reference.  "second": every pass's QP
by qp_ref.solve_box_second_route (trust-region-reflective least squares on the dense E) where no curvature row is active at its optimum; otherwise
by the banded CPU-B solver (oracle/banded_ref.solve_batch, rings of at least banded_ref.MIN_N waypoints) where that solves the pass -- CPU-B is a
box solver that CHECKS the curvature rows (status 6 where one is violated at the box optimum), so a pass whose optimum sits on a curvature row
is beyond both; such a pass goes to the dense oracle on H and f perturbed by a relative 1e-15 (ring_guard.perturbed: what the ring fixtures with
active curvature rows take their spread from).  ("draw", d): that perturbed oracle in every pass, draw d.  The distance between "gi" and the
others is the spread of tests/iqp_guard.py."""
import numpy as np

from oracle import banded_ref, qp_ref, tph_ref
from ring_guard import draw_rng, perturbed

KAPPA_ON = 1e-9         # a curvature row counts as active within this of its bound (1/m)


def scalings_of(A):
    """The n spline scalings a closed-spline matrix of tph_ref.calc_splines encodes (what the engine is given for the first pass)."""
    n = A.shape[0] // 4
    return np.array([-A[4 * i + 2, 4 * i + 5] for i in range(n - 1)] + [A[4 * n - 2, 1]])


def _perturbed_gi(H, f, G, h, n, it, draw):
    Hp, fp = perturbed(H, f, draw_rng("iqp_edges", "pass", n * 100 + it, draw))
    return qp_ref.solve_qp_gi(Hp, fp, G, h)


def _pass(reftrack, normvec, A, kappa_bound, w_veh, route, it):
    """One QP pass: (alpha, curv_error_max, rows of [E; -E] active)."""
    H, f, E, k_ref, aux = tph_ref.assemble_dense(reftrack, normvec, A)
    G, h = tph_ref.constraints_dense(reftrack, E, k_ref, kappa_bound, w_veh)
    n = reftrack.shape[0]
    if route == "gi":
        alpha = qp_ref.solve_qp_gi(H, f, G, h)
    elif route == "second":
        alpha = qp_ref.solve_box_second_route(E, k_ref, -h[n:2 * n], h[:n])
        if np.max(np.abs(E @ alpha + k_ref)) >= kappa_bound - KAPPA_ON:
            st = [-1]
            if n >= banded_ref.MIN_N:
                al, _, st, _, _ = banded_ref.solve_batch(reftrack[None], normvec[None], scalings_of(A)[None] if it == 1 else None, kappa_bound,
                                                         w_veh, nthreads=1)
            alpha = al[0] if st[0] == 0 else _perturbed_gi(H, f, G, h, n, it, 0)
    else:
        alpha = _perturbed_gi(H, f, G, h, n, it, int(route[1]))
    kap = E @ alpha + k_ref
    active = int(np.sum(kap >= kappa_bound - KAPPA_ON) + np.sum(-kap >= kappa_bound - KAPPA_ON))
    return alpha, tph_ref.curv_error(alpha, aux), active


def run(reftrack, normvectors, A, kappa_bound, w_veh, stepsize_interp, iters_min=3, curv_error_allowed=0.01, max_rounds=None, route="gi"):
    reftrack_tmp = np.array(reftrack, dtype=np.float64)
    normvec_tmp = np.array(normvectors, dtype=np.float64)
    A_tmp = A
    rounds = []
    it = 0
    while True:
        it += 1
        alpha, err, active = _pass(reftrack_tmp, normvec_tmp, A_tmp, kappa_bound, w_veh, route, it)
        rec = dict(iter=it, n=reftrack_tmp.shape[0], curv_error_max=err, alpha=alpha.copy(), reftrack=reftrack_tmp.copy(),
                   normvec=normvec_tmp.copy(), kappa_active=active, length=None, ratio=None, stopped=False)
        rounds.append(rec)
        if it < iters_min:
            alpha = alpha * (it * 1.0 / iters_min)
        if it >= iters_min and err <= curv_error_allowed:
            rec["stopped"] = True
            break
        if max_rounds is not None and it >= max_rounds:
            break
        rl = tph_ref.create_raceline(reftrack_tmp[:, :2], normvec_tmp, alpha, stepsize_interp)
        refline_tmp, inds, tv, lengths = rl[0], rl[4], rl[5], rl[7]
        rec["length"] = float(np.cumsum(lengths)[-1])          # (what tph_ref.interp_splines divides)
        rec["ratio"] = rec["length"] / stepsize_interp
        reftrack_tmp[:, 2] -= alpha
        reftrack_tmp[:, 3] += alpha
        ws = tph_ref.interp_track_widths(reftrack_tmp[:, 2:], inds, tv)
        reftrack_tmp = np.column_stack((refline_tmp, ws))
        refline_cl = np.vstack((reftrack_tmp[:, :2], reftrack_tmp[0, :2]))
        _, _, A_tmp, normvec_tmp = tph_ref.calc_splines(refline_cl, use_dist_scaling=False)
    for r in rounds:
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return rounds
