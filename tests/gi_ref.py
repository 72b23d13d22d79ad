"""TEST-ONLY reference of the Goldfarb-Idnani path (csrc/mcq_gi.inc): a plain dense restatement of the method in curvature coordinates, written from
the comments at the top of that file and DESIGN.md section 4.6 -- numpy on the dense E and k_ref of oracle/tph_ref.assemble_dense, no structure used.

    minimise 1/2 |xi + 2 k_ref|^2   s.t.   lo <= E^-1 xi <= hi   (box rows, normal +-E^-T e_i),   -kb <= k_ref + xi <= kb   (curvature rows, +-e_k)

One violated constraint enters per iteration; its normal d is orthogonalised against the working set's N_W = Q R (Gram-Schmidt, twice); what is left,
d2, is the primal step in xi, r = R^-1 Q'd the dual direction; t1 = min u_k / r_k over r_k > 0 keeps the multipliers non-negative (the blocking
constraint leaves by Givens rotations), t2 = -slack / |d2|^2 takes the entering constraint to its bound; t2 <= t1 is a full step and the constraint
joins.  A normal that depends on the working set with nothing to drop: "constraints are inconsistent".

xi and the multipliers are accumulated in longdouble, alpha = E^-1 xi is refined once with a longdouble residual (rings of up to REFINE_N waypoints:
the dense longdouble product is what costs); the projections are float64.

The VIOLATION RULE is pluggable:
  "engine"  box violations in units of the mean free width, curvature violations in units of kappa_bound, a row enters above MCQ_GI_TOLB metres /
            MCQ_GI_TOLK kappa_bound, dependence by |d2| <= MCQ_GI_DEP |d|;
  "qpgen2"  oracle/gi_dense.c's: slack / |row of G| over ALL rows in the order [I; -I; E; -E], |slack| < vsmall is zero, the first one wins a tie,
            dependence by |d2|^2 <= vsmall.

solve() returns a Trace: every event, q after it, the final working set and alpha, and the MARGIN of every decision taken on the way in units of the
engine's resolution (a margin of 1000: the decision would survive a thousand times what the engine resolves)."""
import numpy as np
import scipy.linalg as sla

TOLB, TOLK, DEP = 2e-9, 2e-9, 1e-9          # MCQ_GI_TOLB / MCQ_GI_TOLK / MCQ_GI_DEP of csrc/mcq_gi.inc
F_SCALE = 2.0                               # the factor-2 quirk (oracle/tph_ref.F_SCALE)
REFINE_N = 600
DECIDED = 1000.0                            # a case is admitted only if every margin is at least this many resolutions
ADD, DROP = 0, 1
MCQ_NT, MCQ_KMAX = 256, 120                 # csrc/mcq_kernels.hip, include/mcq.h: what the edges below are the edges OF


def vsmall():
    """qpgen2's: the smallest 1e-60 * 2^k with 1 + 0.1 v > 1 and 1 + 0.2 v > 1."""
    v = 1e-60
    while True:
        v += v
        if 1.0 + 0.1 * v > 1.0 and 1.0 + 0.2 * v > 1.0:
            return v


def small_qcap(nmax):
    """Constraints a SMALL slot holds (gi_small_qcap of csrc/mcq_api.hip): nmax / 8 rounded up to 64, at least 128, at most nmax."""
    return min(max(128, ((nmax // 8 + 63) // 64) * 64), nmax)


def code_of(i, kind, upper):
    """4 i + 2 kind + upper (kind 0: box row, 1: curvature row) -- the engine's code of a constraint."""
    return 4 * i + 2 * kind + upper


class Trace(dict):
    __getattr__ = dict.__getitem__


def solve(E, k_ref, lo, hi, kb, rule="engine", use_kappa=True, step_cap=None):
    E = np.asarray(E, dtype=np.float64)
    n = E.shape[0]
    ld = np.longdouble
    lu = sla.lu_factor(E)
    E_ld = E.astype(ld) if n <= REFINE_N else None
    row_norm = np.sqrt(np.sum(E * E, axis=1))
    vs = vsmall()
    free = hi - lo > 1e-12
    wmean = float(np.mean((hi - lo)[free])) if np.any(free) else 1.0

    def alpha_of(xi):
        x64 = xi.astype(np.float64)
        a = sla.lu_solve(lu, x64)
        if E_ld is not None:
            a = a + sla.lu_solve(lu, (xi - E_ld @ a.astype(ld)).astype(np.float64))
        return a

    Q = np.zeros((n, n), order="F")
    R = np.zeros((n, n), order="F")
    u = np.zeros(n + 1, dtype=ld)
    wk = np.zeros(n, dtype=np.int64)
    box_state = np.zeros(n, dtype=np.int64)       # -1 / +1: the lower / upper box row of waypoint i is in the working set
    kap_state = np.zeros(n, dtype=np.int64)
    xi = (-F_SCALE * np.asarray(k_ref, dtype=np.float64)).astype(ld)
    q = 0
    events, q_at_step = [], []
    m_viol = m_t = m_block = m_dep = np.inf
    window = False
    status = "ok"
    steps = 0
    cap = step_cap if step_cap is not None else 20 * n + 2000
    q_max = 0

    while True:
        a = alpha_of(xi)
        kp = np.asarray(k_ref + xi, dtype=np.float64)
        # violations (positive: violated) of the four rows of every waypoint: lower box, upper box, lower curvature, upper curvature
        v = np.full((n, 4), -1.0)
        v[:, 0] = np.where(box_state == -1, -1.0, lo - a)
        v[:, 1] = np.where(box_state == 1, -1.0, a - hi)
        if use_kappa:
            v[:, 2] = np.where(kap_state < 0, -1.0, -kb - kp)
            v[:, 3] = np.where(kap_state > 0, -1.0, kp - kb)
        if rule == "engine":
            thr = np.array([TOLB, TOLB, TOLK * kb, TOLK * kb])
            unit = np.array([wmean, wmean, kb, kb])
            val = np.where(v > thr, v / unit, 0.0)
            res = np.array([TOLB / wmean, TOLB / wmean, TOLK, TOLK])          # what the engine resolves, in the units of `val`
            window |= bool(np.any((v > thr / DECIDED) & (v < thr * DECIDED)))
            order = val.ravel()                                               # ascending code: the lowest code wins a tie
            back = np.arange(4 * n)
        else:
            val = np.where(v >= vs, v, 0.0)
            val[:, 2:] /= row_norm[:, None]
            res = np.array([TOLB, TOLB, TOLK * kb, TOLK * kb])[None, :] / np.column_stack((np.ones((n, 2)), row_norm, row_norm))
            # [I; -I; E; -E]: upper box rows, lower box rows, upper curvature rows, lower curvature rows -- the first one wins
            order = np.concatenate((val[:, 1], val[:, 0], val[:, 3], val[:, 2]))
            idx = np.arange(n)
            back = np.concatenate((4 * idx + 1, 4 * idx, 4 * idx + 3, 4 * idx + 2))
        k = int(np.argmax(order))
        best = float(order[k])
        if not best > 0.0:
            break
        p = int(back[k])
        rest = order.copy()
        rest[k] = 0.0
        r_p = res[p & 3] if np.ndim(res) == 1 else res[p >> 2, p & 3]
        m_viol = min(m_viol, (best - float(np.max(rest))) / r_p)
        i, kind, upper = p >> 2, (p >> 1) & 1, p & 1
        sg = -1.0 if upper else 1.0
        if kind == 0:
            e = np.zeros(n)
            e[i] = 1.0
            d = sg * sla.lu_solve(lu, e, trans=1)                   # E^-T e_i
            sp = float(hi[i] - a[i]) if upper else float(a[i] - lo[i])
        else:
            d = np.zeros(n)
            d[i] = sg
            sp = sg * float(kp[i]) + kb
        np2 = float(d @ d)
        up = ld(0.0)
        while True:
            steps += 1
            if steps > cap:
                status = "cap"
                break
            q_at_step.append(q)
            if q > 0:
                Qq = Q[:, :q]
                vv = Qq.T @ d
                d2 = d - Qq @ vv
                ww = Qq.T @ d2
                d2 = d2 - Qq @ ww
                vv = vv + ww
                r = sla.solve_triangular(R[:q, :q], vv)
            else:
                d2 = d.copy()
                vv = r = np.zeros(0)
            rho2 = float(d2 @ d2)
            ratio = np.sqrt(rho2 / np2) / DEP
            dep = not rho2 > DEP * DEP * np2 if rule == "engine" else rho2 <= vs
            m_dep = min(m_dep, max(ratio, 1.0 / ratio if ratio > 0.0 else np.inf))
            pos = np.where(r > 0.0)[0]
            has1 = pos.size > 0
            t1, l, nxt = np.inf, -1, np.inf
            if has1:
                cand = np.maximum(u[pos], 0).astype(np.float64) / r[pos]
                j = int(np.argmin(cand))                            # the first minimum
                t1, l = float(cand[j]), int(pos[j])
                if cand.size > 1:
                    nxt = float(np.min(np.delete(cand, j)))
            t2 = np.inf if dep else -sp / rho2
            if not has1 and dep:
                status = "inconsistent"
                break
            full = not dep and (not has1 or t2 <= t1)
            if has1 and not dep:
                m_t = min(m_t, abs(t1 - t2) / max(t1, t2) / TOLB)
            if not full and np.isfinite(nxt):
                m_block = min(m_block, ((nxt - t1) / nxt if nxt > 0.0 else 0.0) / TOLB)
            t = t2 if full else t1
            if not dep:
                xi = xi + ld(t) * d2
                sp += t * rho2
            u[:q] -= ld(t) * r
            up += ld(t)
            if full:
                R[:q, q] = vv
                R[q, q] = np.sqrt(rho2)
                Q[:, q] = d2 / np.sqrt(rho2)
                u[q] = up
                wk[q] = p
                if kind == 0:
                    box_state[i] = 1 if upper else -1
                else:
                    kap_state[i] = 1 if upper else -1
                q += 1
                q_max = max(q_max, q)
                events.append((ADD, p, -1, q))
                break
            # partial step: the blocking constraint leaves
            lcode = int(wk[l])
            if (lcode >> 1) & 1 == 0:
                box_state[lcode >> 2] = 0
            else:
                kap_state[lcode >> 2] = 0
            _delete(Q, R, u, wk, q, l)
            q -= 1
            events.append((DROP, lcode, l, q))
        if status != "ok":
            break
    a = alpha_of(xi)
    ev = np.array(events, dtype=np.int64).reshape(-1, 4)
    return Trace(status=status, events=ev, q_at_step=np.array(q_at_step, dtype=np.int64), steps=steps,
                 adds=int(np.sum(ev[:, 0] == ADD)), drops=int(np.sum(ev[:, 0] == DROP)), q_max=q_max, q_final=q,
                 codes=np.sort(wk[:q].copy()), alpha=a, xi=np.asarray(xi, dtype=np.float64), u=np.asarray(u[:q], dtype=np.float64),
                 n_active_box=int(np.sum(((wk[:q] >> 1) & 1) == 0)), n_active_kappa=int(np.sum(((wk[:q] >> 1) & 1) == 1)),
                 margins=dict(violation=float(m_viol), t1_t2=float(m_t), blocking=float(m_block), dependence=float(m_dep)),
                 window=bool(window), wmean=wmean, n=n)


def _delete(Q, R, u, wk, q, l):
    """Constraint l leaves: column l of R goes, rotations of rows (j, j + 1) restore the triangle, the same on columns (j, j + 1) of Q."""
    R[:q, l:q - 1] = R[:q, l + 1:q]
    R[:q, q - 1] = 0.0
    u[l:q - 1] = u[l + 1:q]
    u[q - 1] = 0
    wk[l:q - 1] = wk[l + 1:q]
    for j in range(l, q - 1):
        aa, bb = R[j, j], R[j + 1, j]
        h = np.hypot(aa, bb)
        cs, sn = (aa / h, bb / h) if h > 0.0 else (1.0, 0.0)
        rj, rj1 = R[j, j:q - 1].copy(), R[j + 1, j:q - 1].copy()
        R[j, j:q - 1] = cs * rj + sn * rj1
        R[j + 1, j:q - 1] = cs * rj1 - sn * rj
        qj, qj1 = Q[:, j].copy(), Q[:, j + 1].copy()
        Q[:, j] = cs * qj + sn * qj1
        Q[:, j + 1] = cs * qj1 - sn * qj
    Q[:, q - 1] = 0.0


def min_margin(tr):
    return min(tr.margins.values())


def decided(tr):
    """Every decision of the trace at least DECIDED resolutions clear, and no violation in the window around the entry threshold."""
    return min_margin(tr) >= DECIDED and not tr.window


# ---- the edges of csrc/mcq_gi.inc a trace can reach, by name ------------------------------------------------------------------------
EDGES = ("backsub/q63", "backsub/q64", "backsub/q65", "backsub/q128", "backsub/q129", "backsub/tail_block_of_one",
         "dots/every_q_mod_16", "sub/beyond_1024_rows", "delete/l0", "delete/last", "delete/q1", "delete/65_to_64", "delete/shift_beyond_1024",
         "set/exactly_n", "slot/qcap-1", "slot/qcap", "slot/qcap+1", "slot/grown", "slot/deletion_after_the_move", "polish/kappa_lists_in_slot", "inconsistent/nonempty",
         "mixed/box_and_kappa")
BATCH_EDGE = "batch/nm>n"                       # a property of the ragged batch, not of a trace
SHARPEST = "polish/121..128_kappa_rows_in_a_small_slot_never_grown"


def edges_hit(tr):
    """Names of the edges the trace reaches (small slot: that of a launch with nmax = n, as the runners launch single cases)."""
    n, qs, ev = tr.n, tr.q_at_step, tr.events
    out = set()
    for qq in (63, 64, 65, 128, 129):
        if np.any(qs == qq):
            out.add("backsub/q%d" % qq)
    if np.any((qs > 64) & (qs % 64 == 1)):
        out.add("backsub/tail_block_of_one")
    if len(set(int(x) % 16 for x in qs if x > 16)) == 16:
        out.add("dots/every_q_mod_16")
    if n > 4 * MCQ_NT and np.any(qs > 0):
        out.add("sub/beyond_1024_rows")
    dr = ev[ev[:, 0] == DROP]
    l, qb = dr[:, 2], dr[:, 3] + 1              # index dropped, q before the deletion
    if np.any((l == 0) & (qb > 1)):
        out.add("delete/l0")
    if np.any((l == qb - 1) & (qb > 1)):
        out.add("delete/last")
    if np.any(qb == 1):
        out.add("delete/q1")
    if np.any(qb == 65):
        out.add("delete/65_to_64")
    if np.any(qb > l + 1 + 4 * MCQ_NT):
        out.add("delete/shift_beyond_1024")
    if tr.q_max == n:
        out.add("set/exactly_n")
    qc = small_qcap(n)
    if qc < n:
        for d, nm in ((-1, "slot/qcap-1"), (0, "slot/qcap"), (1, "slot/qcap+1")):
            if tr.q_max == qc + d:
                out.add(nm)
        if tr.q_max > qc:
            out.add("slot/grown")
        if np.any((qb > qc) & (l < qc)):            # rotations through columns gi_grow copied: R is READ after the move, not only extended
            out.add("slot/deletion_after_the_move")
    if tr.status == "ok" and tr.n_active_kappa > MCQ_KMAX:
        out.add("polish/kappa_lists_in_slot")
        if tr.q_max <= qc and qc < n:
            out.add(SHARPEST)
    if tr.status == "inconsistent" and tr.q_final > 0:
        out.add("inconsistent/nonempty")
    if tr.status == "ok" and tr.n_active_kappa > 0 and tr.n_active_box > 0:
        out.add("mixed/box_and_kappa")
    return sorted(out)


def problem_dense(reftrack, normvec, kappa_bound, w_veh):
    """E, k_ref, lo, hi, H, f, G, h of a ring, by the dense oracle's assembly."""
    from oracle import tph_ref
    ref = np.asarray(reftrack, dtype=np.float64)
    A = tph_ref.calc_splines(np.vstack((ref[:, :2], ref[:1, :2])))[2]
    H, f, E, k_ref, aux = tph_ref.assemble_dense(ref, normvec, A)
    G, h = tph_ref.constraints_dense(ref, E, k_ref, kappa_bound, w_veh)
    lo, hi = -(ref[:, 3] - w_veh / 2), ref[:, 2] - w_veh / 2
    return dict(E=E, k_ref=k_ref, lo=lo, hi=hi, H=H, f=f, G=G, h=h, aux=aux, A=A)


def dense_code(j, n):
    """The engine's code of row j of the dense oracle's G = [I; -I; E; -E]."""
    return (4 * j + 1, 4 * (j - n), 4 * (j - 2 * n) + 3, 4 * (j - 3 * n) + 2)[j // n]
