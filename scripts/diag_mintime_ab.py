"""DIAGNOSTIC: do two builds of the library compute the minimum-time entries alike bit for bit?  One library per process:

    python scripts/diag_mintime_ab.py --dump libA.so A.npz          (a fresh process per library)
    python scripts/diag_mintime_ab.py --dump libB.so B.npz
    python scripts/diag_mintime_ab.py --compare A.npz B.npz         (exit status 1 where a word differs)

Every launch chains all seven entries on the device -- bounds, evaluation, Jacobian, certificate, Hessian, H v (nvec = 2), Newton step (nvec = 5,
refine = 2) -- on the problems of tests/mintime_cases.py at N = 2, 3, 7, 8, 65 with the multipliers of tests/mintime_hess_cases.py's kind (seeded,
uniform): the options plain, safe, energy, linear, gauss5 and all; a ragged launch under nmax = 70; one whose n_list holds 0, 1 and nmax + 1; one
with a NaN in w; one whose step meets a zero pivot.  The step's diagonals come from the launch's own Hessian blocks and bounds (dw: twice the largest absolute block row sum, dg: 1e-6
on equality rows, 1 on the others), so they are the same wherever the blocks are.  Every output array is compared as raw 64-bit (int32: 32-bit)
words, NaN tails included.  No threshold."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

SIZES = (2, 3, 7, 8, 65)
NVEC_HV, NVEC_STEP, REFINE = 2, 5, 2


def launch(eng, mc, option, sizes, nmax=None, n_list=None, nan_at=None, singular=False):
    from global_racetrajectory_optimization_amd import engine
    opts = eng.mintime_opts(**mc.OPTIONS[option])
    probs = [dict(mc.problem(N, option)) for N in sizes]
    if nan_at is not None:
        b, i = nan_at
        probs[b]["w"] = probs[b]["w"].copy()
        probs[b]["w"][i] = np.nan
    rng = np.random.default_rng(90210 + 17 * len(sizes) + sorted(mc.OPTIONS).index(option))
    B, MB = len(probs), engine.MT_BLOCK
    with eng.scope() as dev:
        data, Ns, nmax = eng._mintime_up(dev, probs, opts, nmax, True)
        if n_list is not None:
            data.n_list = dev.up(np.asarray(n_list, dtype=np.int32))
        nw, ng = eng.mintime_sizes(nmax, opts)
        f64 = dict(w0=(B, nw), lbw=(B, nw), ubw=(B, nw), lbg=(B, ng), ubg=(B, ng), g=(B, ng), J=(B,), lap_time=(B,), energy=(B,), x_opt=(B, nmax + 1, 5),
                   u_opt=(B, nmax, 4), tf_opt=(B, nmax, 12), dt_opt=(B, nmax), ax_opt=(B, nmax), ay_opt=(B, nmax), ec_opt=(B, nmax),
                   blocks=(B, nmax, MB, MB), grad_J=(B, nw), grad_energy=(B, nw), r=(B, nw), kkt=(B, 3), hblocks=(B, nmax, MB, MB), y=(B, NVEC_HV, nw),
                   sol=(B, NVEC_STEP, nw + ng), res=(B, NVEC_STEP))
        i32 = dict(status=(B,), inertia=(B, 3), step_status=(B,))
        d = {k: dev.out(s) for k, s in f64.items()}
        d.update({k: dev.out(s, np.int32) for k, s in i32.items()})
        lam_g, lam_x, sigma = rng.uniform(-1.0, 1.0, (B, ng)), rng.uniform(-1.0, 1.0, (B, nw)), rng.uniform(0.5, 1.5, B)
        v, rhs = rng.uniform(-1.0, 1.0, (B, NVEC_HV, nw)), rng.uniform(-1.0, 1.0, (B, NVEC_STEP, nw + ng))
        d_lam = dev.up(lam_g)
        eng.mintime_bounds_device(data, opts, d["w0"], d["lbw"], d["ubw"], d["lbg"], d["ubg"])
        eng.mintime_eval_device(data, opts, d["g"], d["J"], d["status"], d["lap_time"], d["energy"], d["x_opt"], d["u_opt"], d["tf_opt"], d["dt_opt"],
                                d["ax_opt"], d["ay_opt"], d["ec_opt"])
        eng.mintime_jac_device(data, opts, d["blocks"], d["grad_J"], d["grad_energy"])
        eng.mintime_kkt_device(data, opts, d["g"], d["blocks"], d["grad_J"], d["grad_energy"], d_lam, dev.up(lam_x), d["lbw"], d["ubw"], d["lbg"], d["ubg"],
                               d["r"], d["kkt"])
        eng.mintime_hess_device(data, opts, d_lam, dev.up(sigma), d["hblocks"])
        eng.mintime_hessvec_device(data, opts, d["hblocks"], dev.up(v), NVEC_HV, d["y"])
        rows = np.abs(dev.get(d["hblocks"])).sum(axis=3).reshape(B, -1)
        top = np.array([np.max(q[np.isfinite(q)]) if np.any(np.isfinite(q)) else 1.0 for q in rows])
        dw = np.repeat(2.0 * top[:, None] + 1e-3, nw, axis=1)
        dg = np.where(dev.get(d["lbg"]) == dev.get(d["ubg"]), 1e-6, 1.0)
        if singular:        # (a zero pivot at the first variable that is one: H = 0 and dw = 0)
            dw[:] = 0.0
        eng.mintime_step_device(data, opts, dev.out((B, nmax, MB, MB)) if singular else d["hblocks"], d["blocks"], d["grad_energy"], dev.up(dw),
                                dev.up(dg), dev.up(rhs), NVEC_STEP, REFINE, d["sol"], d["res"], d["inertia"], d["step_status"])
        return {k: dev.get(p) for k, p in d.items()}


def dump(lib, path):
    import mintime_cases as mc
    from global_racetrajectory_optimization_amd import engine
    eng = engine.Engine(0, lib_path=lib)
    out = {}
    runs = [(o, dict(option=o, sizes=SIZES)) for o in ("plain", "safe", "energy", "linear", "gauss5", "all")]
    runs += [("ragged", dict(option="all", sizes=(8, 3, 65, 2, 7), nmax=70)),
             ("n_list", dict(option="safe", sizes=(7, 3, 8, 2, 3), nmax=9, n_list=(7, 0, 10, 2, 1))),
             ("nan", dict(option="all", sizes=(3, 8, 7), nan_at=(1, 24 * 5 + 11))),
             ("singular", dict(option="energy", sizes=(3, 7), nmax=8, singular=True))]
    for name, kw in runs:
        res = launch(eng, mc, **kw)
        out.update({"%s/%s" % (name, k): a for k, a in res.items()})
        print("%-8s eval status %s step status %s" % (name, res["status"].tolist(), res["step_status"].tolist()))
    eng.close()
    np.savez(path, **out)
    print("%d arrays written to %s" % (len(out), path))


def words(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32).reshape(-1)


def compare(pa, pb):
    za, zb = np.load(pa), np.load(pb)
    total, differing = 0, 0
    if sorted(za.files) != sorted(zb.files):
        print("the two files hold different arrays")
        return 1
    for k in sorted(za.files):
        a, b = za[k], zb[k]
        if a.shape != b.shape or a.dtype != b.dtype:
            print("%-24s shape or type differs: %s %s / %s %s" % (k, a.shape, a.dtype, b.shape, b.dtype))
            differing += 1
            continue
        n = int(np.count_nonzero(words(a) != words(b)))
        total += a.size
        differing += n
        if n:
            print("%-24s %d of %d words differ" % (k, n, a.size))
    print("%d arrays, %d words, %d differing" % (len(za.files), total, differing))
    return 1 if differing else 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--dump":
        dump(sys.argv[2], sys.argv[3])
    elif len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
