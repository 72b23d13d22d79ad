#!/usr/bin/env python3
"""Records what the reference's OWN export_traj_race and export_traj_ltpl write for two small tracks, once, into
tests/golden/export/reference_files.npz (data only: the calls' input arrays and the bytes of the files they wrote), so that
tests/test_export_ref.py can hold the plain restatement tests/export_ref.py and the package's writers to them without the reference tree.

Run where the reference tree is at hand:   python scripts/make_golden_export.py --reference /path/to/reference

Inputs: rounded_rectangle and handling_track of tests/golden (reftrack, normvec, alpha); raceline by the host shims (tph.create_raceline,
tph.calc_head_curv_an at 2 m), profile by the shims (calc_vel_profile, calc_ax_profile) with the reference's ggv and machine tables.  Per track:
  reftrack, normvec, alpha, spline_lengths, trajectory [m, 7], traj_race_cl [m + 1, 7]       what the two calls are given
  race_file, ltpl_file                                                                       the bytes they wrote (uint8), with the ggv file given
and once: ggv_file, the bytes of the ggv file (its SHA-1 is the files' second line)."""
import argparse
import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TRACKS = ("rounded_rectangle", "handling_track")
PARAMS = dict(v_max=70.0, mass=1200.0, dragcoeff=0.75)      # [REF params/racecar.ini: veh_params]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "export", "reference_files.npz"))
    a = ap.parse_args()
    from global_racetrajectory_optimization_amd import trajectory_planning_helpers as tph
    sys.modules.setdefault("trajectory_planning_helpers", tph)          # the reference package imports it by that name
    try:
        import matplotlib  # noqa: F401
    except ImportError:                                                 # its plot modules are imported, never called
        for name in ("matplotlib", "matplotlib.pyplot", "mpl_toolkits", "mpl_toolkits.mplot3d"):
            sys.modules.setdefault(name, types.ModuleType(name))
        sys.modules["mpl_toolkits.mplot3d"].Axes3D = None
    sys.path.insert(0, a.reference)
    import helper_funcs_glob
    hf = helper_funcs_glob.src
    ggv_path = os.path.join(a.reference, "inputs", "veh_dyn_info", "ggv.csv")
    ggv, axm = tph.import_veh_dyn_info.import_veh_dyn_info(ggv_path, os.path.join(a.reference, "inputs", "veh_dyn_info", "ax_max_machines.csv"))
    P = PARAMS
    out = dict(tracks=np.array(TRACKS), ggv_file=np.fromfile(ggv_path, dtype=np.uint8))
    for name in TRACKS:
        z = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
        ref, nv, al = z["reftrack"], z["normvec"], z["alpha"]
        r = tph.create_raceline.create_raceline(ref[:, :2], nv, al, 2.0)
        psi, kappa = tph.calc_head_curv_an.calc_head_curv_an(r[2], r[3], r[4], r[5])
        el, lengths = r[8], r[7]
        vx = tph.calc_vel_profile.calc_vel_profile(ggv=ggv, ax_max_machines=axm, v_max=P["v_max"], kappa=kappa, el_lengths=el, closed=True,
                                                   filt_window=None, dyn_model_exp=1.0, drag_coeff=P["dragcoeff"], m_veh=P["mass"])
        ax = tph.calc_ax_profile.calc_ax_profile(np.append(vx, vx[0]), el, False)
        traj = np.column_stack((r[6], r[0], psi, kappa, vx, ax))       # (r[6]: s_points_opt_interp)
        race_cl = np.vstack((traj, traj[0, :]))
        race_cl[-1, 0] = np.sum(lengths)
        with tempfile.TemporaryDirectory() as d:
            paths = dict(ggv_file=ggv_path, traj_race_export=os.path.join(d, "race.csv"), traj_ltpl_export=os.path.join(d, "ltpl.csv"))
            hf.export_traj_race.export_traj_race(file_paths=paths, traj_race=race_cl)
            hf.export_traj_ltpl.export_traj_ltpl(file_paths=paths, spline_lengths_opt=lengths, trajectory_opt=traj, reftrack=ref,
                                                 normvec_normalized=nv, alpha_opt=al)
            files = {k: np.fromfile(paths[k], dtype=np.uint8) for k in ("traj_race_export", "traj_ltpl_export")}
        out.update({name + "/reftrack": ref, name + "/normvec": nv, name + "/alpha": al, name + "/spline_lengths": lengths,
                    name + "/trajectory": traj, name + "/traj_race_cl": race_cl, name + "/race_file": files["traj_race_export"],
                    name + "/ltpl_file": files["traj_ltpl_export"]})
        print("%-18s n = %d, m = %d, files of %d and %d bytes" % (name, ref.shape[0], traj.shape[0], files["traj_race_export"].size,
                                                                 files["traj_ltpl_export"].size))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    np.savez_compressed(a.out, **out)
    print("-> %s (%d bytes)" % (a.out, os.path.getsize(a.out)))


if __name__ == "__main__":
    main()
