"""BASELINE config 1: the reference's main_globaltraj.py runs UNTOUCHED on top of the drop-in package (harness notes:
SURVEY.md App. C).  Its runs are recorded with the reference checkout (scripts/record_harness_runs.py, scripts/record_harness_calls.py)
and replayed here from tests/golden without it.  The engine behind opt_min_curv here is the SIMT-interpreted kernel library (test
infrastructure); the `-m gpu` suite covers the real one."""
import io
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNS = os.path.join(ROOT, "tests", "golden", "harness_runs.npz")


def _replay_run(case, capsys, tol=1e-9):
    """One recorded run of the untouched main_globaltraj.py on the drop-in package (scripts/record_harness_runs.py ->
    tests/golden/harness_runs.npz), replayed without the reference tree: prep_track's calls on the raw imported track [REF
    helper_funcs_glob/src/prep_track.py:39-59], the call the script made at the drop-in boundary on what they return, through the drop-in
    package on whatever library engine.default_engine() loads, then the script's raceline / velocity-profile chain [REF
    main_globaltraj.py:371-422, 498-511] through the drop-in's tph on the recorded vehicle parameters.  tol: how far the prepared track and
    the (re-linearised) line the chain starts from may lie from the recorded ones.  Returns what the replay computed and what the script
    printed and exported."""
    import json
    from global_racetrajectory_optimization_amd import trajectory_planning_helpers as tph
    z = np.load(RUNS)
    f = lambda k: z[case + "_" + k]
    entry = str(f("entry"))
    # ---- prep_track: smoothing / re-sampling of the imported track, its splines' normals, the crossing check ----
    interp = tph.spline_approximation.spline_approximation(track=f("prep_track").copy(), **json.loads(str(f("prep_spline_kwargs"))))
    assert interp.shape == f("prep_reftrack_interp").shape and np.max(np.abs(interp - f("prep_reftrack_interp"))) < tol
    normvec0 = tph.calc_splines.calc_splines(path=np.vstack((interp[:, :2], interp[0, :2])))[3]
    assert np.max(np.abs(normvec0 - f("prep_normvec"))) < tol
    crossing = tph.check_normals_crossing.check_normals_crossing(track=interp, normvec_normalized=normvec0, horizon=int(f("prep_horizon")))
    assert bool(crossing) == bool(f("prep_crossing"))
    # the script hands exactly those to the boundary (checked when recording)
    kw = dict(reftrack=interp.copy(), normvectors=normvec0.copy(), **json.loads(str(f("kwargs"))))
    if case + "_A_scalings" in z.files:
        ref = kw["reftrack"]
        kw["A"] = tph.calc_splines.calc_splines(path=np.vstack((ref[:, :2], ref[0, :2])))[2]       # what prep_track hands the script
        assert np.max(np.abs(tph.calc_splines.scalings_from_les_matrix(kw["A"]) - f("A_scalings"))) < 1e-13
    mod, fn = entry.split(".")
    capsys.readouterr()
    res = getattr(getattr(tph, mod), fn)(**kw)
    printed = capsys.readouterr().out
    if entry == "iqp_handler.iqp_handler":
        alpha, reftrack, normvec = res          # main rebinds both [REF main_globaltraj.py:274]
    else:
        alpha = res[0] if entry == "opt_min_curv.opt_min_curv" else res
        reftrack, normvec = kw["reftrack"], kw["normvectors"]
    assert np.max(np.abs(reftrack - f("reftrack_interp"))) < tol and np.max(np.abs(normvec - f("normvec"))) < tol
    p = json.loads(str(f("pars")))
    race, _, cx, cy, inds, tv, s_pts, spl_len, el = tph.create_raceline.create_raceline(
        refline=reftrack[:, :2], normvectors=normvec, alpha=alpha, stepsize_interp=p["stepsize_interp_after_opt"])
    psi, kappa = tph.calc_head_curv_an.calc_head_curv_an(coeffs_x=cx, coeffs_y=cy, ind_spls=inds, t_spls=tv)
    vx = tph.calc_vel_profile.calc_vel_profile(ggv=f("ggv"), ax_max_machines=f("ax_max_machines"), v_max=p["v_max"], kappa=kappa, el_lengths=el,
                                               closed=True, filt_window=p["filt_window"], dyn_model_exp=p["dyn_model_exp"],
                                               drag_coeff=p["dragcoeff"], m_veh=p["mass"])
    ax = tph.calc_ax_profile.calc_ax_profile(vx_profile=np.append(vx, vx[0]), el_lengths=el, eq_length_output=False)
    t = tph.calc_t_profile.calc_t_profile(vx_profile=vx, ax_profile=ax, el_lengths=el)
    traj = np.column_stack((s_pts, race, psi, kappa, vx, ax))
    traj = np.vstack((traj, traj[0]))
    traj[-1, 0] = np.sum(spl_len)
    return dict(alpha=alpha, printed=printed, lap_time=float(t[-1]), traj_race_cl=traj, script_alpha=f("alpha_opt"),
                script_traj_race_cl=f("traj_race_cl"), script_stdout=json.loads(str(f("stdout"))), csv=str(f("csv")),
                ggv=f("ggv"), ax_max_machines=f("ax_max_machines"), pars=p, reftrack_interp=interp)


def _check_exported_run(r, tol=1e-8):
    """What the script printed and exported, against the replay: the lap-time line digit for digit, the race trajectory it held (within
    tol), and outputs/traj_race_cl.csv as written (header, 7 columns, closed: the last row repeats the first point; values to the file's 7
    decimals)."""
    assert "INFO: Estimated laptime: %.2fs" % r["lap_time"] in r["script_stdout"], (r["lap_time"], r["script_stdout"])
    assert r["traj_race_cl"].shape == r["script_traj_race_cl"].shape
    assert np.max(np.abs(r["traj_race_cl"] - r["script_traj_race_cl"])) < tol
    lines = r["csv"].splitlines()
    assert lines[2].replace(" ", "") == "#s_m;x_m;y_m;psi_rad;kappa_radpm;vx_mps;ax_mps2"
    data = np.loadtxt(io.StringIO(r["csv"]), comments="#", delimiter=";")
    assert data.shape[1] == 7 and data.shape[0] > 100
    assert np.allclose(data[0, 1:3], data[-1, 1:3])          # closed: last row repeats the first point
    assert data.shape == r["traj_race_cl"].shape and np.max(np.abs(data - r["traj_race_cl"])) < 1e-6


@pytest.mark.parametrize("opt_type", ["mincurv", "mincurv_iqp", "shortest_path"])
def test_main_globaltraj_untouched(emu_lib, monkeypatch, capsys, opt_type):
    """BASELINE config 1 on rounded_rectangle, one run per opt_type of the untouched script, replayed from its recording (_replay_run)."""
    from global_racetrajectory_optimization_amd import engine
    monkeypatch.setenv("MCQ_LIB", emu_lib)
    monkeypatch.setattr(engine, "_DEFAULT_ENGINE", None)
    r = _replay_run("rr_" + opt_type, capsys)
    monkeypatch.setattr(engine, "_DEFAULT_ENGINE", None)
    marker = {"mincurv": "Solver runtime opt_min_curv", "mincurv_iqp": "Minimum curvature IQP: iteration 3",
              "shortest_path": "Solver runtime opt_shortest_path"}[opt_type]
    assert marker in r["printed"] and any(l.startswith(marker) for l in r["script_stdout"])
    assert np.max(np.abs(r["alpha"] - r["script_alpha"])) < 1e-9
    _check_exported_run(r)
    # the alpha the script got from the drop-in equals the golden single-shot solution
    if opt_type == "mincurv":
        g = np.load(os.path.join(os.path.dirname(__file__), "golden", "rounded_rectangle.npz"))
        assert np.max(np.abs(r["alpha"] - g["alpha"])) < 1e-8
    elif opt_type == "mincurv_iqp":
        g = np.load(os.path.join(os.path.dirname(__file__), "golden", "rounded_rectangle.npz"))
        assert np.max(np.abs(r["alpha"] - g["iqp_alpha"])) < 1e-7
    else:
        z = np.load(os.path.join(os.path.dirname(__file__), "golden", "shortest_path.npz"))
        assert np.max(np.abs(r["alpha"] - z["rounded_rectangle_alpha"])) < 1e-8


def test_main_globaltraj_untouched_on_the_goldfarb_idnani_path(emu_lib, monkeypatch, capsys):
    """$MCQ_ALGORITHM=gi: the untouched script's mincurv_iqp run (recorded with EVERY QP of its flow solved by the engine's Goldfarb-Idnani
    path -- the algorithm of the quadprog it replaces), replayed on that path, ends in the golden IQP state of the default path."""
    from global_racetrajectory_optimization_amd import engine
    monkeypatch.setenv("MCQ_LIB", emu_lib)
    monkeypatch.setenv("MCQ_ALGORITHM", "gi")
    monkeypatch.setattr(engine, "_DEFAULT_ENGINE", None)
    r = _replay_run("rr_mincurv_iqp_gi", capsys)
    monkeypatch.setattr(engine, "_DEFAULT_ENGINE", None)
    assert "Minimum curvature IQP: iteration 3" in r["printed"] and "Minimum curvature IQP: iteration 3" in r["script_stdout"][2]
    assert np.max(np.abs(r["alpha"] - r["script_alpha"])) < 1e-9
    _check_exported_run(r)
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "rounded_rectangle.npz"))
    assert np.max(np.abs(r["alpha"] - g["iqp_alpha"])) < 1e-7


def test_main_globaltraj_untouched_berlin_config1(emu_lib, monkeypatch, capsys):
    """BASELINE config 1 as specified: berlin_2018 (N = 776 at the ini defaults), opt_type = 'mincurv', the untouched script's run end to
    end -- import_track, prep_track, opt_min_curv behind the boundary, create_raceline, velocity profile, lap time, export -- replayed from
    its recording (_replay_run)."""
    from global_racetrajectory_optimization_amd import engine
    monkeypatch.setenv("MCQ_LIB", emu_lib)
    monkeypatch.setattr(engine, "_DEFAULT_ENGINE", None)
    r = _replay_run("berlin_mincurv", capsys)
    monkeypatch.setattr(engine, "_DEFAULT_ENGINE", None)
    assert "Solver runtime opt_min_curv" in r["printed"] and any(l.startswith("INFO: Estimated laptime:") for l in r["script_stdout"])
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "berlin_2018.npz"))
    assert r["reftrack_interp"].shape == (776, 4)
    assert np.max(np.abs(r["reftrack_interp"] - g["reftrack"])) < 1e-9      # the drop-in's prep of the raw track = the golden inputs
    assert np.max(np.abs(r["alpha"] - g["alpha"])) < 1e-6 and np.max(np.abs(r["script_alpha"] - g["alpha"])) < 1e-6
    _check_exported_run(r)
    lap = float([l for l in r["script_stdout"] if "Estimated laptime" in l][0].split(":")[-1].strip().rstrip("s"))
    # the lap time of the golden raceline through the ORACLE's velocity-profile chain (oracle/vel_ref.py)
    from oracle import tph_ref, vel_ref
    from global_racetrajectory_optimization_amd.trajectory_planning_helpers import calc_head_curv_an as ch
    out = tph_ref.create_raceline(g["reftrack"][:, :2], g["normvec"], g["alpha"], 2.0)
    _, kappa = ch.calc_head_curv_an(coeffs_x=out[2], coeffs_y=out[3], ind_spls=out[4], t_spls=out[5])
    p = r["pars"]
    vx = vel_ref.calc_vel_profile(ax_max_machines=r["ax_max_machines"], kappa=kappa, el_lengths=out[8], closed=True,
                                  drag_coeff=p["dragcoeff"], m_veh=p["mass"], ggv=r["ggv"], v_max=p["v_max"], dyn_model_exp=p["dyn_model_exp"])
    assert abs(lap - vel_ref.lap_time_stable(vx, out[8])) < 0.02          # the script prints two decimals


def _replay_recorded_calls(capsys, on_build_box, with_kappa_error=True):
    """The calls the untouched main_globaltraj.py made at the drop-in boundary on berlin_2018 (captured once by
    scripts/record_harness_calls.py -> tests/golden/harness_calls_berlin.npz: keyword arguments as the script passed them
    [REF main_globaltraj.py:264-271, 273-284, 286-290; 337-350 constructed], the ORACLE's outputs for them, the print_debug lines), replayed
    through the drop-in package on whatever library engine.default_engine() loads.  alpha within 1e-6 m of the oracle's (north_star's fp64
    tolerance), upstream's debug lines, upstream's exception types and messages."""
    import hashlib
    import json
    import re
    from global_racetrajectory_optimization_amd import trajectory_planning_helpers as tph
    z = np.load(os.path.join(ROOT, "tests", "golden", "harness_calls_berlin.npz"))

    def matrix(key):
        ref = z[key + "_reftrack"]
        A = tph.calc_splines.calc_splines(path=np.vstack((ref[:, :2], ref[0, :2])))[2]       # what prep_track hands the script [REF prep_track.py:48-51]
        assert np.max(np.abs(tph.calc_splines.scalings_from_les_matrix(A) - z[key + "_A_scalings"])) < 1e-13
        if on_build_box:
            assert hashlib.sha256(np.ascontiguousarray(A).tobytes()).hexdigest() == str(z[key + "_A_sha256"])
        return A

    def guarded(d, what):
        """On the GPU (not on the interpreter, which keeps its own bounds): the tight guard of tests/ring_guard.py on top of the contract."""
        if not on_build_box:
            import ring_guard
            g = ring_guard.guard("harness_calls_berlin", what=what)
            assert d < g, (what, d, g)                                                                  # guard
        return d

    capsys.readouterr()
    # ---- opt_type = 'mincurv' [REF main_globaltraj.py:264-271] ----
    kw = json.loads(str(z["mincurv_kwargs"]))
    assert str(z["mincurv_entry"]) == "opt_min_curv.opt_min_curv" and kw["print_debug"] is True
    alpha = tph.opt_min_curv.opt_min_curv(reftrack=z["mincurv_reftrack"].copy(), normvectors=z["mincurv_normvectors"].copy(), A=matrix("mincurv"), **kw)[0]
    d_mc = float(np.max(np.abs(alpha - z["mincurv_oracle_alpha"])))
    assert alpha.shape == (776,) and d_mc <= 1e-6                                                       # contract
    guarded(d_mc, "mincurv_oracle_alpha")
    out = capsys.readouterr().out
    assert re.search(r"^Solver runtime opt_min_curv: \d+\.\d{3}s$", out, re.M), out
    # the second element of the tuple the script drops with [0]
    curv = tph.opt_min_curv.opt_min_curv(reftrack=z["mincurv_reftrack"].copy(), normvectors=z["mincurv_normvectors"].copy(), A=matrix("mincurv"),
                                         kappa_bound=kw["kappa_bound"], w_veh=kw["w_veh"])[1]
    assert abs(curv - float(z["mincurv_oracle_curv_error_max"])) < 1e-9
    # ---- opt_type = 'mincurv_iqp' [REF main_globaltraj.py:273-284] ----
    kw = json.loads(str(z["iqp_kwargs"]))
    capsys.readouterr()
    a_iqp, rt, nv = tph.iqp_handler.iqp_handler(reftrack=z["iqp_reftrack"].copy(), normvectors=z["iqp_normvectors"].copy(), A=matrix("iqp"), **kw)
    assert a_iqp.shape == z["iqp_oracle_alpha"].shape and rt.shape == z["iqp_oracle_reftrack"].shape and nv.shape == z["iqp_oracle_normvectors"].shape
    d_iqp = float(np.max(np.abs(a_iqp - z["iqp_oracle_alpha"])))
    assert d_iqp <= 1e-6 and np.max(np.abs(rt - z["iqp_oracle_reftrack"])) <= 1e-6 and np.max(np.abs(nv - z["iqp_oracle_normvectors"])) <= 1e-6   # contract
    guarded(d_iqp, "iqp_oracle_alpha")
    guarded(float(np.max(np.abs(rt - z["iqp_oracle_reftrack"]))), "iqp_oracle_reftrack")
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith(("Minimum curvature IQP", "Finished IQP"))]
    assert lines == json.loads(str(z["iqp_stdout"])) and len(lines) == 4              # the three iterations' lines and the closing one, digit for digit
    assert lines[:3] == ["Minimum curvature IQP: iteration %i, curv_error_max: %.4frad/m" % (k + 1, c) for k, c in enumerate(z["iqp_oracle_curv_error_trace"])]
    # ---- opt_type = 'shortest_path' [REF main_globaltraj.py:286-290] ----
    kw = json.loads(str(z["shortest_kwargs"]))
    a_sp = tph.opt_shortest_path.opt_shortest_path(reftrack=z["shortest_reftrack"].copy(), normvectors=z["shortest_normvectors"].copy(), **kw)
    d_sp = float(np.max(np.abs(a_sp - z["shortest_oracle_alpha"])))
    assert d_sp <= 1e-6                                                                                 # contract
    guarded(d_sp, "shortest_oracle_alpha")
    assert re.search(r"^Solver runtime opt_shortest_path: \d+\.\d{3}s$", capsys.readouterr().out, re.M)
    # ---- the re-optimisation call of the mintime branch [REF main_globaltraj.py:337-350] ----
    kw = json.loads(str(z["reopt_kwargs"]))
    a_ro = tph.opt_min_curv.opt_min_curv(reftrack=z["reopt_reftrack"].copy(), normvectors=z["reopt_normvectors"].copy(), A=matrix("reopt"), **kw)[0]
    d_ro = float(np.max(np.abs(a_ro - z["reopt_oracle_alpha"])))
    assert d_ro <= 1e-6 and np.max(np.abs(a_ro)) <= 0.2 + 1e-9                      # contract; corridor 1.0 either side, vehicle 1.6
    guarded(d_ro, "reopt_oracle_alpha")
    # ---- what upstream's callers would see when the QP has no solution ----
    kw = json.loads(str(z["mincurv_kwargs"]))
    narrow = z["mincurv_reftrack"].copy()
    narrow[z["error_narrow_rows"], 2:] = float(z["error_narrow_width"])
    with pytest.raises(RuntimeError) as e1:
        tph.opt_min_curv.opt_min_curv(reftrack=narrow, normvectors=z["mincurv_normvectors"].copy(), A=matrix("mincurv"), **kw)
    assert str(e1.value) == str(z["error_narrow_message"])
    if with_kappa_error:        # (79 s on the SIMT interpreter: the Goldfarb-Idnani path's several hundred steps at N = 776; milliseconds on the GPU)
        with pytest.raises(ValueError) as e2:
            tph.opt_min_curv.opt_min_curv(reftrack=z["mincurv_reftrack"].copy(), normvectors=z["mincurv_normvectors"].copy(), A=matrix("mincurv"),
                                          kappa_bound=float(z["error_kappa_bound"]), w_veh=kw["w_veh"])
        assert str(e2.value) == str(z["error_kappa_message"]) == "constraints are inconsistent, no solution"
    with pytest.raises(RuntimeError, match="Array size of reftrack should be the same as normvectors"):
        tph.opt_min_curv.opt_min_curv(reftrack=z["mincurv_reftrack"].copy(), normvectors=z["mincurv_normvectors"][:-1].copy(), A=matrix("mincurv"), **kw)
    return dict(mincurv=d_mc, iqp=d_iqp, shortest_path=d_sp, reopt=d_ro)


def test_replay_of_the_recorded_calls_on_the_interpreter(emu_lib, monkeypatch, capsys):
    from global_racetrajectory_optimization_amd import engine
    monkeypatch.setenv("MCQ_LIB", emu_lib)
    monkeypatch.setattr(engine, "_DEFAULT_ENGINE", None)
    # (the curvature-bound error case is left to the GPU replay; the mapping itself is covered here by
    #  tests/test_emu_gi.py::test_inconsistent_curvature_rows_are_recognised_by_both_paths and tests/test_host.py)
    d = _replay_recorded_calls(capsys, on_build_box=True, with_kappa_error=False)
    monkeypatch.setattr(engine, "_DEFAULT_ENGINE", None)
    assert max(d.values()) < 1e-7, d


@pytest.mark.gpu
def test_replay_of_the_recorded_calls_on_the_gpu(monkeypatch, capsys):
    """BASELINE config 1 / 2 on the REAL library without the reference tree (the driver's GPU box has none, and the two
    tests below are skipped there): every call main_globaltraj.py makes at the boundary, as recorded, through the drop-in package -> ctypes
    -> C ABI -> libmcq.so on the MI355X."""
    from global_racetrajectory_optimization_amd import engine
    monkeypatch.delenv("MCQ_LIB", raising=False)
    monkeypatch.setattr(engine, "_DEFAULT_ENGINE", None)
    d = _replay_recorded_calls(capsys, on_build_box=False)
    monkeypatch.setattr(engine, "_DEFAULT_ENGINE", None)
    with capsys.disabled():
        import ring_guard
        guards = {k: ring_guard.guard("harness_calls_berlin", what=("shortest" if k == "shortest_path" else k) + "_oracle_alpha") for k in d}
        print("replay of main_globaltraj.py's recorded calls on libmcq.so: max |alpha - oracle| [m] (guard) = %s" % {
            k: "%.1e (%.1e)" % (v, guards[k]) for k, v in d.items()})


@pytest.mark.gpu
@pytest.mark.parametrize("opt_type", ["mincurv", "mincurv_iqp"])
def test_main_globaltraj_untouched_on_the_gpu(monkeypatch, capsys, opt_type):
    """Config 1 on the REAL library: the untouched main_globaltraj.py's runs on Berlin (ini defaults), replayed from their recording
    (_replay_run) through the drop-in package -> ctypes -> C ABI -> libmcq.so on the MI355X.  The recording was made on the SIMT
    interpreter: alpha, the prepared and re-linearised lines and the race trajectory agree with it within north_star's fp64 tolerance
    (1e-6 m), the lap-time line digit for digit."""
    from global_racetrajectory_optimization_amd import engine
    monkeypatch.delenv("MCQ_LIB", raising=False)
    monkeypatch.setattr(engine, "_DEFAULT_ENGINE", None)
    r = _replay_run("berlin_" + opt_type, capsys, tol=1e-6)
    monkeypatch.setattr(engine, "_DEFAULT_ENGINE", None)
    assert any(l.startswith("INFO: Estimated laptime:") for l in r["script_stdout"])
    assert np.max(np.abs(r["alpha"] - r["script_alpha"])) < 1e-6
    if opt_type == "mincurv":
        assert "Solver runtime opt_min_curv" in r["printed"]
        g = np.load(os.path.join(os.path.dirname(__file__), "golden", "berlin_2018.npz"))
        assert np.max(np.abs(r["alpha"] - g["alpha"])) < 1e-6
    else:
        assert "Minimum curvature IQP: iteration 3" in r["printed"] and "Finished IQP!" in r["printed"]
        g = np.load(os.path.join(os.path.dirname(__file__), "golden", "berlin_2018_iqp.npz"))
        assert r["alpha"].shape == g["iqp_alpha"].shape and np.max(np.abs(r["alpha"] - g["iqp_alpha"])) < 1e-6
    _check_exported_run(r, tol=1e-6)
    assert r["traj_race_cl"].shape[0] > 1000
