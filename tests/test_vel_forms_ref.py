"""tests/vel_forms_cases.py and tests/vel_forms_guard.py on their own (no engine, no GPU): the case tables cover what they say, the cases that
are compared with oracle/vel_ref.py meet the caps of tests/test_glue_ref.py::test_velocity_guards_are_capped by the reference alone, and the stored
spreads are what tests/vel_forms_guard.py computes."""
import numpy as np
import pytest

import glue_cases as gc
import vel_forms_cases as fc
import vel_forms_guard as fg
from oracle import vel_ref


def test_case_tables_cover_what_they_say():
    for kind in fc.KINDS:
        Fs = fc.launches(kind)
        assert all(F["closed"] == (kind == "locgg") and (F["loc_gg"] is not None) == (kind != "open") for F in Fs)
        assert all(F["loc_gg"] is None or (F["mu"] is None and F["loc_gg"].shape == F["kappa"].shape + (2,)) for F in Fs)
        if kind != "open_locgg_flat":           # (the flat kind takes the launches of exponent 1.5 / 2.0 only: lengths and batches as they come)
            assert {F["kappa"].shape[1] for F in Fs if F["n_of_track"] is None} >= set(gc.VEL_N)
            assert {F["axm"].shape[0] for F in Fs} >= {1, 63, 64, 65, 129}
        assert any(F["n_of_track"] is not None and len(set(F["track_of"])) < F["track_of"].size for F in Fs)          # ragged rows, many-to-one
        if kind == "locgg":
            continue
        assert {F["filt_window"] for F in Fs} >= ({None, 1, 7} if kind == "open_locgg_flat" else {None, 1, 3, 7}) and any(F["filt_window"] == F["kappa"].shape[1] for F in Fs)
        ends = [F["v_end"] for F in Fs]
        assert any(e is None for e in ends)                                                                          # v_end NULL
        assert any(e is not None and np.any(np.isnan(e)) and not np.all(np.isnan(e)) for e in ends)                  # NaN for some variants only
        assert any(e is not None and np.any(e == 0.0) for e in ends) and any(e is not None and np.any(e > 2.0 * 27.0) for e in ends)
        assert all(np.any(F["v_start"] == 0.0) for F in Fs) and all(np.all(F["v_start"] >= 0.0) for F in Fs)
    assert {F["exp"] for F in fc.launches("open")} == {1.0, 1.5, 2.0} and any(F["mu"] is not None for F in fc.launches("open"))
    assert {F["exp"] for F in fc.launches("open_locgg_flat")} == {1.5, 2.0} and all(F["parity"] for F in fc.launches("open_locgg_flat"))
    for kind in ("locgg", "open_locgg"):
        assert all(F["parity"] == (F["exp"] == 1.0) for F in fc.launches(kind))
        assert sum(F["parity"] for F in fc.launches(kind)) >= 4 and sum(not F["parity"] for F in fc.launches(kind)) >= 10
    # what the issue counted at 24 variants per launch at the most; here every variant of every launch is compared
    assert fc.parity_case_count("open") >= 321 and fc.parity_case_count("locgg") + fc.parity_case_count("open_locgg") >= 87
    assert fc.parity_case_count("open_locgg_flat") >= 234


def test_start_speeds_lie_on_both_sides_of_the_lateral_limit():
    """v_start above and below what point 0 reaches without one, and the limit itself in between, by the oracle."""
    for kind in ("open", "open_locgg"):
        below = above = 0
        for name in ("n17", "n130", "ragged_fw3"):
            F = [x for x in fc.launches(kind) if x["name"] == name][0]
            for v in range(0, F["axm"].shape[0], 3):
                free = fg.ref_case(dict(F, v_start=np.full(F["axm"].shape[0], 1e9), v_end=None), v)[0][0]
                below += F["v_start"][v] < free
                above += F["v_start"][v] > free
        assert below >= 10 and above >= 5, (kind, below, above)


def test_flat_rows_keep_the_sweeps_away_from_every_apex():
    """max |kappa| = 0.001 1/m: the local lateral limit lies above every v_max, yet most profiles stay below v_max somewhere (v_start, v_end)."""
    below = total = 0
    for F in fc.launches("open_locgg_flat"):
        for v in range(F["axm"].shape[0]):
            t, n = fc.row(F, v)
            assert np.max(np.abs(F["kappa"][t, :n])) <= fc.FLAT_KAPPA * (1 + 1e-15)
            assert np.min(F["loc_gg"][t, :n, 1]) / fc.FLAT_KAPPA > F["vmax"][v] ** 2
            if v % 4 == 0:
                total += 1
                below += bool(np.any(fg.ref_case(F, v)[0] < F["vmax"][v]))
    assert below >= 0.8 * total


def test_unclosed_oracle_is_what_the_kernel_documents():
    """The pieces of the specification the kernel's comments cite, on the oracle: negative speeds count as 0, the ends of an unclosed filtered
    profile keep their values, two standing points take +inf."""
    F = [x for x in fc.launches("open") if x["name"] == "n17"][0]
    a = fg.ref_case(dict(F, v_start=np.full(12, -3.0), v_end=np.full(12, -1.0)), 5)
    b = fg.ref_case(dict(F, v_start=np.zeros(12), v_end=np.zeros(12)), 5)
    assert np.array_equal(a[0], b[0]) and a[1] == b[1]
    plain = fg.ref_case(F, 5)[0]
    filt = fg.ref_case(dict(F, filt_window=7), 5)[0]
    assert np.array_equal(filt[:3], plain[:3]) and np.array_equal(filt[-3:], plain[-3:]) and not np.array_equal(filt[3:-3], plain[3:-3])
    F2 = [x for x in fc.launches("open") if x["name"] == "n2"][0]
    r = fg.ref_case(dict(F2, v_start=np.zeros(1), v_end=np.zeros(1)), 0)
    assert np.array_equal(r[0], [0.0, 0.0]) and np.isposinf(r[1])
    vx = np.array([3.0, 4.0, 6.0])
    assert fg.lap_time_open(vx, np.array([7.0, 5.0])) == 2.0 + 1.0
    assert abs(fg.lap_time_open(vx, np.array([7.0, 5.0])) - vel_ref.calc_t_profile(vx, np.array([7.0, 5.0]))[-1]) < 1e-12


# ---- the guards --------------------------------------------------------------------------------------------------------------------------------
def test_stored_spreads_are_complete_and_reproducible():
    ent = fg.entries()
    z = np.load(fg.PATH)
    assert sorted(z.files) == sorted(ent)
    for k in z.files:                                       # arrays of spreads only
        assert z[k].dtype == np.float64 and z[k].ndim == 2 and z[k].shape[1] == 2 and np.all(z[k] >= 0.0) and np.all(np.isfinite(z[k])), k
    for key in ("open/n63", "open/ragged_fw3", "open/gates_mu", "locgg/n130", "open_locgg/n2", "open_locgg/gates", "open_locgg_flat/n257",
                "open_locgg_flat/fw==n17"):
        F = [x for _, x in fc.all_launches() if fg.key(x) == key][0]
        only = list(range(0, F["axm"].shape[0], 9))
        if key == "open/n63":
            only.append(51)                                 # the one case of the table above the floor
        new, old = fg.compute_spread(F, only=only)[only], fg.spread(key)[only]
        assert new.shape == old.shape
        assert np.allclose(np.maximum(4 * new, 1e-13), np.maximum(4 * old, 1e-13), rtol=1e-3, atol=0.0), key


@pytest.mark.parametrize("kind", fc.KINDS + (None,))
def test_guards_are_capped(kind):
    """The caps of tests/test_glue_ref.py::test_velocity_guards_are_capped, per kind and over all: at most 2 % of the cases carry a guard above
    the floor, none above 1e-7 (a sweep's flipped `<` moves a profile by far more: such a case is regenerated from another seed,
    vel_forms_cases.SEEDS, not kept under a wide guard)."""
    S = np.vstack([fg.spread(fg.key(F)) for k, F in fc.all_launches() if F["parity"] and kind in (None, k)])
    assert S.shape == (fc.parity_case_count(kind), 2)
    for qi, q in enumerate(fg.VEL_Q):
        g = np.maximum(fg.FLOOR[q], 4.0 * S[:, qi])
        assert np.mean(g > fg.FLOOR[q]) <= 0.02 and np.max(g) <= 1e-7, (kind, q, float(np.mean(g > fg.FLOOR[q])), float(np.max(g)))
