"""The case tables of tests/test_emu_vel_forms.py (SIMT interpreter) and tests/test_gpu_vel_forms.py (MI355X): the forms of tph.calc_vel_profile
that mcq_vel_profile_device_forms adds -- unclosed rows (v_start, optional v_end) and local limits loc_gg [no_points, 2] -- on the launch tables
of tests/glue_cases.py.  Nothing new is drawn for curvatures, element lengths, vehicles or batch shapes: a launch of glue_cases.vel_launches()
is REINTERPRETED (a row of n curvatures keeps its first n - 1 element lengths) and / or given a smooth per-waypoint loc_gg around
(10, 10) m/s^2 +- 30 %.  v_start cycles through 0 / 3 / 0.5 v_max / 2 v_max (the last above every lateral limit), v_end through none / 0 /
0.4 v_max / 2 v_max with the variant index; "none" is a NaN entry of v_end, or v_end = None where no variant of the launch has one.

KINDS, and what each is compared on:

  open             unclosed + ggv, every launch (exponents 1.0 / 1.5 / 2.0, mu, filter windows up to fw == n, the "gates" tables): PARITY with
                   oracle/vel_ref.py under the full guard of tests/vel_forms_guard.py.
  locgg            closed + loc_gg,   } dyn_model_exp == 1.0: PARITY.
  open_locgg       unclosed + loc_gg, } exponent 1.5 / 2.0: EXCLUDED from the parity comparison, on purpose.  A local lateral limit does not
                   depend on the speed, so a sweep that starts at an apex evaluates 1 - (ay_used / ay_max)^e exactly AT the limit: the radicand is
                   +-1e-16 by construction and its 1/e-th power 1e-8 -- the reference itself moves by up to 5.5e-7 m/s under a relative 1e-15 on
                   its inputs (19 of 152 cases at 1.5 and 60 of 84 at 2.0 above the 1e-9 floor), the same reason for which glue_cases.py keeps
                   exponent 2 off one-row diagrams.  The reference has no answer to the floor there, and a guard wide enough to pass would hide
                   the kernel.  On these cases only what IS decided is asserted (INVARIANTS): the same bits in the reversed launch, vx <= v_max,
                   vx <= the local lateral limit to one rounding (launches without a filter), a time that is finite wherever the profile moves.
  open_locgg_flat  unclosed + loc_gg with exponent 1.5 / 2.0 and every row rescaled to max |kappa| = 0.001 1/m: the lateral limit lies above
                   every v_max of the tables, so the sweeps start only at v_start and run into v_end, away from any apex: PARITY.  This carries
                   the pow path of the local form under the full guard.  A CLOSED row rescaled this way is v_max everywhere -- decided, but
                   trivial -- so for closed rows with loc_gg the full guard bites at exponent 1.0 only and the exponents above 1 rest on the
                   invariants above.  That is a limit of the reference, not a gap papered over with a wider guard.

Left out of all kinds: "b1000" (a thousand oracle runs per kind; the batch shapes around the 64-thread block are in "n5" .. "n64") and
"nan_rows" (its rows come back in vel_forms_checks.check_nan_rules, with the NaN rules of the new form).  A case whose oracle flips a `<` under
an ulp is regenerated from another seed (SEEDS), never kept under a wide guard."""
import functools

import numpy as np

import glue_cases as gc

KINDS = ("open", "locgg", "open_locgg", "open_locgg_flat")
LEFT_OUT = ("b1000", "nan_rows")
FLAT_KAPPA = 0.001
SEEDS = {}                  # (kind, launch) -> seed of loc_gg's ripple (default 7): changed only to move a case off a flipped `<`, see above


def is_closed(kind):
    return kind == "locgg"


def has_loc_gg(kind):
    return kind != "open"


def loc_gg_row(kind, name, t, n):
    """[n, 2] = (ax_max, ay_max) of track row t: two slow waves around 10 m/s^2 and a 2 % ripple."""
    i = np.arange(n)
    r = np.random.default_rng(1000 * t + SEEDS.get((kind, name), 7))
    return np.column_stack((10.0 + 3.0 * np.sin(0.37 * i + t), 10.0 + 3.0 * np.cos(0.23 * i + 2 * t))) * (1.0 + 0.02 * r.standard_normal((n, 2)))


def speeds(L):
    """(v_start [batch], v_end [batch] with NaN = none, or None where no variant has one)."""
    bsz = L["ggv"].shape[0]
    v = np.arange(bsz)
    vmax = L["vmax"]
    vs = np.choose(v % 4, [np.zeros(bsz), np.full(bsz, 3.0), 0.5 * vmax, 2.0 * vmax])
    ve = np.choose((v // 4) % 4, [np.full(bsz, np.nan), np.zeros(bsz), 0.4 * vmax, 2.0 * vmax])
    return vs, (None if np.all(np.isnan(ve)) else ve)


def _form_launch(kind, L):
    T, nmax = L["kappa"].shape
    nt = np.full(T, nmax) if L["n_of_track"] is None else L["n_of_track"]
    F = dict(L)
    F["kind"], F["closed"] = kind, is_closed(kind)
    F["kappa"] = L["kappa"].copy()
    if kind == "open_locgg_flat":
        for t in range(T):
            top = float(np.max(np.abs(L["kappa"][t, :nt[t]])))
            if top > 0.0:
                F["kappa"][t] *= FLAT_KAPPA / top
    F["loc_gg"] = None
    if has_loc_gg(kind):
        F["mu"] = None
        F["loc_gg"] = np.ones((T, nmax, 2))
        for t in range(T):
            F["loc_gg"][t, :nt[t]] = loc_gg_row(kind, L["name"], t, int(nt[t]))
    F["v_start"], F["v_end"] = (None, None) if F["closed"] else speeds(L)
    F["parity"] = kind in ("open", "open_locgg_flat") or L["exp"] == 1.0
    return F


@functools.lru_cache(maxsize=None)
def launches(kind):
    out = []
    for L in gc.vel_launches():
        if L["name"] in LEFT_OUT or (kind == "open_locgg_flat" and L["exp"] == 1.0):
            continue
        out.append(_form_launch(kind, L))
    return out


def all_launches():
    return [(k, F) for k in KINDS for F in launches(k)]


def launch_ids():
    return ["%s/%s" % (k, F["name"]) for k, F in all_launches()]


def row(F, v):
    """(track row, valid entries) of variant v."""
    t = int(F["track_of"][v])
    return t, (F["kappa"].shape[1] if F["n_of_track"] is None else int(F["n_of_track"][t]))


def parity_case_count(kind=None):
    return sum(F["ggv"].shape[0] for k, F in all_launches() if F["parity"] and (kind is None or k == kind))
