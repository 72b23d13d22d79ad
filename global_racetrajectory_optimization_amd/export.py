"""The two files the reference's EXPORT block writes [REF helper_funcs_glob/src/export_traj_race.py, export_traj_ltpl.py], from the tables of
Engine.export_batch.

Format of both: line 1 "# " + a random UUID4, line 2 "# " + the SHA-1 hex digest of the ggv file's bytes (of the empty string without one), then
numpy.savetxt's output: a "# " header line naming the columns and one line per row, every column as %.7f, joined by "; "."""
import hashlib
import uuid

import numpy as np

RACE_COLUMNS = ("s_m", "x_m", "y_m", "psi_rad", "kappa_radpm", "vx_mps", "ax_mps2")
LTPL_COLUMNS = ("x_ref_m", "y_ref_m", "width_right_m", "width_left_m", "x_normvec_m", "y_normvec_m", "alpha_m", "s_racetraj_m",
                "psi_racetraj_rad", "kappa_racetraj_radpm", "vx_racetraj_mps", "ax_racetraj_mps2")
SEP = "; "


def ggv_digest(ggv_file=None):
    """SHA-1 hex digest of the ggv file's bytes; of no bytes at all when there is no file."""
    data = b""
    if ggv_file is not None:
        with open(ggv_file, "rb") as fh:
            data = fh.read()
    return hashlib.sha1(data).hexdigest()


def _write(path, rows, columns, ggv_file):
    rows = np.asarray(rows, dtype=np.float64)
    if rows.ndim != 2 or rows.shape[1] != len(columns):
        raise ValueError("expected a table of %d columns, got shape %s" % (len(columns), rows.shape))
    with open(path, "wb") as fh:
        fh.write(("# %s\n# %s\n" % (uuid.uuid4(), ggv_digest(ggv_file))).encode("ascii"))
        np.savetxt(fh, rows, fmt=SEP.join(["%.7f"] * len(columns)), header=SEP.join(columns))


def write_traj_race(path, race_cl, ggv_file=None):
    """The race trajectory file: race_cl (m + 1, 7) = [s, x, y, psi, kappa, vx, ax], closed (Engine.export_batch's race_cl)."""
    _write(path, race_cl, RACE_COLUMNS, ggv_file)


def write_traj_ltpl(path, ltpl, ggv_file=None):
    """The local planner's file: ltpl (n + 1, 12), the closed table of Engine.export_batch.  The file holds its first n rows: upstream builds the
    closed table and writes the unclosed one, and the planner reads what upstream writes."""
    ltpl = np.asarray(ltpl, dtype=np.float64)
    if ltpl.ndim != 2 or ltpl.shape[0] < 2:
        raise ValueError("expected the closed table (n + 1, %d), got shape %s" % (len(LTPL_COLUMNS), ltpl.shape))
    _write(path, ltpl[:-1], LTPL_COLUMNS, ggv_file)


def read_table(path):
    """(uuid, ggv digest, column names, rows) of a file either writer made."""
    with open(path, "r") as fh:
        lines = fh.read().splitlines()
    names = tuple(lines[2][2:].split(SEP))
    rows = np.array([[float(c) for c in ln.split(SEP)] for ln in lines[3:]], dtype=np.float64).reshape(-1, len(names))
    return lines[0][2:], lines[1][2:], names, rows
