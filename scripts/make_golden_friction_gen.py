#!/usr/bin/env python3
"""Records, once, what the friction-map generation is held to, into tests/golden/friction_gen/reference.npz (data only), so that
tests/test_fgen_ref.py can hold the plain restatement tests/fgen_ref.py to it, and the device tests the engine, without the reference tree and
without matplotlib's verdicts being recomputed.

Run where the reference tree is at hand:   python scripts/make_golden_friction_gen.py --reference /path/to/reference

Per track T of the reference's four track files:
  T/reftrack [n, 4]                         the track file as the reference loads it
  T/bound_right, T/bound_left [n, 2]        the reference's own calc_trackboundaries
  T/grid [6]                                x0, x1, y0, y1 (the integer range), nx, ny at cell width 2.0
  T/mask_right, T/mask_left                 packed bits [nx * ny] at cell width 2.0: the reference's bool_OnTrack for both inside_trackbound values,
                                            from matplotlib's Path.contains_points (empty maps included)
  T/mask_left_0.7 (the two small tracks)    the same at cell width 0.7 for the side that gives cells
small/<name>/...                            reftrack, cellwidth, mask (packed) of the small and open tracks of tests/fgen_cases.py, by the
                                            reference's statements on the reference's boundaries
script/rr_csv, script/rr_json (uint8)       the two files the reference's script itself writes for rounded_rectangle at 2.0, byte for byte
script/berlin_sha256                        SHA-256 (hex) of the two files for berlin_2018 at 2.0, and script/berlin_cells their cell count
The script is executed from its text, read from the reference at generation time, with its USER INPUT values and output paths substituted and
its plots off; nothing of that text is kept.
paths/points [k, 2], paths/verdicts         the point set (lattice, random points, contour corners) and matplotlib's verdicts, packed bits
                                            [cases, k], for every (polygon, radius) of tests/fgen_cases.path_cases()
paths/tiny                                  verdicts [4, 7, k] (packed) of the paths of 0 .. 3 vertices at every radius"""
import argparse
import hashlib
import os
import re
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def run_script(reference, track, cellwidth, inside, tmp):
    """The reference's script from its text: (csv bytes, json bytes)."""
    with open(os.path.join(reference, "main_gen_frictionmap.py")) as fh:
        text = fh.read()
    p_map, p_data = os.path.join(tmp, track + "_tpamap.csv"), os.path.join(tmp, track + "_tpadata.json")
    for pat, val in ((r"^track_name = .*$", "track_name = %r" % track), (r"^initial_mue = .*$", "initial_mue = 0.8"),
                     (r"^cellwidth_m = .*$", "cellwidth_m = %r" % cellwidth), (r"^inside_trackbound = .*$", "inside_trackbound = %r" % inside),
                     (r"^bool_show_plots = .*$", "bool_show_plots = False"), (r"^path2tpamap_file = .*$", "path2tpamap_file = %r" % p_map),
                     (r"^path2tpadata_file = .*$", "path2tpadata_file = %r" % p_data)):
        text, k = re.subn(pat, val, text, flags=re.M)
        assert k == 1, pat
    exec(compile(text, "<reference script>", "exec"), {"__file__": os.path.join(reference, "main_gen_frictionmap.py"), "__name__": "__main__"})
    with open(p_map, "rb") as a, open(p_data, "rb") as b:
        return a.read(), b.read()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "friction_gen", "reference.npz"))
    a = ap.parse_args()
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.path as mpl_path
    sys.path.insert(0, a.reference)
    import frictionmap
    rf = frictionmap.src.reftrack_functions

    def on_track(ref, cw, inside):          # [REF main_gen_frictionmap.py:64-127], on the reference's own boundaries
        closed = rf.check_isclosed_refline(refline=ref[:, :2])
        b_right, b_left = rf.calc_trackboundaries(reftrack=ref)
        if closed and inside == "right":
            b_in, b_out, sign = b_right, b_left, -1
        else:
            b_in, b_out, sign = b_left, b_right, 1
        dd = int(np.ceil(np.amax(ref[:, 2]) + np.amax(ref[:, 3]) + 5.0))
        rng = [int(np.floor(np.amin(ref[:, 0]) - dd)), int(np.ceil(np.amax(ref[:, 0]) + dd)),
               int(np.floor(np.amin(ref[:, 1]) - dd)), int(np.ceil(np.amax(ref[:, 1]) + dd))]
        xg, yg = np.arange(rng[0], rng[1] + 0.1, cw), np.arange(rng[2], rng[3] + 0.1, cw)
        pts = np.column_stack((np.repeat(xg, yg.shape[0]), np.tile(yg, xg.shape[0])))
        d = cw * 1.1
        if closed:
            m = mpl_path.Path(b_out).contains_points(pts, radius=d * sign) & ~mpl_path.Path(b_in).contains_points(pts, radius=-(d * sign))
        else:
            m = mpl_path.Path(np.vstack((b_in, np.flipud(b_out)))).contains_points(pts, radius=-d)
        return m, rng, xg, yg

    import fgen_cases as fc
    import fgen_ref as fr
    out = {}
    for t in fc.TRACKS:
        ref = rf.load_reftrack(path2track=os.path.join(a.reference, "inputs", "tracks", t + ".csv"))
        out[t + "/reftrack"] = ref
        out[t + "/bound_right"], out[t + "/bound_left"] = rf.calc_trackboundaries(reftrack=ref)
        for inside in ("right", "left"):
            m, rng, xg, yg = on_track(ref, 2.0, inside)
            out["%s/mask_%s" % (t, inside)] = np.packbits(m)
            print(t, inside, 2.0, int(m.sum()), "of", m.size)
        out[t + "/grid"] = np.array(rng + [xg.shape[0], yg.shape[0]], dtype=np.float64)
        if t in fc.SMALL_TRACKS:
            m, _, _, _ = on_track(ref, 0.7, fc.INSIDE[t])
            out["%s/mask_%s_0.7" % (t, fc.INSIDE[t])] = np.packbits(m)
            print(t, fc.INSIDE[t], 0.7, int(m.sum()), "of", m.size)
    np.savez_compressed(a.out, **out)          # (fgen_cases.small_tracks reads the handling track from it)
    for name, (ref, cw) in fc.small_tracks().items():
        m, rng, xg, yg = on_track(ref, cw, fc.SMALL_INSIDE)
        out["small/%s/reftrack" % name], out["small/%s/cellwidth" % name] = ref, np.float64(cw)
        out["small/%s/mask" % name] = np.packbits(m)
        out["small/%s/closed" % name] = np.bool_(rf.check_isclosed_refline(refline=ref[:, :2]))
        out["small/%s/bound_right" % name], out["small/%s/bound_left" % name] = rf.calc_trackboundaries(reftrack=ref)
        print("small", name, cw, int(m.sum()), "of", m.size, "closed" if out["small/%s/closed" % name] else "open")
    with tempfile.TemporaryDirectory() as tmp:
        csv, js = run_script(a.reference, "rounded_rectangle", 2.0, fc.INSIDE["rounded_rectangle"], tmp)
        out["script/rr_csv"], out["script/rr_json"] = np.frombuffer(csv, dtype=np.uint8), np.frombuffer(js, dtype=np.uint8)
        csv, js = run_script(a.reference, "berlin_2018", 2.0, fc.INSIDE["berlin_2018"], tmp)
        out["script/berlin_sha256"] = np.array([hashlib.sha256(csv).hexdigest(), hashlib.sha256(js).hexdigest()])
        out["script/berlin_cells"] = np.int64(csv.count(b"\n") - 1)
        print("script: rounded_rectangle", out["script/rr_csv"].size, "bytes; berlin cells", int(out["script/berlin_cells"]))
    polys = fc.polygons()
    pts = np.vstack((fc.base_points(), fc.corner_points(fr.contour)))
    out["paths/points"] = pts
    out["paths/verdicts"] = np.packbits(np.array([mpl_path.Path(polys[n]).contains_points(pts, radius=r) for n, r in fc.path_cases()]), axis=1)
    tiny = np.zeros((4, len(fc.RADII), pts.shape[0]), dtype=bool)
    for k, v in enumerate(fc.tiny_paths()):
        for j, r in enumerate(fc.RADII):
            tiny[k, j] = mpl_path.Path(v.reshape(-1, 2)).contains_points(pts, radius=r) if v.shape[0] else False
    out["paths/tiny"] = np.packbits(tiny, axis=2)
    np.savez_compressed(a.out, **out)
    print("%s: %d bytes, %d points, %d path cases" % (a.out, os.path.getsize(a.out), pts.shape[0], len(fc.path_cases())))


if __name__ == "__main__":
    main()
