"""A float64 restatement of what mcq_points_in_path_device and mcq_friction_gen_device compute (include/mcq.h "friction map generation"):
matplotlib's Path.contains_points with a radius -- agg's contour of the polygon at half the radius, then the crossing test -- the reference's
track boundaries [REF frictionmap/src/reftrack_functions.py] and its grid of cells [REF main_gen_frictionmap.py:88-130].  Plain Python floats,
one rounding per operation, in the order the header states them; numpy only carries the arrays and runs the crossing test edge by edge.  Held
bit for bit to matplotlib's recorded verdicts, numpy.arange and the reference's own boundaries by tests/test_fgen_ref.py."""
import math

import numpy as np

EPS = 1e-14                 # agg's vertex_dist_epsilon: closer vertices are one vertex
DEN_EPS = 1e-30             # agg's intersection_epsilon
MITER_LIMIT, INNER_LIMIT = 4.0, 1.01
ST_NONFINITE, ST_FEW, ST_OVERFLOW, ST_GRID = 1, 2, 4, 8      # MCQ_FGEN_* (include/mcq.h)
MAX_DIST_CLOSED = 10.0


def _dist(ax, ay, bx, by):
    dx, dy = bx - ax, by - ay
    return math.sqrt(dx * dx + dy * dy)


def _cross(ax, ay, bx, by, qx, qy):
    return (qx - bx) * (by - ay) - (qy - by) * (bx - ax)


def kept_vertices(verts):
    """The vertices agg's contour generator works on: a vertex within EPS of the previous kept one is dropped, then trailing vertices within EPS
    of the first."""
    kept = []
    for x, y in np.asarray(verts, dtype=np.float64).reshape(-1, 2).tolist():
        if kept and not _dist(kept[-1][0], kept[-1][1], x, y) > EPS:
            continue
        kept.append((x, y))
    while len(kept) > 1 and not _dist(kept[-1][0], kept[-1][1], kept[0][0], kept[0][1]) > EPS:
        kept.pop()
    return kept


def _miter(out, v0, v1, v2, dx1, dy1, dx2, dy2, revert, mlimit, dbevel, wabs, wsign):
    lim = wabs * mlimit
    ax, ay, bx, by = v0[0] + dx1, v0[1] - dy1, v1[0] + dx1, v1[1] - dy1
    cx, cy, dx, dy = v1[0] + dx2, v1[1] - dy2, v2[0] + dx2, v2[1] - dy2
    num = (ay - cy) * (dx - cx) - (ax - cx) * (dy - cy)
    den = (bx - ax) * (dy - cy) - (by - ay) * (dx - cx)
    failed, exceeded, di, px, py = True, True, 1.0, v1[0], v1[1]
    if not abs(den) < DEN_EPS:
        r = num / den
        px, py = ax + r * (bx - ax), ay + r * (by - ay)
        di = _dist(v1[0], v1[1], px, py)
        if di <= lim:
            out.append((px, py))
            exceeded = False
        failed = False
    else:
        qx, qy = v1[0] + dx1, v1[1] - dy1
        if (_cross(v0[0], v0[1], v1[0], v1[1], qx, qy) < 0.0) == (_cross(v1[0], v1[1], v2[0], v2[1], qx, qy) < 0.0):
            out.append((qx, qy))
            exceeded = False
    if not exceeded:
        return
    if revert:
        out.append((v1[0] + dx1, v1[1] - dy1))
        out.append((v1[0] + dx2, v1[1] - dy2))
    elif failed:
        ml = mlimit * wsign
        out.append((v1[0] + dx1 + dy1 * ml, v1[1] - dy1 + dx1 * ml))
        out.append((v1[0] + dx2 - dy2 * ml, v1[1] - dy2 - dx2 * ml))
    else:
        x1, y1, x2, y2 = v1[0] + dx1, v1[1] - dy1, v1[0] + dx2, v1[1] - dy2
        t = (lim - dbevel) / (di - dbevel)
        out.append((x1 + (px - x1) * t, y1 + (py - y1) * t))
        out.append((x2 + (px - x2) * t, y2 + (py - y2) * t))


def contour(verts, radius):
    """The polygon the crossing test runs on, [c, 2]: the path itself for radius 0, else agg's contour at half the radius (miter joins, limit 4;
    inner joins reverted, limit 1.01).  A path of fewer than 3 vertices, or one whose kept vertices are fewer than 2, gives no polygon."""
    verts = np.asarray(verts, dtype=np.float64).reshape(-1, 2)
    if verts.shape[0] < 3:
        return np.zeros((0, 2))
    if radius == 0.0:
        return verts.copy()
    w = float(radius) * 0.5
    wabs, wsign = (-w, -1.0) if w < 0.0 else (w, 1.0)
    kv = kept_vertices(verts)
    m = len(kv)
    if m < 2:
        return np.zeros((0, 2))
    lens = [_dist(kv[i][0], kv[i][1], kv[(i + 1) % m][0], kv[(i + 1) % m][1]) for i in range(m)]
    out = []
    for i in range(m):
        v0, v1, v2 = kv[i - 1], kv[i], kv[(i + 1) % m]
        len1, len2 = lens[i - 1], lens[i]
        dx1, dy1 = w * (v1[1] - v0[1]) / len1, w * (v1[0] - v0[0]) / len1
        dx2, dy2 = w * (v2[1] - v1[1]) / len2, w * (v2[0] - v1[0]) / len2
        cp = (v2[0] - v1[0]) * (v1[1] - v0[1]) - (v2[1] - v1[1]) * (v1[0] - v0[0])
        if (cp > EPS and w > 0.0) or (cp < -EPS and w < 0.0):
            limit = (len1 if len1 < len2 else len2) / wabs
            if limit < INNER_LIMIT:
                limit = INNER_LIMIT
            _miter(out, v0, v1, v2, dx1, dy1, dx2, dy2, True, limit, 0.0, wabs, wsign)
        else:
            dx, dy = (dx1 + dx2) / 2.0, (dy1 + dy2) / 2.0
            _miter(out, v0, v1, v2, dx1, dy1, dx2, dy2, False, MITER_LIMIT, math.sqrt(dx * dx + dy * dy), wabs, wsign)
    return np.array(out, dtype=np.float64).reshape(-1, 2)


def crossing(poly, points):
    """matplotlib's crossing test of points [k, 2] against the closed polygon [c, 2]; a point that is not finite is outside."""
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    tx, ty = pts[:, 0], pts[:, 1]
    inside = np.zeros(pts.shape[0], dtype=bool)
    c = poly.shape[0]
    if c == 0 or pts.shape[0] == 0:
        return inside
    with np.errstate(invalid="ignore", over="ignore"):
        for e in range(c):
            x0, y0 = poly[e]
            x1, y1 = poly[(e + 1) % c]
            f0, f1 = y0 >= ty, y1 >= ty
            inside ^= (f0 != f1) & ((((y1 - ty) * (x0 - x1)) >= ((x1 - tx) * (y0 - y1))) == f1)
    return inside & np.isfinite(tx) & np.isfinite(ty)


def contains_points(verts, points, radius=0.0):
    verts = np.asarray(verts, dtype=np.float64).reshape(-1, 2)
    return crossing(contour(verts, radius), points)


# ---- the reference's track boundaries and grid ----------------------------------------------------------------------------------------------------
def check_isclosed_refline(refline):
    refline = np.asarray(refline, dtype=np.float64)
    dx, dy = float(refline[-1, 0] - refline[0, 0]), float(refline[-1, 1] - refline[0, 1])
    return math.sqrt(dx * dx + dy * dy) <= MAX_DIST_CLOSED


def calc_trackboundaries(reftrack):
    """(right, left) [n, 2]: numpy.gradient's differences on the (closed: cyclic) line, the normal (gy, -gx) / sqrt(gy^2 + gx^2), p +- normal * width."""
    ref = np.asarray(reftrack, dtype=np.float64)
    n = ref.shape[0]
    closed = check_isclosed_refline(ref[:, :2])
    right, left = np.empty((n, 2)), np.empty((n, 2))
    p = ref.tolist()
    for i in range(n):
        if closed:
            a, b, h = p[i - 1], p[(i + 1) % n], 2.0
        elif i == 0:
            a, b, h = p[0], p[1], 1.0
        elif i == n - 1:
            a, b, h = p[n - 2], p[n - 1], 1.0
        else:
            a, b, h = p[i - 1], p[i + 1], 2.0
        gx, gy = (b[0] - a[0]) / h, (b[1] - a[1]) / h
        s = (gy * gy + gx * gx) + 0.0
        nf = (1.0 / math.sqrt(s)) if s != 0.0 else math.inf
        nx, ny = _mul(gy, nf), _mul(-gx, nf)
        right[i] = (p[i][0] + nx * p[i][2], p[i][1] + ny * p[i][2])
        left[i] = (p[i][0] - nx * p[i][3], p[i][1] - ny * p[i][3])
    return right, left


def _mul(a, b):
    with np.errstate(invalid="ignore"):
        return float(np.float64(a) * np.float64(b))      # (0 * inf is NaN without a Python exception)


def arange(start, stop, step):
    """numpy.arange's float64 values for Python numbers: ceil((stop - start) / step) entries, entry i = start + i * ((start + step) - start)."""
    start, stop, step = float(start), float(stop), float(step)
    k = int(math.ceil((stop - start) / step))
    if k <= 0:
        return np.zeros(0)
    nxt = start + step
    delta = nxt - start
    out = [start + i * delta for i in range(k)]
    if k > 1:
        out[1] = nxt
    return np.array(out)


def grid_range(reftrack):
    """x0, x1, y0, y1: the reference's integer range around the line."""
    ref = np.asarray(reftrack, dtype=np.float64)
    dd = int(math.ceil(float(ref[:, 2].max()) + float(ref[:, 3].max()) + 5.0))
    return (int(math.floor(float(ref[:, 0].min()) - dd)), int(math.ceil(float(ref[:, 0].max()) + dd)),
            int(math.floor(float(ref[:, 1].min()) - dd)), int(math.ceil(float(ref[:, 1].max()) + dd)))


def grid_axes(reftrack, cellwidth):
    x0, x1, y0, y1 = grid_range(reftrack)
    return arange(x0, x1 + 0.1, cellwidth), arange(y0, y1 + 0.1, cellwidth)


def grid_points(xg, yg):
    """x-major, y inner: the reference's coordinates array."""
    return np.column_stack((np.repeat(xg, yg.shape[0]), np.tile(yg, xg.shape[0])))


def polygons(reftrack, cellwidth, inside_right=True):
    """[(vertices, radius)] whose verdicts combine to the mask: closed tracks outside & ~inside, open tracks the single polygon."""
    ref = np.asarray(reftrack, dtype=np.float64)
    right, left = calc_trackboundaries(ref)
    d = cellwidth * 1.1
    if check_isclosed_refline(ref[:, :2]):
        inside, outside, sign = (right, left, -1) if inside_right else (left, right, 1)
        return [(outside, d * sign), (inside, -(d * sign))], True
    return [(np.vstack((left, np.flipud(right))), -d)], False


def status_of(reftrack, cellwidth=None):
    """The refusals of mcq_friction_gen_device that do not depend on cmax (the grid's with a cell width)."""
    ref = np.asarray(reftrack, dtype=np.float64)
    if ref.shape[0] < 3:
        return ST_FEW
    if not np.isfinite(ref).all():
        return ST_NONFINITE
    with np.errstate(invalid="ignore", divide="ignore"):
        right, left = calc_trackboundaries(ref)
    if not (np.isfinite(right).all() and np.isfinite(left).all()):
        return ST_NONFINITE
    if cellwidth is not None:
        nx, ny = grid_counts(ref, cellwidth)
        if nx * ny > 2 ** 31 - 1:
            return ST_GRID
    return 0


def grid_counts(reftrack, cellwidth):
    """nx, ny: numpy.arange's lengths, without the arrays."""
    x0, x1, y0, y1 = grid_range(reftrack)
    return tuple(max(int(math.ceil(((b + 0.1) - a) / float(cellwidth))), 0) for a, b in ((x0, x1), (y0, y1)))


def gen_cells(reftrack, cellwidth, inside_right=True):
    """(cells [c, 2], mask [nx * ny], xg, yg) of a track that is not refused."""
    xg, yg = grid_axes(reftrack, cellwidth)
    pts = grid_points(xg, yg)
    polys, closed = polygons(reftrack, cellwidth, inside_right)
    mask = contains_points(polys[0][0], pts, polys[0][1])
    if closed:
        mask &= ~contains_points(polys[1][0], pts, polys[1][1])
    return pts[mask], mask, xg, yg
