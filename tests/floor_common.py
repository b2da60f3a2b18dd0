"""The floor-map contract of include/opd_detr.h (opd_floor_*) restated in numpy, operation for operation, for any float type:
``np.float64`` is what the device evaluates (without fused multiply-adds), ``np.longdouble`` is the yardstick the fixture's ``truth`` was
computed with.  Also: reading a fixture case back into a model, a model into an ``opd_floor_config``, and the device calls.

A model is a dict: method, H [9], points [N,2], triangles [T,3] int32, affine [T,6], tps_w [N,2], tps_affine [6], dist (fx, fy, cx, cy,
k1, k2, p1, p2, k3) or None, fm (width, height, scale_x, scale_y), zones (list of [n,2] arrays), priority [Z] (NaN = none), allow_overlap."""

import ctypes as C
import os

import numpy as np

from office_person_detection_vit_amd import _capi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "floor_maps.npz")
HOMOGRAPHY, PWA, TPS = 0, 1, 2
VALID, WITHIN, EXTRAPOLATED = 1, 2, 4
REC_DTYPE = np.dtype([("px", np.float64, 2), ("mm", np.float64, 2), ("zone_mask", np.uint64), ("triangle", np.int32), ("flags", np.uint32)])
assert REC_DTYPE.itemsize == 48


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def foot_points(boxes, dt=np.float64):
    b = np.asarray(boxes, np.float32).reshape(-1, 4).astype(dt)
    return b[:, 0] + b[:, 2] / dt(2), b[:, 1] + b[:, 3]


def undistort(x, y, dist, dt=np.float64):
    """OpenCV's undistortPoints with P = K: five fixed-point iterations on the normalised point, the start value kept where 1 / radial < 0."""
    fx, fy, cx, cy, k1, k2, p1, p2, k3 = (dt(v) for v in dist)
    ifx, ify = dt(1) / fx, dt(1) / fy
    x = (x - cx) * ifx
    y = (y - cy) * ify
    x0, y0 = x.copy(), y.copy()
    live = np.ones(x.shape, bool)
    for _ in range(5):
        r2 = x * x + y * y
        icdist = dt(1) / (dt(1) + ((k3 * r2 + k2) * r2 + k1) * r2)
        stop = live & (icdist < 0)
        x = np.where(stop, x0, x)
        y = np.where(stop, y0, y)
        live &= ~stop
        dx = dt(2) * p1 * x * y + p2 * (r2 + dt(2) * x * x)
        dy = p1 * (r2 + dt(2) * y * y) + dt(2) * p2 * x * y
        x = np.where(live, (x0 - dx) * icdist, x)
        y = np.where(live, (y0 - dy) * icdist, y)
    return x * fx + cx, y * fy + cy


def distort(x, y, dist, dt=np.float64):
    """The forward model (pixels -> pixels), for the round trip."""
    fx, fy, cx, cy, k1, k2, p1, p2, k3 = (dt(v) for v in dist)
    x = (x - cx) / fx
    y = (y - cy) / fy
    r2 = x * x + y * y
    rad = dt(1) + ((k3 * r2 + k2) * r2 + k1) * r2
    xd = x * rad + (dt(2) * p1 * x * y + p2 * (r2 + dt(2) * x * x))
    yd = y * rad + (p1 * (r2 + dt(2) * y * y) + dt(2) * p2 * x * y)
    return xd * fx + cx, yd * fy + cy


def triangle_tables(points, triangles, dt=np.float64):
    """[T][8]: inverse of [[x0 - x2, x1 - x2], [y0 - y2, y1 - y2]] row-major, the last vertex, the centroid (numpy's mean of the three)."""
    p = np.asarray(points, np.float64).astype(dt)
    v0, v1, v2 = (p[np.asarray(triangles)[:, k]] for k in range(3))
    a, b, c, d = v0[:, 0] - v2[:, 0], v1[:, 0] - v2[:, 0], v0[:, 1] - v2[:, 1], v1[:, 1] - v2[:, 1]
    with np.errstate(divide="ignore", invalid="ignore"):
        det = a * d - b * c
        cols = [d / det, -b / det, -c / det, a / det, v2[:, 0], v2[:, 1], ((v0[:, 0] + v1[:, 0]) + v2[:, 0]) / dt(3), ((v0[:, 1] + v1[:, 1]) + v2[:, 1]) / dt(3)]
    return np.stack(cols, 1)


def pwa_search(model, x, y, dt=np.float64, diag=None):
    q = triangle_tables(model["points"], model["triangles"], dt)
    dx, dy = x[:, None] - q[None, :, 4], y[:, None] - q[None, :, 5]
    b0 = q[None, :, 0] * dx + q[None, :, 1] * dy
    b1 = q[None, :, 2] * dx + q[None, :, 3] * dy
    b2 = (dt(1) - b0) - b1
    ok = (b0 >= dt(-1e-12)) & (b1 >= dt(-1e-12)) & (b2 >= dt(-1e-12))
    inside = ok.any(1)
    first = ok.argmax(1)
    cx, cy = q[None, :, 6] - x[:, None], q[None, :, 7] - y[:, None]
    d = np.sqrt(cx * cx + cy * cy)
    nearest = d.argmin(1)
    if diag is not None:
        diag["bary"] = np.abs(np.stack([b0, b1, b2], -1)).min(axis=(1, 2))
        ds = np.sort(d, 1)
        diag["centroid_gap"] = (ds[:, 1] - ds[:, 0]) / ds[:, 1] if d.shape[1] > 1 else np.full(len(x), np.inf)
    return np.where(inside, first, nearest).astype(np.int32), ~inside


def tps_sum(w, u, dt=np.float64):
    """Lane l adds w_i u_i for i = l, l + 64, ... in ascending order; an xor butterfly adds the 64 partial sums."""
    part = np.zeros((u.shape[0], 64), dt)
    for i in range(u.shape[1]):
        part[:, i % 64] += w[i] * u[:, i]
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        part = part + part[:, lane ^ o]
    return part[:, 0]


def transform_points(model, x, y, dt=np.float64, diag=None):
    """Camera points -> (fx, fy, triangle, flags)."""
    x, y = np.asarray(x, dt), np.asarray(y, dt)
    n = len(x)
    tri = np.full(n, -1, np.int32)
    flags = np.full(n, VALID, np.uint32)
    method = int(model["method"])
    if model.get("dist") is not None and method != HOMOGRAPHY:
        x, y = undistort(x, y, model["dist"], dt)
    if method == HOMOGRAPHY:
        H = np.asarray(model["H"], np.float64).astype(dt).reshape(9)
        u, v, w = (H[0] * x + H[1] * y) + H[2], (H[3] * x + H[4] * y) + H[5], (H[6] * x + H[7] * y) + H[8]
        fx, fy = u / w, v / w
    elif method == PWA:
        tri, extra = pwa_search(model, x, y, dt, diag)
        flags = flags | np.where(extra, EXTRAPOLATED, 0).astype(np.uint32)
        a = np.asarray(model["affine"], np.float64).astype(dt)[tri]
        fx = (a[:, 0] * x + a[:, 1] * y) + a[:, 2]
        fy = (a[:, 3] * x + a[:, 4] * y) + a[:, 5]
    else:
        p = np.asarray(model["points"], np.float64).astype(dt)
        w = np.asarray(model["tps_w"], np.float64).astype(dt)
        ta = np.asarray(model["tps_affine"], np.float64).astype(dt)
        dx, dy = x[:, None] - p[None, :, 0], y[:, None] - p[None, :, 1]
        r = np.sqrt(dx * dx + dy * dy)
        with np.errstate(divide="ignore", invalid="ignore"):
            u = np.where(r > 0, r * r * np.log(np.where(r > 0, r, dt(1))), dt(0))
        fx = ((ta[0] + ta[1] * x) + ta[2] * y) + tps_sum(w[:, 0], u, dt)
        fy = ((ta[3] + ta[4] * x) + ta[5] * y) + tps_sum(w[:, 1], u, dt)
    width, height = dt(model["fm"][0]), dt(model["fm"][1])
    within = (0 <= fx) & (fx < width) & (0 <= fy) & (fy < height)
    return fx, fy, tri, flags | np.where(within, WITHIN, 0).astype(np.uint32)


def zone_ranks(priority, n):
    """Position of every zone when sorted by (priority or +inf, index)."""
    pr = np.full(n, np.nan) if priority is None or len(priority) == 0 else np.asarray(priority, np.float64)
    key = np.where(np.isnan(pr), np.inf, pr)
    order = sorted(range(n), key=lambda z: (key[z], z))
    rank = np.zeros(n, np.int32)
    rank[order] = np.arange(n, dtype=np.int32)
    return rank


def classify(model, fx, fy, dt=np.float64):
    """ZoneClassifier.classify as a 64-bit mask per point: the reference's ray cast edge by edge, then its allow_overlap rule."""
    fx, fy = np.asarray(fx, dt), np.asarray(fy, dt)
    zones = model["zones"]
    masks = np.zeros(len(fx), np.uint64)
    for z, poly in enumerate(zones):
        poly = np.asarray(poly, np.float64).astype(dt)
        inside = np.zeros(len(fx), bool)
        for i in range(len(poly)):
            (p1x, p1y), (p2x, p2y) = poly[i], poly[(i + 1) % len(poly)]
            cond = (fy > min(p1y, p2y)) & (fy <= max(p1y, p2y)) & (fx <= max(p1x, p2x))
            if p1y != p2y:
                xinters = (fy - p1y) * (p2x - p1x) / (p2y - p1y) + p1x
                cond &= (fx <= xinters) if p1x != p2x else True
            inside ^= cond          # (p1y == p2y: the range test is empty)
        masks |= np.where(inside, np.uint64(1) << np.uint64(z), np.uint64(0))
    if not model["allow_overlap"] and len(zones):
        rank = zone_ranks(model.get("priority"), len(zones))
        by_rank = np.argsort(rank)
        out = np.zeros_like(masks)
        for z in by_rank[::-1]:   # the best rank is written last
            bit = np.uint64(1) << np.uint64(z)
            out = np.where(masks & bit != 0, bit, out)
        masks = out
    return masks


def run(model, boxes=None, pts=None, dt=np.float64, diag=None):
    """``opd_floor_transform`` (boxes) / ``opd_floor_transform_points`` (pts) -> px [n,2], triangle, flags, zone masks."""
    x, y = foot_points(boxes, dt) if boxes is not None else (np.asarray(pts, np.float64)[:, 0].astype(dt), np.asarray(pts, np.float64)[:, 1].astype(dt))
    fx, fy, tri, flags = transform_points(model, x, y, dt, diag)
    return np.stack([fx, fy], 1), tri, flags, classify(model, fx, fy, dt)


def edge_distance(model, fx, fy):
    """Distance of every point to the nearest polygon edge (inf without zones)."""
    best = np.full(len(fx), np.inf)
    for poly in model["zones"]:
        poly = np.asarray(poly, np.float64)
        for i in range(len(poly)):
            a, b = poly[i], poly[(i + 1) % len(poly)]
            ab = b - a
            t = np.clip(((fx - a[0]) * ab[0] + (fy - a[1]) * ab[1]) / max(float(ab @ ab), 1e-300), 0.0, 1.0)
            best = np.minimum(best, np.hypot(fx - (a[0] + t * ab[0]), fy - (a[1] + t * ab[1])))
    return best


# ---- the fixture -------------------------------------------------------------------------------------------------------------------
MODEL_KEYS = ("method", "H", "points", "triangles", "affine", "tps_w", "tps_affine", "dist", "fm", "zone_vertices", "zone_offsets", "priority", "allow_overlap")


def pack_model(model):
    """A model as flat arrays (what the fixture stores)."""
    zones = model["zones"]
    off = np.cumsum([0] + [len(z) for z in zones]).astype(np.int32)
    return {"method": np.int32(model["method"]), "H": np.asarray(model.get("H", np.eye(3)), np.float64).reshape(9),
            "points": np.asarray(model.get("points", np.zeros((0, 2))), np.float64).reshape(-1, 2),
            "triangles": np.asarray(model.get("triangles", np.zeros((0, 3))), np.int32).reshape(-1, 3),
            "affine": np.asarray(model.get("affine", np.zeros((0, 6))), np.float64).reshape(-1, 6),
            "tps_w": np.asarray(model.get("tps_w", np.zeros((0, 2))), np.float64).reshape(-1, 2),
            "tps_affine": np.asarray(model.get("tps_affine", np.zeros(6)), np.float64).reshape(6),
            "dist": np.zeros(0) if model.get("dist") is None else np.asarray(model["dist"], np.float64),
            "fm": np.asarray(model["fm"], np.float64),
            "zone_vertices": np.concatenate([np.asarray(z, np.float64).reshape(-1, 2) for z in zones]) if zones else np.zeros((0, 2)),
            "zone_offsets": off, "priority": np.asarray(model.get("priority", np.full(len(zones), np.nan)), np.float64).reshape(-1),
            "allow_overlap": np.int32(bool(model["allow_overlap"]))}


def unpack_model(get):
    """``get(key)`` -> array; the inverse of pack_model."""
    off = get("zone_offsets")
    zv = get("zone_vertices")
    dist = get("dist")
    return {"method": int(get("method")), "H": get("H"), "points": get("points"), "triangles": get("triangles"), "affine": get("affine"),
            "tps_w": get("tps_w"), "tps_affine": get("tps_affine"), "dist": None if len(dist) == 0 else dist, "fm": get("fm"),
            "zones": [zv[off[z]:off[z + 1]] for z in range(len(off) - 1)], "priority": get("priority"), "allow_overlap": bool(get("allow_overlap"))}


def case_names(g):
    return [str(s) for s in g["cases"]]


def case_model(g, name):
    return unpack_model(lambda k: g[f"{name}_{k}"])


def bound(g, name):
    """4 e64 + 4 ulp(max |coordinate| of the case): a fixed-order wave sum and the device's log / sqrt may each move a result by about
    what float64 itself does (e64: the float64 restatement's distance from the long-double truth), and not more."""
    return 4.0 * float(g[f"{name}_e64"]) + 4.0 * float(np.spacing(np.abs(g[f"{name}_truth_px"]).max()))


# ---- the C-ABI ---------------------------------------------------------------------------------------------------------------------
def make_config(model):
    """(opd_floor_config, keep-alive list) of a model."""
    m = pack_model(model)
    keep = [np.ascontiguousarray(m[k]) for k in ("points", "triangles", "affine", "tps_w", "zone_vertices", "zone_offsets", "priority")]
    ptr = lambda a: a.ctypes.data if a.size else None
    cfg = _capi.OpdFloorConfig(method=int(m["method"]), n_points=len(keep[0]), n_triangles=len(keep[1]), n_zones=len(keep[5]) - 1,
                               has_distortion=int(len(m["dist"]) > 0), allow_overlap=int(m["allow_overlap"]), width_px=int(m["fm"][0]), height_px=int(m["fm"][1]),
                               scale_x_mm_per_px=float(m["fm"][2]), scale_y_mm_per_px=float(m["fm"][3]))
    cfg.H[:] = m["H"].tolist()
    cfg.tps_affine[:] = m["tps_affine"].tolist()
    if len(m["dist"]):
        cfg.intrinsics[:] = m["dist"][:4].tolist()
        cfg.distortion[:] = m["dist"][4:].tolist()
    cfg.points, cfg.triangles, cfg.affine, cfg.tps_weights, cfg.zone_vertices = (ptr(a) for a in keep[:5])
    cfg.zone_offsets = keep[5].ctypes.data
    cfg.zone_priority = ptr(keep[6])
    return cfg, keep


def create(lib, model, device=0):
    cfg, keep = make_config(model)
    h = C.c_void_p()
    _capi.check(lib.opd_floor_create(C.byref(cfg), device, C.byref(h)), "opd_floor_create")
    return h


def device_transform(lib, h, boxes=None, pts=None):
    n = len(boxes) if boxes is not None else len(pts)
    out = np.zeros(n, REC_DTYPE)
    if boxes is not None:
        b = np.ascontiguousarray(boxes, np.float32).reshape(-1, 4)
        _capi.check(lib.opd_floor_transform(h, b.ctypes.data, n, _capi.OPD_MEM_HOST, out.ctypes.data), "opd_floor_transform")
    else:
        p = np.ascontiguousarray(pts, np.float64).reshape(-1, 2)
        _capi.check(lib.opd_floor_transform_points(h, p.ctypes.data, n, out.ctypes.data), "opd_floor_transform_points")
    return out


def device_classify(lib, h, floor_xy):
    p = np.ascontiguousarray(floor_xy, np.float64).reshape(-1, 2)
    out = np.zeros(len(p), np.uint64)
    _capi.check(lib.opd_floor_classify(h, p.ctypes.data, len(p), out.ctypes.data), "opd_floor_classify")
    return out
