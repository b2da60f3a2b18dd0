"""Write tests/golden/floor_maps.npz: seeded floor-map models and inputs, the long-double result of the restatement in
tests/floor_common.py rounded to float64 (``truth``), the float64 restatement's own distance from it (``e64``) and, with
``--reference DIR`` (a checkout of the reference project; its ``cv2`` import is satisfied by an empty placeholder module, no cv2 function
is reached with distortion off), the outputs of the reference's own classes for the distortion-off cases (``ref_*``).

Points are kept only where every decision of the long-double run is clear (margins below); the generator asserts that at most 2 % of the
drawn points are dropped, that the reference's decisions equal the restatement's on every kept point and that its coordinates lie within
4 e64 + 4 ulp of the case's largest coordinate.

    python tools/gen_floor_golden.py [--reference DIR]
"""

import argparse
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import floor_common as F  # noqa: E402
from office_person_detection_vit_amd import floor as FL  # noqa: E402

LD = np.longdouble
N_DRAW = 300
MARGIN_BARY, MARGIN_CENTROID, MARGIN_BOUNDS, MARGIN_EDGE = 1e-9, 1e-9, 1e-6, 1e-6

# the reference configuration (config.yaml): homography, floor map, zones
CONFIG_H = [[-0.8795888447, -2.8974379541, 417.8510123786], [-1.5459702925, -3.4570021203, 1054.0107447082], [-0.0011928509, -0.0035480452, 1.0]]
CONFIG_FM = (1878, 1369, 28.1926406926406, 28.241430700447)
CONFIG_ZONES = [{"id": "zone_1", "polygon": [[859, 912], [1095, 912], [1095, 1350], [859, 1350]], "priority": 1},
                {"id": "zone_2", "polygon": [[1095, 912], [1331, 912], [1331, 1350], [1095, 1350]], "priority": 2},
                {"id": "zone_3", "polygon": [[1331, 912], [1567, 912], [1567, 1350], [1331, 1350]], "priority": 3}]
DIST = (1250.0, 1250.0, 640.0, 360.0, -0.1, 0.05, 1e-3, 1e-3, 0.0)


def zone_dicts(polys, prios=None):
    return [{"id": f"z{i}", "polygon": [[float(x), float(y)] for x, y in p], **({} if prios is None or prios[i] is None else {"priority": prios[i]})}
            for i, p in enumerate(polys)]


def control_points(rng, n):
    """n camera points, at least 12 px apart, and smoothly warped floor points that fill the floor map."""
    pts = []
    while len(pts) < n:
        p = rng.uniform((40, 40), (1240, 680))
        if all(np.hypot(*(p - q)) >= 12 for q in pts):
            pts.append(p)
    src = np.round(np.array(pts), 2)
    dst = np.stack([1.4 * src[:, 0] + 40 + 25 * np.sin(src[:, 1] / 150.0), 1.8 * src[:, 1] + 30 + 20 * np.cos(src[:, 0] / 200.0)], 1)
    return src, np.round(dst, 3)


def polygons(kind, rng):
    if kind == "none":
        return [], None
    if kind == "concave":   # one concave polygon (an L with a notch)
        return [np.array([[300, 200], [1500, 200], [1500, 700], [900, 700], [900, 450], [700, 450], [700, 1100], [300, 1100]], float)], None
    if kind == "many":      # 64 zones: a triangle, a 64-gon, 62 cells of a grid that overlap their neighbours
        t = np.linspace(0, 2 * np.pi, 64, endpoint=False)
        polys = [np.array([[100, 100], [700, 150], [350, 650]], float), np.stack([940 + 420.5 * np.cos(t), 690 + 390.25 * np.sin(t)], 1)]
        for k in range(62):
            x0, y0 = 30 + 225 * (k % 8), 20 + 165 * (k // 8)
            polys.append(np.array([[x0, y0], [x0 + 260.5, y0 + 3], [x0 + 255, y0 + 190.25], [x0 - 4, y0 + 186]], float))
        prios = [None if k % 3 == 0 else float(rng.integers(1, 6)) for k in range(64)]
        return polys, prios
    if kind in ("overlap_prio", "overlap_plain", "overlap_all"):   # two overlapping zones (and a third inside both)
        polys = [np.array([[200, 200], [1200, 220], [1180, 1000], [220, 980]], float), np.array([[700, 100], [1700, 120], [1680, 1250], [720, 1200]], float),
                 np.array([[800, 400], [1100, 400], [1100, 800], [800, 800]], float)]
        return polys, ([3.0, 1.0, 1.0] if kind == "overlap_prio" else None)
    raise ValueError(kind)


def draw_inputs(rng, n, as_points):
    """Boxes whose foot points (or points that) cover the frame and a margin around it."""
    foot = rng.uniform((-100, -60), (1380, 800), (n, 2))
    if as_points:
        return None, foot
    w, h = rng.uniform(20, 200, n), rng.uniform(40, 400, n)
    return np.stack([foot[:, 0] - w / 2, foot[:, 1] - h, w, h], 1).astype(np.float32), None


def build_cases():
    rng = np.random.default_rng(20240607)
    cases = {}
    # the reference configuration: half of the boxes aimed at the zones through the inverse homography
    Hm = np.array(CONFIG_H)
    floor = rng.uniform((800, 850), (1620, 1400), (N_DRAW // 2, 2))
    back = (np.linalg.inv(Hm) @ np.concatenate([floor, np.ones((len(floor), 1))], 1).T).T
    foot = back[:, :2] / back[:, 2:]
    w, h = rng.uniform(20, 200, len(foot)), rng.uniform(40, 400, len(foot))
    aimed = np.stack([foot[:, 0] - w / 2, foot[:, 1] - h, w, h], 1).astype(np.float32)
    cases["homography_config"] = (FL.model_homography(Hm, CONFIG_FM, CONFIG_ZONES, allow_overlap=False),
                                  np.concatenate([aimed, draw_inputs(rng, N_DRAW - len(aimed), False)[0]]), None, CONFIG_ZONES)
    for name, n, zones_kind, overlap in (("pwa_n3", 3, "concave", False), ("pwa_t_small", 24, "none", False), ("pwa_t_mid", 40, "overlap_plain", False),
                                         ("pwa_t_big", 90, "many", False), ("pwa_overlap_all", 40, "many", True)):
        src, dst = control_points(rng, n)
        polys, prios = polygons(zones_kind, rng)
        zd = zone_dicts(polys, prios)
        cases[name] = (FL.model_piecewise_affine(src, dst, CONFIG_FM, zd, allow_overlap=overlap), *draw_inputs(rng, N_DRAW, False), zd)
        cases[name][0]["_src_dst"] = (src, dst)
    for name, n, zones_kind, overlap in (("tps_n3", 3, "overlap_prio", False), ("tps_n64", 64, "overlap_all", True), ("tps_n65", 65, "concave", False)):
        src, dst = control_points(rng, n)
        polys, prios = polygons(zones_kind, rng)
        zd = zone_dicts(polys, prios)
        cases[name] = (FL.model_thin_plate_spline(src, dst, CONFIG_FM, zd, allow_overlap=overlap), *draw_inputs(rng, N_DRAW, name != "tps_n64"), zd)
        cases[name][0]["_src_dst"] = (src, dst)
    src, dst = control_points(rng, 40)
    zd = zone_dicts(*polygons("overlap_prio", rng))
    cases["pwa_distortion"] = (FL.model_piecewise_affine(src, dst, CONFIG_FM, zd, distortion=DIST), *draw_inputs(rng, N_DRAW, True), zd)
    return cases


def reference_outputs(ref_root, model, boxes, pts, zones):
    """The reference's own classes on the kept inputs: px, triangle, extrapolated, within, zone ids."""
    if "cv2" not in sys.modules:
        sys.modules["cv2"] = types.ModuleType("cv2")
    if ref_root not in sys.path:
        sys.path.insert(0, ref_root)
    from src.transform import FloorMapConfig, HomographyTransformer, PiecewiseAffineTransformer, ThinPlateSplineTransformer
    from src.zone import ZoneClassifier
    fm = FloorMapConfig(width_px=int(model["fm"][0]), height_px=int(model["fm"][1]), scale_x_mm_per_px=float(model["fm"][2]), scale_y_mm_per_px=float(model["fm"][3]))
    if model["method"] == F.HOMOGRAPHY:
        t = HomographyTransformer(np.asarray(model["H"]).reshape(3, 3), fm)
    elif model["method"] == F.PWA:
        t = PiecewiseAffineTransformer(*model["_src_dst"], fm)
        assert np.array_equal(t.delaunay.simplices, model["triangles"])
    else:
        t = ThinPlateSplineTransformer(*model["_src_dst"], fm, regularization=0.0)
    zc = ZoneClassifier(zones, allow_overlap=model["allow_overlap"])
    if boxes is not None:
        res = t.transform_batch([tuple(float(v) for v in b) for b in boxes])
    else:
        res = [t.transform_pixel((float(p[0]), float(p[1]))) for p in pts]
    ids = [z["id"] for z in zones]
    masks = np.array([sum(1 << ids.index(i) for i in zc.classify(r.floor_coords_px)) for r in res], np.uint64)
    mm = np.array([r.floor_coords_mm for r in res], np.float64)
    return (np.array([r.floor_coords_px for r in res], np.float64), np.array([getattr(r, "triangle_index", -1) for r in res], np.int32),
            np.array([getattr(r, "is_extrapolated", False) for r in res]), np.array([r.is_within_bounds for r in res]), masks, mm)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("OPD_REFERENCE_ROOT"))
    ap.add_argument("--out", default=F.GOLDEN)
    args = ap.parse_args()
    out = {"cases": np.array([], dtype="U32"), "margins": np.array([MARGIN_BARY, MARGIN_CENTROID, MARGIN_BOUNDS, MARGIN_EDGE])}
    names = []
    for name, (model, boxes, pts, zones) in build_cases().items():
        diag = {}
        px, tri, flags, masks = F.run(model, boxes, pts, LD, diag)
        keep = np.ones(len(px), bool)
        if model["method"] == F.PWA:
            keep &= (diag["bary"] >= MARGIN_BARY) & (diag["centroid_gap"] >= MARGIN_CENTROID)
        W, Hh = model["fm"][0], model["fm"][1]
        fx, fy = px[:, 0].astype(np.float64), px[:, 1].astype(np.float64)
        keep &= (np.abs(fx) >= MARGIN_BOUNDS) & (np.abs(fx - W) >= MARGIN_BOUNDS) & (np.abs(fy) >= MARGIN_BOUNDS) & (np.abs(fy - Hh) >= MARGIN_BOUNDS)
        keep &= F.edge_distance(model, fx, fy) >= MARGIN_EDGE
        dropped = int((~keep).sum())
        assert dropped <= 0.02 * len(keep), (name, dropped)
        boxes = None if boxes is None else boxes[keep]
        pts = None if pts is None else pts[keep]
        truth = px[keep].astype(np.float64)
        p64, t64, f64, m64 = F.run(model, boxes, pts, np.float64)
        assert np.array_equal(t64, tri[keep]) and np.array_equal(f64, flags[keep]) and np.array_equal(m64, masks[keep]), name
        e64 = float(np.abs(p64.astype(LD) - px[keep]).max())
        rec = F.pack_model(model)
        rec.update(truth_px=truth, truth_tri=tri[keep], truth_flags=flags[keep], truth_mask=masks[keep], e64=np.float64(e64),
                   boxes=np.zeros((0, 4), np.float32) if boxes is None else boxes, pts=np.zeros((0, 2)) if pts is None else pts)
        line = f"{name}: kept {int(keep.sum())}/{len(keep)}, e64 = {e64:.3e}, max |coordinate| = {np.abs(truth).max():.1f}"
        if model.get("dist") is not None:
            x, y = (pts[:, 0], pts[:, 1]) if pts is not None else F.foot_points(boxes)
            ux, uy = F.undistort(x, y, model["dist"])
            rx, ry = F.distort(ux, uy, model["dist"])
            rec["e_rt"] = np.float64(max(np.abs(rx - x).max(), np.abs(ry - y).max()))
            line += f", round trip e_rt = {float(rec['e_rt']):.3e} px"
        elif args.reference:
            rpx, rtri, rext, rwithin, rmask, rmm = reference_outputs(args.reference, model, boxes, pts, zones)
            if model["method"] == F.PWA:
                assert np.array_equal(rtri, tri[keep]) and np.array_equal(rext, (flags[keep] & F.EXTRAPOLATED) != 0), name
            assert np.array_equal(rwithin, (flags[keep] & F.WITHIN) != 0) and np.array_equal(rmask, masks[keep]), name
            d = float(np.abs(rpx - truth).max())
            limit = 4 * e64 + 4 * float(np.spacing(np.abs(truth).max()))
            assert d <= limit, (name, d, limit)
            rec.update(ref_px=rpx, ref_tri=rtri, ref_extrapolated=rext, ref_within=rwithin, ref_mask=rmask, ref_mm=rmm)
            line += f", reference within {d:.3e} (limit {limit:.3e})"
        print(line)
        names.append(name)
        out.update({f"{name}_{k}": v for k, v in rec.items()})
    out["cases"] = np.array(names)
    np.savez_compressed(args.out, **out)
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
