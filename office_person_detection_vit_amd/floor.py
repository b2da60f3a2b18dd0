"""``HipFloorMapper``: the reference's Phase 3 (``TransformPhase``, src/pipeline/phases/transform.py) per detection on the device.

Foot point -> optional lens undistortion -> homography / piecewise affine / thin-plate spline -> floor pixels, mm and the bounds test ->
``ZoneClassifier.classify`` run in ``csrc/kernels_floor.hip`` behind the ``opd_floor_*`` calls of ``include/opd_detr.h``.  The set-up stays
on the host and in numpy / scipy, as the reference computes it: affine matrices by ``lstsq``, spline coefficients by ``np.linalg.solve``,
the triangulation by ``scipy.spatial.Delaunay``.  The device never triangulates."""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
import json
import logging
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _capi
from .data_models import Detection

logger = logging.getLogger(__name__)

SUPPORTED_METHODS = ("homography", "piecewise_affine", "thin_plate_spline")
REC_DTYPE = np.dtype([("px", np.float64, 2), ("mm", np.float64, 2), ("zone_mask", np.uint64), ("triangle", np.int32), ("flags", np.uint32)])


@dataclass
class TransformResult:   # src/transform/homography.py:21-37
    floor_coords_px: Optional[Tuple[float, float]] = None
    floor_coords_mm: Optional[Tuple[float, float]] = None
    is_valid: bool = False
    error_reason: Optional[str] = None
    is_within_bounds: bool = False


@dataclass
class PWATransformResult:   # src/transform/piecewise_affine.py:28-48
    floor_coords_px: Optional[Tuple[float, float]] = None
    floor_coords_mm: Optional[Tuple[float, float]] = None
    is_valid: bool = False
    error_reason: Optional[str] = None
    is_within_bounds: bool = False
    triangle_index: int = -1
    is_extrapolated: bool = False


# ---- models: plain dicts of arrays (tests/floor_common.py restates the kernel on the same dicts) ---------------------------------------
def _floormap(fm) -> Tuple[int, int, float, float]:
    """(width_px, height_px, scale_x, scale_y) from a 4-tuple, a ``floormap`` config section or an object with FloorMapConfig's fields."""
    if isinstance(fm, dict):
        return (int(fm.get("image_width", 1878)), int(fm.get("image_height", 1369)), float(fm.get("image_x_mm_per_pixel", 28.1926406926406)),
                float(fm.get("image_y_mm_per_pixel", 28.241430700447)))
    if hasattr(fm, "width_px"):
        return int(fm.width_px), int(fm.height_px), float(fm.scale_x_mm_per_px), float(fm.scale_y_mm_per_px)
    w, h, sx, sy = fm
    return int(w), int(h), float(sx), float(sy)


def _zones(zones) -> Tuple[List[np.ndarray], np.ndarray, List[str]]:
    """ZoneClassifier._validate_zones: polygons, priorities (NaN = none) and ids."""
    if not isinstance(zones, (list, tuple)):
        raise ValueError("zones must be a list")
    polys, prio, ids = [], [], []
    for i, z in enumerate(zones):
        if not isinstance(z, dict) or "id" not in z or "polygon" not in z:
            raise ValueError(f"zones[{i}] needs 'id' and 'polygon'")
        if z["id"] in ids:
            raise ValueError(f"duplicate zone id: {z['id']}")
        poly = np.asarray([(float(p[0]), float(p[1])) for p in z["polygon"]], np.float64).reshape(-1, 2)
        if len(poly) < 3:
            raise ValueError(f"zones[{i}].polygon needs at least 3 vertices")
        polys.append(poly)
        prio.append(float(z["priority"]) if z.get("priority") is not None else float("nan"))
        ids.append(z["id"])
    return polys, np.asarray(prio, np.float64), ids


def _base(method: int, floormap, zones, allow_overlap: bool, distortion) -> dict:
    polys, prio, ids = _zones(zones or [])
    dist = None
    if distortion is not None and method != _capi.OPD_FLOOR_HOMOGRAPHY:
        d = np.asarray(distortion, np.float64).reshape(9)   # fx, fy, cx, cy, k1, k2, p1, p2, k3
        if np.any(np.abs(d[4:]) >= 1e-10):                  # DistortionParams.is_zero: all-zero coefficients mean no corrector
            dist = d
    return {"method": method, "fm": np.asarray(_floormap(floormap), np.float64), "zones": polys, "priority": prio, "zone_ids": ids,
            "allow_overlap": bool(allow_overlap), "dist": dist}


def model_homography(H, floormap, zones, allow_overlap: bool = False) -> dict:
    H = np.array(H, dtype=np.float64)
    if H.shape != (3, 3):
        raise ValueError(f"the homography must be 3x3: {H.shape}")
    if abs(np.linalg.det(H)) < 1e-10:
        raise ValueError("the homography is singular")
    return dict(_base(_capi.OPD_FLOOR_HOMOGRAPHY, floormap, zones, allow_overlap, None), H=H.reshape(9))


def _points(src, dst):
    src, dst = np.array(src, dtype=np.float64).reshape(-1, 2), np.array(dst, dtype=np.float64).reshape(-1, 2)
    if len(src) < 3:
        raise ValueError("at least 3 point correspondences are needed")
    if len(src) != len(dst):
        raise ValueError("src_points and dst_points differ in length")
    return src, dst


def model_piecewise_affine(src, dst, floormap, zones, simplices=None, distortion=None, allow_overlap: bool = False) -> dict:
    src, dst = _points(src, dst)
    if simplices is None:
        try:
            from scipy.spatial import Delaunay
        except ImportError as e:
            raise RuntimeError("piecewise_affine without `simplices` triangulates with scipy.spatial.Delaunay, and scipy is not installed; "
                               "pass the triangles as `simplices`") from e
        simplices = Delaunay(src).simplices
    tri = np.asarray(simplices, np.int32).reshape(-1, 3)
    affine = np.empty((len(tri), 6), np.float64)
    for i, s in enumerate(tri):   # PiecewiseAffineTransformer._compute_affine_matrices
        src_aug = np.vstack([src[s].T, np.ones(3)])
        dst_aug = np.vstack([dst[s].T, np.ones(3)])
        A, _, _, _ = np.linalg.lstsq(src_aug.T, dst_aug.T, rcond=None)
        affine[i] = A.T[:2].reshape(6)
    return dict(_base(_capi.OPD_FLOOR_PWA, floormap, zones, allow_overlap, distortion), points=src, triangles=tri, affine=affine)


def model_thin_plate_spline(src, dst, floormap, zones, regularization: float = 0.0, distortion=None, allow_overlap: bool = False) -> dict:
    src, dst = _points(src, dst)
    n = len(src)
    K = np.zeros((n, n))   # ThinPlateSplineTransformer._compute_tps_coefficients, entry by entry as it is there: the solve below is
    for i in range(n):     # ill-conditioned enough for a last-bit difference in K to show in the coefficients
        for j in range(n):
            if i != j:
                r = np.array([np.linalg.norm(src[i] - src[j])])
                K[i, j] = (r ** 2 * np.log(r))[0] if r[0] > 0 else 0.0
    P = np.hstack([np.ones((n, 1)), src])
    L = np.zeros((n + 3, n + 3))
    L[:n, :n] = K + regularization * np.eye(n)
    L[:n, n:] = P
    L[n:, :n] = P.T
    v = np.zeros((n + 3, 2))
    v[:n] = dst
    cx, cy = np.linalg.solve(L, v[:, 0]), np.linalg.solve(L, v[:, 1])
    return dict(_base(_capi.OPD_FLOOR_TPS, floormap, zones, allow_overlap, distortion), points=src, tps_w=np.stack([cx[:n], cy[:n]], 1),
                tps_affine=np.concatenate([cx[n:], cy[n:]]))


def make_config(model: dict):
    """(opd_floor_config, arrays it points into) of a model."""
    z = model["zones"]
    arr = lambda key, dt, shape: np.ascontiguousarray(np.asarray(model.get(key, ()), dt).reshape(shape))
    keep = [arr("points", np.float64, (-1, 2)), arr("triangles", np.int32, (-1, 3)), arr("affine", np.float64, (-1, 6)), arr("tps_w", np.float64, (-1, 2)),
            np.ascontiguousarray(np.concatenate(z)) if z else np.zeros((0, 2)), np.cumsum([0] + [len(p) for p in z]).astype(np.int32),
            np.ascontiguousarray(np.asarray(model.get("priority", np.full(len(z), np.nan)), np.float64))]
    fm, dist = model["fm"], model.get("dist")
    cfg = _capi.OpdFloorConfig(method=int(model["method"]), n_points=len(keep[0]), n_triangles=len(keep[1]), n_zones=len(z), has_distortion=int(dist is not None),
                               allow_overlap=int(bool(model["allow_overlap"])), width_px=int(fm[0]), height_px=int(fm[1]),
                               scale_x_mm_per_px=float(fm[2]), scale_y_mm_per_px=float(fm[3]))
    cfg.H[:] = np.asarray(model.get("H", np.eye(3)), np.float64).reshape(9).tolist()
    cfg.tps_affine[:] = np.asarray(model.get("tps_affine", np.zeros(6)), np.float64).reshape(6).tolist()
    if dist is not None:
        cfg.intrinsics[:] = [float(v) for v in dist[:4]]
        cfg.distortion[:] = [float(v) for v in dist[4:]]
    ptr = lambda a: a.ctypes.data if a.size else None
    cfg.points, cfg.triangles, cfg.affine, cfg.tps_weights, cfg.zone_vertices = (ptr(a) for a in keep[:5])
    cfg.zone_offsets, cfg.zone_priority = keep[5].ctypes.data, ptr(keep[6])
    return cfg, keep


class HipFloorMapper:
    """Transformer + ``ZoneClassifier`` of one camera, on one device.  Build it with ``homography``, ``piecewise_affine``,
    ``thin_plate_spline`` or ``from_config``."""

    REC_DTYPE = REC_DTYPE

    def __init__(self, model: dict, device: int = 0):
        self.model = model
        self.device = int(device)
        self.method = SUPPORTED_METHODS[int(model["method"])]
        self.zone_ids: List[str] = list(model.get("zone_ids") or [f"zone_{i}" for i in range(len(model["zones"]))])
        self.allow_overlap = bool(model["allow_overlap"])
        self._lib = _capi.load_library()
        cfg, _keep = make_config(model)
        handle = C.c_void_p()
        _capi.check(self._lib.opd_floor_create(C.byref(cfg), self.device, C.byref(handle)), "opd_floor_create")
        self._handle: Optional[C.c_void_p] = handle

    # ---- constructors ----------------------------------------------------------------------------------------------------------------
    @classmethod
    def homography(cls, H, floormap, zones, allow_overlap: bool = False, device: int = 0) -> "HipFloorMapper":
        return cls(model_homography(H, floormap, zones, allow_overlap), device)

    @classmethod
    def piecewise_affine(cls, src, dst, floormap, zones, simplices=None, distortion=None, allow_overlap: bool = False, device: int = 0) -> "HipFloorMapper":
        return cls(model_piecewise_affine(src, dst, floormap, zones, simplices, distortion, allow_overlap), device)

    @classmethod
    def thin_plate_spline(cls, src, dst, floormap, zones, regularization: float = 0.0, distortion=None, allow_overlap: bool = False,
                          device: int = 0) -> "HipFloorMapper":
        return cls(model_thin_plate_spline(src, dst, floormap, zones, regularization, distortion, allow_overlap), device)

    @classmethod
    def from_config(cls, cfg: dict, device: int = 0) -> "HipFloorMapper":
        return cls(model_from_config(cfg), device)

    # ---- the device calls --------------------------------------------------------------------------------------------------------------
    def _require(self) -> C.c_void_p:
        if self._handle is None:
            raise RuntimeError("this HipFloorMapper is closed")
        return self._handle

    def transform_records(self, bboxes) -> np.ndarray:
        """``opd_floor_transform``: [n] records (REC_DTYPE) of [n][4] (x, y, w, h) boxes, handed on as float32."""
        b = np.ascontiguousarray(np.asarray(bboxes, dtype=np.float32).reshape(-1, 4))
        out = np.zeros(len(b), REC_DTYPE)
        if len(b):
            _capi.check(self._lib.opd_floor_transform(self._require(), b.ctypes.data, len(b), _capi.OPD_MEM_HOST, out.ctypes.data), "opd_floor_transform")
        return out

    def _result(self, r):
        px, mm = (float(r["px"][0]), float(r["px"][1])), (float(r["mm"][0]), float(r["mm"][1]))
        valid, within = bool(r["flags"] & _capi.OPD_FLOOR_VALID), bool(r["flags"] & _capi.OPD_FLOOR_WITHIN)
        if self.method == "homography":
            return TransformResult(floor_coords_px=px, floor_coords_mm=mm, is_valid=valid, is_within_bounds=within)
        return PWATransformResult(floor_coords_px=px, floor_coords_mm=mm, is_valid=valid, is_within_bounds=within, triangle_index=int(r["triangle"]),
                                  is_extrapolated=bool(r["flags"] & _capi.OPD_FLOOR_EXTRAPOLATED))

    def transform_batch(self, bboxes: Sequence[Tuple[float, float, float, float]]) -> list:
        return [self._result(r) for r in self.transform_records(bboxes)] if len(bboxes) else []

    def transform_pixel(self, image_point: Tuple[float, float]):
        p = np.asarray([image_point[0], image_point[1]], np.float64)
        out = np.zeros(1, REC_DTYPE)
        _capi.check(self._lib.opd_floor_transform_points(self._require(), p.ctypes.data, 1, out.ctypes.data), "opd_floor_transform_points")
        return self._result(out[0])

    def _ids(self, mask: int) -> List[str]:
        return [zid for z, zid in enumerate(self.zone_ids) if (int(mask) >> z) & 1]

    def classify_batch(self, floor_points: Sequence[Tuple[float, float]]) -> List[List[str]]:
        p = np.ascontiguousarray(np.asarray(floor_points, np.float64).reshape(-1, 2))
        masks = np.zeros(len(p), np.uint64)
        if len(p):
            _capi.check(self._lib.opd_floor_classify(self._require(), p.ctypes.data, len(p), masks.ctypes.data), "opd_floor_classify")
        return [self._ids(m) for m in masks]

    def classify(self, floor_point: Tuple[float, float]) -> List[str]:
        return self.classify_batch([floor_point])[0]

    # ---- Phase 3 on detections -----------------------------------------------------------------------------------------------------
    def _fill(self, det: Detection, r) -> None:
        """``_apply_transform_result`` plus the zone step of ``TransformPhase.execute`` for one record."""
        if r["flags"] & _capi.OPD_FLOOR_VALID:
            det.floor_coords = (float(r["px"][0]), float(r["px"][1]))
            det.floor_coords_mm = (float(r["mm"][0]), float(r["mm"][1]))
            if det.bbox:
                x, y, w, h = det.bbox
                det.camera_coords = (x + w / 2.0, y + h)
            det.zone_ids = self._ids(r["zone_mask"])
        else:
            det.floor_coords = None
            det.floor_coords_mm = None
            det.zone_ids = []

    def apply(self, detections: Sequence[Detection]) -> Sequence[Detection]:
        """Fill ``floor_coords``, ``floor_coords_mm``, ``camera_coords`` and ``zone_ids`` of every detection, in place."""
        if len(detections):
            for det, r in zip(detections, self.transform_records([d.bbox for d in detections])):
                self._fill(det, r)
        return detections

    @staticmethod
    def zone_counts(detections: Sequence[Detection]) -> Dict[str, int]:
        """``Aggregator.get_zone_counts`` (src/aggregation/aggregator.py:52-75)."""
        counts: Dict[str, int] = {}
        for det in detections:
            for zid in (det.zone_ids if det.zone_ids else ["unclassified"]):
                counts[zid] = counts.get(zid, 0) + 1
        return counts

    def info(self) -> dict:
        info = _capi.OpdFloorModelInfo()
        _capi.check(self._lib.opd_floor_info(self._require(), C.byref(info)), "opd_floor_info")
        return {name: int(getattr(info, name)) for name, _ in _capi.OpdFloorModelInfo._fields_}

    def close(self) -> None:
        if self._handle is not None:
            self._lib.opd_floor_destroy(self._handle)
            self._handle = None

    def __del__(self):  # pragma: no cover - best effort
        try:
            self.close()
        except Exception:
            pass


def model_from_config(cfg: dict) -> dict:
    """The keys ``TransformPhase.initialize`` reads, with its defaults and fall-backs: an unknown method falls back to the homography,
    distortion is read for piecewise_affine / thin_plate_spline only and dropped when disabled or all-zero, ``allow_overlap`` is False."""
    transform = cfg.get("transform", {}) or {}
    method = transform.get("method", "homography")
    if method not in SUPPORTED_METHODS:
        logger.warning(f"Unknown transform method '{method}', falling back to 'homography'")
        method = "homography"
    zones = cfg.get("zones", []) or []
    floormap = cfg.get("floormap", {}) or {}
    if method == "homography":
        matrix = (cfg.get("homography", {}) or {}).get("matrix")
        if matrix is None:
            raise ValueError("homography.matrix is not set")
        return model_homography(matrix, floormap, zones, allow_overlap=False)
    distortion = None
    d = transform.get("lens_distortion", {}) or {}
    if d.get("enabled", False):
        focal = (cfg.get("camera_params", {}) or {}).get("focal_length", 1250.0)
        distortion = [float(d.get("focal_length_x", focal)), float(d.get("focal_length_y", focal)), float(d.get("center_x", 640.0)), float(d.get("center_y", 360.0)),
                      float(d.get("k1", 0.0)), float(d.get("k2", 0.0)), float(d.get("p1", 0.0)), float(d.get("p2", 0.0)), float(d.get("k3", 0.0))]
    path = (cfg.get("calibration", {}) or {}).get("correspondence_file")
    if not path:
        raise ValueError(f"{method} needs calibration.correspondence_file")
    with open(path, encoding="utf-8") as f:
        points = json.load(f).get("point_correspondences", [])
    src, dst = [p["src_point"] for p in points], [p["dst_point"] for p in points]
    if method == "piecewise_affine":
        return model_piecewise_affine(src, dst, floormap, zones, distortion=distortion)
    return model_thin_plate_spline(src, dst, floormap, zones, regularization=0.0, distortion=distortion)
