"""High-resolution tiled detection (BASELINE.json configs[4]: a 4K office frame -> 2 x 2 tiles of 1080p, batched through the
detector, per-tile detections gathered and merged on the orchestrator).

The reference has no tiling mode; this is the workload the benchmark contract names, built from the path's own pieces:
tiles are ordinary frames for ``detect_batch`` (device-side resize, frame sharding over ranks when the wrapped detector is a
``ShardedDetector``) and tile boxes are shifted back into frame coordinates.

Seams.  A body cut by a tile edge gives two partial boxes whose IoU is near zero, so IoU-NMS alone would count it twice.
Therefore (a) neighbouring tiles OVERLAP (``overlap`` = fraction of the base tile each interior edge is pushed into the
neighbour; default 1/8, i.e. 240 px of a 1920-px tile, more than a standing person's width in a 4K office view), so a body
narrower than the band is seen whole by at least one tile; and (b) the merge is a greedy non-maximum MERGE: in descending
score order a box is dropped when its IoU with a kept box exceeds ``nms_threshold`` (the per-frame path's rule), and when it
comes from a different tile than a kept box, one of the two is cut by an interior tile edge and their intersection covers more
than ``merge_threshold`` of the smaller box, the kept box grows to their union (the two parts of one body).  ``overlap=0``
with ``tile_sizes=None`` is the plain shift + IoU-NMS of round 1."""

from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

from .data_models import Detection

DEFAULT_OVERLAP = 0.125


def tile_grid(height: int, width: int, rows: int = 2, cols: int = 2, overlap: float = 0.0) -> List[Tuple[int, int, int, int]]:
    """(y0, x0, h, w) of a rows x cols grid covering the frame; the last row / column of the base grid takes the remainder and
    every interior edge is moved ``overlap`` x (base tile size) into the neighbouring tile."""
    if rows < 1 or cols < 1 or height < rows or width < cols:
        raise ValueError("tile grid does not fit the frame")
    if not 0.0 <= overlap < 0.5:
        raise ValueError("overlap must be in [0, 0.5)")
    th, tw = height // rows, width // cols
    oy, ox = int(round(th * overlap)), int(round(tw * overlap))
    out = []
    for r in range(rows):
        for c in range(cols):
            y0, x0 = r * th, c * tw
            y1 = height if r == rows - 1 else y0 + th
            x1 = width if c == cols - 1 else x0 + tw
            y0, x0, y1, x1 = max(0, y0 - oy), max(0, x0 - ox), min(height, y1 + oy), min(width, x1 + ox)
            out.append((y0, x0, y1 - y0, x1 - x0))
    return out


def split_tiles(frame: np.ndarray, rows: int = 2, cols: int = 2, overlap: float = 0.0):
    """Contiguous tile copies (the detector requires contiguous uint8 HxWx3 frames) and their (y0, x0) origins."""
    grid = tile_grid(frame.shape[0], frame.shape[1], rows, cols, overlap)
    return [np.ascontiguousarray(frame[y:y + h, x:x + w]) for y, x, h, w in grid], [(y, x) for y, x, _, _ in grid]


def _iou_iomin(a, b) -> Tuple[float, float]:
    iw = min(a[2], b[2]) - max(a[0], b[0])
    ih = min(a[3], b[3]) - max(a[1], b[1])
    if iw <= 0 or ih <= 0:
        return 0.0, 0.0
    inter = iw * ih
    aa, ab = max(0.0, a[2] - a[0]) * max(0.0, a[3] - a[1]), max(0.0, b[2] - b[0]) * max(0.0, b[3] - b[1])
    union, small = aa + ab - inter, min(aa, ab)
    return (inter / union if union > 0 else 0.0), (inter / small if small > 0 else 0.0)


def merge_tile_detections(tile_dets: Sequence[Sequence[Detection]], origins: Sequence[Tuple[int, int]],
                          nms_threshold: float = 0.4, tile_sizes: Optional[Sequence[Tuple[int, int]]] = None,
                          frame_size: Optional[Tuple[int, int]] = None, merge_threshold: float = 0.5,
                          edge_tolerance: float = 0.01) -> List[Detection]:
    """Tile-local detections -> frame coordinates, then the greedy merge described in the module docstring.

    ``tile_sizes`` ((h, w) per tile) and ``frame_size`` ((H, W)) tell which box sides are cut by an INTERIOR tile edge (within
    ``edge_tolerance`` x tile size of it); without them no box counts as cut and the merge is plain IoU-NMS.
    ``query_index`` is kept per tile; ``camera_coords`` (foot point) is recomputed in frame coordinates."""
    if len(tile_dets) != len(origins) or (tile_sizes is not None and len(tile_sizes) != len(origins)):
        raise ValueError("one origin (and size) per tile is required")
    cands = []   # [xyxy, score, tile, cut, detection]
    for t, (dets, (y0, x0)) in enumerate(zip(tile_dets, origins)):
        for d in dets:
            x, y, w, h = d.bbox
            box = [x + x0, y + y0, x + x0 + w, y + y0 + h]
            cut = False
            if tile_sizes is not None and frame_size is not None:
                th, tw = tile_sizes[t]
                ty, tx = edge_tolerance * th, edge_tolerance * tw
                cut = ((x0 > 0 and x <= tx) or (x0 + tw < frame_size[1] and x + w >= tw - tx) or
                       (y0 > 0 and y <= ty) or (y0 + th < frame_size[0] and y + h >= th - ty))
            cands.append([box, float(d.confidence), t, cut, d])
    cands.sort(key=lambda c: -c[1])   # stable: ties keep tile / query order
    kept: List[list] = []
    for c in cands:
        absorbed = False
        if nms_threshold < 1.0:
            for k in kept:
                iou, iomin = _iou_iomin(c[0], k[0])
                if c[2] != k[2] and (c[3] or k[3]) and iomin > merge_threshold:   # two parts of one body: checked first, the
                    k[0] = [min(k[0][0], c[0][0]), min(k[0][1], c[0][1]), max(k[0][2], c[0][2]), max(k[0][3], c[0][3])]   # parts' IoU may be high too
                    k[3] = k[3] and c[3]   # a part that was not cut completes the body
                    absorbed = True
                elif iou > nms_threshold:
                    absorbed = True
                if absorbed:
                    break
        if not absorbed:
            kept.append(c)
    out = []
    for box, score, _, _, d in kept:
        bbox = (box[0], box[1], box[2] - box[0], box[3] - box[1])
        out.append(Detection(bbox=bbox, confidence=d.confidence, class_id=d.class_id, class_name=d.class_name,
                             camera_coords=(bbox[0] + bbox[2] / 2, bbox[1] + bbox[3]), features=d.features, query_index=d.query_index))
    return out


class TiledDetector:
    """``detect`` / ``detect_batch`` on frames that are cut into ``rows x cols`` overlapping tiles first.  ``detector`` is
    anything with ``detect_batch`` (a loaded ``HipDetrDetector`` or a ``ShardedDetector``).

    ``native=True``: a frame is ONE call of the wrapped detector's ``detect_tiled`` (``HipDetrDetector``: the frame is uploaded once, its
    tiles are cut and resampled on the device and the merge below runs there in a kernel, the same lists field for field); a wrapped
    detector without ``detect_tiled`` is refused, there is no silent fallback to the host path.

    ``mixed_sizes=True`` (with ``native=True``): a grid whose tiles differ in size (interior tiles at the default overlap: 2 x 3, 3 x 3, ...; a
    frame side that does not divide) goes through the wrapped detector's ``detect_tiled_ragged`` instead of being refused: every tile at its
    own model size inside one canvas, one ragged forward, the same lists field for field.  A grid of one size takes the calls it always took.
    ``features="reid"`` on such a grid goes to ``detect_tiled_ragged_reid`` where the wrapped detector has it, else the Re-ID rows are a separate
    call on the merged detections.

    ``detect_and_track_hybrid`` / ``track_hybrid_batch`` take a ``HipLightweightTracker``: the reference's hybrid mode on tiled frames, inside the
    wrapped detector's tiled call where that is possible."""

    def __init__(self, detector, rows: int = 2, cols: int = 2, nms_threshold: float = 0.4, overlap: float = DEFAULT_OVERLAP,
                 merge_threshold: float = 0.5, native: bool = False, mixed_sizes: bool = False):
        self.detector, self.rows, self.cols, self.nms_threshold = detector, rows, cols, nms_threshold
        self.overlap, self.merge_threshold, self.native, self.mixed_sizes = overlap, merge_threshold, bool(native), bool(mixed_sizes)

    def _need_detect_tiled(self, staged: bool = False) -> None:
        if not hasattr(self.detector, "detect_tiled") or (staged and not hasattr(self.detector, "detect_tiled_stages")):
            raise ValueError("native=True needs a detector with detect_tiled (a HipDetrDetector); "
                             f"{type(self.detector).__name__} has none")

    def _native_grid(self, frames: Sequence[np.ndarray], staged: bool = False):
        self._need_detect_tiled(staged)
        if len({(f.shape[0], f.shape[1]) for f in frames}) != 1:
            raise ValueError("native=True takes frames of one size")
        return tile_grid(frames[0].shape[0], frames[0].shape[1], self.rows, self.cols, self.overlap)

    def _mixed(self, grid) -> bool:
        """Whether ``grid`` goes through ``detect_tiled_ragged``: ``mixed_sizes=True`` and tiles of more than one size (without the keyword the
        wrapped detector's calls refuse such a grid, as they always did)."""
        if not self.mixed_sizes or len({(t[2], t[3]) for t in grid}) == 1:
            return False
        if not hasattr(self.detector, "detect_tiled_ragged"):
            raise ValueError(f"mixed_sizes=True needs a detector with detect_tiled_ragged (a HipDetrDetector); {type(self.detector).__name__} has none")
        return True

    def _staged_call(self, grid):
        """The wrapped detector's tiled method that runs the feature and track stages inside the call for ``grid``."""
        return self.detector.detect_tiled_ragged if self._mixed(grid) else self.detector.detect_tiled_stages

    def detect_batch(self, frames: Sequence[np.ndarray], floor_map=None) -> List[List[Detection]]:
        """``floor_map``: a ``HipFloorMapper``; the merged detections come back with its four fields filled (``native=True``: inside the call)."""
        if self.native:
            self._need_detect_tiled()
            if len(frames) == 0:
                return []
            grid = self._native_grid(frames)
            if self._mixed(grid):
                return self.detector.detect_tiled_ragged(frames, grid, self.nms_threshold, self.merge_threshold, floor_map=floor_map)
            if floor_map is None:
                return self.detector.detect_tiled(frames, grid, self.nms_threshold, self.merge_threshold)
            self._need_detect_tiled(staged=True)
            return self.detector.detect_tiled_stages(frames, grid, self.nms_threshold, self.merge_threshold, floor_map=floor_map)
        tiles, origins, sizes = [], [], []
        for f in frames:
            t, o = split_tiles(f, self.rows, self.cols, self.overlap)
            tiles.extend(t)
            origins.append(o)
            sizes.append([(x.shape[0], x.shape[1]) for x in t])
        per_tile = self.detector.detect_batch(tiles) if tiles else []
        n = self.rows * self.cols
        out = [merge_tile_detections(per_tile[i * n:(i + 1) * n], origins[i], self.nms_threshold, sizes[i],
                                     (frames[i].shape[0], frames[i].shape[1]), self.merge_threshold) for i in range(len(frames))]
        if floor_map is not None:
            for dets in out:
                floor_map.apply(dets)
        return out

    def detect(self, frame: np.ndarray, floor_map=None) -> List[Detection]:
        return self.detect_batch([frame], floor_map=floor_map)[0] if floor_map is not None else self.detect_batch([frame])[0]

    def _check_features(self, features: Optional[str], reid, allow_none: bool) -> None:
        if features == "encoder":
            raise ValueError("features='encoder' does not exist for tiled detection: a box merged from two tiles' maps has no encoder row")
        if features not in (("color", "reid") + ((None,) if allow_none else ())):
            raise ValueError(f"features must be {'None, ' if allow_none else ''}'color' or 'reid', got {features!r}")
        if features == "reid" and reid is None:
            raise ValueError("features='reid' needs reid= a loaded HipReIDExtractor or HipOSNetReIDExtractor")

    def _host_features(self, frame: np.ndarray, dets: List[Detection], features: Optional[str], reid) -> np.ndarray:
        """The separate feature call on merged detections: the colour histograms of the wrapped detector, or the rows of ``reid``."""
        if features is None or not dets:
            return np.array([])
        rows = reid.extract_features(frame, [d.bbox for d in dets]) if features == "reid" else self.detector.extract_color_features(frame, dets)
        for det, row in zip(dets, rows):
            det.features = row
        return rows

    def _native_reid(self, features: Optional[str], reid) -> bool:
        """Whether the Re-ID rows can come from inside the wrapped detector's tiled call (``detect_tiled_reid``): ``native=True``, a detector with
        that method, and ``reid`` a loaded ``HipReIDExtractor`` / ``HipOSNetReIDExtractor``."""
        if not (self.native and features == "reid" and hasattr(self.detector, "detect_tiled_reid")):
            return False
        from .reid import _ReIDExtractorBase
        return isinstance(reid, _ReIDExtractorBase) and reid.is_loaded

    def _reid_call(self, frame: np.ndarray, features: Optional[str], reid):
        """``(method, grid)`` of the wrapped detector's tiled call that brings the Re-ID rows itself, or ``(None, None)``: ``detect_tiled_reid`` for
        a grid of one size, ``detect_tiled_ragged_reid`` for a mixed grid under ``mixed_sizes=True`` where the detector has it."""
        if not self._native_reid(features, reid):
            return None, None
        grid = self._native_grid([frame])
        if not self._mixed(grid):
            return self.detector.detect_tiled_reid, grid
        if hasattr(self.detector, "detect_tiled_ragged_reid"):
            return self.detector.detect_tiled_ragged_reid, grid
        return None, None

    def detect_with_features(self, frame: np.ndarray, features: str = "color", reid=None, reid_slots: int = 32) -> Tuple[List[Detection], np.ndarray]:
        """Merged detections + their (N, 256) colour-histogram rows (``features="reid"``: the (N, 512) rows of ``reid``), assigned to
        ``det.features``.  ``native=True`` with colour: inside the wrapped detector's one tiled call (``detect_tiled_stages``); with a loaded
        ``HipReIDExtractor`` / ``HipOSNetReIDExtractor``: inside ``detect_tiled_reid``, for the first ``reid_slots`` merged records."""
        self._check_features(features, reid, allow_none=False)
        call, grid = self._reid_call(frame, features, reid)
        if call is not None:
            dets = call([frame], grid, reid, self.nms_threshold, self.merge_threshold, reid_slots=reid_slots)[0]
            return dets, (np.stack([d.features for d in dets]) if dets else np.array([]))
        if self.native and features == "color":
            grid = self._native_grid([frame], staged=True)   # (refuses a detector without detect_tiled)
            call = self._staged_call(grid)
            dets = call([frame], grid, self.nms_threshold, self.merge_threshold, features="color")[0]
            return dets, (np.stack([d.features for d in dets]) if dets else np.array([]))
        dets = self.detect(frame)
        return dets, self._host_features(frame, dets, features, reid)

    def detect_and_track(self, frame: np.ndarray, tracker, features: Optional[str] = "color", reid=None, reid_slots: int = 32) -> List[Detection]:
        """``detect_with_features(frame)`` then ``tracker.update(detections)``; ``native=True`` (colour rows, motion only, or the rows of a loaded
        ``HipReIDExtractor`` / ``HipOSNetReIDExtractor``): ONE tiled call with one host wait, the merged records and their rows entering ``tracker``
        where they lie.  Returns the detections that got an id."""
        self._check_features(features, reid, allow_none=True)
        call, grid = self._reid_call(frame, features, reid)
        if call is not None:
            dets = call([frame], grid, reid, self.nms_threshold, self.merge_threshold, reid_slots=reid_slots, trackers=[tracker])[0]
            return [d for d in dets if d.track_id is not None]
        if self.native and features != "reid":
            grid = self._native_grid([frame], staged=True)
            call = self._staged_call(grid)
            dets = call([frame], grid, self.nms_threshold, self.merge_threshold, features=features, trackers=[tracker])[0]
            return [d for d in dets if d.track_id is not None]
        dets = self.detect(frame)
        self._host_features(frame, dets, features, reid)
        return tracker.update(dets)

    def _native_hybrid(self, method: str, frames: Sequence[np.ndarray], lwt):
        """The grid when ``lwt`` (a ``HipLightweightTracker``) can enter the wrapped detector's tiled call ``method``, else None: ``native=True``, a
        detector with the method, the tracker on its device with room for ``tiles x queries`` records, and a grid of one size or ``mixed_sizes=True``."""
        if not (self.native and hasattr(self.detector, method)) or len(frames) == 0:
            return None
        if any(not isinstance(f, np.ndarray) for f in frames) or len({(f.shape[0], f.shape[1]) for f in frames}) != 1:
            return None
        grid = tile_grid(frames[0].shape[0], frames[0].shape[1], self.rows, self.cols, self.overlap)
        if len({(t[2], t[3]) for t in grid}) != 1 and not self.mixed_sizes:
            return None
        slots = len(grid) * int(getattr(self.detector, "num_queries", 0) or 0)
        if slots < 1 or getattr(lwt, "device", None) != getattr(self.detector, "device_ordinal", None) or getattr(lwt, "max_tracks", 0) < slots:
            return None
        return grid

    def detect_and_track_hybrid(self, frame: np.ndarray, lwt) -> List[Detection]:
        """``lwt.update_with_detections(frame, self.detect(frame))``, the detection frame of the reference's hybrid mode on a tiled frame;
        ``native=True``: ONE tiled call with one host wait (``detect_tiled_hybrid``), the merged records entering ``lwt`` where they lie and its
        gray pyramid built from the frame as uploaded.  Same ids and track states either way."""
        grid = self._native_hybrid("detect_tiled_hybrid", [frame], lwt)
        if grid is None:
            return lwt.update_with_detections(frame, self.detect(frame))
        return self.detector.detect_tiled_hybrid([frame], grid, [lwt], self.nms_threshold, self.merge_threshold)[0]

    def track_hybrid_batch(self, frames: Sequence[np.ndarray], lwt, key_frames: Sequence) -> list:
        """The reference's hybrid loop over consecutive tiled frames of one camera: a ``List[Detection]`` per key frame, a ``List[(track_id, bbox)]``
        per in-between frame (``lwt.interpolate``).  ``native=True``: runs of frames in one call each (``track_tiled_hybrid_batch``)."""
        frames, keys = list(frames), [bool(k) for k in key_frames]
        if len(keys) != len(frames):
            raise ValueError(f"{len(frames)} frames, {len(keys)} key flags")
        grid = self._native_hybrid("track_tiled_hybrid_batch", frames, lwt)
        if grid is None:
            return [lwt.update_with_detections(f, self.detect(f)) if k else lwt.interpolate(f) for f, k in zip(frames, keys)]
        return self.detector.track_tiled_hybrid_batch(frames, grid, lwt, keys, self.nms_threshold, self.merge_threshold)
