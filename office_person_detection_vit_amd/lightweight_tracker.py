"""``HipLightweightTracker``: the reference's ``LightweightTracker`` (src/tracking/lightweight_tracker.py:211-455) with every track number
on the device.

``update_with_detections`` is one ``opd_lwt_update`` and ``interpolate`` one ``opd_lwt_interpolate`` (``csrc/kernels_lwt.hip``,
``csrc/opd_lwt.cpp``): Kalman filters, IoU matching, ids, counters and the flow points live in the handle's device memory, the gray
pyramid and Lucas-Kanade launches of the flow handle run on the same stream, and each call waits for the device once.  What comes back is
what the reference returns: ids, and ``(track_id, bbox)`` pairs.  ``tracks`` reads the device state back on demand.
``interpolate_sequence`` runs up to 64 in-between frames behind one wait (``opd_lwt_interpolate_sequence``), and
``HipDetrDetector.detect_and_track_hybrid`` / ``track_hybrid_batch`` take the tracker inside the detect call, with the same results.  In
``TrackingPhase.initialize`` the swap is one line:

    self.lightweight_tracker = HipLightweightTracker(max_age=..., iou_threshold=..., use_optical_flow=...)"""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
import logging
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _capi
from .optical_flow import HipOpticalFlowTracker

logger = logging.getLogger(__name__)


@dataclass
class HipLightweightTrack:
    """What the reference's ``LightweightTrack`` shows, read back from the device (``features`` is kept on the host: the reference only
    stores it)."""

    track_id: int
    bbox: Tuple[float, float, float, float]
    center: np.ndarray
    age: int = 0
    time_since_update: int = 0
    hits: int = 1
    features: Optional[np.ndarray] = None


class HipLightweightTracker:
    def __init__(self, max_age: int = 30, iou_threshold: float = 0.3, use_optical_flow: bool = True, *, device: int = 0, max_tracks: int = 256):
        if not iou_threshold > 0:   # the reference's matching loop never ends for it: an all-zero matrix still passes `max < 0` as false
            raise ValueError(f"iou_threshold must be positive, got {iou_threshold}")
        if not max_age > 0:
            raise ValueError("max_age must be positive (a zero means 'the default' to the native library)")
        self.max_age, self.iou_threshold, self.use_optical_flow = int(max_age), float(iou_threshold), bool(use_optical_flow)
        self.device, self.max_tracks = int(device), int(max_tracks)
        self._lib = _capi.load_library()   # raises when the library was not built: there is no host fallback
        self._h = C.c_void_p()             # made by the first call: constructing a tracker touches no device, as the reference's does not
        self._key = None
        self._features: Dict[int, Optional[np.ndarray]] = {}
        logger.info("HipLightweightTracker initialized: max_age=%d, iou_threshold=%.2f, optical_flow=%s", max_age, iou_threshold, use_optical_flow)

    # ---- the handle: made for the first frame's size; a larger frame makes a new one, which starts without tracks -------------------
    def _ensure(self, h: int, w: int) -> None:
        if self._h and (not self.use_optical_flow or (h <= self._key[0] and w <= self._key[1])):
            return
        if self._h and self._info().n_tracks:
            raise RuntimeError(f"frame of {h} x {w} pixels exceeds the {self._key[0]} x {self._key[1]} the tracker was made for, and it holds tracks: reset() first")
        self.close()
        cfg = _capi.OpdLwtConfig(struct_size=C.sizeof(_capi.OpdLwtConfig), max_tracks=self.max_tracks, max_dets=self.max_tracks, max_age=self.max_age,
                                 use_optical_flow=int(self.use_optical_flow), iou_threshold=self.iou_threshold,
                                 flow=_capi.OpdFlowConfig(max_h=max(h, 1), max_w=max(w, 1), max_points=1))
        _capi.check(self._lib.opd_lwt_create(C.byref(cfg), self.device, C.byref(self._h)), "opd_lwt_create")
        self._key = (h, w)

    def _frame(self, frame):
        if not self.use_optical_flow:
            return None, _capi.OPD_MEM_HOST, 0, 0, None
        return HipOpticalFlowTracker._frame(frame)

    def _info(self):
        info = _capi.OpdLwtStatus()
        _capi.check(self._lib.opd_lwt_info(self._h, C.byref(info)), "opd_lwt_info")
        return info

    # ---- the reference's surface ----------------------------------------------------------------------------------------------------
    def update_with_detections(self, frame, detections: Sequence) -> Sequence:
        """Sets ``track_id`` on every detection in place and returns the list."""
        n = len(detections)
        boxes = np.array([d.bbox for d in detections], np.float32).reshape(n, 4)
        ptr, kind, h, w, _keep = self._frame(frame)
        self._ensure(h, w)
        ids = np.full(max(n, 1), -1, np.int32)
        _capi.check(self._lib.opd_lwt_update(self._h, ptr, kind, h, w, boxes.ctypes.data_as(C.c_void_p), n, ids.ctypes.data_as(C.c_void_p)), "opd_lwt_update")
        return self._adopt(detections, ids[:n].tolist())

    def _adopt(self, detections: Sequence, ids: Sequence[int]) -> Sequence:
        """The host half of a detection frame, behind ``opd_lwt_update`` or the fused detect call (``detect_and_track_hybrid``)."""
        for det, tid in zip(detections, ids):
            det.track_id = tid
            if det.features is not None:
                self._features.setdefault(tid, det.features)   # (a track keeps the feature it was created with)
        if len(self._features) > self._info().n_tracks:   # tracks have died: forget their features (one read-back, only then); never more than max_tracks stay
            self._prune(self._records())
        return detections

    def interpolate(self, frame) -> List[Tuple[int, Tuple[float, float, float, float]]]:
        """``[(track_id, (x, y, w, h))]`` of every live track: moved with its flow point, or to its Kalman prediction."""
        if not self._h:
            return []
        ptr, kind, h, w, _keep = self._frame(frame)
        cap = self._info().n_tracks
        recs, n = (_capi.OpdLwtRec * max(cap, 1))(), C.c_int()
        _capi.check(self._lib.opd_lwt_interpolate(self._h, ptr, kind, h, w, recs, cap, C.byref(n)), "opd_lwt_interpolate")
        return [(int(recs[i].track_id), tuple(float(v) for v in recs[i].bbox)) for i in range(n.value)]

    SEQUENCE_MAX = 64   # frames of one opd_lwt_interpolate_sequence

    def interpolate_sequence(self, frames: Sequence) -> List[List[Tuple[int, Tuple[float, float, float, float]]]]:
        """What ``[self.interpolate(f) for f in frames]`` returns, bit for bit, with one host wait for every 64 frames (one
        ``opd_lwt_interpolate_sequence``) instead of one per frame.  With optical flow the frames share one size and lie all on the host or all
        on the device."""
        frames = list(frames)
        if not self._h:
            return [[] for _ in frames]
        out: list = []
        for k in range(0, len(frames), self.SEQUENCE_MAX):
            run = [self._frame(f) for f in frames[k:k + self.SEQUENCE_MAX]]
            if len({(kind, h, w) for _, kind, h, w, _ in run}) != 1:
                raise ValueError("interpolate_sequence: the frames must share one size and lie all on the host or all on the device")
            _, kind, h, w, _ = run[0]
            ptrs = (C.c_void_p * len(run))(*[r[0] for r in run]) if self.use_optical_flow else None
            cap = self.max_tracks
            recs, counts = (_capi.OpdLwtRec * (cap * len(run)))(), (C.c_int32 * len(run))()
            _capi.check(self._lib.opd_lwt_interpolate_sequence(self._h, ptrs, kind, len(run), h, w, recs, cap, counts), "opd_lwt_interpolate_sequence")
            for f in range(len(run)):
                out.append([(int(recs[f * cap + i].track_id), tuple(float(v) for v in recs[f * cap + i].bbox)) for i in range(counts[f])])
        return out

    def reset(self) -> None:
        if self._h:
            _capi.check(self._lib.opd_lwt_reset(self._h), "opd_lwt_reset")
        self._features = {}

    def get_active_tracks(self) -> List[HipLightweightTrack]:
        return [t for t in self.tracks if t.time_since_update == 0]

    @property
    def tracks(self) -> List[HipLightweightTrack]:
        if not self._h:
            return []
        recs = self._records()
        self._prune(recs)
        return [HipLightweightTrack(track_id=int(t.track_id), bbox=tuple(float(v) for v in t.bbox), center=np.array(list(t.center)), age=int(t.age),
                                    time_since_update=int(t.time_since_update), hits=int(t.hits), features=self._features.get(int(t.track_id)))
                for t in recs]

    def _records(self):
        n = C.c_int()
        _capi.check(self._lib.opd_lwt_get(self._h, None, 0, C.byref(n)), "opd_lwt_get")
        out = (_capi.OpdLwtTrack * max(n.value, 1))()
        _capi.check(self._lib.opd_lwt_get(self._h, out, n.value, C.byref(n)), "opd_lwt_get")
        return [out[i] for i in range(n.value)]

    def _prune(self, recs) -> None:
        alive = {int(t.track_id) for t in recs}
        self._features = {k: v for k, v in self._features.items() if k in alive}

    @property
    def next_id(self) -> int:
        return int(self._info().next_id) if self._h else 1

    def info(self):
        """The native handle's ``opd_lwt_status`` (tracks, next id, flow points, launches and host waits of the last call); None before the first call."""
        return self._info() if self._h else None

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.opd_lwt_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:   # interpreter shutdown
            pass
