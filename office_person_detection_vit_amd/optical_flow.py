"""``HipOpticalFlowTracker``: the reference's ``OpticalFlowTracker`` (src/tracking/lightweight_tracker.py:57-208) on the device.

Same constructor, attributes and methods; gray conversion, pyramid and pyramidal Lucas-Kanade run in ``csrc/kernels_flow.hip`` behind
the ``opd_flow_*`` calls of ``include/opd_detr.h``.  The reference's ``LightweightTracker`` can keep its Kalman and IoU logic and take
this class as its ``of_tracker``; ``HipLightweightTracker`` (lightweight_tracker.py) replaces the whole of it.  The previous frame lives on the device as a gray pyramid (there is no ``prev_gray`` array here)."""

from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _capi

TERM_CRITERIA_COUNT, TERM_CRITERIA_EPS = 1, 2   # cv2's values, so that lk_params reads like the reference's


class HipOpticalFlowTracker:
    def __init__(self, max_corners: int = 100, quality_level: float = 0.3, min_distance: float = 7.0, block_size: int = 7, *,
                 device: int = 0):
        # the corner-detector arguments are stored and unused, as in the reference (its points are the box centres)
        self.max_corners = max_corners
        self.quality_level = quality_level
        self.min_distance = min_distance
        self.block_size = block_size
        self.device = device
        self.lk_params = {"winSize": (21, 21), "maxLevel": 3, "criteria": (TERM_CRITERIA_EPS | TERM_CRITERIA_COUNT, 30, 0.01)}
        self.prev_points: Optional[np.ndarray] = None   # (N, 1, 2) float32
        self.prev_track_ids: List[int] = []
        self._has_reference = False
        self._handle: Optional[C.c_void_p] = None
        self._key = None

    # ---- the handle: created for the first frame's size, again when the size, the parameters or the point count outgrow it ----------
    def _params(self):
        win, level, (_, iters, eps) = self.lk_params["winSize"], self.lk_params["maxLevel"], self.lk_params["criteria"]
        if win[0] != win[1]:
            raise ValueError(f"winSize must be square, got {win}")
        return int(win[0]), int(level), int(iters), float(eps)

    def _ensure_handle(self, h: int, w: int, n: int) -> None:
        params = self._params()
        win, level, iters, eps = params
        # validated before anything is given up: a bad value leaves the handle and its reference as they were.  cv2 takes maxLevel = 0
        # (no pyramid) and epsilon = 0; the C-ABI reads a zero field as the reference's default, so neither can be asked for here
        if level < 1 or eps <= 0:
            raise ValueError("maxLevel must be at least 1 and the criteria's epsilon positive (the C-ABI reads a zero as its default)")
        if self._handle is not None and self._key[:3] == (h, w, params) and n <= self._key[3]:
            return
        lib = _capi.load_library()
        self.close()
        capacity = max(n, int(self.max_corners), 1)
        cfg = _capi.OpdFlowConfig(max_h=h, max_w=w, max_points=capacity, win=win, max_level=level, max_iter=iters, epsilon=eps)
        handle = C.c_void_p()
        _capi.check(lib.opd_flow_create(C.byref(cfg), int(self.device), C.byref(handle)), "opd_flow_create")
        self._handle, self._key = handle, (h, w, params, capacity)

    @staticmethod
    def _frame(frame):
        """(pointer, mem_kind, h, w, keep-alive) of a BGR uint8 [h][w][3] frame: a numpy array, or a torch device tensor read in place
        (work queued on the tensor's current stream is waited for first; a tensor written on another stream is the caller's to finish)."""
        if hasattr(frame, "data_ptr") and getattr(frame, "is_cuda", False):
            if tuple(frame.shape[2:]) != (3,) or frame.dim() != 3 or frame.element_size() != 1 or not frame.is_contiguous():
                raise ValueError("a device frame must be a contiguous uint8 [h][w][3] tensor")
            # the handle's stream is not ordered after the stream that wrote the tensor: wait for that one (sharding.py does the same)
            import torch
            torch.cuda.current_stream(frame.device).synchronize()
            return C.c_void_p(int(frame.data_ptr())), _capi.OPD_MEM_DEVICE, int(frame.shape[0]), int(frame.shape[1]), frame
        arr = np.ascontiguousarray(frame)
        if arr.dtype != np.uint8 or arr.ndim != 3 or arr.shape[2] != 3:
            raise ValueError(f"a frame must be uint8 [h][w][3] BGR, got {arr.dtype} {arr.shape}")
        return C.c_void_p(arr.ctypes.data), _capi.OPD_MEM_HOST, arr.shape[0], arr.shape[1], arr

    # ---- the reference's surface -----------------------------------------------------------------------------------------------------
    def initialize(self, frame, detections: Sequence) -> None:
        """Track the box centres of the detections that carry a ``track_id``, from this frame on."""
        points, track_ids = [], []
        for det in detections:
            if det.track_id is not None:
                x, y, w, h = det.bbox
                points.append([x + w / 2, y + h / 2])
                track_ids.append(det.track_id)
        ptr, kind, h, w, _keep = self._frame(frame)
        self._ensure_handle(h, w, len(points))
        self._has_reference = False
        _capi.check(_capi.load_library().opd_flow_set_reference(self._handle, ptr, kind, h, w), "opd_flow_set_reference")
        self._has_reference = True
        if points:
            self.prev_points = np.array(points, dtype=np.float32).reshape(-1, 1, 2)
            self.prev_track_ids = track_ids
        else:
            self.prev_points = None
            self.prev_track_ids = []

    def track(self, frame) -> Dict[int, np.ndarray]:
        """track_id -> position (x, y) in ``frame`` of every point that could be followed; the others leave the state."""
        if not self._has_reference or self.prev_points is None or len(self.prev_points) == 0:
            return {}
        ptr, kind, h, w, _keep = self._frame(frame)
        if self._key is None or self._key[:3] != (h, w, self._params()):
            raise RuntimeError("frame size or lk_params changed since initialize(): call initialize() again")
        pts = np.ascontiguousarray(self.prev_points.reshape(-1, 2), dtype=np.float32)
        nxt = np.empty_like(pts)
        status = np.empty(len(pts), np.uint8)
        _capi.check(_capi.load_library().opd_flow_track(self._handle, ptr, kind, h, w, pts.ctypes.data_as(C.c_void_p), len(pts),
                                                        nxt.ctypes.data_as(C.c_void_p), status.ctypes.data_as(C.c_void_p)), "opd_flow_track")
        good = np.flatnonzero(status == 1)
        tracked = {self.prev_track_ids[i]: nxt[i].copy() for i in good}
        if len(good):
            self.prev_points = nxt[good].reshape(-1, 1, 2)
            self.prev_track_ids = [self.prev_track_ids[i] for i in good]
        else:
            self.prev_points = None
            self.prev_track_ids = []
        return tracked

    def reset(self) -> None:
        self.prev_points = None
        self.prev_track_ids = []
        self._has_reference = False

    def close(self) -> None:
        """Free the device buffers (also done when the object is collected)."""
        if self._handle is not None:
            _capi.load_library().opd_flow_destroy(self._handle)
        self._handle, self._key, self._has_reference = None, None, False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
