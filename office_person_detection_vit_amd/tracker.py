"""``HipTracker``: the reference's ``Tracker`` (src/tracking/tracker.py) with the per-frame work on the device.

``update(detections)`` is one ``opd_track_update``: Kalman predict, the three cost matrices, the five association stages, Kalman update with
the re-update after an occlusion, new tracks and deletions (``csrc/kernels_track.hip``, ``csrc/opd_assoc.cpp``, ``csrc/opd_track.cpp``).
The Kalman state, the boxes and the feature history live on the device; what ``TrackingPhase`` and the exporters read of a track
(``track_id``, ``detection``, counters, ``trajectory``) is kept here on the host.  In ``TrackingPhase.initialize`` the swap is one line:

    self.tracker = HipTracker(max_age=..., min_hits=..., iou_threshold=..., appearance_weight=..., motion_weight=...)

One difference from the reference: a low-confidence detection never starts a track, also when no track is alive (the reference starts
one from every detection in that one case)."""

from __future__ import annotations

import ctypes as C
import re
from dataclasses import dataclass, field
import logging
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _capi
from .data_models import Detection

logger = logging.getLogger(__name__)


MAX_STREAM_TRACKERS = 64   # trackers of one streams call (the native TRACK_MAX_CAMERAS)


def plan_stream_calls(lengths: Sequence[int], max_batch: Optional[int] = None, max_trackers: int = MAX_STREAM_TRACKERS) -> List[List[Tuple[int, int, int]]]:
    """Cut the cameras' runs of ``lengths[c]`` frames into streams calls: a list of calls, each a list of ``(camera, start, stop)`` with at most
    ``max_batch`` frames (None: no limit) and at most ``max_trackers`` cameras in all.  Every frame is in exactly one call, a camera's frames keep
    their order across the calls, and a camera without frames is in none.  The policy: every call takes the cameras that still have frames, in
    camera order (at most ``max_trackers``, and no more than there is room for), and shares its room among them evenly, so that the cameras advance
    side by side and a call has as few steps as its frames allow; room a short camera leaves goes to the ones behind it."""
    if max_batch is not None and max_batch < 1:
        raise ValueError(f"max_batch must be at least 1, got {max_batch}")
    if not 1 <= max_trackers <= MAX_STREAM_TRACKERS:
        raise ValueError(f"max_trackers must be 1 .. {MAX_STREAM_TRACKERS}, got {max_trackers}")
    at = [0] * len(lengths)
    calls: List[List[Tuple[int, int, int]]] = []
    first = 0   # the camera a call starts with: round robin, so that no camera waits for the others to finish
    while any(at[c] < n for c, n in enumerate(lengths)):
        order = [c % len(lengths) for c in range(first, first + len(lengths))]
        cams = [c for c in order if at[c] < lengths[c]][:max_trackers if max_batch is None else min(max_trackers, max_batch)]
        room = sum(lengths[c] - at[c] for c in cams) if max_batch is None else max_batch
        call = []
        for i, c in enumerate(cams):
            take = lengths[c] - at[c] if max_batch is None else min(lengths[c] - at[c], max(1, room // (len(cams) - i)))
            call.append((c, at[c], at[c] + take))
            at[c] += take
            room -= take
        calls.append(sorted(call))
        first = (cams[-1] + 1) % len(lengths)
    return calls


@dataclass
class HipTrack:
    """What the reference's ``Track`` shows to its readers; the Kalman state is fetched from the device on demand."""

    track_id: int
    detection: Detection
    age: int = 1
    hits: int = 1
    time_since_update: int = 0
    trajectory: List[Tuple[float, float]] = field(default_factory=list)
    _owner: Optional["HipTracker"] = field(default=None, repr=False, compare=False)

    def is_confirmed(self, min_hits: int = 3) -> bool:
        return self.hits >= min_hits

    def is_tentative(self) -> bool:
        return not self.is_confirmed()

    def get_state(self) -> dict:
        x = self._owner._state_of(self.track_id) if self._owner is not None else [float("nan")] * 4
        return {"track_id": self.track_id, "position": [x[0], x[1]], "velocity": [x[2], x[3]], "age": self.age, "hits": self.hits,
                "time_since_update": self.time_since_update, "trajectory_length": len(self.trajectory)}


class HipTracker:
    def __init__(self, max_age: int = 30, min_hits: int = 3, iou_threshold: float = 0.3, appearance_weight: float = 0.7, motion_weight: float = 0.3,
                 max_position_distance: float = 150.0, high_conf_threshold: float = 0.5, *, feature_dim: int = 512, max_tracks: int = 256,
                 max_dets: int = 256, device: str = "hip:0"):
        if abs(appearance_weight + motion_weight - 1.0) > 1e-6:   # SimilarityCalculator.__init__
            raise ValueError(f"appearance_weight ({appearance_weight}) + motion_weight ({motion_weight}) must equal 1.0")
        for name, v in (("max_age", max_age), ("min_hits", min_hits), ("high_conf_threshold", high_conf_threshold)):
            if not v > 0:
                raise ValueError(f"{name} must be positive (a zero means 'the default' to the native library)")
        self.max_age, self.min_hits, self.iou_threshold = max_age, min_hits, iou_threshold
        self.appearance_weight, self.motion_weight = appearance_weight, motion_weight
        self.max_position_distance, self.high_conf_threshold = max_position_distance, high_conf_threshold
        self.feature_dim, self.max_tracks, self.max_dets = int(feature_dim), int(max_tracks), int(max_dets)
        self.device_ordinal = int(str(device).split(":")[1]) if ":" in str(device) else 0
        self.tracks: List[HipTrack] = []
        self.next_id = 1
        self._lib = _capi.load_library()   # raises when the library was not built: there is no host fallback
        self._h = C.c_void_p()   # made by the first update: constructing a tracker touches no device, as the reference's does not
        logger.info("HipTracker initialized: max_age=%s, min_hits=%s, high_conf_threshold=%s, feature_dim=%s", max_age, min_hits, high_conf_threshold, feature_dim)

    def _ensure(self) -> None:
        if self._h:
            return
        weights_default = self.appearance_weight == 0.7 and self.motion_weight == 0.3
        cfg = _capi.OpdTrackConfig(struct_size=C.sizeof(_capi.OpdTrackConfig), max_tracks=self.max_tracks, max_dets=self.max_dets, feature_dim=self.feature_dim,
                                   max_age=int(self.max_age), min_hits=int(self.min_hits), iou_threshold=float(self.iou_threshold),
                                   appearance_weight=0.0 if weights_default else float(self.appearance_weight),
                                   motion_weight=0.0 if weights_default else float(self.motion_weight),
                                   max_position_distance=float(self.max_position_distance) if self.max_position_distance > 0 else -1.0,
                                   high_conf_threshold=float(self.high_conf_threshold))
        _capi.check(self._lib.opd_track_create(C.byref(cfg), self.device_ordinal, C.byref(self._h)), "opd_track_create")

    # ---- the reference's surface ----------------------------------------------------------------------------------------------------
    def update(self, detections: List[Detection]) -> List[Detection]:
        """Sets ``track_id`` on the detections in place and returns those that have one."""
        n, D = len(detections), self.feature_dim
        boxes, foot, conf = np.zeros((n, 4), np.float32), np.zeros((n, 2), np.float32), np.zeros(n, np.float32)
        has = np.zeros(n, np.uint8)
        feats = None
        for j, det in enumerate(detections):
            if det.camera_coords is None:
                raise ValueError(f"detection {j} has no camera_coords: a track cannot be started or updated without a foot point")
            boxes[j], foot[j], conf[j] = det.bbox, det.camera_coords, det.confidence
            if det.features is not None:
                f = np.asarray(det.features, np.float32).reshape(-1)
                if f.shape[0] != D:
                    raise ValueError(f"detection {j} has a feature of width {f.shape[0]}, the tracker was made for {D}")
                if feats is None:
                    feats = np.zeros((n, D), np.float32)
                feats[j], has[j] = f, 1
        self._ensure()
        ids = np.full(max(n, 1), -1, np.int32)
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)   # noqa: E731
        rc = self._lib.opd_track_update(self._h, p(boxes), p(foot), p(conf), p(feats), p(has), _capi.OPD_MEM_HOST, n, p(ids))
        if rc != 0 and "counted as one without detections" in _capi.last_error():
            self._apply([], ids[:0])   # out of slots: the native side aged every track and matched none; the mirror follows before the error is raised
        _capi.check(rc, "opd_track_update")
        self._apply(detections, ids[:n])
        return [det for det in detections if det.track_id is not None]

    def update_sequence(self, detections_per_frame: List[List[Detection]]) -> List[List[Detection]]:
        """``[self.update(d) for d in detections_per_frame]`` as ONE ``opd_track_update_sequence``: every frame's detections go to the device
        once, the association runs there between the frames, and the host waits once.  Same ids, same track states.  In
        ``TrackingPhase.execute`` the loop over ``tracker.update`` becomes this one call.  Where a frame runs out of slots the frames before
        it are applied, that frame counts as one without detections, and the error is raised as ``update`` raises it."""
        frames = [list(d) for d in detections_per_frame]
        if not frames:
            return []
        D = self.feature_dim
        counts = np.array([len(f) for f in frames], np.int32)
        if counts.max() > self.max_dets:
            raise ValueError(f"a frame has {int(counts.max())} detections, the tracker was made for max_dets = {self.max_dets}")
        flat = [det for f in frames for det in f]
        n = len(flat)
        boxes, foot, conf = np.zeros((n, 4), np.float32), np.zeros((n, 2), np.float32), np.zeros(n, np.float32)
        has = np.zeros(n, np.uint8)
        feats = None
        for j, det in enumerate(flat):
            if det.camera_coords is None:
                raise ValueError(f"detection {j} has no camera_coords: a track cannot be started or updated without a foot point")
            boxes[j], foot[j], conf[j] = det.bbox, det.camera_coords, det.confidence
            if det.features is not None:
                f = np.asarray(det.features, np.float32).reshape(-1)
                if f.shape[0] != D:
                    raise ValueError(f"detection {j} has a feature of width {f.shape[0]}, the tracker was made for {D}")
                if feats is None:
                    feats = np.zeros((n, D), np.float32)
                feats[j], has[j] = f, 1
        self._ensure()
        ids, done = np.full(max(n, 1), -1, np.int32), C.c_int32(0)
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)   # noqa: E731
        rc = self._lib.opd_track_update_sequence(self._h, p(boxes), p(foot), p(conf), p(feats), p(has), _capi.OPD_MEM_HOST, p(counts), len(frames), p(ids),
                                                 C.byref(done))
        stopped = rc != 0 and "counted as one without detections" in _capi.last_error()
        if rc != 0 and not stopped:
            _capi.check(rc, "opd_track_update_sequence")
        return self._replay(frames, ids, done.value, rc, "opd_track_update_sequence")

    @staticmethod
    def update_streams(trackers: Sequence["HipTracker"], detections_per_camera: Sequence[List[List[Detection]]]) -> List[List[List[Detection]]]:
        """``[t.update_sequence(d) for t, d in zip(trackers, detections_per_camera)]`` with the cameras side by side on the device
        (``opd_track_update_streams``): one native call and one host wait for up to 64 cameras, as many steps as the longest camera has frames.
        Same ids, same track states.  In ``TrackingPhase.execute`` with several cameras, the loop over cameras and frames becomes this one call.
        Where a camera runs out of slots it stops as ``update_sequence`` does; every other camera runs to its end, then the error is raised."""
        trackers, per_camera = list(trackers), [[list(d) for d in cam] for cam in detections_per_camera]
        if len(trackers) != len(per_camera):
            raise ValueError(f"{len(trackers)} trackers for {len(per_camera)} cameras")
        if len({id(t) for t in trackers}) != len(trackers):
            raise ValueError("a tracker is named twice; a tracker follows one camera")
        for c, (t, cam) in enumerate(zip(trackers, per_camera)):
            if cam and max(len(f) for f in cam) > t.max_dets:
                raise ValueError(f"a frame of camera {c} has {max(len(f) for f in cam)} detections, its tracker was made for max_dets = {t.max_dets}")
        out: List[List[List[Detection]]] = [[] for _ in trackers]
        failed: Optional[RuntimeError] = None
        for call in plan_stream_calls([len(cam) for cam in per_camera]):
            cams = [trackers[c] for c, _, _ in call]
            if len({t.device_ordinal for t in cams}) > 1:   # (the native call wants one device: camera by camera instead)
                for c, a, b in call:
                    out[c].extend(trackers[c].update_sequence(per_camera[c][a:b]))
                continue
            runs = [per_camera[c][a:b] for c, a, b in call]
            camera_of = np.array([i for i, run in enumerate(runs) for _ in run], np.int32)   # camera after camera; the native side steps across them
            frames = [f for run in runs for f in run]
            counts = np.array([len(f) for f in frames], np.int32)
            n = int(counts.sum())
            with_feats = any(det.features is not None for f in frames for det in f)
            boxes, foot, conf, has = np.zeros((n, 4), np.float32), np.zeros((n, 2), np.float32), np.zeros(n, np.float32), np.zeros(n, np.uint8)
            widths = np.array([cams[i].feature_dim for i in camera_of], np.int64)
            feats = np.zeros(int((counts * widths).sum()), np.float32) if with_feats else None
            j = at = 0
            for i, f in zip(camera_of, frames):
                D = cams[i].feature_dim
                for det in f:
                    if det.camera_coords is None:
                        raise ValueError(f"detection {j} has no camera_coords: a track cannot be started or updated without a foot point")
                    boxes[j], foot[j], conf[j] = det.bbox, det.camera_coords, det.confidence
                    if det.features is not None:
                        v = np.asarray(det.features, np.float32).reshape(-1)
                        if v.shape[0] != D:
                            raise ValueError(f"detection {j} has a feature of width {v.shape[0]}, its tracker was made for {D}")
                        feats[at:at + D], has[j] = v, 1
                    j += 1
                    at += D
            for t in cams:
                t._ensure()
            lib = cams[0]._lib
            handles = (C.c_void_p * len(cams))(*[t._h.value for t in cams])
            ids, done = np.full(max(n, 1), -1, np.int32), np.zeros(len(cams), np.int32)
            p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)   # noqa: E731
            rc = lib.opd_track_update_streams(handles, len(cams), p(camera_of), len(frames), p(boxes), p(foot), p(conf), p(feats), p(has), _capi.OPD_MEM_HOST, p(counts),
                                              p(ids), p(done))
            err = HipTracker._replay_streams(cams, runs, ids, done, rc, "opd_track_update_streams", out, [c for c, _, _ in call])
            failed = failed or err
            if err is not None:
                break
        if failed is not None:
            raise failed
        return out

    @staticmethod
    def _replay_streams(cams, runs, ids: np.ndarray, done: np.ndarray, rc: int, what: str, out: list, into: List[int], stride: Optional[int] = None,
                        message: Optional[str] = None) -> Optional[RuntimeError]:
        """``_replay`` per camera after a streams call whose frames lay camera after camera (``ids`` likewise): the cameras that ran to their end
        first, then the stopped ones, each of which raises as ``update_sequence`` does; returns the first such error instead of raising it, so
        that every camera's mirror follows its native tracker."""
        if message is None:
            message = _capi.last_error() if rc != 0 else ""
        stopped = rc != 0 and "counted as one without detections" in message
        if rc != 0 and not stopped:
            _capi.check(rc, what)
        named = re.search(r"cameras out of slots: ([0-9, ]+)", message)
        out_of_slots = {int(v) for v in named.group(1).split(",")} if named else set()
        failed: Optional[RuntimeError] = None
        at = 0
        for i, (t, run) in enumerate(zip(cams, runs)):
            rows = sum(stride if stride is not None else len(f) for f in run)
            try:
                out[into[i]].extend(t._replay(run, ids[at:at + rows], int(done[i]), rc if i in out_of_slots else 0, what, stride=stride))
            except RuntimeError:
                failed = failed or RuntimeError(f"{what} failed (code {rc}): {message}")
            at += rows
        return failed

    def _replay(self, frames: List[List[Detection]], ids: np.ndarray, done: int, rc: int, what: str, stride: Optional[int] = None) -> List[List[Detection]]:
        """The mirror after a sequence call: ``_apply`` frame by frame for the ``done`` frames the native side applied (the last of them an empty
        one when it ran out of slots, before the error is raised).  ``ids``: packed frame after frame, or ``stride`` apart."""
        message = _capi.last_error() if rc != 0 else ""
        out, at = [], 0
        for f, dets in enumerate(frames[:done]):
            last = f == done - 1
            if rc != 0 and last:
                self._apply([], ids[:0])
            else:
                self._apply(dets, ids[at:at + len(dets)], verify=last)
                out.append([det for det in dets if det.track_id is not None])
            at += stride if stride is not None else len(dets)
        if rc != 0:
            raise RuntimeError(f"{what} failed (code {rc}): {message}")
        return out

    def get_tracks(self) -> List[HipTrack]:
        return self.tracks.copy()

    def get_confirmed_tracks(self) -> List[HipTrack]:
        return [t for t in self.tracks if t.is_confirmed(self.min_hits)]

    def reset(self) -> None:
        if self._h:
            _capi.check(self._lib.opd_track_reset(self._h), "opd_track_reset")
        self.tracks, self.next_id = [], 1

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.opd_track_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:   # interpreter shutdown
            pass

    # ---- the host mirror ------------------------------------------------------------------------------------------------------------
    def _records(self):
        n = C.c_int()
        _capi.check(self._lib.opd_track_get(self._h, None, 0, C.byref(n)), "opd_track_get")
        recs = (_capi.OpdTrackRec * max(n.value, 1))()
        _capi.check(self._lib.opd_track_get(self._h, recs, n.value, C.byref(n)), "opd_track_get")
        return [recs[i] for i in range(n.value)]

    def _state_of(self, track_id: int) -> List[float]:
        for r in self._records():
            if r.track_id == track_id:
                return [float(v) for v in r.x]
        raise KeyError(f"track {track_id} is not alive")

    def _apply(self, detections: List[Detection], ids: np.ndarray, verify: bool = True) -> None:
        """Replay on the host objects what the native update did to its counters: predict, matches, new tracks, deletions.  ``verify=False``:
        a frame of a sequence call that is not its last, so the native side is already further on."""
        by_id: Dict[int, HipTrack] = {t.track_id: t for t in self.tracks}
        for t in self.tracks:
            t.time_since_update += 1
        for det, tid in zip(detections, ids.tolist()):
            if tid < 0:
                continue
            det.track_id = tid
            t = by_id.get(tid)
            if t is None:
                t = HipTrack(track_id=tid, detection=det, trajectory=[det.camera_coords], _owner=self)
                self.tracks.append(t)
                by_id[tid] = t
            else:
                t.detection = det
                t.age += 1
                t.hits += 1
                t.time_since_update = 0
                t.trajectory.append(det.camera_coords)
        self.tracks = [t for t in self.tracks if t.time_since_update < self.max_age]
        if not verify:
            return
        info = _capi.OpdTrackStatus()
        _capi.check(self._lib.opd_track_info(self._h, C.byref(info)), "opd_track_info")
        self.next_id = info.next_id
        if info.n_tracks != len(self.tracks):
            raise RuntimeError(f"host mirror out of step with the native tracker: {len(self.tracks)} tracks here, {info.n_tracks} there")
