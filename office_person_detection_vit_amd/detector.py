"""``HipDetrDetector`` — the reference's Phase-2 detector surface on top of libopd_hip.so.

Drop-in for the class the pipeline instantiates in ``DetectionPhase.initialize``
(``src/pipeline/phases/detection.py:34-54``): same constructor keywords, attributes and methods as the DETR-era
``ViTDetector`` (deleted ``src/detection/vit_detector.py``; method map in ``coverage.json:1``; its stand-in with the
identical interface is ``src/detection/yolov8_detector.py:19-254``) and the same error conventions:

* ``detect*`` before ``load_model`` -> ``RuntimeError("Model not loaded. Call load_model() first.")``
  (``yolov8_detector.py:102-103``),
* load failure -> ``RuntimeError("Failed to load DETR model: ...")`` chained (``:86-88``),
* inference errors are logged and re-raised (``:130-132``) — the phase turns them into an empty list per frame
  (``detection.py:124-127``).

All arithmetic runs in hand-written HIP kernels behind the C-ABI of ``include/opd_detr.h``; there is no CPU or PyTorch
fallback — without the built library or without a GPU every call raises.
"""

from __future__ import annotations

from concurrent.futures import ThreadPoolExecutor
import ctypes as C
from dataclasses import dataclass
import logging
import os
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _capi
from .data_models import Detection
from .feature_extractor import FeatureExtractor

logger = logging.getLogger(__name__)

PERSON_LABEL = 1  # COCO "person" in DETR's label space (tests/test_detection_phase.py:71 uses class_id=1)
DEFAULT_MODEL_NAME = "facebook/detr-resnet-50"


def model_input_size(height: int, width: int, shortest_edge: int = 800, longest_edge: int = 1333) -> Tuple[int, int]:
    """HF DETR size rule (HF:image_transforms.py:206-242): shortest edge -> 800 unless the longest would pass 1333."""
    size, raw_size = shortest_edge, None
    mn, mx = float(min(height, width)), float(max(height, width))
    if mx / mn * size > longest_edge:
        raw_size = longest_edge * mn / mx
        size = int(round(raw_size))
    if (height <= width and height == size) or (width <= height and width == size):
        return height, width
    if width < height:
        return (int(raw_size * height / width) if raw_size is not None else int(size * height / width)), size
    return size, (int(raw_size * width / height) if raw_size is not None else int(size * width / height))


def resize_frame(frame: np.ndarray, out_h: int, out_w: int) -> np.ndarray:
    """PIL bilinear resize of a uint8 HxWx3 frame, exactly what HF's image processor does on the host
    (HF:models/detr/image_processing_pil_detr.py:497-549).  Used for batches of mixed frame sizes and as the reference
    of the device-side resize (``opd_detr_*_resized``, bit-exact with this function)."""
    if frame.shape[0] == out_h and frame.shape[1] == out_w:
        return frame
    from PIL import Image

    return np.asarray(Image.fromarray(frame).resize((out_w, out_h), resample=Image.BILINEAR))


# The native tiled entries that take a chunk of frames (``HipDetrDetector._tiled_chunks`` runs them all): how each spells the model size in its
# argument list ("HW": H, W; "tile_HW": the per-tile sizes; "HW,tile_HW": H, W, and the per-tile sizes or NULL) and the stage block it takes behind
# the parameters.  A further entry is a row here, its block (if new) in ``_tiled_chunks`` and a public method that checks its arguments.
_TILED_ENTRIES = {
    "opd_detr_detect_tiled": ("HW", None),
    "opd_detr_detect_tiled_stages": ("HW", _capi.OpdTileStages),
    "opd_detr_detect_tiled_ragged": ("tile_HW", _capi.OpdTileStages),   # (the one entry whose block may be null)
    "opd_detr_detect_tiled_reid": ("HW", _capi.OpdTileReidStages),
    "opd_detr_detect_tiled_ragged_reid": ("tile_HW", _capi.OpdTileReidStages),
    "opd_detr_detect_tiled_hybrid": ("HW,tile_HW", _capi.OpdTileHybrid),
}


@dataclass
class _TileGrid:
    """The checked geometry of a tiled call (``HipDetrDetector._tiled_geometry``)."""
    h: int   # frame size
    w: int
    T: int   # tiles per frame
    S: int   # merged-record slots per frame: tiles x queries
    win: np.ndarray   # [T, 4] int32 windows (y0, x0, h, w)
    sizes: List[Tuple[int, int]]   # the model size of every tile (``tile_model_sizes``)
    one_size: bool   # whether all windows have one size
    tile_hw: np.ndarray   # [T, 2] int32 ``sizes``

    def size_args(self, spelling: str) -> tuple:
        """The model size as an entry spells it (``_TILED_ENTRIES``)."""
        if spelling == "HW":
            return self.sizes[0]
        ptr = self.tile_hw.ctypes.data_as(C.c_void_p)
        if spelling == "tile_HW":
            return (ptr,)
        return (*self.sizes[0], None) if self.one_size else (0, 0, ptr)


def _check_tracker_list(items, n_frames: int, name: str) -> Optional[list]:
    """``items`` (``trackers=`` or ``lwts=``) as a list with one distinct tracker per frame; ``None`` stays ``None``."""
    if items is None:
        return None
    items = list(items)
    if len(items) != n_frames:
        raise ValueError(f"{len(items)} trackers for {n_frames} frames: frame f enters {name}[f]")
    if len({id(t) for t in items}) != len(items):
        raise ValueError("a tracker is named twice: a tracker takes one frame per call")
    return items


def _check_tiled_features(features: Optional[str]) -> None:
    if features not in (None, "color"):
        if features == "encoder":
            raise ValueError("features='encoder' does not exist for tiled detection: a box merged from two tiles' maps has no encoder row")
        raise ValueError(f"features must be None or 'color', got {features!r}")


def _track_feature_kind(features: Optional[str], reid) -> int:
    """The checks of ``features=`` / ``reid=`` of the detect-and-track calls, and the ``OPD_TRACK_FEAT_*`` value of ``features``."""
    if features not in (None, "encoder", "color", "reid"):
        raise ValueError(f"features must be None, 'encoder', 'color' or 'reid', got {features!r}")
    if features == "reid" and reid is None:
        raise ValueError("features='reid' needs reid= a loaded HipReIDExtractor or HipOSNetReIDExtractor")
    if features == "reid" and not reid.is_loaded:
        raise RuntimeError("Re-ID model is not loaded: call load_model() first")
    return {None: _capi.OPD_TRACK_FEAT_NONE, "encoder": _capi.OPD_TRACK_FEAT_ENCODER, "color": _capi.OPD_TRACK_FEAT_COLOR, "reid": _capi.OPD_TRACK_FEAT_REID}[features]


def _floor_fields(block, floor_map, rows: int) -> np.ndarray:
    """``floor`` / ``floor_out`` of a stage block: the mapper's handle and ``rows`` zeroed floor records for the call to fill by position."""
    floor = np.zeros(rows, floor_map.REC_DTYPE)
    block.floor, block.floor_out = floor_map._require().value, floor.ctypes.data
    return floor


def _tracker_fields(block, trackers: list, S: int):
    """``trackers`` / ``track_ids`` (/ ``n_featured`` where the block has it) of a stage block for the trackers of one chunk, handles made already:
    ``(ids [n * S], handle array, n_featured)``, which the caller holds until the call has returned."""
    n = len(trackers)
    handles = (C.c_void_p * n)(*[t._h.value for t in trackers])
    ids, n_featured = np.full(n * S, -1, np.int32), np.zeros(n, np.int32)
    block.trackers, block.track_ids = C.addressof(handles), ids.ctypes.data
    if hasattr(block, "n_featured"):
        block.n_featured = n_featured.ctypes.data
    return ids, handles, n_featured


def _hybrid_runs(keys: List[bool], max_frames: int, max_keys: int):
    """The runs a hybrid sequence goes down in: from each start the longest run within ``max_frames`` frames and ``max_keys`` key frames."""
    start = 0
    while start < len(keys):
        end, n_key = start, 0
        while end < len(keys) and end - start < max_frames and (not keys[end] or n_key < max_keys):
            n_key += keys[end]
            end += 1
        yield start, end
        start = end


def _hybrid_run_buffers(frames: list, keys: List[bool], Rec, stride: int, cap: int):
    """Inputs and outputs of one hybrid-sequence call: the frame pointers and key flags, ``stride`` records of type ``Rec``, a count and ``stride``
    ids per key frame, ``cap`` tracker records and a count per in-between frame, and ``frames_done``."""
    F, K = len(frames), sum(keys)
    recs, counts, ids = (Rec * (max(K, 1) * stride))(), (C.c_int32 * max(K, 1))(), np.full(max(K, 1) * stride, -1, np.int32)
    lrecs, lcounts, done = (_capi.OpdLwtRec * (max(F - K, 1) * cap))(), (C.c_int32 * max(F - K, 1))(), C.c_int32(0)
    ptrs = (C.c_void_p * F)(*[f.ctypes.data for f in frames])
    flags = (C.c_uint8 * F)(*[int(k) for k in keys])
    return ptrs, flags, recs, counts, ids, lrecs, lcounts, done


def _hybrid_run_results(lwt, keys: List[bool], per_key: List[List[Detection]], ids: np.ndarray, stride: int, lrecs, lcounts, cap: int) -> list:
    """One entry per frame of a run: the detections of a key frame with their ids adopted by ``lwt``, the ``(track_id, bbox)`` list of an in-between frame."""
    out, k, j = [], 0, 0
    for key in keys:
        if key:
            out.append(lwt._adopt(per_key[k], ids[k * stride:k * stride + len(per_key[k])].tolist()))
            k += 1
        else:
            out.append([(int(lrecs[j * cap + i].track_id), tuple(float(v) for v in lrecs[j * cap + i].bbox)) for i in range(lcounts[j])])
            j += 1
    return out


class HipDetrDetector:
    """DETR person detector running on one MI355X through libopd_hip.so."""

    def __init__(
        self,
        model_name: str = DEFAULT_MODEL_NAME,
        confidence_threshold: float = 0.5,
        device: Optional[str] = None,
        nms_threshold: float = 0.4,
        model_path: Optional[str] = None,
        iou_threshold: Optional[float] = None,
        max_batch: int = 8,
        max_size: Tuple[int, int] = (800, 1333),
        resize: bool = True,
        device_resize: bool = True,
        use_graph: bool = True,
        streams: int = 1,
        pinned_staging: bool = True,
        dtype: str = "fp16",
        frame_lists: bool = True,
        device_nms: bool = False,
    ):
        """
        Args mirror ``config.yaml.disabled:33-44`` (``model_name``, ``confidence_threshold``, ``nms_threshold``,
        ``device``, ``batch_size`` -> ``max_batch``).  ``model_path`` is a local ``.safetensors`` file with the HF
        ``DetrForObjectDetection`` state dict (or a directory holding ``model.safetensors``); hub loading by NAME is
        impossible offline, so ``model_name`` alone resolves only through ``$OPD_DETR_WEIGHTS``.
        ``iou_threshold`` is the keyword ``DetectionPhase.initialize`` passes (``src/pipeline/phases/detection.py:47-52``:
        ``model_path``, ``confidence_threshold``, ``device``, ``iou_threshold``): the same knob as ``nms_threshold``, which it
        overrides when given.
        ``device``: ``"hip"``, ``"hip:N"``, ``"cuda"``, ``"cuda:N"`` or None (= GPU 0).  ``"cpu"``/``"mps"`` are refused.
        ``streams``: detector handles (each with its own HIP stream and workspace; the weights are shared) that
        ``detect_batch`` keeps busy at once when a call spans several ``max_batch`` chunks; 1 = strictly serial.
        ``dtype``: 16-bit operand type of the device path: ``"fp16"`` (default: meets the 1e-3 box tolerance) or ``"bf16"``
        (``OPD_FLAG_BF16``: the type the DETR-era config's deployment target names; same speed, 8 mantissa bits: boxes drift ~4x more).
        ``pinned_staging``: stack the caller's frames into page-locked memory (``opd_host_alloc``) so that the upload is
        one DMA; False stacks into ordinary numpy memory.
        ``frame_lists``: hand a chunk of same-sized contiguous frames to the library as a list of pointers
        (``opd_detr_detect_frames``: each frame is uploaded from where it lies) instead of stacking it first; False always stacks.
        ``device_nms``: run the person filter and NMS on the device inside every detect call (``opd_detr_set_nms``) instead of on the
        host behind it: the same ``Detection`` lists; feature, floor and Re-ID stages of the fused calls then work on final records only.
        """
        self.model_name = model_name
        self.model_path = model_path
        self.confidence_threshold = confidence_threshold
        if iou_threshold is not None:
            nms_threshold = float(iou_threshold)
        self.nms_threshold = nms_threshold
        self.iou_threshold = nms_threshold  # the YOLO-era spelling of the same knob
        self.device = self._setup_device(device)
        self.max_batch = int(max_batch)
        self.max_size = (int(max_size[0]), int(max_size[1]))
        self.resize = resize
        self.device_resize = device_resize  # resize camera-resolution frames on the GPU (False: PIL on the host)
        self.use_graph = use_graph  # replay the forward as a captured hipGraph (False: launch every kernel eagerly)
        if dtype not in ("fp16", "bf16"):
            raise ValueError("dtype must be 'fp16' or 'bf16'")
        self.dtype = dtype
        self.streams = max(1, int(streams))
        self.model: Optional[int] = None  # opaque opd_detr* once loaded (handle 0)
        self._handles: List[int] = []  # all handles, handle 0 first
        self.pinned_staging = bool(pinned_staging)
        self.frame_lists = bool(frame_lists)
        self.device_nms = bool(device_nms)
        self._nms_set: Optional[float] = None  # device_nms: the threshold the handles were last given
        self._staging: dict = {}  # handle slot -> (pinned pointer, capacity in bytes)
        self.feature_extractor = FeatureExtractor()
        self._lib = None
        self._info = None
        self._last_orig: List[Tuple[int, int]] = []
        logger.info(f"HipDetrDetector initialized with model: {model_name}")
        logger.info(f"Using device: {self.device}")
        logger.info(f"Confidence threshold: {confidence_threshold}")

    # ------------------------------------------------------------------------------------------------------------
    def _setup_device(self, device: Optional[str] = None) -> str:
        if device is None:
            return "hip:0"
        d = str(device).lower()
        if d in ("cpu", "mps"):
            raise ValueError(f"HipDetrDetector runs on an AMD GPU only; device={device!r} is not supported")
        if d in ("hip", "cuda"):
            return "hip:0"
        if d.startswith(("hip:", "cuda:")):
            return "hip:" + d.split(":", 1)[1]
        raise ValueError(f"unknown device {device!r}")

    @property
    def device_ordinal(self) -> int:
        return int(self.device.split(":")[1])

    def _resolve_weights(self) -> str:
        cand = self.model_path or os.environ.get("OPD_DETR_WEIGHTS")
        if cand is None:
            raise FileNotFoundError(
                f"no local weights for {self.model_name!r}: pass model_path=<.safetensors> or set OPD_DETR_WEIGHTS "
                "(hub download by name is not available)")
        if os.path.isdir(cand):
            cand = os.path.join(cand, "model.safetensors")
        if not os.path.exists(cand):
            raise FileNotFoundError(f"weight file not found: {cand}")
        return cand

    def load_model(self) -> None:
        """Parse the checkpoint natively, fold FrozenBN, upload to the GPU (``opd_detr_create``)."""
        try:
            lib = _capi.load_library()
            path = self._resolve_weights()
            cfg = _capi.OpdConfig(struct_size=C.sizeof(_capi.OpdConfig), max_batch=self.max_batch,
                                  max_height=self.max_size[0], max_width=self.max_size[1],
                                  flags=(0 if self.use_graph else _capi.OPD_FLAG_NO_GRAPH) | (_capi.OPD_FLAG_BF16 if self.dtype == "bf16" else 0) |
                                        (_capi.OPD_FLAG_MULTI_STREAM if self.streams > 1 else 0))
            self._lib = lib
            handle = C.c_void_p()
            rc = lib.opd_detr_create(C.byref(cfg), path.encode("utf-8"), self.device_ordinal, C.byref(handle))
            _capi.check(rc, "opd_detr_create")
            self._handles.append(handle.value)
            for _ in range(1, self.streams):   # further handles share the first one's weights in HBM
                clone = C.c_void_p()
                _capi.check(lib.opd_detr_clone(handle, C.byref(clone)), "opd_detr_clone")
                self._handles.append(clone.value)
            info = _capi.OpdModelInfo()
            _capi.check(lib.opd_detr_info(C.c_void_p(self._handles[0]), C.byref(info)), "opd_detr_info")
            self.model, self._info = self._handles[0], info
            self._sync_nms()
            logger.info(f"Model loaded: {path}")
        except Exception as e:
            self.close()
            logger.error(f"Failed to load model: {e}")
            raise RuntimeError(f"Failed to load DETR model: {e}") from e

    def _sync_nms(self) -> None:
        """``device_nms``: hand ``nms_threshold`` to every handle when it has changed since the last time (callers assign the attribute;
        assigning ``device_nms`` itself switches the mode from the next call on)."""
        if not self.device_nms:
            if self._nms_set is not None:
                for h in self._handles:
                    _capi.check(self._lib.opd_detr_set_nms(C.c_void_p(h), PERSON_LABEL, -1.0), "opd_detr_set_nms")
                self._nms_set = None
            return
        thr = float(self.nms_threshold)
        if self._nms_set is None or thr != self._nms_set:
            if not thr >= 0.0:
                raise ValueError(f"device_nms needs nms_threshold >= 0, got {thr!r}")
            for h in self._handles:
                _capi.check(self._lib.opd_detr_set_nms(C.c_void_p(h), PERSON_LABEL, thr), "opd_detr_set_nms")
            self._nms_set = thr

    def close(self) -> None:
        # communicator lanes bound to this detector's handles go first (sharding.NativeExchange registers itself here); the library also
        # detaches any lane that outlives its handle (opd_detr_destroy), so the order is a courtesy, not a requirement
        for ex in list(getattr(self, "_exchanges", [])):
            ex.close()
        self._exchanges = []
        if self._lib is not None:
            for h in self._handles:
                self._lib.opd_detr_destroy(C.c_void_p(h))
            for ptr, _ in self._staging.values():
                self._lib.opd_host_free(C.c_void_p(ptr))
        self._staging = {}
        self._handles = []
        self.model = None
        self._nms_set = None

    def __del__(self):  # pragma: no cover - best effort
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------------------------------------------------
    def _require_model(self) -> None:
        if self.model is None:
            raise RuntimeError("Model not loaded. Call load_model() first.")

    def _stage_array(self, slot: int, shape: Tuple[int, ...]) -> np.ndarray:
        """uint8 array of ``shape`` to stack a batch into: page-locked memory owned by handle ``slot`` (grown on demand,
        freed in ``close``; valid until the slot's next batch), or plain numpy memory without ``pinned_staging``."""
        n = int(np.prod(shape))
        if not self.pinned_staging or self._lib is None:
            return np.empty(shape, np.uint8)
        ptr, cap = self._staging.get(slot, (None, 0))
        if cap < n:
            if ptr:
                self._lib.opd_host_free(C.c_void_p(ptr))
                self._staging.pop(slot)
            p = C.c_void_p()
            _capi.check(self._lib.opd_host_alloc(n, C.byref(p)), "opd_host_alloc")
            ptr, cap = p.value, n
            self._staging[slot] = (ptr, cap)
        return np.ctypeslib.as_array((C.c_uint8 * n).from_address(ptr)).reshape(shape)

    def _stack(self, slot: int, frames: Sequence[np.ndarray]) -> np.ndarray:
        batch = self._stage_array(slot, (len(frames),) + tuple(frames[0].shape))
        for i, f in enumerate(frames):
            batch[i] = f
        return batch

    def _preprocess_batch(self, frames: Sequence[np.ndarray], slot: int = 0):
        """Host part of ``_preprocess_batch`` (deleted vit_detector.py 562-578): validate, resize to the model size,
        stack to one contiguous uint8 [B,H,W,3] BGR block.  BGR->RGB, 1/255 and mean/std run on the device.

        Frames whose model-input sizes differ form a RAGGED batch: like HF's ``DetrImageProcessor.pad``
        (``image_processing_detr.py:639-668``) every frame sits in the top-left corner of a canvas of the batch-maximum
        size, and the per-frame valid sizes are returned so that the device applies the padding-mask paths.

        Frames of ONE size that need resizing are NOT resized here: the batch stays at camera resolution and the
        returned ``target`` = (H, W) tells the caller to use the device-side resize (bit-exact with PIL's bilinear,
        ``opd_detr_*_resized``); ``device_resize=False`` or mixed sizes keep the host PIL path.
        Returns (batch, original sizes, valid sizes [B,2] int32 or None, target (H, W) or None)."""
        if len(frames) == 0:
            raise ValueError("empty frame batch")
        orig, out = [], []
        for f in frames:
            if not isinstance(f, np.ndarray) or f.ndim != 3 or f.shape[2] != 3 or f.dtype != np.uint8:
                raise ValueError("frames must be uint8 numpy arrays of shape (H, W, 3) in BGR order")
            orig.append((int(f.shape[0]), int(f.shape[1])))
        if self.resize and self.device_resize and len(set(orig)) == 1:
            th, tw = model_input_size(orig[0][0], orig[0][1], self.max_size[0], self.max_size[1])
            if (th, tw) != orig[0]:
                return self._stack(slot, frames), orig, None, (th, tw)
        for f in frames:
            if self.resize:
                th, tw = model_input_size(f.shape[0], f.shape[1], self.max_size[0], self.max_size[1])
                f = resize_frame(f, th, tw)
            out.append(f)
        shapes = {o.shape for o in out}
        if len(shapes) == 1:
            return self._stack(slot, out), orig, None, None
        H, W = max(o.shape[0] for o in out), max(o.shape[1] for o in out)
        if max(H, W) > max(self.max_size) or H * W > self.max_size[0] * self.max_size[1]:
            raise ValueError(f"ragged batch canvas {H}x{W} exceeds the configured maximum {self.max_size} (either orientation)")
        canvas = self._stage_array(slot, (len(out), H, W, 3))
        canvas[...] = 0
        for i, o in enumerate(out):
            canvas[i, :o.shape[0], :o.shape[1]] = o
        valid = np.asarray([[o.shape[0], o.shape[1]] for o in out], dtype=np.int32)
        return canvas, orig, valid, None

    def forward_raw(self, frames: Sequence[np.ndarray], want_encoder: bool = True):
        """Model outputs for a batch of BGR frames: (logits [B,Q,C+1], pred_boxes [B,Q,4], encoder [B,hw,256] | None)."""
        self._require_model()
        batch, orig, valid, target = self._preprocess_batch(frames)
        B, H, W, _ = batch.shape
        if target is not None:
            H, W = target
        Q, ncls, D = self._info.num_queries, self._info.num_classes_plus1, self._info.d_model
        fh, fw = _feature_hw(H), _feature_hw(W)
        logits = np.empty((B, Q, ncls), np.float32)
        boxes = np.empty((B, Q, 4), np.float32)
        enc = np.empty((B, fh * fw, D), np.float32) if want_encoder else None
        if target is not None:
            rc = self._lib.opd_detr_forward_resized(C.c_void_p(self.model), batch.ctypes.data_as(C.c_void_p), _capi.OPD_MEM_HOST,
                                                    B, batch.shape[1], batch.shape[2], H, W, logits.ctypes.data_as(C.c_void_p),
                                                    boxes.ctypes.data_as(C.c_void_p),
                                                    enc.ctypes.data_as(C.c_void_p) if enc is not None else None)
            _capi.check(rc, "opd_detr_forward_resized")
            self._last_orig = orig
            return logits, boxes, enc
        rc = self._lib.opd_detr_forward_ragged(C.c_void_p(self.model), batch.ctypes.data_as(C.c_void_p),
                                               _capi.OPD_PIXELS_U8_BGR_HWC, _capi.OPD_MEM_HOST, B, H, W,
                                               valid.ctypes.data_as(C.c_void_p) if valid is not None else None,
                                               logits.ctypes.data_as(C.c_void_p), boxes.ctypes.data_as(C.c_void_p),
                                               enc.ctypes.data_as(C.c_void_p) if enc is not None else None)
        _capi.check(rc, "opd_detr_forward")
        self._last_orig = orig
        return logits, boxes, enc

    def _detect_records(self, frames: Sequence[np.ndarray], handle: Optional[int] = None):
        model = self.model if handle is None else handle
        B, Q = len(frames), self._info.num_queries
        recs = (_capi.OpdDet * (B * Q))()
        counts = (C.c_int32 * B)()
        self._detect_into(frames, model, C.addressof(recs), C.addressof(counts), on_device=False)
        return recs, counts, Q

    def _detect_records_floor(self, frames: Sequence[np.ndarray], floor_map, handle: Optional[int] = None):
        """``_detect_records`` plus the ``[B * Q]`` floor records of the person records (row = frame * Q + query_index), from ONE
        ``opd_detr_detect_frames_floor`` call, when the chunk can go down as a list of host frames; else ``None`` in their place
        (the caller then runs ``floor_map.apply`` on the detections)."""
        target = self._frame_list_target(frames) if (self.frame_lists and len(frames)) else None
        if target is None or int(floor_map.device) != self.device_ordinal:
            return (*self._detect_records(frames, handle), None)
        model = self.model if handle is None else handle
        B, Q = len(frames), self._info.num_queries
        recs, counts = (_capi.OpdDet * (B * Q))(), (C.c_int32 * B)()
        floor = np.zeros(B * Q, floor_map.REC_DTYPE)
        ptrs = (C.c_void_p * B)(*[f.ctypes.data for f in frames])
        rc = self._lib.opd_detr_detect_frames_floor(C.c_void_p(model), floor_map._require(), ptrs, B, int(frames[0].shape[0]), int(frames[0].shape[1]),
                                                    target[0], target[1], float(self.confidence_threshold), PERSON_LABEL, recs, counts, floor.ctypes.data)
        _capi.check(rc, "opd_detr_detect_frames_floor")
        self._last_orig = [(int(f.shape[0]), int(f.shape[1])) for f in frames]
        return recs, counts, Q, floor

    def _frame_list_target(self, frames: Sequence[np.ndarray]) -> Optional[Tuple[int, int]]:
        """(H, W) of the model input when the chunk can go down as a LIST of frame pointers (``opd_detr_detect_frames``: every frame
        uploaded from where it lies, no stacked copy): contiguous uint8 [h, w, 3] frames of ONE size, model size reached on the device."""
        f0 = frames[0]
        for f in frames:
            if not isinstance(f, np.ndarray) or f.dtype != np.uint8 or f.ndim != 3 or f.shape != f0.shape or f.shape[2] != 3 or not f.flags.c_contiguous:
                return None
        h, w = int(f0.shape[0]), int(f0.shape[1])
        if not self.resize:
            return (h, w)
        th, tw = model_input_size(h, w, self.max_size[0], self.max_size[1])
        return (th, tw) if ((th, tw) == (h, w) or self.device_resize) else None

    def _detect_into(self, frames: Sequence[np.ndarray], model: int, rec_ptr: int, cnt_ptr: int, on_device: bool) -> None:
        """One ``max_batch`` chunk of host frames -> ``[B][Q]`` ``opd_det`` records at ``rec_ptr`` and ``[B]`` counts at
        ``cnt_ptr``; ``on_device``: both are HIP device pointers on this detector's GPU (``OPD_MEM_HOST_PIXELS_DEVICE_OUT``)."""
        if len(frames) == 0:
            raise ValueError("empty frame batch")
        target = self._frame_list_target(frames) if self.frame_lists else None
        if target is not None:
            kind = _capi.OPD_MEM_HOST_PIXELS_DEVICE_OUT if on_device else _capi.OPD_MEM_HOST
            recs, counts = C.cast(C.c_void_p(rec_ptr), C.POINTER(_capi.OpdDet)), C.cast(C.c_void_p(cnt_ptr), C.POINTER(C.c_int32))
            ptrs = (C.c_void_p * len(frames))(*[f.ctypes.data for f in frames])
            rc = self._lib.opd_detr_detect_frames(C.c_void_p(model), ptrs, kind, len(frames), int(frames[0].shape[0]), int(frames[0].shape[1]),
                                                  target[0], target[1], float(self.confidence_threshold), recs, counts)
            _capi.check(rc, "opd_detr_detect_frames")
            self._last_orig = [(int(f.shape[0]), int(f.shape[1])) for f in frames]
            return
        batch, orig, valid, target = self._preprocess_batch(frames, self._handles.index(model))
        B, H, W, _ = batch.shape
        kind = _capi.OPD_MEM_HOST_PIXELS_DEVICE_OUT if on_device else _capi.OPD_MEM_HOST
        recs, counts = C.cast(C.c_void_p(rec_ptr), C.POINTER(_capi.OpdDet)), C.cast(C.c_void_p(cnt_ptr), C.POINTER(C.c_int32))
        if target is not None:   # camera-resolution batch: resize on the device, boxes come back in camera pixels
            rc = self._lib.opd_detr_detect_resized(C.c_void_p(model), batch.ctypes.data_as(C.c_void_p), kind,
                                                   B, H, W, target[0], target[1], float(self.confidence_threshold), recs, counts)
            _capi.check(rc, "opd_detr_detect_resized")
        else:
            hw = np.asarray(orig, dtype=np.int32).reshape(B, 2)
            rc = self._lib.opd_detr_detect_ragged(C.c_void_p(model), batch.ctypes.data_as(C.c_void_p),
                                                  _capi.OPD_PIXELS_U8_BGR_HWC, kind, B, H, W,
                                                  valid.ctypes.data_as(C.c_void_p) if valid is not None else None,
                                                  float(self.confidence_threshold), hw.ctypes.data_as(C.c_void_p), recs, counts)
            _capi.check(rc, "opd_detr_detect")
        self._last_orig = orig

    @property
    def num_queries(self) -> int:
        self._require_model()
        return int(self._info.num_queries)

    def detect_records_into(self, frames: Sequence[np.ndarray], records, counts) -> None:
        """Frame-sharded callers (``sharding.ShardedDetector``): detect ``frames`` (at most ``max_batch``) and write their fixed-size
        records / counts into caller-owned int32 buffers ``records`` ``[len(frames), Q, 8]`` and ``counts`` ``[len(frames)]``.
        The buffers are anything with ``data_ptr()`` / ``is_cuda`` / ``is_contiguous()`` (torch tensors: the library itself never
        imports torch); device buffers are written by the post-process kernel directly, so the records can go into a collective
        without touching the host."""
        self._require_model()
        if len(frames) == 0:
            return
        if len(frames) > self.max_batch:
            raise ValueError(f"{len(frames)} frames exceed max_batch = {self.max_batch}")
        if not (records.is_contiguous() and counts.is_contiguous()):
            raise ValueError("records / counts must be contiguous")
        self._sync_nms()
        self._detect_into(frames, self.model, int(records.data_ptr()), int(counts.data_ptr()), on_device=bool(records.is_cuda))

    def detect_records_at(self, frames: Sequence[np.ndarray], rec_ptr: int, cnt_ptr: int) -> None:
        """The same with raw DEVICE pointers on this detector's GPU (``sharding.NativeExchange``: slots of the send buffer of an
        ``opd_comm`` bound to handle 0, ``opd_comm_buffers``)."""
        self._require_model()
        if len(frames) > self.max_batch:
            raise ValueError(f"{len(frames)} frames exceed max_batch = {self.max_batch}")
        if len(frames):
            self._sync_nms()
            self._detect_into(frames, self.model, int(rec_ptr), int(cnt_ptr), on_device=True)

    def _postprocess_batch(self, recs, counts, Q: int, floor=None, floor_map=None) -> List[List[Detection]]:
        """``_postprocess_batch`` (deleted vit_detector.py 591-647): person filter + NMS (C-ABI), xyxy -> xywh, foot point.
        ``floor``: the fused call's floor records; every kept detection takes the row of its query (Phase 3's four fields)."""
        if self._nms_set is None:   # (else the handles suppressed on the device, _sync_nms: the records are final already, in the same order)
            rc = self._lib.opd_person_nms_batch(recs, counts, len(counts), Q, PERSON_LABEL, float(self.nms_threshold))   # in place
            _capi.check(rc, "opd_person_nms_batch")
        results: List[List[Detection]] = []
        for b in range(len(counts)):
            dets = []
            for i in range(int(counts[b])):
                r = recs[b * Q + i]
                bbox = (float(r.x1), float(r.y1), float(r.x2 - r.x1), float(r.y2 - r.y1))
                dets.append(Detection(bbox=bbox, confidence=float(r.score), class_id=PERSON_LABEL, class_name="person",
                                      camera_coords=self._get_foot_position(bbox), query_index=int(r.query_index)))
                if floor is not None:
                    floor_map._fill(dets[-1], floor[b * Q + int(r.query_index)])
            results.append(dets)
        return results

    def _detect_chunk(self, chunk: Sequence[np.ndarray], floor_map, handle: Optional[int] = None):
        """(detections per frame, whether their floor fields are filled) of one ``max_batch`` chunk."""
        if floor_map is None:
            return self._postprocess_batch(*self._detect_records(chunk, handle)), True
        recs, counts, Q, floor = self._detect_records_floor(chunk, floor_map, handle)
        return self._postprocess_batch(recs, counts, Q, floor, floor_map), floor is not None

    def detect_batch(self, frames: List[np.ndarray], floor_map=None) -> List[List[Detection]]:
        """Batched detection (deleted vit_detector.py 508-550; ``.kiro/specs/office-person-detection/design.md:646-653``).
        ``floor_map``: a ``HipFloorMapper``; the detections come back with ``floor_coords``, ``floor_coords_mm``, ``camera_coords`` and
        ``zone_ids`` filled as the reference's Phase 3 fills them: inside the detect call where the chunk goes down as a list of host
        frames, by ``floor_map.apply`` afterwards where it does not (ragged or pre-resized batches)."""
        self._require_model()
        if len(frames) == 0:
            return []
        self._sync_nms()
        try:
            chunks = [frames[i:i + self.max_batch] for i in range(0, len(frames), self.max_batch)]
            if len(self._handles) > 1 and len(chunks) > 1:
                return self._detect_chunks_overlapped(chunks, floor_map)
            out: List[List[Detection]] = []
            for chunk in chunks:
                dets, filled = self._detect_chunk(chunk, floor_map)
                if not filled:
                    for d in dets:
                        floor_map.apply(d)
                out.extend(dets)
            return out
        except Exception as e:
            logger.error(f"Detection failed: {e}")
            raise

    def detect_tiled(self, frames: Sequence[np.ndarray], tiles: Sequence[Tuple[int, int, int, int]], nms_threshold: float = 0.4,
                     merge_threshold: float = 0.5, edge_tolerance: float = 0.01) -> List[List[Detection]]:
        """Tiled detection in one native call per chunk (``opd_detr_detect_tiled``): every frame is uploaded once, its ``tiles``
        (``tiling.tile_grid``'s ``(y0, x0, h, w)`` list, ONE size) are resampled on the device from where the frame lies, detected as a
        batch, suppressed per tile at ``self.nms_threshold`` and merged across the seams on the device by ``tiling.merge_tile_detections``'s
        rule (``nms_threshold``, ``merge_threshold``, ``edge_tolerance``: its arguments).  One list of frame-coordinate detections per frame,
        what ``TiledDetector.detect_batch`` builds on the host, field for field."""
        self._require_model()
        frames, tiles = list(frames), [tuple(int(v) for v in t) for t in tiles]
        grid = self._tiled_geometry(frames, tiles, one_size=True)
        if grid is None:
            return []
        return self._tiled_chunks("opd_detr_detect_tiled", frames, grid, (nms_threshold, merge_threshold, edge_tolerance))

    def _tiled_geometry(self, frames: list, tiles: list, one_size: bool, reid=None) -> Optional[_TileGrid]:
        """The checks of every tiled call, in one order: the tiles, ``reid`` loaded (where the call has one), the frames, and for tiles that may
        differ in size (``one_size=False``) the canvas of their model sizes.  ``None`` without frames.  ``one_size=True`` refuses a grid of more than
        one size and leaves a tile without height or width to the native refusal; ``one_size=False`` refuses such a tile here."""
        if not tiles or any(len(t) != 4 for t in tiles):
            raise ValueError("tiles must be a non-empty list of (y0, x0, h, w)")
        if len(tiles) > self.max_batch:
            raise ValueError(f"the {len(tiles)} tiles of one frame exceed max_batch = {self.max_batch}")
        uniform = len({(t[2], t[3]) for t in tiles}) == 1
        if one_size and not uniform:
            raise ValueError("tiles of more than one size: one forward has one model size")
        if not one_size and any(t[2] < 1 or t[3] < 1 for t in tiles):
            raise ValueError("tiles must have a height and a width of at least 1")
        if reid is not None and not getattr(reid, "is_loaded", True):
            raise RuntimeError("Re-ID model is not loaded: call load_model() first")
        if len(frames) == 0:
            return None
        f0 = frames[0]
        for f in frames:
            if not isinstance(f, np.ndarray) or f.dtype != np.uint8 or f.ndim != 3 or f.shape[2] != 3 or f.shape != f0.shape or not f.flags.c_contiguous:
                raise ValueError("frames must be contiguous uint8 numpy arrays of shape (H, W, 3) in BGR order, all of one size")
        sizes = self.tile_model_sizes(tiles)
        H, W = max(s[0] for s in sizes), max(s[1] for s in sizes)
        if not one_size and (max(H, W) > max(self.max_size) or H * W > self.max_size[0] * self.max_size[1]):
            raise ValueError(f"ragged batch canvas {H}x{W} exceeds the configured maximum {self.max_size} (either orientation)")
        T = len(tiles)
        return _TileGrid(h=int(f0.shape[0]), w=int(f0.shape[1]), T=T, S=T * self._info.num_queries, win=np.asarray(tiles, dtype=np.int32).reshape(T, 4),
                         sizes=sizes, one_size=uniform, tile_hw=np.asarray(sizes, dtype=np.int32).reshape(T, 2))

    def _tile_params(self, nms_threshold: float, merge_threshold: float, edge_tolerance: float) -> _capi.OpdTileParams:
        return _capi.OpdTileParams(struct_size=C.sizeof(_capi.OpdTileParams), person_label=PERSON_LABEL, tile_nms_threshold=float(self.nms_threshold),
                                   merge_nms_threshold=float(nms_threshold), merge_threshold=float(merge_threshold), edge_tolerance=float(edge_tolerance))

    def _tiled_chunks(self, entry: str, frames: list, grid: _TileGrid, thresholds: tuple, staged: bool = True, features: Optional[str] = None, reid=None,
                      reid_slots: int = 0, floor_map=None, trackers=None) -> List[List[Detection]]:
        """Every fused tiled call: ``entry`` (a row of ``_TILED_ENTRIES``) on chunks of ``max_batch // tiles`` checked frames, its stage block filled
        from ``features`` / ``reid``, ``floor_map`` and ``trackers`` (``HipTracker``s, for the hybrid entry ``HipLightweightTracker``s; ``staged=False``:
        a null block, which ``opd_detr_detect_tiled_ragged`` alone takes), and the merged records made into detections: feature rows by position
        (colour) or by slot (Re-ID), floor rows and track ids by position, row ``b * S + k`` for record k of frame b.  Everything the native call
        reads or writes is a local of the loop and so outlives the call."""
        spelling, Block = _TILED_ENTRIES[entry]
        hybrid = Block is _capi.OpdTileHybrid
        call = getattr(self._lib, entry)
        S = grid.S
        params = self._tile_params(*thresholds)
        head = (grid.h, grid.w, grid.win.ctypes.data_as(C.c_void_p), grid.T, *grid.size_args(spelling), float(self.confidence_threshold), C.byref(params))
        per = max(1, self.max_batch // grid.T)
        out: List[List[Detection]] = []
        try:
            for i in range(0, len(frames), per):
                chunk = frames[i:i + per]
                n = len(chunk)
                recs, counts = (_capi.OpdTileDet * (n * S))(), (C.c_int32 * n)()
                ptrs = (C.c_void_p * n)(*[f.ctypes.data for f in chunk])
                st = feats = slot_map = n_person = floor = ids = None
                if Block is _capi.OpdTileStages and staged:
                    st = Block(struct_size=C.sizeof(Block), feature_kind=_capi.OPD_TRACK_FEAT_COLOR if features == "color" else _capi.OPD_TRACK_FEAT_NONE)
                    if features == "color" and trackers is None:
                        feats = np.empty((n, S, 256), np.float32)
                elif Block is _capi.OpdTileReidStages:   # a chunk shares its crop slots; with trackers the rows stay on the device
                    slots = max(1, min(int(reid_slots) * n, int(reid.max_crops)))
                    slot_map, n_person = np.full(slots, -1, np.int32), np.zeros(1, np.int32)
                    st = Block(struct_size=C.sizeof(Block), slots=slots, reid=reid._handle.value, slot_map=slot_map.ctypes.data, n_person=n_person.ctypes.data)
                    if trackers is None:
                        feats = np.empty((slots, int(reid.feature_dim)), np.float32)
                elif hybrid:
                    st = Block(struct_size=C.sizeof(Block))
                if feats is not None:
                    st.features = feats.ctypes.data
                if floor_map is not None:
                    floor = _floor_fields(st, floor_map, n * S)
                if trackers is not None:
                    for t in trackers[i:i + n]:
                        t._ensure(grid.h, grid.w) if hybrid else t._ensure()
                    ids, handles, n_featured = _tracker_fields(st, trackers[i:i + n], S)
                blocks = () if Block is None else (C.byref(st) if st is not None else None,)
                rc = call(C.c_void_p(self.model), ptrs, n, *head, *blocks, recs, counts)
                # a tracker out of slots: records, rows and ids were delivered (every record of that tracker -1: its mirror ages like the native side),
                # so the mirrors follow first and the error is raised behind them, with the message as the call left it
                if not (rc != 0 and ids is not None and not hybrid and "counted as one without detections" in _capi.last_error()):
                    _capi.check(rc, entry)
                message = _capi.last_error() if rc != 0 else ""
                chunk_dets = [self._tile_records(recs, b * S, int(counts[b])) for b in range(n)]
                for b, dets in enumerate(chunk_dets):
                    if floor is not None:
                        for k, det in enumerate(dets):
                            floor_map._fill(det, floor[b * S + k])
                    if hybrid:
                        chunk_dets[b] = trackers[i + b]._adopt(dets, ids[b * S:b * S + len(dets)].tolist())
                    elif ids is not None:
                        trackers[i + b]._apply(dets, ids[b * S:b * S + len(dets)])
                if slot_map is not None and feats is not None:
                    self._rows_by_slot(chunk, chunk_dets, S, feats, slot_map[:min(int(n_person[0]), len(slot_map))], reid)
                elif feats is not None:
                    for b, dets in enumerate(chunk_dets):
                        for det, row in zip(dets, feats[b, :len(dets)].copy()):
                            det.features = row
                out.extend(chunk_dets)
                if rc != 0:
                    raise RuntimeError(f"{entry} failed (code {rc}): {message}")
            self._last_orig = [(grid.h, grid.w)] * len(frames)
            return out
        except Exception as e:
            logger.error(f"Detection failed: {e}")
            raise

    @staticmethod
    def _rows_by_slot(chunk: list, chunk_dets: List[List[Detection]], S: int, feats: np.ndarray, slot_map: np.ndarray, reid) -> None:
        """Re-ID rows of a chunk: row k of ``feats`` belongs to merged record ``slot_map[k] = b * S + position``; the records beyond the slots get
        theirs through ONE standalone ``reid.extract_features_batch``."""
        row_of = {int(p): k for k, p in enumerate(slot_map)}
        missing = []
        for b, dets in enumerate(chunk_dets):
            for k, det in enumerate(dets):
                if b * S + k in row_of:
                    det.features = feats[row_of[b * S + k]].copy()
                else:
                    missing.append((b, k))
        if missing:
            rows = reid.extract_features_batch(chunk, [[chunk_dets[b][k].bbox for (bb, k) in missing if bb == b] for b in range(len(chunk))])
            for (b, k), row in zip(missing, rows):
                chunk_dets[b][k].features = row

    def _tiled_separate(self, plain, frames: list, tiles: list, thresholds: tuple, rows=None, floor_map=None, trackers=None, lwts=None) -> List[List[Detection]]:
        """Where the fused conditions fail, the separate calls one after the other: ``plain`` (``self.detect_tiled`` or ``self.detect_tiled_ragged``,
        looked up on the instance by the caller), then per frame ``lwts[f].update_with_detections``, the feature rows ``rows(frame, dets)``,
        ``floor_map.apply`` and ``trackers[f].update``, each where given."""
        out = plain(frames, tiles, *thresholds)
        for b, dets in enumerate(out):
            if lwts is not None:
                lwts[b].update_with_detections(frames[b], dets)
            if rows is not None:
                for det, row in zip(dets, rows(frames[b], dets)):
                    det.features = row
            if floor_map is not None:
                floor_map.apply(dets)
            if trackers is not None:
                trackers[b].update(dets)
        return out

    def detect_tiled_stages(self, frames: Sequence[np.ndarray], tiles: Sequence[Tuple[int, int, int, int]], nms_threshold: float = 0.4,
                            merge_threshold: float = 0.5, edge_tolerance: float = 0.01, features: Optional[str] = None, floor_map=None,
                            trackers=None) -> List[List[Detection]]:
        """``detect_tiled`` with the stages behind it in the same call.  (A method of its own: ``detect_tiled`` keeps the parameter list it has.)
        ``features="color"``, ``floor_map=`` (a ``HipFloorMapper``) and ``trackers=`` (one ``HipTracker`` per frame) run the stages of
        ``extract_color_features``, ``floor_map.apply`` and ``tracker.update`` on the merged records INSIDE the call, behind the same one host
        wait (``opd_detr_detect_tiled_stages``): ``det.features``, the four floor fields and ``track_id`` come back filled, with the bits the
        separate calls give.  With trackers the colour rows enter them on the device and ``det.features`` stays ``None``, as in
        ``detect_and_track``.  Where the fused conditions fail (a tracker or floor map on another GPU, ``max_dets`` below ``tiles x queries``, a
        ``feature_dim`` other than 256 with colour features, a frame side above 4096 with colour features) the separate calls run one after the
        other, with the same results.  With none of the three given this is ``detect_tiled`` itself."""
        return self._tiled_staged("opd_detr_detect_tiled_stages", self.detect_tiled, frames, tiles, (nms_threshold, merge_threshold, edge_tolerance), features, floor_map, trackers)

    def _tiled_staged(self, entry: str, plain, frames, tiles, thresholds: tuple, features: Optional[str], floor_map, trackers) -> List[List[Detection]]:
        """``detect_tiled_stages`` and ``detect_tiled_ragged``: ``entry`` for a grid of one size or for any grid, ``plain`` the method without stages."""
        self._require_model()
        frames, tiles = list(frames), [tuple(int(v) for v in t) for t in tiles]
        _check_tiled_features(features)
        trackers = _check_tracker_list(trackers, len(frames), "trackers")
        one_size = entry == "opd_detr_detect_tiled_stages"
        grid = self._tiled_geometry(frames, tiles, one_size)
        if grid is None:
            return []
        staged = not (features is None and floor_map is None and trackers is None)
        if one_size and not staged:
            return plain(frames, tiles, *thresholds)
        if staged and not self._tiled_stages_fused(grid.h, grid.w, grid.S, features, floor_map, trackers):
            return self._tiled_separate(plain, frames, tiles, thresholds, self.extract_color_features if features == "color" else None, floor_map, trackers)
        return self._tiled_chunks(entry, frames, grid, thresholds, staged=staged, features=features, floor_map=floor_map, trackers=trackers)

    def tile_model_sizes(self, tiles: Sequence[Tuple[int, int, int, int]]) -> List[Tuple[int, int]]:
        """The model size (H, W) of each ``(y0, x0, h, w)`` tile: ``model_input_size`` of its window under ``max_size``, the window itself with
        ``resize=False`` -- what ``detect_batch`` gives contiguous copies of the tiles."""
        return [model_input_size(int(t[2]), int(t[3]), self.max_size[0], self.max_size[1]) if self.resize else (int(t[2]), int(t[3])) for t in tiles]

    def detect_tiled_ragged(self, frames: Sequence[np.ndarray], tiles: Sequence[Tuple[int, int, int, int]], nms_threshold: float = 0.4,
                            merge_threshold: float = 0.5, edge_tolerance: float = 0.01, features: Optional[str] = None, floor_map=None,
                            trackers=None) -> List[List[Detection]]:
        """``detect_tiled`` / ``detect_tiled_stages`` for ``tiles`` that DIFFER in size (``opd_detr_detect_tiled_ragged``): a grid with interior
        tiles at the default overlap (2 x 3, 3 x 3, ...) or a frame side that does not divide.  Every tile gets the model size ``detect_batch``
        would give a contiguous copy of it (``tile_model_sizes``); the device resamples each window to that size into one zero-padded canvas,
        the forward runs as a ragged batch, and suppression, merge and the stages run as in the other tiled calls, behind one host wait.  The
        lists are those of ``TiledDetector(native=False)``, field for field.  Frames go in chunks of ``max_batch // len(tiles)``.
        ``features`` (``None`` or ``"color"``), ``floor_map`` and ``trackers`` as in ``detect_tiled_stages``, with the same fallback to the
        separate calls where the fused conditions fail.  Re-ID rows inside the call are a method of their own for such a grid,
        ``detect_tiled_ragged_reid``."""
        return self._tiled_staged("opd_detr_detect_tiled_ragged", self.detect_tiled_ragged, frames, tiles, (nms_threshold, merge_threshold, edge_tolerance), features, floor_map,
                                  trackers)

    def _tiled_stages_fused(self, h: int, w: int, S: int, features: Optional[str], floor_map, trackers) -> bool:
        """Whether the stages of a tiled call can run inside it (``detect_tiled`` has the conditions)."""
        color = features == "color"
        if color and (max(h, w) > 4096 or self._info.d_model != 256):
            return False
        if floor_map is not None and int(floor_map.device) != self.device_ordinal:
            return False
        for t in trackers or []:
            if t.device_ordinal != self.device_ordinal or t.max_dets < S or (color and t.feature_dim != 256):
                return False
        return True

    def detect_tiled_reid(self, frames: Sequence[np.ndarray], tiles: Sequence[Tuple[int, int, int, int]], reid, nms_threshold: float = 0.4,
                          merge_threshold: float = 0.5, edge_tolerance: float = 0.01, reid_slots: int = 32, floor_map=None,
                          trackers=None) -> List[List[Detection]]:
        """``detect_tiled`` with the Re-ID rows of ``reid`` (a loaded ``HipReIDExtractor`` / ``HipOSNetReIDExtractor``) for the merged records INSIDE
        the call (``opd_detr_detect_tiled_reid``): the crops are planned on the device from the merged records and cut from the whole frames where
        they were uploaded, the Re-ID forward runs in front of the call's one host wait.  Frames go in chunks of ``max_batch // len(tiles)``; a chunk
        of n frames shares ``min(reid_slots * n, reid.max_crops)`` crop slots, handed out in (frame, score) order.  Without ``trackers`` every
        detection comes back with ``det.features`` filled (records beyond the slots through one standalone ``reid.extract_features_batch``), so the
        lists equal ``detect_tiled`` + ``reid.extract_features`` (+ ``floor_map.apply``) whatever ``reid_slots`` is.  With ``trackers`` (one
        ``HipTracker`` per frame) the rows enter them on the device, ``det.features`` stays ``None`` and ``track_id`` is filled, as in
        ``detect_and_track``; a record beyond the slots enters without a feature.  Where the fused conditions fail (``reid`` without a native
        handle or on another GPU; a tracker on another GPU, with ``max_dets`` below ``tiles x queries`` or with a ``feature_dim`` other than the
        Re-ID model's; a floor map on another GPU) the separate calls run one after the other, with the same results."""
        return self._tiled_with_reid("opd_detr_detect_tiled_reid", self.detect_tiled, frames, tiles, reid, (nms_threshold, merge_threshold, edge_tolerance), reid_slots, floor_map,
                                     trackers)

    def _tiled_with_reid(self, entry: str, plain, frames, tiles, reid, thresholds: tuple, reid_slots: int, floor_map, trackers) -> List[List[Detection]]:
        """``detect_tiled_reid`` and ``detect_tiled_ragged_reid``: ``entry`` for a grid of one size or for any grid, ``plain`` the method without Re-ID."""
        self._require_model()
        frames, tiles = list(frames), [tuple(int(v) for v in t) for t in tiles]
        if reid is None:
            raise ValueError(f"{entry[len('opd_detr_'):]} needs reid= a loaded HipReIDExtractor or HipOSNetReIDExtractor")
        trackers = _check_tracker_list(trackers, len(frames), "trackers")
        grid = self._tiled_geometry(frames, tiles, entry == "opd_detr_detect_tiled_reid", reid)
        if grid is None:
            return []
        if not self._tiled_reid_fused(grid.S, reid, floor_map, trackers):
            return self._tiled_separate(plain, frames, tiles, thresholds, lambda frame, dets: reid.extract_features(frame, [d.bbox for d in dets]), floor_map, trackers)
        return self._tiled_chunks(entry, frames, grid, thresholds, reid=reid, reid_slots=reid_slots, floor_map=floor_map, trackers=trackers)

    def detect_tiled_ragged_reid(self, frames: Sequence[np.ndarray], tiles: Sequence[Tuple[int, int, int, int]], reid, nms_threshold: float = 0.4,
                                 merge_threshold: float = 0.5, edge_tolerance: float = 0.01, reid_slots: int = 32, floor_map=None,
                                 trackers=None) -> List[List[Detection]]:
        """``detect_tiled_reid`` for ``tiles`` that DIFFER in size (``opd_detr_detect_tiled_ragged_reid``): the source step and forward of
        ``detect_tiled_ragged``, and behind the seam merge the Re-ID, floor and track stages of ``detect_tiled_reid``, slots, rows and fallback
        to the separate calls included.  The lists equal ``detect_tiled_ragged`` + ``reid.extract_features`` (+ ``floor_map.apply``,
        + ``tracker.update``)."""
        return self._tiled_with_reid("opd_detr_detect_tiled_ragged_reid", self.detect_tiled_ragged, frames, tiles, reid, (nms_threshold, merge_threshold, edge_tolerance), reid_slots,
                                     floor_map, trackers)

    # ---- the hybrid tracker inside a tiled call --------------------------------------------------------------------------------------
    def _detect_tiled_any(self, frames, tiles, nms_threshold: float, merge_threshold: float, edge_tolerance: float) -> List[List[Detection]]:
        """``detect_tiled``, or for tiles of more than one size ``detect_tiled_ragged``: the separate call the hybrid tiled methods equal."""
        call = self.detect_tiled if len({(t[2], t[3]) for t in tiles}) == 1 else self.detect_tiled_ragged
        return call(frames, tiles, nms_threshold, merge_threshold, edge_tolerance)

    def _tile_records(self, recs, base: int, cnt: int) -> List[Detection]:
        dets = []
        for k in range(cnt):
            r = recs[base + k]
            bbox = (r.x, r.y, r.w, r.h)
            dets.append(Detection(bbox=bbox, confidence=float(r.score), class_id=int(r.label), class_name="person",
                                  camera_coords=(bbox[0] + bbox[2] / 2, bbox[1] + bbox[3]), features=None, query_index=int(r.query_index)))
        return dets

    def detect_tiled_hybrid(self, frames: Sequence[np.ndarray], tiles: Sequence[Tuple[int, int, int, int]], lwts, nms_threshold: float = 0.4,
                            merge_threshold: float = 0.5, edge_tolerance: float = 0.01, floor_map=None) -> List[List[Detection]]:
        """``detect_tiled`` (tiles of several sizes: ``detect_tiled_ragged``) and, per frame f, ``lwts[f].update_with_detections(frames[f], dets)``
        (+ ``floor_map.apply``) as ONE native call per chunk with one host wait (``opd_detr_detect_tiled_hybrid``): the merged records enter the
        ``HipLightweightTracker`` where the seam merge left them, and the gray pyramid of the new reference frame is built from the WHOLE frame
        the tiled source uploaded, not uploaded again.  Returns the merged detections with ``track_id`` set: same ids, track states and flow
        points as the separate calls.  Where a tracker is on another GPU or has ``max_tracks`` below ``tiles x queries`` (or the floor map is on
        another GPU) the separate calls run one after the other."""
        self._require_model()
        frames, tiles = list(frames), [tuple(int(v) for v in t) for t in tiles]
        lwts = _check_tracker_list(lwts, len(frames), "lwts")
        grid = self._tiled_geometry(frames, tiles, one_size=False)
        if grid is None:
            return []
        thresholds = (nms_threshold, merge_threshold, edge_tolerance)
        fused = all(t.device == self.device_ordinal and t.max_tracks >= grid.S for t in lwts) and (floor_map is None or int(floor_map.device) == self.device_ordinal)
        if not fused:
            return self._tiled_separate(self._detect_tiled_any, frames, tiles, thresholds, floor_map=floor_map, lwts=lwts)
        return self._tiled_chunks("opd_detr_detect_tiled_hybrid", frames, grid, thresholds, floor_map=floor_map, trackers=lwts)

    def track_tiled_hybrid_batch(self, frames: Sequence[np.ndarray], tiles: Sequence[Tuple[int, int, int, int]], lwt, key_frames: Sequence,
                                 nms_threshold: float = 0.4, merge_threshold: float = 0.5, edge_tolerance: float = 0.01) -> list:
        """``track_hybrid_batch`` on TILED frames of one camera: ``key_frames[f]`` true makes frame f a detection frame (``detect_tiled_hybrid``),
        false an in-between frame (``lwt.interpolate``).  One entry per frame: a ``List[Detection]`` (merged, ``track_id`` set) for a key frame, a
        ``List[(track_id, bbox)]`` for an in-between frame, ids and track states those of the per-frame loop.  The frames go down in runs of at
        most ``max_batch // len(tiles)`` key frames and 64 frames, each run ONE native call with one tiled forward and one host wait
        (``opd_detr_detect_tiled_sequence_hybrid``).  Where the conditions of ``detect_tiled_hybrid`` fail, the per-frame loop runs instead."""
        self._require_model()
        frames, tiles, keys = list(frames), [tuple(int(v) for v in t) for t in tiles], [bool(k) for k in key_frames]
        if len(keys) != len(frames):
            raise ValueError(f"{len(frames)} frames, {len(keys)} key flags")
        grid = self._tiled_geometry(frames, tiles, one_size=False)
        if grid is None:
            return []
        out: list = []
        for start, end in _hybrid_runs(keys, lwt.SEQUENCE_MAX, max(1, self.max_batch // len(tiles))):
            out.extend(self._track_tiled_hybrid_run(frames[start:end], tiles, grid, lwt, keys[start:end], (nms_threshold, merge_threshold, edge_tolerance)))
        return out

    def _track_tiled_hybrid_run(self, frames: list, tiles: list, grid: _TileGrid, lwt, keys: List[bool], thresholds: tuple) -> list:
        S = grid.S
        fused = lwt.device == self.device_ordinal and lwt.max_tracks >= S
        if fused and not any(keys) and not lwt._h:   # (no handle yet and no detection frame to make one: nothing to interpolate)
            fused = False
        if not fused:
            return [lwt.update_with_detections(f, self._detect_tiled_any([f], tiles, *thresholds)[0]) if k else lwt.interpolate(f) for f, k in zip(frames, keys)]
        lwt._ensure(grid.h, grid.w)
        params = self._tile_params(*thresholds)
        K, cap = sum(keys), lwt.max_tracks
        ptrs, flags, recs, counts, ids, lrecs, lcounts, done = _hybrid_run_buffers(frames, keys, _capi.OpdTileDet, S, cap)
        rc = self._lib.opd_detr_detect_tiled_sequence_hybrid(C.c_void_p(self.model), lwt._h, ptrs, flags, len(frames), grid.h, grid.w, grid.win.ctypes.data_as(C.c_void_p), grid.T,
                                                             *grid.size_args("HW,tile_HW"), float(self.confidence_threshold), C.byref(params), recs, counts, ids.ctypes.data,
                                                             lrecs, cap, lcounts, C.byref(done))
        _capi.check(rc, "opd_detr_detect_tiled_sequence_hybrid")
        self._last_orig = [(grid.h, grid.w)] * K
        return _hybrid_run_results(lwt, keys, [self._tile_records(recs, k * S, int(counts[k])) for k in range(K)], ids, S, lrecs, lcounts, cap)

    def _tiled_reid_fused(self, S: int, reid, floor_map, trackers) -> bool:
        """Whether the Re-ID stage of a tiled call can run inside it (``detect_tiled_reid`` has the conditions)."""
        if getattr(reid, "_handle", None) is None or reid._ordinal() != self.device_ordinal:
            return False
        if floor_map is not None and int(floor_map.device) != self.device_ordinal:
            return False
        for t in trackers or []:
            if t.device_ordinal != self.device_ordinal or t.max_dets < S or t.feature_dim != int(reid.feature_dim):
                return False
        return True

    def _detect_chunks_overlapped(self, chunks: List[List[np.ndarray]], floor_map=None) -> List[List[Detection]]:
        """Chunk k runs on handle ``k % streams``; one worker thread per handle drives its chunks in order.

        The C-ABI calls release the GIL and every handle owns its stream, so host preprocessing, uploads and the
        tail of one batch overlap the trunk of the next.  Each chunk's result is what the
        serial loop returns for it: the handles hold identical weights and the kernels are batch-invariant.
        """
        n = len(self._handles)
        results: List[Optional[List[List[Detection]]]] = [None] * len(chunks)
        filled = [True] * len(chunks)

        def worker(j: int) -> None:
            for k in range(j, len(chunks), n):
                results[k], filled[k] = self._detect_chunk(chunks[k], floor_map, self._handles[j])

        with ThreadPoolExecutor(max_workers=n) as pool:
            for fut in [pool.submit(worker, j) for j in range(min(n, len(chunks)))]:
                fut.result()
        for k, r in enumerate(results):   # (the mapper's own calls use ONE stream and staging buffer: made here, by one thread)
            if not filled[k]:
                for dets in r:
                    floor_map.apply(dets)
        return [dets for r in results for dets in r]

    def detect(self, frame: np.ndarray, floor_map=None) -> List[Detection]:
        """Single-frame detection (``yolov8_detector.py:90-132``); ``floor_map``: see ``detect_batch``."""
        self._require_model()
        self._sync_nms()
        try:
            dets, filled = self._detect_chunk([frame], floor_map)
            dets = dets[0]
            if not filled:
                floor_map.apply(dets)
            logger.debug(f"Detected {len(dets)} persons")
            return dets
        except Exception as e:
            logger.error(f"Detection failed: {e}")
            raise

    def detect_with_features(self, frame: np.ndarray, features: str = "encoder", reid=None,
                             reid_slots: int = 32) -> Tuple[List[Detection], np.ndarray]:
        """Detection + (N, 256) appearance features; assigns ``det.features`` (``yolov8_detector.py:134-159``).
        ``features="encoder"``: pooled from the DETR encoder map (deleted vit_detector.py 148-171, 224-273).
        ``features="color"``: the colour histogram of every detection's crop of ``frame``, the feature the reference's
        ``detect_with_features`` returns today (``yolov8_detector.py:161-190``).
        ``features="reid"``: the (N, 512) rows of ``reid`` (a loaded ``HipReIDExtractor`` / ``HipOSNetReIDExtractor``), what the
        reference's configured pipeline gets from ``ReIDFeatureExtractor.extract_features(frame, bboxes)`` after the detect
        call: here inside it, for the first ``reid_slots`` person records (``opd_detr_detect_frames_reid``)."""
        self._require_model()
        if features not in ("encoder", "color", "reid"):
            raise ValueError(f"features must be 'encoder', 'color' or 'reid', got {features!r}")
        self._sync_nms()
        if features == "reid":
            if reid is None:
                raise ValueError("features='reid' needs reid= a loaded HipReIDExtractor or HipOSNetReIDExtractor")
            return self._detect_with_reid(frame, reid, int(reid_slots))
        color = features == "color"
        target = self._frame_list_target([frame]) if (self.frame_lists and isinstance(frame, np.ndarray)) else None
        if target is not None and self._info.d_model == 256 and not (color and max(frame.shape[:2]) > 4096):
            # one C-ABI call: the records and the feature of every person record come back behind one host wait
            Q, D = self._info.num_queries, self._info.d_model
            recs, counts = (_capi.OpdDet * Q)(), (C.c_int32 * 1)()
            feats = np.empty((1, Q, D), np.float32)
            ptrs = (C.c_void_p * 1)(frame.ctypes.data)
            name = "opd_detr_detect_frames_color" if color else "opd_detr_detect_frames_features"
            rc = getattr(self._lib, name)(C.c_void_p(self.model), ptrs, 1, int(frame.shape[0]), int(frame.shape[1]), target[0], target[1],
                                          float(self.confidence_threshold), PERSON_LABEL, recs, counts,
                                          feats.ctypes.data_as(C.POINTER(C.c_float)))
            _capi.check(rc, name)
            self._last_orig = [(int(frame.shape[0]), int(frame.shape[1]))]
            detections = self._postprocess_batch(recs, counts, Q)[0]
            features = feats[0, [d.query_index for d in detections]] if detections else np.array([])
            for i, det in enumerate(detections):
                det.features = features[i]
            return detections, features
        detections = self.detect(frame)
        features = self.extract_color_features(frame, detections) if color else self.extract_features(frame, detections)
        for i, det in enumerate(detections):
            if i < len(features):
                det.features = features[i]
        return detections, features

    def _detect_with_reid(self, frame: np.ndarray, reid, slots: int) -> Tuple[List[Detection], np.ndarray]:
        if not reid.is_loaded:
            raise RuntimeError("Re-ID model is not loaded: call load_model() first")
        slots = max(1, min(slots, int(reid.max_crops)))
        target = self._frame_list_target([frame]) if (self.frame_lists and isinstance(frame, np.ndarray)) else None
        E = int(reid.feature_dim)
        if target is None or reid._ordinal() != self.device_ordinal:   # (ragged or pre-resized chunk, or another GPU: two calls)
            detections = self.detect(frame)
            rows = reid.extract_features(frame, [d.bbox for d in detections])
        else:
            # one C-ABI call: the records and the Re-ID row of every person record (up to `slots`) come back behind one host wait
            Q = self._info.num_queries
            recs, counts = (_capi.OpdDet * Q)(), (C.c_int32 * 1)()
            feats, slot_map, n_person = np.empty((slots, E), np.float32), np.empty(slots, np.int32), C.c_int32(0)
            ptrs = (C.c_void_p * 1)(frame.ctypes.data)
            rc = self._lib.opd_detr_detect_frames_reid(C.c_void_p(self.model), reid._handle, ptrs, 1, int(frame.shape[0]), int(frame.shape[1]),
                                                       target[0], target[1], float(self.confidence_threshold), PERSON_LABEL, slots, recs, counts,
                                                       feats.ctypes.data, slot_map.ctypes.data, C.byref(n_person))
            _capi.check(rc, "opd_detr_detect_frames_reid")
            self._last_orig = [(int(frame.shape[0]), int(frame.shape[1]))]
            detections = self._postprocess_batch(recs, counts, Q)[0]
            row_of = {int(q): k for k, q in enumerate(slot_map[:min(int(n_person.value), slots)])}   # (one frame: slot = query_index)
            rows = np.zeros((len(detections), E), np.float32)
            missing = [i for i, d in enumerate(detections) if d.query_index not in row_of]
            for i, d in enumerate(detections):
                if d.query_index in row_of:
                    rows[i] = feats[row_of[d.query_index]]
            if missing:   # more person records than slots: the remainder through the standalone call
                rows[missing] = reid.extract_features(frame, [detections[i].bbox for i in missing])
        for i, det in enumerate(detections):
            det.features = rows[i]
        return detections, rows

    def detect_and_track(self, frame: np.ndarray, tracker, features: Optional[str] = "color", reid=None, reid_slots: int = 32) -> List[Detection]:
        """``detect_with_features(frame)`` followed by ``tracker.update(detections)`` (the reference's loop, ``detection.py:91-94`` and
        ``tracking.py:183-210``) as ONE native call with one host wait: the kept records and their feature rows enter ``tracker`` (a
        ``HipTracker``) where they lie on the device (``opd_detr_detect_frames_track``).  Returns what ``tracker.update`` returns, the
        detections that got an id; ``det.features`` stays ``None`` since the rows never leave the device.  ``features``: ``"encoder"``,
        ``"color"``, ``"reid"`` (with ``reid=``) or ``None`` for motion only.  Needs ``device_nms=True``, a frame that goes down as a frame
        list and all handles on one GPU; otherwise the two calls run one after the other, with the same ids and track states."""
        self._require_model()
        kind = _track_feature_kind(features, reid)
        self._sync_nms()
        target = self._fused_track_target([frame], tracker, features, reid)
        Q = self._info.num_queries
        fused = target is not None
        if not fused:
            if features is None:
                return tracker.update(self.detect(frame))
            return tracker.update(self.detect_with_features(frame, features=features, reid=reid, reid_slots=reid_slots)[0])
        tracker._ensure()
        slots = max(1, min(int(reid_slots), int(reid.max_crops), int(tracker.max_dets))) if features == "reid" else 0
        recs, counts = (_capi.OpdDet * Q)(), (C.c_int32 * 1)()
        ids, n_featured = np.full(Q, -1, np.int32), np.zeros(1, np.int32)
        ptrs, handles = (C.c_void_p * 1)(frame.ctypes.data), (C.c_void_p * 1)(tracker._h.value)
        rc = self._lib.opd_detr_detect_frames_track(C.c_void_p(self.model), reid._handle if features == "reid" else None, handles, ptrs, 1, int(frame.shape[0]),
                                                    int(frame.shape[1]), target[0], target[1], float(self.confidence_threshold), PERSON_LABEL, kind, slots,
                                                    recs, counts, ids.ctypes.data, n_featured.ctypes.data)
        if rc != 0 and "counted as one without detections" in _capi.last_error():
            tracker._apply([], ids[:0])   # out of slots: as in HipTracker.update, the mirror follows before the error is raised
        _capi.check(rc, "opd_detr_detect_frames_track")
        self._last_orig = [(int(frame.shape[0]), int(frame.shape[1]))]
        detections = self._postprocess_batch(recs, counts, Q)[0]
        tracker._apply(detections, ids[:len(detections)])
        return [det for det in detections if det.track_id is not None]

    def detect_and_track_hybrid(self, frame: np.ndarray, lwt) -> List[Detection]:
        """``dets = self.detect(frame); lwt.update_with_detections(frame, dets)`` (the detection frame of the reference's hybrid mode,
        ``tracking.py`` with ``hybrid_mode.enabled``) as ONE native call with one host wait (``opd_detr_detect_frames_hybrid``): the kept
        records enter ``lwt`` (a ``HipLightweightTracker``) where they lie on the device, and the gray pyramid of the new reference frame
        is built from the frame the detector has uploaded already.  Returns the detections with ``track_id`` set; same ids, track states
        and flow points as the two calls.  Needs ``device_nms=True``, a frame that goes down as a frame list, both handles on one GPU and
        ``lwt.max_tracks >= num_queries``; otherwise the two calls run one after the other.  No feature rows: ``det.features`` is None."""
        self._require_model()
        self._sync_nms()
        target = self._frame_list_target([frame]) if (self.frame_lists and isinstance(frame, np.ndarray)) else None
        Q = self._info.num_queries
        if self._nms_set is None or target is None or lwt.device != self.device_ordinal or lwt.max_tracks < Q:
            return lwt.update_with_detections(frame, self.detect(frame))
        h, w = int(frame.shape[0]), int(frame.shape[1])
        lwt._ensure(h, w)
        recs, counts = (_capi.OpdDet * Q)(), (C.c_int32 * 1)()
        ids = np.full(Q, -1, np.int32)
        ptrs, handles = (C.c_void_p * 1)(frame.ctypes.data), (C.c_void_p * 1)(lwt._h.value)
        rc = self._lib.opd_detr_detect_frames_hybrid(C.c_void_p(self.model), handles, ptrs, 1, h, w, target[0], target[1], float(self.confidence_threshold),
                                                     PERSON_LABEL, recs, counts, ids.ctypes.data)
        _capi.check(rc, "opd_detr_detect_frames_hybrid")
        self._last_orig = [(h, w)]
        detections = self._postprocess_batch(recs, counts, Q)[0]
        return lwt._adopt(detections, ids[:len(detections)].tolist())

    def track_hybrid_batch(self, frames: Sequence[np.ndarray], lwt, key_frames: Sequence) -> list:
        """The reference's hybrid loop over CONSECUTIVE frames of one camera: ``key_frames[f]`` true makes frame f a detection frame
        (``detect_and_track_hybrid``), false an in-between frame (``lwt.interpolate``).  Returns one entry per frame: a ``List[Detection]``
        for a key frame, a ``List[(track_id, bbox)]`` for an in-between frame -- what the per-frame loop returns, ids and track states
        included.  The frames go down in runs of at most ``max_batch`` key frames and 64 frames, each run ONE native call with one batched
        forward and one host wait (``opd_detr_detect_sequence_hybrid``).  Where the conditions of ``detect_and_track_hybrid`` fail, the
        per-frame loop runs instead."""
        self._require_model()
        frames, keys = list(frames), [bool(k) for k in key_frames]
        if len(keys) != len(frames):
            raise ValueError(f"{len(frames)} frames, {len(keys)} key flags")
        out: list = []
        for start, end in _hybrid_runs(keys, lwt.SEQUENCE_MAX, self.max_batch):
            out.extend(self._track_hybrid_run(frames[start:end], lwt, keys[start:end]))
        return out

    def _track_hybrid_run(self, frames: List[np.ndarray], lwt, keys: List[bool]) -> list:
        self._sync_nms()
        target = self._frame_list_target(frames) if (self.frame_lists and all(isinstance(f, np.ndarray) for f in frames)) else None
        Q = self._info.num_queries
        fused = self._nms_set is not None and target is not None and lwt.device == self.device_ordinal and lwt.max_tracks >= Q
        h, w = (int(frames[0].shape[0]), int(frames[0].shape[1])) if target is not None else (0, 0)
        if fused and not any(keys) and not lwt._h:   # (no handle yet and no detection frame to make one: nothing to interpolate)
            fused = False
        if not fused:
            return [lwt.update_with_detections(f, self.detect(f)) if k else lwt.interpolate(f) for f, k in zip(frames, keys)]
        lwt._ensure(h, w)
        K, cap = sum(keys), lwt.max_tracks
        ptrs, flags, recs, counts, ids, lrecs, lcounts, done = _hybrid_run_buffers(frames, keys, _capi.OpdDet, Q, cap)
        rc = self._lib.opd_detr_detect_sequence_hybrid(C.c_void_p(self.model), lwt._h, ptrs, flags, len(frames), h, w, target[0], target[1], float(self.confidence_threshold),
                                                       PERSON_LABEL, recs, counts, ids.ctypes.data, lrecs, cap, lcounts, C.byref(done))
        _capi.check(rc, "opd_detr_detect_sequence_hybrid")
        self._last_orig = [(h, w)] * K
        return _hybrid_run_results(lwt, keys, self._postprocess_batch(recs, counts, Q) if K else [], ids, Q, lrecs, lcounts, cap)

    def _fused_track_target(self, frames: Sequence[np.ndarray], tracker, features: Optional[str], reid) -> Optional[Tuple[int, int]]:
        """The model input size when ``frames`` can enter ``tracker`` inside the detect call (``detect_and_track`` has the conditions), else None."""
        target = self._frame_list_target(frames) if (self.frame_lists and all(isinstance(f, np.ndarray) for f in frames)) else None
        Q = self._info.num_queries
        width = {None: None, "encoder": self._info.d_model, "color": 256, "reid": int(reid.feature_dim) if reid is not None else None}[features]
        fused = (self._nms_set is not None and target is not None and tracker.device_ordinal == self.device_ordinal and tracker.max_dets >= Q
                 and (width is None or tracker.feature_dim == width))
        if features in ("encoder", "color"):
            fused = fused and self._info.d_model == 256 and not (features == "color" and max(frames[0].shape[:2]) > 4096)
        if features == "reid":
            fused = fused and reid._ordinal() == self.device_ordinal
        return target if fused else None

    def detect_and_track_batch(self, frames: Sequence[np.ndarray], tracker, features: Optional[str] = "color", reid=None, reid_slots: int = 32) -> List[List[Detection]]:
        """``[self.detect_and_track(f, tracker, ...) for f in frames]`` for CONSECUTIVE frames of one camera, in chunks of ``max_batch``: each chunk
        is ONE native call with one batched forward and one host wait (``opd_detr_detect_sequence_track``); the association between the frames
        of a chunk runs on the device.  Same ids and track states as the loop.  For Re-ID a chunk shares
        ``min(max_crops, max_dets, reid_slots * len(chunk))`` crop slots, handed out in (frame, score) order.  Where the conditions of the fused
        single-frame call fail, the loop runs instead."""
        self._require_model()
        kind = _track_feature_kind(features, reid)
        frames = list(frames)
        out: List[List[Detection]] = []
        for start in range(0, len(frames), self.max_batch):
            chunk = frames[start:start + self.max_batch]
            self._sync_nms()
            target = self._fused_track_target(chunk, tracker, features, reid)
            if target is None:
                out.extend(self.detect_and_track(f, tracker, features=features, reid=reid, reid_slots=reid_slots) for f in chunk)
                continue
            tracker._ensure()
            B, Q = len(chunk), self._info.num_queries
            slots = max(1, min(int(reid.max_crops), int(tracker.max_dets), int(reid_slots) * B)) if features == "reid" else 0
            recs, counts = (_capi.OpdDet * (B * Q))(), (C.c_int32 * B)()
            ids, n_featured, done = np.full(B * Q, -1, np.int32), np.zeros(B, np.int32), C.c_int32(0)
            ptrs = (C.c_void_p * B)(*[f.ctypes.data for f in chunk])
            h, w = int(chunk[0].shape[0]), int(chunk[0].shape[1])
            rc = self._lib.opd_detr_detect_sequence_track(C.c_void_p(self.model), reid._handle if features == "reid" else None, tracker._h, ptrs, B, h, w, target[0],
                                                          target[1], float(self.confidence_threshold), PERSON_LABEL, kind, slots, recs, counts, ids.ctypes.data,
                                                          n_featured.ctypes.data, C.byref(done))
            if rc != 0 and "counted as one without detections" not in _capi.last_error():
                _capi.check(rc, "opd_detr_detect_sequence_track")
            self._last_orig = [(h, w)] * B
            per_frame = self._postprocess_batch(recs, counts, Q)
            out.extend(tracker._replay(per_frame, ids, done.value, rc, "opd_detr_detect_sequence_track", stride=Q))
        return out

    def detect_and_track_streams(self, frames_per_camera: Sequence[Sequence[np.ndarray]], trackers: Sequence, features: Optional[str] = "color", reid=None,
                                 reid_slots: int = 32) -> List[List[List[Detection]]]:
        """``[self.detect_and_track_batch(f, t, ...) for f, t in zip(frames_per_camera, trackers)]`` with the cameras in ONE native call
        (``opd_detr_detect_streams_track``): one forward over up to ``max_batch`` frames of up to 64 cameras, one host wait, and the cameras'
        tracker steps side by side on the device.  ``tracker.plan_stream_calls`` cuts longer runs into calls; the results do not depend on
        the cut.  Same ids and track states as the per-camera calls.  Where the conditions of ``detect_and_track`` fail for a tracker, or the
        cameras' frames differ in size, the per-camera ``detect_and_track_batch`` runs instead.  Where a camera runs out of slots it stops
        as under ``detect_and_track_batch``; the other cameras of that call finish, then the error is raised."""
        from .tracker import HipTracker, plan_stream_calls
        self._require_model()
        kind = _track_feature_kind(features, reid)
        per_camera, trackers = [list(f) for f in frames_per_camera], list(trackers)
        if len(trackers) != len(per_camera):
            raise ValueError(f"{len(trackers)} trackers for {len(per_camera)} cameras")
        if len({id(t) for t in trackers}) != len(trackers):
            raise ValueError("a tracker is named twice; a tracker follows one camera")
        self._sync_nms()
        every = [f for cam in per_camera for f in cam]
        sizes = {(f.shape[0], f.shape[1]) if isinstance(f, np.ndarray) else None for f in every}
        if not every or len(sizes) != 1 or any(self._fused_track_target(every[:1], t, features, reid) is None for t in trackers):
            return [self.detect_and_track_batch(f, t, features=features, reid=reid, reid_slots=reid_slots) for f, t in zip(per_camera, trackers)]
        out: List[List[List[Detection]]] = [[] for _ in trackers]
        Q = self._info.num_queries
        for call in plan_stream_calls([len(cam) for cam in per_camera], self.max_batch):
            cams = [trackers[c] for c, _, _ in call]
            runs = [per_camera[c][a:b] for c, a, b in call]
            chunk = [f for run in runs for f in run]   # camera after camera; the native side steps across them
            target = self._fused_track_target(chunk, cams[0], features, reid)
            if target is None:   # (a frame that cannot go down as a frame list)
                for (c, a, b), t in zip(call, cams):
                    out[c].extend(self.detect_and_track_batch(per_camera[c][a:b], t, features=features, reid=reid, reid_slots=reid_slots))
                continue
            for t in cams:
                t._ensure()
            B = len(chunk)
            camera_of = np.array([i for i, run in enumerate(runs) for _ in run], np.int32)
            slots = max(1, min(int(reid.max_crops), min(int(t.max_dets) for t in cams), int(reid_slots) * B)) if features == "reid" else 0
            recs, counts = (_capi.OpdDet * (B * Q))(), (C.c_int32 * B)()
            ids, n_featured, done = np.full(B * Q, -1, np.int32), np.zeros(B, np.int32), np.zeros(len(cams), np.int32)
            ptrs = (C.c_void_p * B)(*[f.ctypes.data for f in chunk])
            handles = (C.c_void_p * len(cams))(*[t._h.value for t in cams])
            h, w = int(chunk[0].shape[0]), int(chunk[0].shape[1])
            rc = self._lib.opd_detr_detect_streams_track(C.c_void_p(self.model), reid._handle if features == "reid" else None, handles, len(cams),
                                                         camera_of.ctypes.data_as(C.c_void_p), ptrs, B, h, w, target[0], target[1], float(self.confidence_threshold),
                                                         PERSON_LABEL, kind, slots, recs, counts, ids.ctypes.data, n_featured.ctypes.data, done.ctypes.data)
            if rc != 0 and "counted as one without detections" not in _capi.last_error():
                _capi.check(rc, "opd_detr_detect_streams_track")
            message = _capi.last_error() if rc != 0 else ""
            self._last_orig = [(h, w)] * B
            per_frame = self._postprocess_batch(recs, counts, Q)
            dets, at = [], 0
            for run in runs:
                dets.append(per_frame[at:at + len(run)])
                at += len(run)
            err = HipTracker._replay_streams(cams, dets, ids, done, rc, "opd_detr_detect_streams_track", out, [c for c, _, _ in call], stride=Q, message=message)
            if err is not None:
                raise err
        return out

    def extract_color_features(self, frame: np.ndarray, detections: List[Detection]) -> np.ndarray:
        """(N, 256) float32 colour-histogram features of the detections' crops of ``frame`` (BGR uint8 ``[H, W, 3]``), on the
        device: ``FeatureExtractor.extract_batch`` on the crops ``YOLOv8Detector.extract_features`` cuts
        (``yolov8_detector.py:161-190``).  Boxes travel as float32, as in ``extract_features``.  Returns ``np.array([])`` for no
        detections (``yolov8_detector.py:171-172``)."""
        if len(detections) == 0:
            return np.array([])
        if not isinstance(frame, np.ndarray) or frame.dtype != np.uint8 or frame.ndim != 3 or frame.shape[2] != 3:
            raise ValueError("frame must be a uint8 [H, W, 3] BGR array")
        frame = np.ascontiguousarray(frame)
        boxes = np.ascontiguousarray(np.asarray([d.bbox for d in detections], dtype=np.float32).reshape(-1, 4))
        hw = np.array(frame.shape[:2], np.int32)
        feats = np.empty((len(boxes), 256), np.float32)
        ptrs = (C.c_void_p * 1)(frame.ctypes.data)
        lib = self._lib or _capi.load_library()   # (needs no model handle)
        rc = lib.opd_color_features(int(self.device_ordinal), ptrs, hw.ctypes.data_as(C.c_void_p), 1, _capi.OPD_MEM_HOST,
                                    boxes.ctypes.data_as(C.c_void_p), None, len(boxes), feats.ctypes.data_as(C.c_void_p))
        _capi.check(rc, "opd_color_features")
        return feats

    def extract_features(self, frame: np.ndarray, detections: List[Detection]) -> np.ndarray:
        """ROI mean-pool + L2 norm on the encoder map of the LAST forward (frame 0), on the device
        (``src/tracking/feature_extractor.py:39-88``).  Returns ``np.array([])`` when there is nothing to pool
        (``yolov8_detector.py:171-172``)."""
        self._require_model()
        if len(detections) == 0:
            return np.array([])
        boxes = np.asarray([d.bbox for d in detections], dtype=np.float32).reshape(-1, 4)
        feats = np.empty((len(detections), self._info.d_model), np.float32)
        for s in range(0, len(detections), 128):
            chunk = np.ascontiguousarray(boxes[s:s + 128])
            rc = self._lib.opd_detr_roi_features(C.c_void_p(self.model), 0, chunk.ctypes.data_as(C.c_void_p), len(chunk),
                                                 int(frame.shape[0]), int(frame.shape[1]),
                                                 feats[s:s + 128].ctypes.data_as(C.c_void_p))
            _capi.check(rc, "opd_detr_roi_features")
        return feats

    def _get_foot_position(self, bbox: Tuple[float, float, float, float]) -> Tuple[float, float]:
        """Centre of the bottom edge (``yolov8_detector.py:229-241``)."""
        x, y, w, h = bbox
        return (x + w / 2, y + h)

    def get_attention_map(self, frame: np.ndarray, layer_index: int = -1) -> Optional[np.ndarray]:
        """Attention map for visualisation (deleted vit_detector.py 392-446; ``Visualizer.draw_attention_map``,
        ``src/visualization/visualizer.py:148-200``, takes a 1-D or 2-D array in [0, 1]).  The DETR-era source is gone, so the
        definition is this build's: detect on ``frame``, then the decoder's cross-attention weights of layer ``layer_index``,
        averaged over the heads and over the queries of the kept person detections (all queries when there is none), as a
        ``(feature_h, feature_w)`` float32 array scaled so that its maximum is 1.  Like the reference's detector this call is
        single-threaded: the map is read from the state the ``detect`` inside it leaves on handle 0, so no other call on this
        detector may run between the two (the library refuses a map that does not fit the buffer sized here)."""
        self._require_model()
        dets = self.detect(frame)
        fh, fw = (_feature_hw(s) for s in self._model_hw(frame))
        q = np.asarray(sorted({d.query_index for d in dets if d.query_index is not None}), dtype=np.int32)
        out = np.empty((fh * fw,), np.float32)
        rc = self._lib.opd_detr_attention_map(C.c_void_p(self.model), 0, int(layer_index), q.ctypes.data_as(C.c_void_p) if len(q) else None,
                                              len(q), out.ctypes.data_as(C.c_void_p), int(out.size))
        _capi.check(rc, "opd_detr_attention_map")
        mx = float(out.max())
        return (out / mx if mx > 0 else out).reshape(fh, fw)

    def _model_hw(self, frame: np.ndarray) -> Tuple[int, int]:
        """Model-input size of a frame under this detector's resize policy."""
        if self.resize:
            return model_input_size(frame.shape[0], frame.shape[1], self.max_size[0], self.max_size[1])
        return int(frame.shape[0]), int(frame.shape[1])

    # ------------------------------------------------------------------------------------------------------------
    def set_profiling(self, enabled: bool) -> None:
        self._require_model()
        _capi.check(self._lib.opd_detr_set_profiling(C.c_void_p(self.model), int(enabled)), "opd_detr_set_profiling")

    def stage_times_ms(self) -> List[float]:
        self._require_model()
        ms = (C.c_float * 8)()
        _capi.check(self._lib.opd_detr_stage_times(C.c_void_p(self.model), ms), "opd_detr_stage_times")
        return [float(v) for v in ms]


def _feature_hw(n: int) -> int:
    """Spatial size after the stem (s2), max-pool (s2) and three stride-2 stages: five times ⌊(n-1)/2⌋+1."""
    for _ in range(5):
        n = (n - 1) // 2 + 1
    return n
