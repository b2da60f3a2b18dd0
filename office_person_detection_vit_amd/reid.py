"""Re-ID appearance features on the device: the CLIP ViT image tower behind the reference's ``ReIDFeatureExtractor`` surface.

``HipReIDExtractor`` mirrors ``ReIDFeatureExtractor`` (reference ``src/tracking/reid_feature_extractor.py:369-463``) with
``model_type="clip"``: ``extract_features(image, bboxes)`` returns float32 ``(N, 512)`` rows of unit norm, computed by
``opd_reid_extract`` (``include/opd_detr.h``): crop, BGR -> RGB, Pillow-exact bicubic resize + centre crop + normalisation, the
ViT forward and the L2 normalisation all run in HIP kernels (``csrc/kernels_reid.hip``).  Weights come from a local safetensors
file; nothing is downloaded.

``HipOSNetReIDExtractor`` mirrors the reference's ``OSNetReIDExtractor`` (lines 175-365): torchreid's ``osnet_x1_0`` without its
classifier, Pillow-exact bilinear resize to 256 x 128 and ImageNet normalisation, all on the device (``csrc/kernels_osnet.hip``),
from a local ``.safetensors`` or torchreid ``.pth`` / ``.pth.tar`` file.  ``create_reid_extractor`` is the façade's dispatch.

Either extractor can also be handed to ``HipDetrDetector.detect_with_features(frame, features="reid", reid=extractor)``: the rows
then come back inside the detect call (``opd_detr_detect_frames_reid``), the same bits as ``extract_features(frame, bboxes)``.
"""

from __future__ import annotations

import contextlib
import ctypes as C
import os
import tempfile
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _capi

BBox = Tuple[float, float, float, float]


def _resolve_weights(model_path: Optional[str], model_name: Optional[str]) -> str:
    for cand in (model_path, model_name):
        if not cand:
            continue
        if os.path.isdir(cand):
            for fn in ("model.safetensors", "pytorch_model.safetensors"):
                if os.path.isfile(os.path.join(cand, fn)):
                    return os.path.join(cand, fn)
            raise FileNotFoundError(f"no model.safetensors in the local directory {cand!r} (this build never downloads weights)")
        if os.path.isfile(cand):
            return cand
        if cand is model_path:
            raise FileNotFoundError(f"CLIP weight file {cand!r} does not exist (this build never downloads weights)")
    raise FileNotFoundError(f"CLIP weights not found locally (model_path={model_path!r}, model_name={model_name!r}); this build never "
                            "downloads weights: pass model_path= a safetensors file or model_name= a local directory")


class _ReIDExtractorBase:
    """Lifecycle and ``extract_*`` of one ``opd_reid`` handle.  A subclass states ``model_type``, the C-ABI's model code, the label of
    its error messages, how its weight file is found (``_resolve``) and, if the file needs converting, ``_weights_file``."""

    def __init__(self, model_name: Optional[str], model_path: Optional[str], device: str, max_crops: int, use_graph: bool):
        self.model_type = type(self).model_type
        self.model_name = model_name
        self.model_path = model_path
        self.device = device
        self.max_crops = int(max_crops)
        self.use_graph = use_graph
        self._handle: Optional[C.c_void_p] = None
        self._feature_dim = 512

    # ---- lifecycle ---------------------------------------------------------------------------------------------------------------
    def _ordinal(self) -> int:
        d = str(self.device)
        return int(d.split(":", 1)[1]) if ":" in d else 0

    @contextlib.contextmanager
    def _weights_file(self, path: str):
        yield path

    def load_model(self) -> None:
        if self._handle is not None:
            return
        path = self._resolve()
        lib = _capi.load_library()
        cfg = _capi.OpdReidConfig()
        cfg.struct_size = C.sizeof(_capi.OpdReidConfig)
        cfg.max_crops = self.max_crops
        cfg.flags = 0 if self.use_graph else _capi.OPD_FLAG_NO_GRAPH
        cfg.model = self._model_code
        h = C.c_void_p()
        with self._weights_file(path) as wpath:
            rc = lib.opd_reid_create(C.byref(cfg), wpath.encode(), self._ordinal(), C.byref(h))
        if rc != 0:
            raise RuntimeError(f"Failed to load {self._model_label} Re-ID model: {_capi.last_error()} (code {rc})")
        self._handle = h
        info = _capi.OpdReidModelInfo()
        _capi.check(lib.opd_reid_info(h, C.byref(info)), "opd_reid_info")
        self._feature_dim = int(info.feature_dim)
        self.info = info

    def cleanup(self) -> None:
        if self._handle is not None:
            _capi.load_library().opd_reid_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.cleanup()
        except Exception:
            pass

    @property
    def is_loaded(self) -> bool:
        return self._handle is not None

    @property
    def feature_dim(self) -> int:
        return self._feature_dim

    # ---- features ----------------------------------------------------------------------------------------------------------------
    def extract_features(self, image: np.ndarray, bboxes: Sequence[BBox]) -> np.ndarray:
        """``image`` = uint8 [H][W][3] BGR frame, ``bboxes`` = (x, y, w, h) in pixels -> float32 (N, feature_dim), unit rows."""
        return self.extract_features_batch([image], [bboxes])

    def extract_features_batch(self, frames: Sequence[np.ndarray], bboxes_per_frame: Sequence[Sequence[BBox]]) -> np.ndarray:
        """Many frames in one call: the boxes of every frame, in order, -> float32 (sum of counts, feature_dim)."""
        if not self.is_loaded:
            raise RuntimeError("Re-ID model is not loaded: call load_model() first")
        if len(frames) != len(bboxes_per_frame):
            raise ValueError("frames and bboxes_per_frame differ in length")
        boxes: List[BBox] = []
        owner: List[int] = []
        for f, bb in enumerate(bboxes_per_frame):
            for b in bb:
                boxes.append(tuple(float(v) for v in b))
                owner.append(f)
        n = len(boxes)
        out = np.zeros((n, self._feature_dim), dtype=np.float32)
        if n == 0:
            return out
        keep = []
        ptrs = (C.c_void_p * len(frames))()
        hw = np.zeros((len(frames), 2), dtype=np.int32)
        for f, fr in enumerate(frames):
            a = np.ascontiguousarray(fr, dtype=np.uint8)
            if a.ndim != 3 or a.shape[2] != 3:
                raise ValueError(f"frame {f} must be uint8 [H][W][3] BGR, got shape {a.shape}")
            keep.append(a)
            ptrs[f] = a.ctypes.data
            hw[f] = a.shape[:2]
        bx = np.asarray(boxes, dtype=np.float32).reshape(n, 4)
        own = np.asarray(owner, dtype=np.int32)
        rc = _capi.load_library().opd_reid_extract(self._handle, ptrs, hw.ctypes.data, len(frames), _capi.OPD_MEM_HOST, bx.ctypes.data,
                                                   own.ctypes.data, n, out.ctypes.data)
        _capi.check(rc, "opd_reid_extract")
        return out

    def extract_single(self, crop: np.ndarray) -> np.ndarray:
        """Features of one already-cropped BGR image: (feature_dim,)."""
        h, w = crop.shape[:2]
        return self.extract_features(crop, [(0.0, 0.0, float(w), float(h))])[0]


def torchreid_state_dict(path: str) -> "dict[str, np.ndarray]":
    """The float tensors of a torchreid checkpoint (``.pth`` / ``.pth.tar``) as torchreid's ``load_pretrained_weights`` sees them:
    ``state_dict`` unwrapped when present, a ``module.`` prefix stripped, ``classifier.*`` dropped.  Read with
    ``torch.load(map_location="cpu", weights_only=True)``; torch is imported only here."""
    import torch
    ck = torch.load(path, map_location="cpu", weights_only=True)
    sd = ck["state_dict"] if isinstance(ck, dict) and "state_dict" in ck else ck
    out = {}
    for k, v in sd.items():
        if k.startswith("module."):
            k = k[7:]
        if k.startswith("classifier.") or not torch.is_tensor(v) or not v.is_floating_point():
            continue
        out[k] = v.detach().float().contiguous().numpy()
    return out


class HipReIDExtractor(_ReIDExtractorBase):
    """Drop-in for the reference's ``ReIDFeatureExtractor(model_type="clip")``."""

    model_type = "clip"
    _model_code = _capi.OPD_REID_MODEL_CLIP
    _model_label = "CLIP"

    def __init__(self, model_type: str = "clip", model_name: Optional[str] = None, model_path: Optional[str] = None,
                 device: str = "hip:0", max_crops: int = 64, use_graph: bool = True):
        model_type = str(model_type).lower()   # (the reference lower-cases it too)
        if model_type != "clip":
            raise ValueError(f"HipReIDExtractor runs CLIP only, not model_type {model_type!r}: use HipOSNetReIDExtractor for 'osnet', "
                             "or create_reid_extractor(model_type=...)")
        super().__init__(model_name, model_path, device, max_crops, use_graph)

    def _resolve(self) -> str:
        return _resolve_weights(self.model_path, self.model_name)


class HipOSNetReIDExtractor(_ReIDExtractorBase):
    """Drop-in for the reference's ``OSNetReIDExtractor`` (``ReIDFeatureExtractor(model_type="osnet")``): torchreid ``osnet_x1_0``
    features (512, unit rows) on the device.  ``model_path`` is a ``.safetensors`` file with torchreid's key names or a torchreid
    ``.pth`` / ``.pth.tar`` checkpoint; nothing is downloaded (the reference's ImageNet download and ResNet18 fallback do not exist
    here)."""

    model_type = "osnet"
    _model_code = _capi.OPD_REID_MODEL_OSNET
    _model_label = "OSNet"

    def __init__(self, model_path: Optional[str] = None, device: str = "hip:0", max_crops: int = 64, use_graph: bool = True):
        super().__init__(None, model_path, device, max_crops, use_graph)

    def _resolve(self) -> str:
        if not self.model_path:
            raise FileNotFoundError("OSNet needs model_path= a local .safetensors or torchreid .pth / .pth.tar file; this build never "
                                    "downloads weights and has no ResNet18 fallback")
        if not os.path.isfile(self.model_path):
            raise FileNotFoundError(f"OSNet weight file {self.model_path!r} does not exist (this build never downloads weights)")
        return self.model_path

    @contextlib.contextmanager
    def _weights_file(self, path: str):
        if path.endswith(".safetensors"):
            yield path
            return
        from .weights import save_safetensors
        sd = torchreid_state_dict(path)
        fd, tmp = tempfile.mkstemp(suffix=".safetensors")
        os.close(fd)
        try:
            save_safetensors(sd, tmp)
            yield tmp
        finally:
            os.remove(tmp)


def create_reid_extractor(model_type: str = "clip", model_name: Optional[str] = None, model_path: Optional[str] = None,
                          device: str = "hip:0", max_crops: int = 64, use_graph: bool = True):
    """The reference façade's dispatch (``ReIDFeatureExtractor(model_type=...)``): ``"clip"`` -> ``HipReIDExtractor``, ``"osnet"`` ->
    ``HipOSNetReIDExtractor`` (case-insensitive); anything else raises ``ValueError``.  ``model_name`` only applies to CLIP."""
    kind = str(model_type).lower()
    if kind == "clip":
        return HipReIDExtractor(model_type="clip", model_name=model_name, model_path=model_path, device=device, max_crops=max_crops,
                                use_graph=use_graph)
    if kind == "osnet":
        return HipOSNetReIDExtractor(model_path=model_path, device=device, max_crops=max_crops, use_graph=use_graph)
    raise ValueError(f"unknown Re-ID model_type {model_type!r}: expected 'clip' or 'osnet'")
