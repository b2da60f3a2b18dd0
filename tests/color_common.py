"""Shared by the colour-histogram tests (test_color_features_cpu.py, test_color_features_gpu.py) and tools/gen_color_golden.py: the
golden fixture, the exact evaluation of the feature formula, and the ctypes call of ``opd_color_features``."""

from __future__ import annotations

import ctypes as C
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "color_features.npz")
FRAME_H, FRAME_W, FRAME_SEED = 96, 160, 4242
UNIFORM_BGR = (17, 200, 90)            # painted over rows 60..79, columns 100..129 of the golden frame

# (x, y, w, h) on the 96 x 160 golden frame; what each one is there for
GOLDEN_BOXES = np.array([
    (-10.5, -4.2, 50.3, 40.9),         # partly outside: top-left
    (140.2, 70.7, 40.0, 40.0),         # partly outside: bottom-right
    (200.0, 10.0, 20.0, 20.0),         # degenerate: right of the frame
    (50.0, 50.0, 0.4, 10.0),           # degenerate: no column left after truncation
    (30.0, 20.0, -5.0, 10.0),          # degenerate: negative width
    (33.0, 21.0, 1.0, 1.0),            # 1 x 1 crop
    (100.0, 60.0, 30.0, 20.0),         # uniform crop
    (4.0, 10.0, 37.0, 25.0),           # row starts at byte 12: 0 mod 4
    (5.0, 11.0, 37.0, 25.0),           # 15: 3 mod 4
    (6.0, 12.0, 38.0, 26.0),           # 18: 2 mod 4
    (7.0, 13.0, 39.0, 27.0),           # 21: 1 mod 4
    (12.7, 8.3, 41.6, 55.2),           # fractional
    (0.0, 0.0, 160.0, 96.0),           # the whole frame
    (159.0, 0.0, 1.0, 96.0),           # one column
    (0.0, 95.0, 160.0, 1.0),           # one row
    (3.0, 3.0, 2.0, 2.0),              # 2 x 2: a row shorter than one 12-byte group
], dtype=np.float32)


def golden_frame() -> np.ndarray:
    from office_person_detection_vit_amd.frames import structured_frames
    frame = np.ascontiguousarray(structured_frames(1, FRAME_H, FRAME_W, seed=FRAME_SEED)[0]).copy()
    frame[60:80, 100:130] = UNIFORM_BGR
    return frame


def exact_rows(crops) -> np.ndarray:
    """The feature formula evaluated exactly up to ONE float64 rounding per operation on exact integers: integer bin counts and
    integer sum v, sum v^2 per channel, mean = S / n, std = sqrt(n * Q - S^2) / n, x / (||x|| + 1e-8), all float64, never float32."""
    out = np.zeros((len(crops), 256), np.float64)
    for i, crop in enumerate(crops):
        px = np.asarray(crop).reshape(-1, 3).astype(np.int64)
        n = px.shape[0]
        for c in range(3):
            out[i, 64 * c:64 * c + 64] = np.bincount(px[:, c] >> 2, minlength=64)
            s, q = int(px[:, c].sum()), int((px[:, c] * px[:, c]).sum())
            out[i, 192 + 2 * c] = s / n
            out[i, 193 + 2 * c] = math.sqrt(n * q - s * s) / n
        out[i] /= math.sqrt(math.fsum(float(v) * float(v) for v in out[i])) + 1e-8
    return out


def device_color_features(lib, frames, boxes, box_frame=None, mem_kind=0, device=0) -> np.ndarray:
    """``opd_color_features`` on a list of uint8 [h, w, 3] host frames, or (``mem_kind`` = 1) of ``(device pointer, h, w)`` tuples."""
    from office_person_detection_vit_amd import _capi
    boxes = np.ascontiguousarray(np.asarray(boxes, np.float32).reshape(-1, 4))
    if mem_kind == 0:
        frames = [np.ascontiguousarray(f) for f in frames]
        ptrs = (C.c_void_p * len(frames))(*[f.ctypes.data for f in frames])
        hw = np.array([f.shape[:2] for f in frames], np.int32)
    else:
        ptrs = (C.c_void_p * len(frames))(*[int(p) for p, _, _ in frames])
        hw = np.array([(h, w) for _, h, w in frames], np.int32)
    owner = None if box_frame is None else np.ascontiguousarray(np.asarray(box_frame, np.int32))
    out = np.full((len(boxes), 256), np.nan, np.float32)
    rc = lib.opd_color_features(device, ptrs, hw.ctypes.data_as(C.c_void_p), len(frames), mem_kind, boxes.ctypes.data_as(C.c_void_p),
                                owner.ctypes.data_as(C.c_void_p) if owner is not None else None, len(boxes), out.ctypes.data_as(C.c_void_p))
    _capi.check(rc, "opd_color_features")
    return out
