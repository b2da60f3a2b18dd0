"""Shared pieces of the crop-planner tests (test_crop_plan_cpu.py, test_detect_reid_gpu.py): the boxes, and the three hooks of
csrc/opd_crop_test_api.cpp behind one call that returns their arrays by name."""

from __future__ import annotations

import numpy as np

from office_person_detection_vit_amd import _capi

SPECS = {"clip": (_capi.OPD_REID_MODEL_CLIP, 224, 224), "osnet": (_capi.OPD_REID_MODEL_OSNET, 256, 128)}   # model code, out_h, out_w
FRAMES = [(720, 1280), (96, 160)]
SIZES = [1, 2, 3, 7, 64, 127, 128, 129, 223, 224, 225, 719, 1279]
# Tap counts: ksize = 2 ceil(support) + 1 with support = (bicubic ? 2 : 1) max(1, in / out).  The largest in / out a 720 x 1280 frame
# allows is 1280 / 128 = 10 (OSNet, bilinear: 21 taps) and 720 / 224 (CLIP keeps the aspect, so its shortest edge goes to 224; bicubic: 15).
CAP = 24
FIELDS = ("geom", "meta", "src_off", "bx", "by", "ch", "cv")


def size_boxes(H, W):
    """Every width x height of SIZES, origins walking over the frame (a third of them start left of / above it), then the special
    cases: partly off-frame, negative origins, zero and negative sizes, NaN, the whole frame, a 1-pixel-wide box, a degenerate one."""
    boxes = []
    for i, w in enumerate(SIZES):
        for j, h in enumerate(SIZES):
            k = i * len(SIZES) + j
            x = (k * 37.25) % W - (20.5 if k % 3 == 0 else 0.0)
            y = (k * 23.75) % H - (10.25 if k % 3 == 1 else 0.0)
            boxes.append((x, y, float(w), float(h)))
    nan = float("nan")
    boxes += [(-30.5, H - 40.2, 120.0, 200.0), (W - 29.4, -10.0, 80.0, 40.0), (-5.0, -5.0, 3.0, 3.0), (-5.0, -5.0, 30.0, 60.0),
              (W - 0.1, H - 0.1, 5.0, 5.0), (10.0, 10.0, 0.0, 50.0), (10.0, 10.0, 50.0, 0.0), (10.0, 10.0, -4.0, 50.0),
              (50.0, 40.0, 20.0, -1.0), (nan, 10.0, 20.0, 30.0), (10.0, nan, 20.0, 30.0), (10.0, 10.0, nan, 30.0),
              (10.0, 10.0, 20.0, nan), (nan, nan, nan, nan), (0.0, 0.0, float(W), float(H)), (-3.0, -3.0, W + 6.0, H + 6.0),
              (W / 2, 5.0, 1.0, H / 2), (40.0, 30.0, 0.4, 50.0), (10.99, 20.01, 0.99, 60.0), (0.0, 0.0, 1.0, 1.0)]
    return np.ascontiguousarray(np.asarray(boxes, np.float32))


def plan(lib, which, spec, boxes, H, W, cap=CAP):
    """The plan of `boxes` on an H x W frame by hook `which` ("device", "host", "staged"): dict of the arrays of FIELDS."""
    model, OH, OW = SPECS[spec]
    b = np.ascontiguousarray(np.asarray(boxes, np.float32).reshape(-1, 4))
    n = len(b)
    out = {"geom": np.full((n, 13), -7, np.int32), "meta": np.full((n, 4), -7, np.int32), "src_off": np.full(n, -7, np.int64),
           "bx": np.full((n, OW, 2), -7, np.int32), "by": np.full((n, OH, 2), -7, np.int32),
           "ch": np.full((n, OW, cap), -7, np.int32), "cv": np.full((n, OH, cap), -7, np.int32)}
    rc = getattr(lib, "opd_test_crop_plan_" + which)(model, b.ctypes.data, n, H, W, *[out[k].ctypes.data for k in FIELDS], cap)
    _capi.check(rc, "opd_test_crop_plan_" + which)
    return out


def assert_same_plan(a, b, boxes, what):
    for k in FIELDS:
        if not np.array_equal(a[k], b[k]):
            bad = int(np.flatnonzero((a[k] != b[k]).reshape(len(boxes), -1).any(axis=1))[0])
            raise AssertionError(f"{what}: {k} differs first at box {bad} = {tuple(boxes[bad])}")
