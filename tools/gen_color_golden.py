"""Write tests/golden/color_features.npz: the reference's own `FeatureExtractor.extract_batch` (src/tracking/feature_extractor.py:90-137,
loaded by file path: the module needs numpy only) on the crops of tests/color_common.py's golden boxes of a small stored frame.

The crops are cut by the rule of `YOLOv8Detector.extract_features` (src/detection/yolov8_detector.py:176-185), restated below because
that module imports cv2 and ultralytics; the rectangles it gives are recorded too.  Also recorded: the reference's rows for a list that
holds a None and an empty crop, and d_ref = max |reference row - exactly evaluated formula| (color_common.exact_rows), the term the
device test adds to its derived bound.

    python tools/gen_color_golden.py <reference checkout>/src/tracking/feature_extractor.py
"""

from __future__ import annotations

import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import color_common as CC  # noqa: E402


def detector_rects(boxes, H, W):
    """(x1, y1, x2, y2, kept) per box; kept = 0: the detector substitutes a 64 x 32 zero image."""
    rects = []
    for x, y, w, h in boxes.tolist():
        x1, y1, x2, y2 = int(max(0, x)), int(max(0, y)), int(min(W, x + w)), int(min(H, y + h))
        rects.append((x1, y1, x2, y2, int(x2 > x1 and y2 > y1)))
    return np.array(rects, np.int32)


def main():
    spec = importlib.util.spec_from_file_location("reference_feature_extractor", sys.argv[1])
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    fx = ref.FeatureExtractor()
    frame = CC.golden_frame()
    rects = detector_rects(CC.GOLDEN_BOXES, *frame.shape[:2])
    crops = [frame[y1:y2, x1:x2] if kept else np.zeros((64, 32, 3), np.uint8) for x1, y1, x2, y2, kept in rects]
    rows = fx.extract_batch(crops)
    assert rows.dtype == np.float32 and rows.shape == (len(crops), 256)
    mixed = fx.extract_batch([crops[0], None, frame[0:0, 0:0], crops[6]])
    empty = fx.extract_batch([])
    d_ref = float(np.abs(rows.astype(np.float64) - CC.exact_rows(crops)).max())
    np.savez_compressed(CC.GOLDEN, frame=frame, boxes=CC.GOLDEN_BOXES, rects=rects, rows=rows, mixed_rows=mixed,
                        empty_shape=np.array(empty.shape, np.int64), empty_dtype=np.array(str(empty.dtype)), d_ref=np.float64(d_ref),
                        numpy_version=np.array(np.__version__))
    print("wrote", CC.GOLDEN, rows.shape, rows.dtype, "mixed", mixed.dtype, "d_ref", d_ref, os.path.getsize(CC.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
