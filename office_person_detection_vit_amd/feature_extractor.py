"""``detector.feature_extractor``: the attribute the reference's callers expect (``src/pipeline/phases/tracking.py:195-207``).

The detector pools appearance features on the device (``opd_detr_roi_features``, ``kernels_untyped.hip::roi_features_kernel``).
This host class serves callers that hold an encoder map in numpy already.  Contract of the reference class
(``src/tracking/feature_extractor.py:39-88``): boxes are (x, y, w, h) in image pixels, mapped to the (h, w, C) map by
truncation, clamped to at least one cell, mean-pooled and L2-normalised with ``+1e-8``.  All boxes are pooled at once from
one summed-area table of the map (float64), not cell by cell.

``extract_batch`` is the reference's default appearance feature, the colour histogram of a list of BGR crops
(``src/tracking/feature_extractor.py:90-137``), and ``crop_boxes`` the crop rule its detector feeds it with
(``src/detection/yolov8_detector.py:176-185``).  The device computes the same rows (``opd_color_features``,
``opd_detr_detect_frames_color``, ``kernels_hist.hip``); this host form is what the GPU tests compare them with."""

from __future__ import annotations

import numpy as np

_EPS = 1e-8


def roi_cells(bboxes: np.ndarray, map_hw, image_hw) -> np.ndarray:
    """(N, 4) xywh pixel boxes -> (N, 4) int cell ranges [x0, y0, x1, y1) on the feature map (truncate, then clamp so that
    every range holds at least one cell)."""
    h, w = map_hw
    img_h, img_w = image_hw
    b = np.asarray(bboxes, dtype=np.float64).reshape(-1, 4)
    lo = np.trunc(b[:, :2] / (img_w, img_h) * (w, h)).astype(np.int64)
    hi = np.trunc((b[:, :2] + b[:, 2:]) / (img_w, img_h) * (w, h)).astype(np.int64)
    lo = np.clip(lo, 0, (w - 1, h - 1))
    hi = np.maximum(lo + 1, np.minimum(hi, (w, h)))
    return np.concatenate([lo, hi], axis=1)


COLOR_DIM = 256     # 3 x 64 bin counts + (mean, std) of B, G, R = 198 numbers, zero-padded
COLOR_BINS = 64     # np.histogram(bins=64, range=(0, 256)) on uint8: value v lands in bin v >> 2


def crop_boxes(frame: np.ndarray, boxes) -> list:
    """The crops of (x, y, w, h) boxes on a BGR ``[H, W, 3]`` frame (views, not copies): columns ``int(max(0, x))`` up to
    ``int(min(W, x + w))``, rows alike, in Python floats; a box that leaves no pixel gives a 64 x 32 zero image."""
    H, W = frame.shape[:2]
    crops = []
    for box in boxes:
        x, y, w, h = (float(v) for v in box)
        cols = slice(int(max(0, x)), int(min(W, x + w)))
        rows = slice(int(max(0, y)), int(min(H, y + h)))
        empty = cols.stop <= cols.start or rows.stop <= rows.start
        crops.append(np.zeros((64, 32, 3), dtype=np.uint8) if empty else frame[rows, cols])
    return crops


class FeatureExtractor:
    def normalize_features(self, features: np.ndarray) -> np.ndarray:
        if features.size == 0:
            return features
        return features / (np.sqrt((features * features).sum(axis=1, keepdims=True)) + _EPS)

    def extract_roi_features(self, encoder_features: np.ndarray, bboxes, image_shape) -> np.ndarray:
        if encoder_features.ndim != 3:
            raise ValueError(f"Expected 3D encoder features, got {encoder_features.ndim}D")
        h, w, c = encoder_features.shape
        if len(bboxes) == 0:
            return np.array([]).reshape(0, c)
        cells = roi_cells(np.asarray(bboxes), (h, w), image_shape)
        sat = np.zeros((h + 1, w + 1, c), dtype=np.float64)
        sat[1:, 1:] = encoder_features.astype(np.float64).cumsum(axis=0).cumsum(axis=1)
        x0, y0, x1, y1 = cells.T
        total = sat[y1, x1] - sat[y0, x1] - sat[y1, x0] + sat[y0, x0]
        pooled = total / ((x1 - x0) * (y1 - y0))[:, None]
        return self.normalize_features(pooled.astype(encoder_features.dtype if encoder_features.dtype.kind == "f" else np.float64))

    def extract_batch(self, crops) -> np.ndarray:
        """Colour-histogram feature of every BGR crop, ``(len(crops), 256)``: 64 bin counts of B, of G, of R, then mean and
        population std of B, of G, of R (float64), zero-padded, as float32, L2-normalised row by row.  A ``None`` or empty crop
        gives a zero row -- a float64 one, which makes the whole result float64, as in the reference; a crop that is not
        ``[h, w, >= 3]`` gives a float32 zero row.  No crops: ``(0, 256)``."""
        if not crops:
            return np.array([]).reshape(0, COLOR_DIM)
        rows = []
        for crop in crops:
            if crop is None or crop.size == 0:
                rows.append(np.zeros(COLOR_DIM))
                continue
            row = np.zeros(COLOR_DIM, dtype=np.float32)
            if crop.ndim == 3 and crop.shape[2] >= 3:
                for c in range(3):
                    channel = crop[:, :, c]
                    row[c * COLOR_BINS:(c + 1) * COLOR_BINS] = np.histogram(channel, bins=COLOR_BINS, range=(0, 256))[0]
                    row[3 * COLOR_BINS + 2 * c] = channel.mean()
                    row[3 * COLOR_BINS + 2 * c + 1] = channel.std()
            rows.append(row)
        return self.normalize_features(np.array(rows))
