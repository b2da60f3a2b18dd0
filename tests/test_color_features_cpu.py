"""Colour-histogram appearance features, host side (no GPU): ``FeatureExtractor.extract_batch`` and ``crop_boxes`` against rows and
rectangles recorded from the reference's own code (tests/golden/color_features.npz, tools/gen_color_golden.py), the exact evaluation
of the formula that the device bound is built from, and the two C-ABI entry points being declared and exported."""

import os
import re
import subprocess

import numpy as np

import color_common as CC
from office_person_detection_vit_amd import _capi
from office_person_detection_vit_amd.feature_extractor import FeatureExtractor, crop_boxes


def _golden():
    return np.load(CC.GOLDEN)


def test_fixture_frame_and_boxes_are_the_shared_ones():
    g = _golden()
    assert np.array_equal(g["frame"], CC.golden_frame()) and g["frame"].dtype == np.uint8 and g["frame"].shape == (CC.FRAME_H, CC.FRAME_W, 3)
    assert np.array_equal(g["boxes"], CC.GOLDEN_BOXES) and g["boxes"].dtype == np.float32


def test_fixture_holds_every_edge_case():
    g = _golden()
    frame, boxes, rects = g["frame"], g["boxes"].astype(np.float64), g["rects"]
    x1, y1, x2, y2, kept = rects.T
    outside = (boxes[:, 0] < 0) | (boxes[:, 1] < 0) | (boxes[:, 0] + boxes[:, 2] > CC.FRAME_W) | (boxes[:, 1] + boxes[:, 3] > CC.FRAME_H)
    assert (outside & (kept == 1)).any(), "a box partly outside the frame"
    assert (kept == 0).any(), "a degenerate box"
    assert ((x2 - x1 == 1) & (y2 - y1 == 1) & (kept == 1)).any(), "a 1 x 1 crop"
    uniform = [k for k in range(len(rects)) if kept[k] and (x2[k] - x1[k]) * (y2[k] - y1[k]) > 1
               and (frame[y1[k]:y2[k], x1[k]:x2[k]].reshape(-1, 3) == frame[y1[k], x1[k]]).all()]
    assert uniform, "a uniform crop"
    assert {int(3 * a) % 4 for a, k in zip(x1, kept) if k} >= {0, 1, 2, 3}, "row starts at every byte alignment mod 4"


def test_crop_rule_matches_the_recorded_rectangles():
    g = _golden()
    frame, rects = g["frame"], g["rects"]
    crops = crop_boxes(frame, g["boxes"])
    assert len(crops) == len(rects)
    for crop, (x1, y1, x2, y2, kept) in zip(crops, rects):
        assert crop.dtype == np.uint8
        if kept:
            assert np.array_equal(crop, frame[y1:y2, x1:x2]) and crop.shape == (y2 - y1, x2 - x1, 3)
        else:
            assert crop.shape == (64, 32, 3) and not crop.any()


def test_extract_batch_equals_the_reference_rows_exactly():
    g = _golden()
    rows = FeatureExtractor().extract_batch(crop_boxes(g["frame"], g["boxes"]))
    assert rows.dtype == g["rows"].dtype == np.float32 and rows.shape == g["rows"].shape == (len(g["boxes"]), 256)
    assert np.array_equal(rows, g["rows"])
    assert not rows[:, 198:].any()


def test_degenerate_box_gives_the_dummy_crop_row():
    g = _golden()
    rows = FeatureExtractor().extract_batch(crop_boxes(g["frame"], g["boxes"]))
    want = np.zeros(256, np.float32)
    want[[0, 64, 128]] = np.float32(1.0 / np.sqrt(3.0))
    for k in np.flatnonzero(g["rects"][:, 4] == 0):
        assert np.abs(rows[k] - want).max() <= 2.0 ** -24   # 1/sqrt(3) in float32 arithmetic: within one ulp of 0.577


def test_empty_inputs():
    g = _golden()
    fx = FeatureExtractor()
    empty = fx.extract_batch([])
    assert empty.shape == tuple(g["empty_shape"]) == (0, 256) and str(empty.dtype) == str(g["empty_dtype"])
    crops = crop_boxes(g["frame"], g["boxes"])
    mixed = fx.extract_batch([crops[0], None, g["frame"][0:0, 0:0], crops[6]])
    assert mixed.dtype == g["mixed_rows"].dtype and mixed.shape == g["mixed_rows"].shape == (4, 256)
    assert np.array_equal(mixed, g["mixed_rows"])
    assert not mixed[1].any() and not mixed[2].any()


def test_reference_rows_lie_next_to_the_exact_evaluation():
    """d_ref, the distance between the reference's float32 rows and the formula evaluated in float64 on exact integers, is what the
    device test adds to its derived 2^-23.  It is recomputed here and must be the recorded number.  Sanity of its size: the
    reference rounds each unit-norm row's entries (<= 1) to float32 after a float32 norm and a float32 division, three roundings
    of relative size 2^-24 at most, so it stays below 3 * 2^-24 plus the std entries' own error (far below one ulp of the row)."""
    g = _golden()
    crops = crop_boxes(g["frame"], g["boxes"])
    d = float(np.abs(g["rows"].astype(np.float64) - CC.exact_rows(crops)).max())
    print(f"d_ref recomputed {d:.6e}, recorded {float(g['d_ref']):.6e}")
    assert d == float(g["d_ref"])
    assert d <= 4 * 2.0 ** -24
    exact = CC.exact_rows(crops)
    uniform = int(np.flatnonzero((g["boxes"] == (100.0, 60.0, 30.0, 20.0)).all(axis=1))[0])
    assert (exact[uniform, [193, 195, 197]] == 0.0).all() and (g["rows"][uniform, [193, 195, 197]] == 0.0).all()


def test_bins_are_value_shifted_right_by_two():
    v = np.arange(256, dtype=np.uint8)
    crop = np.stack([v, v, v], axis=1).reshape(16, 16, 3)
    row = FeatureExtractor().extract_batch([crop])[0]
    assert (row[:192] == row[0]).all() and row[0] > 0   # 4 values per bin, every bin of every channel


def test_capi_declares_the_color_entry_points():
    assert "opd_color_features" in _capi.API and "opd_detr_detect_frames_color" in _capi.API
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "opd_detr.h")).read()
    declared = set(re.findall(r"\b(opd_[a-z0-9_]+)\s*\(", header))
    assert {"opd_color_features", "opd_detr_detect_frames_color"} <= declared


def test_built_library_exports_the_color_entry_points():
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], check=True, capture_output=True, text=True).stdout
    names = {l.split()[2] for l in out.splitlines() if len(l.split()) == 3 and l.split()[1] == "T"}
    assert {"opd_color_features", "opd_detr_detect_frames_color"} <= names
    lib = _capi.load_library()
    assert lib.opd_color_features.argtypes == _capi.API["opd_color_features"][1]
