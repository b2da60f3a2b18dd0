"""CPU-only tests of the crop planner's shared routine (csrc/opd_crop.h: what crop_plan_kernel evaluates per thread), instantiated on the
host: it equals the planning opd_reid_extract does today (crop_geometry + opd_resize_coeffs_filter) bit for bit, for both crop specs,
over box widths / heights 1 .. 1279 on a 720 x 1280 and a 96 x 160 frame, with off-frame, empty, negative and NaN boxes; and the new
entry point is declared and refuses null handles without a device."""

import ctypes as C
import os
import re

import numpy as np
import pytest

import crop_plan_common as P
from office_person_detection_vit_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return _capi.load_library(test_hooks=True)


@pytest.mark.parametrize("hw", P.FRAMES)
@pytest.mark.parametrize("spec", sorted(P.SPECS))
def test_host_instantiation_equals_the_staged_plan(lib, spec, hw):
    H, W = hw
    boxes = P.size_boxes(H, W)
    host = P.plan(lib, "host", spec, boxes, H, W)
    staged = P.plan(lib, "staged", spec, boxes, H, W)
    P.assert_same_plan(host, staged, boxes, f"{spec} {H}x{W}")
    zero = host["meta"][:, 3] == 1
    assert zero.any() and (~zero).sum() >= len(P.SIZES) ** 2 // 2          # both kinds are in the set
    assert host["meta"][~zero, 0].max() <= P.CAP and host["meta"][~zero, 1].max() <= P.CAP
    if hw == (720, 1280):                                                  # the largest tap counts the frame allows are reached
        assert host["meta"][~zero, 0].max() == (21 if spec == "osnet" else 15)
    _, OH, OW = P.SPECS[spec]
    g = host["geom"][~zero]
    assert (g[:, 9] >= g[:, 1]).all() and (g[:, 11] <= g[:, 3]).all() and (g[:, 10] >= g[:, 0]).all() and (g[:, 12] <= g[:, 2]).all()
    assert (g[:, 0] >= 0).all() and (g[:, 1] >= 0).all() and (g[:, 2] <= W).all() and (g[:, 3] <= H).all()   # the window lies in the frame
    assert np.array_equal(host["src_off"][~zero], (g[:, 9].astype(np.int64) * W + g[:, 10]) * 3)
    assert (host["meta"][~zero, 2] == 3 * W).all()


@pytest.mark.parametrize("hw", P.FRAMES)
def test_host_geometry_equals_the_geometry_hook(lib, hw):
    """opd_test_reid_geometry = crop_geometry with the CLIP spec, through the hook the Re-ID tests have used all along."""
    H, W = hw
    boxes = P.size_boxes(H, W)
    want = np.zeros((len(boxes), 13), np.int32)
    assert lib.opd_test_reid_geometry(boxes.ctypes.data, len(boxes), H, W, want.ctypes.data) == 0
    np.testing.assert_array_equal(P.plan(lib, "host", "clip", boxes, H, W)["geom"], want)


@pytest.mark.parametrize("hw", P.FRAMES)
def test_host_tables_equal_opd_resize_coeffs_filter(lib, hw):
    """Axis by axis against the table hooks: opd_test_reid_coeffs (bicubic, the window's outputs) for CLIP, opd_test_resize_coeffs
    (bilinear, the whole axis) for OSNet."""
    H, W = hw
    boxes = P.size_boxes(H, W)
    for spec in ("clip", "osnet"):
        _, OH, OW = P.SPECS[spec]
        got = P.plan(lib, "host", spec, boxes, H, W)
        checked = 0
        for i in np.flatnonzero(got["meta"][:, 3] == 0)[::3]:
            x1, y1, x2, y2, _, rh, rw, top, left, wy0, wx0, _, _ = (int(v) for v in got["geom"][i])
            for in_size, out_size, first, count, lo, o, ks, b, c in ((x2 - x1, rw, left, OW, wx0, x1, got["meta"][i, 0], got["bx"][i], got["ch"][i]),
                                                                      (y2 - y1, rh, top, OH, wy0, y1, got["meta"][i, 1], got["by"][i], got["cv"][i])):
                if spec == "clip":
                    bounds, coeffs = np.zeros((count, 2), np.int32), np.zeros((count, P.CAP), np.int32)
                    k = lib.opd_test_reid_coeffs(in_size, out_size, first, count, bounds.ctypes.data, coeffs.ctypes.data, P.CAP)
                else:
                    assert (first, count) == (0, out_size)
                    bounds, packed = np.zeros((out_size, 2), np.int32), np.zeros(out_size * P.CAP, np.int32)
                    k = lib.opd_test_resize_coeffs(in_size, out_size, bounds.ctypes.data, packed.ctypes.data, packed.size)
                    coeffs = np.zeros((out_size, P.CAP), np.int32)                    # (this hook packs its rows: [out_size][k])
                    coeffs[:, :k] = packed[:out_size * k].reshape(out_size, k)
                assert k == ks, (spec, i, tuple(boxes[i]))
                bounds[:, 0] -= lo - o                                  # first taps relative to the source window
                assert np.array_equal(b, bounds) and np.array_equal(c, coeffs), (spec, i, tuple(boxes[i]))
            checked += 1
        assert checked >= 20


def test_entry_point_is_declared():
    header = open(os.path.join(ROOT, "include", "opd_detr.h")).read()
    name = "opd_detr_detect_frames_reid"
    assert name in _capi.API and re.search(r"OPD_API\s+\w+\s+" + name + r"\s*\(", header)
    m = re.search(name + r"\s*\(([^;]*)\)\s*;", header)
    params = [p for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",") if p.strip()]
    assert len(params) == len(_capi.API[name][1]) == 16
    for hook in ("opd_test_crop_plan_device", "opd_test_crop_plan_host"):
        assert hook in _capi.TEST_API and hook not in _capi.API


def test_null_handles_are_refused_without_a_device(lib):
    recs, counts = (_capi.OpdDet * 4)(), (C.c_int32 * 1)()
    feats, slot_map, n_person = np.zeros((1, 512), np.float32), np.zeros(1, np.int32), C.c_int32(-1)
    frame = np.zeros((32, 32, 3), np.uint8)
    ptrs = (C.c_void_p * 1)(frame.ctypes.data)
    rc = lib.opd_detr_detect_frames_reid(None, None, ptrs, 1, 32, 32, 32, 32, 0.5, 1, 1, recs, counts, feats.ctypes.data, slot_map.ctypes.data,
                                         C.byref(n_person))
    assert rc == _capi.OPD_EINVAL and "null" in _capi.last_error()
    assert n_person.value == -1 and not feats.any()
