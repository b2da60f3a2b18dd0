"""Optical flow without a GPU: the numpy restatement of the kernel contract (flow_common.py) against the recorded fixture and against
analytic displacements, the new C-ABI names, and the state logic of ``HipOpticalFlowTracker`` that needs no library."""

import os
import re

import numpy as np
import pytest

import flow_common as F
from office_person_detection_vit_amd import HipOpticalFlowTracker, _capi
from office_person_detection_vit_amd.data_models import Detection

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return np.load(F.GOLDEN)


def test_reflect_and_pyramid_rules():
    assert F.reflect101([-2, -1, 0, 4, 5, 6], 5).tolist() == [2, 1, 0, 4, 3, 2]
    assert F.reflect101([-3, 2, 3], 2).tolist() == [1, 0, 1] and F.reflect101([-1, 5], 1).tolist() == [0, 0]
    assert [F.top_level(h, w, 21, 3) for h, w in ((22, 30), (48, 64), (97, 131), (720, 1280))] == [0, 1, 2, 3]
    assert F.top_level(720, 1280, 21, 1) == 1
    g = F.gray_u8(np.array([[[255, 255, 255], [0, 0, 0], [255, 0, 0], [0, 255, 0], [0, 0, 255]]], np.uint8))
    assert g.tolist() == [[255, 0, 29, 150, 76]]
    flat = F.pyr_down(np.full((9, 7), 93, np.uint8))
    assert flat.shape == (5, 4) and (flat == 93).all()       # the filter sums to 256
    sx, sy = F.scharr(np.tile(np.arange(8, dtype=np.uint8) * 3, (6, 1)))
    assert (sx[:, 1:-1] == 96).all() and (sx[:, [0, -1]] == 0).all() and not sy.any()   # a ramp of 3 per pixel: 32 * 3; reflect-101 edges


@pytest.mark.parametrize("name", list(F.LK_CASES))
def test_restatement_reproduces_the_fixture(golden, name):
    h, w, seed, n = F.LK_CASES[name]
    f0, f1 = F.structured_pair(h, w, seed)
    pts = golden[f"{name}_pts"]
    assert len(pts) == n + 2
    for tag, eps in (("fixed", 0.0), ("default", 0.01)):
        diag = {}
        nxt, st = F.lk_restatement(f0, f1, pts, epsilon=eps, diag=diag)
        assert np.array_equal(st, golden[f"{name}_status_{tag}"])
        assert np.abs(nxt - golden[f"{name}_next_{tag}"]).max() <= 1e-9       # float64 on the same integers: rounding of libm / BLAS-free sums
        eig, border, stop = golden["margins"]
        assert (diag["eig"] >= eig).all() and (diag["border"] >= border).all() and diag["converged"].all()
        if eps == 0.0:
            assert (diag["stop"] >= stop).all()
    assert 0 < golden[f"{name}_status_fixed"][:n].sum() < n and not golden[f"{name}_status_fixed"][n:].any()   # found and lost points; flat, outside
    n32, s32 = F.lk_restatement(f0, f1, pts, epsilon=0.0, dtype=np.float32)
    assert n32.dtype == np.float32 and np.array_equal(s32, golden[f"{name}_status_fixed"])
    d = float(np.abs(n32.astype(np.float64) - golden[f"{name}_next_fixed"]).max())
    print(f"{name}: d_f32 = {d:.3e}, recorded {float(golden[f'{name}_d_f32']):.3e}")
    assert 0 < float(golden[f"{name}_d_f32"]) < 1e-3


@pytest.mark.parametrize("k", range(3))
def test_restatement_recovers_analytic_displacements(golden, k):
    shift = F.SHIFTS[k]
    a, b = F.analytic_pair(shift)
    pts = golden["shift_pts"]
    nxt, st = F.lk_restatement(a, b, pts)
    assert st.all() and np.array_equal(st, golden[f"shift{k}_status"])
    err = float(np.abs(nxt - pts - np.array(shift)).max())
    print(f"shift {shift}: max error {err:.4f} px over {len(pts)} points, recorded e_ref {float(golden[f'shift{k}_e_ref']):.4f}")
    assert abs(err - float(golden[f"shift{k}_e_ref"])) <= 1e-9
    assert err <= 0.1                                                        # uint8 quantisation of a smooth texture: a small fraction of a pixel


def test_border_points_of_the_fixture(golden):
    a, b = F.analytic_pair(F.SHIFTS[0])
    nxt, st = F.lk_restatement(a, b, golden["border_pts"])
    assert st.all() and np.array_equal(st, golden["border_status"]) and np.abs(nxt - golden["border_next"]).max() <= 1e-9
    h, w = F.SHIFT_HW
    p = golden["border_pts"]
    assert (np.minimum(np.minimum(p[:, 0], w - 1 - p[:, 0]), np.minimum(p[:, 1], h - 1 - p[:, 1])) == 3).all()


def test_new_names_in_the_binding_and_the_header():
    names = ["opd_flow_create", "opd_flow_destroy", "opd_flow_set_reference", "opd_flow_track"]
    header = open(os.path.join(ROOT, "include", "opd_detr.h")).read()
    for name in names:
        assert name in _capi.API and re.search(r"OPD_API\s+\w+\s+" + name + r"\s*\(", header), name
    assert "opd_flow_test_level" in _capi.TEST_API and "opd_flow_test_level" not in header
    assert [f[0] for f in _capi.OpdFlowConfig._fields_] == ["max_h", "max_w", "max_points", "win", "max_level", "max_iter", "epsilon",
                                                            "min_eig_threshold"]
    assert re.search(r"int max_h, max_w;.*int max_points;.*int win;.*int max_level;.*int max_iter;.*float epsilon;.*float min_eig_threshold;",
                     header, re.S)
    lib = _capi.load_library()
    assert lib.opd_flow_track.argtypes == _capi.API["opd_flow_track"][1]


def test_tracker_state_logic_without_the_library(monkeypatch):
    def no_library(*a, **k):
        raise AssertionError("the library must not be loaded here")
    monkeypatch.setattr(_capi, "load_library", no_library)
    t = HipOpticalFlowTracker(max_corners=50, quality_level=0.2, min_distance=5.0, block_size=5)
    assert (t.max_corners, t.quality_level, t.min_distance, t.block_size) == (50, 0.2, 5.0, 5)
    assert t.lk_params == {"winSize": (21, 21), "maxLevel": 3, "criteria": (3, 30, 0.01)}
    assert t.prev_points is None and t.prev_track_ids == []
    frame = np.zeros((48, 64, 3), np.uint8)
    assert t.track(frame) == {}                               # nothing initialised
    # initialize() keeps the detections that carry a track id: (x + w / 2, y + h / 2) as (N, 1, 2) float32
    calls = []

    class FakeLib:
        def opd_flow_create(self, cfg, device, out):
            calls.append(("create", cfg._obj.max_h, cfg._obj.max_w, cfg._obj.max_points, cfg._obj.win, cfg._obj.max_level, cfg._obj.max_iter))
            out._obj.value = 1
            return 0

        def opd_flow_set_reference(self, handle, ptr, kind, h, w):
            calls.append(("ref", kind, h, w))
            return 0

        def opd_flow_destroy(self, handle):
            calls.append(("destroy",))

    monkeypatch.setattr(_capi, "load_library", lambda *a, **k: FakeLib())
    dets = [Detection(bbox=(10.0, 20.0, 4.0, 6.0), confidence=0.9, class_id=1, class_name="person", camera_coords=(12.0, 26.0), track_id=7),
            Detection(bbox=(1.0, 2.0, 3.0, 4.0), confidence=0.9, class_id=1, class_name="person", camera_coords=(2.5, 6.0)),
            Detection(bbox=(30.5, 8.0, 3.0, 5.0), confidence=0.9, class_id=1, class_name="person", camera_coords=(32.0, 13.0), track_id=2)]
    t.initialize(frame, dets)
    assert calls == [("create", 48, 64, 50, 21, 3, 30), ("ref", _capi.OPD_MEM_HOST, 48, 64)]
    assert t.prev_track_ids == [7, 2]
    assert t.prev_points.dtype == np.float32 and t.prev_points.shape == (2, 1, 2)
    assert t.prev_points.reshape(-1, 2).tolist() == [[12.0, 23.0], [32.0, 10.5]]
    t.initialize(frame, [dets[1]])                            # no tracked detection: the frame is the reference, there are no points
    assert t.prev_points is None and t.prev_track_ids == [] and calls[-1] == ("ref", _capi.OPD_MEM_HOST, 48, 64) and len(calls) == 3
    assert t.track(frame) == {}
    t.initialize(frame, dets)
    t.reset()
    assert t.prev_points is None and t.prev_track_ids == [] and t.track(frame) == {}
    with pytest.raises(ValueError, match="uint8"):
        t.initialize(frame.astype(np.float32), dets)
    t.close()
    assert calls[-1] == ("destroy",)
