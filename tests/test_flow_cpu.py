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


# ---- every window and pyramid depth: tests/golden/flow_windows.npz (tools/gen_flow_windows_golden.py) ----------------------------------
# The device tests of test_flow_windows_gpu.py compare with this fixture under the bounds 4 * d_f32 (fixed work) and 0.02 px; here the
# restatement is pinned to it, and float32 restatements that carry one deliberate mistake each (flow_common.DEFECTS, and a pyramid one
# level too deep) show that those bounds would catch a kernel that made it.
_PYRAMIDS = {}


def _pyramids(name):
    if name not in _PYRAMIDS:
        h, w, _, win, max_level = F.WINDOW_CASES[name][:5]
        f0, f1 = F.window_pair(name)
        _PYRAMIDS[name] = F.pyramid(f0, win, max_level), F.pyramid(f1, win, max_level)
    return _PYRAMIDS[name]


def _lk(name, pts, epsilon, **kw):
    p = F.window_params(name)
    a, b = _pyramids(name)
    return F.lk_pyramids(a, b, pts, p["win"], p["max_iter"], epsilon, p["min_eig"], **kw)


def _has_found_points(name):
    return F.WINDOW_CASES[name][6].get("random") is not False


@pytest.fixture(scope="module")
def windows():
    return F.load_windows()


def test_window_cases_cover_the_documented_range(windows):
    cases, _ = windows
    assert list(cases) == list(F.WINDOW_CASES)
    by = {}
    for name, (h, w, seed, win, max_level, shift, more) in F.WINDOW_CASES.items():
        by.setdefault((win, max_level), []).append(F.top_level(h, w, win, max_level))
    for win in range(3, 22, 2):                                   # all ten windows the interface accepts, shallow and deep
        assert (win, 3) in by and max(by[(win, 7)]) >= 3, win
    assert [F.window_top(f"w{win}_240x320_l7") for win in range(3, 22, 2)] == [6, 5, 5, 4, 4, 4, 3, 3, 3, 3]
    assert F.WINDOW_CASES[F.BOUNDARY_CASE][:5] == (97, 131, 1013, 13, 3) and F.window_top(F.BOUNDARY_CASE) == 2
    assert [s.shape for s in _pyramids(F.BOUNDARY_CASE)[0]] == [(97, 131), (49, 66), (25, 33)]     # the next one, 13 x 17, is no larger than the window
    assert F.window_top(F.EIGHT_LEVEL_CASE) == 7 and _pyramids(F.EIGHT_LEVEL_CASE)[0][7].shape == (6, 6)
    assert F.window_top("w21_22x30_l3") == F.window_top("w5_3x40_l3") == 0
    for name in ("w3_1x1_l3", "w7_2x5_l3", "w21_6x8_l3"):         # frames smaller than the window: >= 32 points, all lost
        h, w, _, win = F.WINDOW_CASES[name][:4]
        assert h < win and w < win and len(cases[name]["pts"]) >= 32 and not cases[name]["status_fixed"].any()
    assert F.window_params("w9_iter1")["max_iter"] == 1 and F.window_params("w9_iter5")["max_iter"] == 5
    hi, lo = cases["w9_eig1e-2"], cases["w9_eig1e-6"]
    assert F.window_params("w9_eig1e-2")["min_eig"] == 1e-2 and F.window_params("w9_eig1e-6")["min_eig"] == 1e-6
    assert np.array_equal(hi["pts"], lo["pts"]) and int((hi["status_fixed"] != lo["status_fixed"]).sum()) >= 4


@pytest.mark.parametrize("name", list(F.WINDOW_CASES))
def test_restatement_reproduces_the_windows_fixture(windows, name):
    cases, margins = windows
    g = cases[name]
    h, w, _, win, max_level, _, more = F.WINDOW_CASES[name]
    eig, border, stop, f32_limit, small_border = margins
    pts, kind = g["pts"], g["kind"]
    assert len(_pyramids(name)[0]) == F.top_level(h, w, win, max_level) + 1
    # the range-test margin: 1 px, but 0.5 px for the outside point at win = 3 and the exit point at win <= 5, where no position has 1 px
    # at every level (tools/gen_flow_windows_golden.py); the outside point at win = 3 has integer coordinates, so its tests are exact
    small = ((kind == 2) & (win == 3)) | ((kind == 3) & (win <= 5))
    need = np.where(small, small_border, border)
    assert small_border == 0.5 and border == 1.0 and np.array_equal(pts[(kind == 2) & (win == 3)], np.rint(pts[(kind == 2) & (win == 3)]))
    for tag, eps in (("fixed", 0.0), ("default", 0.01)):
        diag = {}
        nxt, st = _lk(name, pts, eps, diag=diag)
        assert np.array_equal(st, g[f"status_{tag}"])
        assert np.abs(nxt - g[f"next_{tag}"]).max() <= 1e-9
        assert (diag["eig"] >= eig).all() and (diag["border"] >= need).all()
        assert "max_iter" in more or diag["converged"].all()      # (with max_iter 1 or 5 the iteration count is the stop)
        if eps == 0.0:
            assert (diag["stop"] >= stop).all()
    n32, s32 = _lk(name, pts, 0.0, dtype=np.float32)
    assert n32.dtype == np.float32 and np.array_equal(s32, g["status_fixed"])
    per_point = np.abs(n32.astype(np.float64) - g["next_fixed"]).max(axis=1)
    print(f"{name}: {len(pts)} points, found {int(g['status_fixed'].sum())}, d_f32 = {per_point.max():.3e}, recorded {g['d_f32']:.3e}")
    assert abs(per_point.max() - g["d_f32"]) <= 1e-9 and 0 < g["d_f32"] <= f32_limit == 2.5e-4
    # quotas and the lost points
    random = kind == 0
    assert 32 <= int(random.sum()) <= 48 and g["drawn"][1] <= 4000
    if _has_found_points(name):
        assert int((g["status_fixed"] & g["status_default"])[random].sum()) >= 24
    assert not g["status_fixed"][~random].any() and not g["status_default"][~random].any()
    assert (kind == 2).sum() == 1 and (kind == 1).sum() == (F.window_rect(h, w, win) is not None)
    x = float(pts[kind == 2][0, 0])
    if win < 21:                                                  # lost at this window, in range at 21
        assert np.floor(x - (win - 1) // 2) < -win and np.floor(x - 10) >= -21
        assert (kind == 3).sum() == _has_found_points(name)
    else:
        assert x < -21 - 10
    if (kind == 1).any():
        y0, y1, x0, x1 = F.window_rect(h, w, win)
        fx, fy = pts[kind == 1][0]
        assert y1 - y0 >= win + 8 and x1 - x0 >= win + 8
        assert x0 <= fx - (win - 1) // 2 and fx + (win + 1) // 2 < x1 and y0 <= fy - (win - 1) // 2 and fy + (win + 1) // 2 < y1


def _defect_cases():
    """(defect, case) for every case the defect applies to.  Cases without found points are left out: there no position depends on a
    window sum, a range test or the offset (a lost point keeps its coordinates).  The eigenvalue's normalisation: 2 * 441 in place of
    2 * win^2 divides the eigenvalue by 441 / win^2, and every fixture point has its eigenvalue 10 x clear of the threshold, so the
    mistake can show only where 441 / win^2 > 10: at win 3 and 5 (49 and 17.6), not at the two threshold cases of win 9 (5.4)."""
    out = []
    for name, (h, w, seed, win, max_level, shift, more) in F.WINDOW_CASES.items():
        if not _has_found_points(name):
            continue
        out.append(("last_sample", name))
        if win * win > 64:
            out.append(("partial_round", name))
        if win < 21:
            out += [("range_21", name), ("half_10", name)]
        if 10 * win * win < 441:
            out.append(("eig_441", name))
    return out


@pytest.mark.parametrize("defect,name", _defect_cases())
def test_the_bounds_catch_a_kernel_with_the_default_window_left_in(windows, defect, name):
    g = windows[0][name]
    nxt, st = _lk(name, g["pts"], 0.0, dtype=np.float32, defect=defect)
    flips = int((st != g["status_fixed"]).sum())
    d = np.abs(nxt.astype(np.float64) - g["next_fixed"]).max(axis=1)
    print(f"{name} with {defect}: {flips} statuses flip, largest distance {d.max():.3e} against 4 * d_f32 = {4 * g['d_f32']:.3e}")
    assert flips > 0 or d.max() > 4.0 * g["d_f32"]
    if defect == "range_21":                                      # ... and it is the exit point that shows it
        k = np.flatnonzero(g["kind"] == 3)[0]
        assert st[k] != g["status_fixed"][k] or d[k] > 4.0 * g["d_f32"]


def test_the_bounds_catch_a_pyramid_one_level_too_deep(windows):
    """plan_levels with '<' in place of '<=': at win = 13 the 13 x 17 level of 97 x 131 would be built and used."""
    name = F.BOUNDARY_CASE
    g = windows[0][name]
    p = F.window_params(name)
    deeper = [levels + [F.pyr_down(levels[-1])] for levels in _pyramids(name)]
    assert deeper[0][3].shape == (13, 17)
    nxt, st = F.lk_pyramids(deeper[0], deeper[1], g["pts"], p["win"], p["max_iter"], 0.0, p["min_eig"], dtype=np.float32)
    d = np.abs(nxt.astype(np.float64) - g["next_fixed"]).max(axis=1)
    print(f"{name}, four levels: {int((st != g['status_fixed']).sum())} statuses flip, largest distance {d.max():.3e} against {4 * g['d_f32']:.3e}")
    assert (st != g["status_fixed"]).any() or d.max() > 4.0 * g["d_f32"]
