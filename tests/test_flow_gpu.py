"""Pyramidal Lucas-Kanade on the device (csrc/kernels_flow.hip behind ``opd_flow_*``) against the float64 restatement of the same
contract (flow_common.py, pinned by test_flow_cpu.py and tests/golden/flow.npz).

Bounds.  Gray and pyramid are integer: bit-exact.  Every fixture point takes each of its decisions (range, eigenvalue, stop) at a
recorded margin from the threshold, so status is compared on every point, none left out.  At fixed work (epsilon = 0: a level ends by
the swing test alone; the C-ABI reads a zero as its default, so the handle gets a negative epsilon, which switches the step-length
test off and gives the same result) positions lie within 4 * d_f32 of the float64 restatement, d_f32 = max |float32 restatement -
float64 restatement| over the fixture's points of that frame size (rows do not depend on which other points a call carries:
test_rows_are_independent); the factor 4 is for another summation order over 441 terms.  With the default criteria one side may stop a
step earlier, and a stopping step is at most epsilon per level: 2 * epsilon = 0.02 px."""

import ctypes as C
import faulthandler

import numpy as np
import pytest
import torch

import flow_common as F
from office_person_detection_vit_amd import HipOpticalFlowTracker, _capi
from office_person_detection_vit_amd.data_models import Detection

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _time_limit():
    """Every test runs under its own limit: a hang ends the process (with a traceback) instead of holding the GPU."""
    faulthandler.dump_traceback_later(120, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def lib():
    return _capi.load_library(test_hooks=True)


@pytest.fixture(scope="module")
def golden():
    return np.load(F.GOLDEN)


@pytest.fixture(scope="module")
def pairs():
    return {name: F.structured_pair(h, w, seed) for name, (h, w, seed, _) in F.LK_CASES.items()}


class Flow:
    """A handle that is destroyed with the block."""

    def __init__(self, lib, h, w, max_points=128, **cfg):
        self.lib, self.h = lib, F.flow_create(lib, h, w, max_points, **cfg)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.lib.opd_flow_destroy(self.h)

    def pair(self, f0, f1, pts, mem_kind=0):
        F.flow_set_reference(self.lib, self.h, f0, mem_kind)
        return F.flow_track(self.lib, self.h, f1, pts, mem_kind)


@pytest.mark.parametrize("hw,levels", [((22, 30), 1), ((48, 64), 2), ((97, 131), 3), ((720, 1280), 4)])
def test_gray_and_pyramid_are_bit_exact(lib, hw, levels):
    from office_person_detection_vit_amd.frames import noise_frame
    frame = noise_frame(hw[0], hw[1], seed=hw[0])          # white noise: every rounding of the filter is exercised
    want = F.pyramid(frame)
    assert len(want) == levels
    with Flow(lib, *hw) as fl:
        F.flow_set_reference(lib, fl.h, frame)
        got = F.flow_levels(lib, fl.h)
        assert len(got) == levels
        for l, (g, w) in enumerate(zip(got, want)):
            assert g.shape == w.shape and np.array_equal(g, w), (l, int((g != w).sum()))
    # a smaller frame in a larger handle, at an odd device address (byte loads instead of dwords): the same levels
    with Flow(lib, hw[0] + 9, hw[1] + 7) as fl:
        odd = torch.zeros(frame.size + 1, dtype=torch.uint8, device="cuda")
        odd[1:] = torch.from_numpy(frame).cuda().reshape(-1)
        torch.cuda.synchronize()
        F.flow_set_reference(lib, fl.h, (odd.data_ptr() + 1, hw[0], hw[1]), mem_kind=_capi.OPD_MEM_DEVICE)
        for g, w in zip(F.flow_levels(lib, fl.h), want):
            assert np.array_equal(g, w)


@pytest.mark.parametrize("n", [1, 64, 100])
@pytest.mark.parametrize("name", list(F.LK_CASES))
def test_lk_parity_at_fixed_work(lib, golden, pairs, name, n):
    h, w = F.LK_CASES[name][:2]
    pts, want, status = golden[f"{name}_pts"][:n], golden[f"{name}_next_fixed"][:n], golden[f"{name}_status_fixed"][:n]
    bound = 4.0 * float(golden[f"{name}_d_f32"])
    with Flow(lib, h, w, epsilon=-1.0, max_iter=30) as fl:
        got, st = fl.pair(*pairs[name], pts)
    d = np.abs(got.astype(np.float64) - want).max(axis=1)
    print(f"{name} n={n}: max |device - float64| = {d.max():.3e} (point {int(d.argmax())}), bound 4 * d_f32 = {bound:.3e}; found {int(st.sum())}")
    assert np.array_equal(st, status)
    assert d.max() <= bound


@pytest.mark.parametrize("name", list(F.LK_CASES))
def test_default_criteria_and_lost_points(lib, golden, pairs, name):
    h, w, _, n = F.LK_CASES[name]
    pts, want, status = golden[f"{name}_pts"], golden[f"{name}_next_default"], golden[f"{name}_status_default"]
    with Flow(lib, h, w) as fl:
        got, st = fl.pair(*pairs[name], pts)
        d = np.abs(got.astype(np.float64) - want).max(axis=1)
        print(f"{name}: default criteria, max |device - float64| = {d.max():.3e}, bound 0.02; found {int(st.sum())} of {len(pts)}")
        assert np.array_equal(st, status)
        assert d.max() <= 0.02
        assert st[n:].tolist() == [0, 0]                       # the flat region; the point more than a window outside the frame
        assert pts[n + 1][0] < -21
        # no points: fine, and the frame still becomes the reference
        rc = lib.opd_flow_track(fl.h, C.c_void_p(pairs[name][0].ctypes.data), 0, h, w, None, 0, None, None)
        assert rc == _capi.OPD_OK
        back, st_back = F.flow_track(lib, fl.h, pairs[name][1], pts)
        assert np.array_equal(back, got) and np.array_equal(st_back, st)


@pytest.mark.parametrize("k", range(3))
def test_ground_truth_displacement(lib, golden, k):
    shift = F.SHIFTS[k]
    a, b = F.analytic_pair(shift)
    pts = golden["shift_pts"]
    with Flow(lib, *F.SHIFT_HW) as fl:
        got, st = fl.pair(a, b, pts)
    err = float(np.abs(got.astype(np.float64) - pts - np.array(shift)).max())
    bound = float(golden[f"shift{k}_e_ref"]) + 0.02
    print(f"shift {shift}: device error {err:.4f} px, bound e_ref + 0.02 = {bound:.4f}")
    assert st.all()
    assert err <= bound
    assert np.abs(got.astype(np.float64) - golden[f"shift{k}_next"]).max() <= 0.02


def test_points_three_pixels_from_the_border(lib, golden):
    a, b = F.analytic_pair(F.SHIFTS[0])
    with Flow(lib, *F.SHIFT_HW) as fl:
        got, st = fl.pair(a, b, golden["border_pts"])
    assert np.array_equal(st, golden["border_status"]) and st.all()
    assert np.abs(got.astype(np.float64) - golden["border_next"]).max() <= 0.02


def test_rows_are_independent(lib, golden, pairs):
    name = "720x1280"
    h, w = F.LK_CASES[name][:2]
    pts = golden[f"{name}_pts"][:100]
    with Flow(lib, h, w) as fl:
        got, st = fl.pair(*pairs[name], pts)
        perm = np.random.default_rng(1).permutation(len(pts))
        got_p, st_p = fl.pair(*pairs[name], pts[perm])
        assert np.array_equal(got_p, got[perm]) and np.array_equal(st_p, st[perm])
        F.flow_set_reference(lib, fl.h, pairs[name][0])
        for i in range(len(pts)):                              # each point alone, going back and forth between the two frames
            one, s1 = F.flow_track(lib, fl.h, pairs[name][1], pts[i:i + 1])
            assert np.array_equal(one[0], got[i]) and s1[0] == st[i], i
            assert lib.opd_flow_track(fl.h, C.c_void_p(pairs[name][0].ctypes.data), 0, h, w, None, 0, None, None) == _capi.OPD_OK


def test_reference_hand_over_and_memory_kinds(lib, golden, pairs):
    name = "97x131"
    h, w, seed, _ = F.LK_CASES[name]
    f0, f1 = pairs[name]
    f2 = F.structured_pair(h, w, seed, shift=(3, 2))[1]
    pts = golden[f"{name}_pts"]
    with Flow(lib, h, w) as fl:
        first = fl.pair(f0, f1, pts)
        chained = F.flow_track(lib, fl.h, f2, pts)            # set_reference(f0); track(f1); track(f2)
        direct = fl.pair(f1, f2, pts)                          # set_reference(f1); track(f2)
        assert np.array_equal(chained[0], direct[0]) and np.array_equal(chained[1], direct[1])
        want = F.pyramid(f1)
        for g, wl in zip(F.flow_levels(lib, fl.h, which=1), want):   # the pyramid the reference replaced is f1's
            assert np.array_equal(g, wl)
        keep = [torch.from_numpy(f).cuda() for f in (f0, f1)]
        torch.cuda.synchronize()
        dev = fl.pair(*[(t.data_ptr(), h, w) for t in keep], pts, mem_kind=_capi.OPD_MEM_DEVICE)
        assert np.array_equal(dev[0], first[0]) and np.array_equal(dev[1], first[1])


def test_refusals(lib, golden, pairs):
    name = "97x131"
    h, w = F.LK_CASES[name][:2]
    f0, f1 = pairs[name]
    pts = np.ascontiguousarray(golden[f"{name}_pts"][:8])
    out, st = np.zeros((8, 2), np.float32), np.zeros(8, np.uint8)
    vp = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    handle = C.c_void_p()
    for cfg, text in ((dict(win=20), "must be odd"), (dict(win=23), "must be odd"), (dict(max_level=8), "max_level"), (dict(max_h=0), "max_h")):
        c = _capi.OpdFlowConfig(**{**dict(max_h=h, max_w=w, max_points=8), **cfg})
        assert lib.opd_flow_create(C.byref(c), 0, C.byref(handle)) == _capi.OPD_EINVAL and text in _capi.last_error(), cfg
        assert not handle.value
    assert lib.opd_flow_create(None, 0, C.byref(handle)) == _capi.OPD_EINVAL and "null argument" in _capi.last_error()
    with Flow(lib, h, w, max_points=8) as fl:
        def track(frame=f1, kind=0, hh=h, ww=w, p=pts, n=8, o=out, s=st):
            return lib.opd_flow_track(fl.h, vp(frame), kind, hh, ww, vp(p), n, vp(o), vp(s))

        assert track() == _capi.OPD_ESTATE and "no reference frame" in _capi.last_error()
        assert lib.opd_flow_set_reference(fl.h, None, 0, h, w) == _capi.OPD_EINVAL and "null frame" in _capi.last_error()
        assert lib.opd_flow_set_reference(fl.h, vp(f0), 0, h + 1, w) == _capi.OPD_EINVAL and "created for up to" in _capi.last_error()
        assert lib.opd_flow_set_reference(fl.h, vp(f0), 0, h, w + 1) == _capi.OPD_EINVAL and "created for up to" in _capi.last_error()
        assert lib.opd_flow_set_reference(fl.h, vp(f0), 5, h, w) == _capi.OPD_EINVAL and "mem_kind must be" in _capi.last_error()
        assert lib.opd_flow_set_reference(fl.h, vp(f0), _capi.OPD_MEM_DEVICE, h, w) == _capi.OPD_EINVAL and "not device-accessible" in _capi.last_error()
        assert track() == _capi.OPD_ESTATE                      # none of the refused calls set a reference
        F.flow_set_reference(lib, fl.h, f0)
        want = F.flow_track(lib, fl.h, f1, pts)
        F.flow_set_reference(lib, fl.h, f0)
        small = np.ascontiguousarray(f1[:h - 1])
        for kwargs, text in ((dict(frame=None), "null frame"), (dict(p=None), "null point"), (dict(o=None), "null point"), (dict(s=None), "null point"),
                             (dict(hh=h + 1), "created for up to"), (dict(frame=small, hh=h - 1), "the reference has"), (dict(n=9), "9 points"),
                             (dict(n=-1), "-1 points"), (dict(kind=_capi.OPD_MEM_DEVICE), "not device-accessible"), (dict(kind=2), "mem_kind must be")):
            assert track(**kwargs) == _capi.OPD_EINVAL, kwargs
            assert text in _capi.last_error(), (kwargs, _capi.last_error())
        got = F.flow_track(lib, fl.h, f1, pts)                  # the handle is as it was: same reference, same answer
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        hh, ww, nl = C.c_int(), C.c_int(), C.c_int()
        assert lib.opd_flow_test_level(fl.h, 0, 7, None, C.byref(hh), C.byref(ww), C.byref(nl)) == _capi.OPD_EINVAL


def test_tracker_end_to_end(lib, golden):
    shift = F.SHIFTS[1]
    a, b = F.analytic_pair(shift)
    pts = np.concatenate([golden["shift_pts"][:6], np.array([[-60.0, 100.0]], np.float32)])     # the last one is lost
    want, status = F.lk_restatement(a, b, pts)
    assert status.tolist() == [1] * 6 + [0]
    dets = [Detection(bbox=(float(x) - 10.0, float(y) - 20.0, 20.0, 40.0), confidence=0.9, class_id=1, class_name="person",
                      camera_coords=(float(x), float(y) + 20.0), track_id=100 + i) for i, (x, y) in enumerate(pts)]
    dets.insert(2, Detection(bbox=(5.0, 5.0, 9.0, 9.0), confidence=0.5, class_id=1, class_name="person", camera_coords=(9.5, 14.0)))
    t = HipOpticalFlowTracker()
    assert t.track(a) == {}
    t.initialize(a, dets)
    assert t.prev_track_ids == [100 + i for i in range(7)] and np.array_equal(t.prev_points.reshape(-1, 2), pts)
    tracked = t.track(b)
    assert sorted(tracked) == [100 + i for i in range(6)]
    for i in range(6):
        v = tracked[100 + i]
        assert v.shape == (2,) and v.dtype == np.float32 and np.abs(v.astype(np.float64) - want[i]).max() <= 0.02, i
    assert t.prev_track_ids == [100 + i for i in range(6)]
    assert t.prev_points.shape == (6, 1, 2) and t.prev_points.dtype == np.float32
    assert np.array_equal(t.prev_points.reshape(-1, 2), np.stack([tracked[100 + i] for i in range(6)]))
    # the next frame: b is the reference now; a device-resident frame gives what the host frame gives
    second = t.track(torch.from_numpy(a).cuda())
    back, st_back = F.lk_restatement(b, a, np.stack([tracked[100 + i] for i in range(6)]))
    for i in np.flatnonzero(st_back):
        assert np.abs(second[100 + i].astype(np.float64) - back[i]).max() <= 0.02
    t.reset()
    assert t.track(a) == {} and t.prev_points is None
    t.close()
