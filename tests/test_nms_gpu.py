"""GPU tests of the on-device person filter + NMS (-m gpu): ``person_nms_kernel`` through ``opd_detr_nms_records`` on every case of
tests/nms_common.py, the refusals of the two new entry points, and ``opd_detr_set_nms`` / ``HipDetrDetector(device_nms=True)`` end to
end through every detect path.

Everything here is an equality: the first ``counts[f]`` records of each frame bytewise, and the counts, against ``opd_person_nms_batch``
on a host copy of the same records; ``Detection`` lists field for field between the two modes.  The seeded detector at threshold 0.05
labels nearly every query a person, and on the 180 x 320 frame of test_detect_reid_gpu.py suppression keeps one record of them."""

import ctypes as C
import faulthandler

import numpy as np
import pytest
import torch

import color_common as CC
import nms_common as N
from office_person_detection_vit_amd import HipDetrDetector, HipFloorMapper, HipOSNetReIDExtractor, _capi
from office_person_detection_vit_amd.frames import structured_frames
from office_person_detection_vit_amd.weights import DetrArch, ensure_osnet_weight_file, ensure_weight_file

pytestmark = pytest.mark.gpu

PERSON = 1
THRESHOLD = 0.05
CASES = N.cases()
FM = (1878, 1369, 28.1926406926406, 28.241430700447)
ZONES = [{"id": "zone_1", "polygon": [[859, 912], [1095, 912], [1095, 1350], [859, 1350]], "priority": 1},
         {"id": "zone_2", "polygon": [[1095, 912], [1331, 912], [1331, 1350], [1095, 1350]], "priority": 2}]


@pytest.fixture(autouse=True)
def _time_limit():
    """Every test runs under its own limit: a hang ends the process (with a traceback) instead of holding the GPU."""
    faulthandler.dump_traceback_later(300, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def lib():
    return _capi.load_library(test_hooks=True)


def _pair(weight_cache, max_size):
    path = ensure_weight_file(weight_cache, DetrArch(), 0, 1.0, "r50")
    out = []
    for on in (False, True):
        d = HipDetrDetector(model_path=path, max_batch=2, max_size=max_size, resize=True, confidence_threshold=THRESHOLD, device_nms=on)
        d.load_model()
        out.append(d)
    return out


@pytest.fixture(scope="module")
def small(weight_cache):
    """(host-NMS detector, device-NMS detector) at 256 x 320."""
    pair = _pair(weight_cache, (256, 320))
    yield pair
    for d in pair:
        d.close()


@pytest.fixture(scope="module")
def wide(weight_cache):
    """The same at 288 x 512, the handle of test_detect_reid_gpu.py."""
    pair = _pair(weight_cache, (288, 512))
    yield pair
    for d in pair:
        d.close()


@pytest.fixture(scope="module")
def ext(weight_cache):
    e = HipOSNetReIDExtractor(model_path=ensure_osnet_weight_file(weight_cache, "half"), max_crops=128)
    e.load_model()
    yield e
    e.cleanup()


def _frames(n, h, w, seed):
    frames = [np.ascontiguousarray(f).copy() for f in structured_frames(n, h, w, seed=seed)]
    for f in frames:
        f[60:80, 100:130] = CC.UNIFORM_BGR   # (the frames of test_detect_reid_gpu.py, whose person counts are known)
    return frames


def _device_nms(lib, model, case):
    """opd_detr_nms_records on a device copy of the case (uploaded through torch tensors): (rc, dets, counts) back on the host."""
    dets = torch.from_numpy(case["dets"].view(np.int32).reshape(len(case["counts"]), case["stride"], 8).copy()).cuda()
    counts = torch.from_numpy(case["counts"].copy()).cuda()
    rc = lib.opd_detr_nms_records(C.c_void_p(model), C.c_void_p(dets.data_ptr()), C.c_void_p(counts.data_ptr()), len(case["counts"]), case["stride"],
                                  case["label"], C.c_float(float(case["thr"])))
    torch.cuda.synchronize()
    return rc, dets.cpu().numpy().reshape(len(case["counts"]), case["stride"] * 8).view(N.DET), counts.cpu().numpy()


def _as_case(dets, counts, thr, label=PERSON):
    return {"name": "records", "dets": dets, "counts": counts, "stride": dets.shape[1], "label": label, "thr": np.float32(thr), "expect_counts": None}


def _raw(lib, det, frames, mem_kind=_capi.OPD_MEM_HOST, out=None):
    """opd_detr_detect_frames on `det`'s handle 0: (dets [B][Q], counts [B]) as the call leaves them (host outputs unless `out` is given)."""
    B, Q = len(frames), det.num_queries
    target = det._frame_list_target(frames)
    dets, counts = np.zeros((B, Q), N.DET), np.zeros(B, np.int32)
    ptrs = (C.c_void_p * B)(*[f.ctypes.data for f in frames])
    rec_ptr, cnt_ptr = out if out else (dets.ctypes.data, counts.ctypes.data)
    rc = lib.opd_detr_detect_frames(C.c_void_p(det.model), ptrs, mem_kind, B, frames[0].shape[0], frames[0].shape[1], target[0], target[1], THRESHOLD,
                                    C.cast(C.c_void_p(rec_ptr), C.POINTER(_capi.OpdDet)), C.cast(C.c_void_p(cnt_ptr), C.POINTER(C.c_int32)))
    _capi.check(rc, "opd_detr_detect_frames")
    return dets, counts


def _host_nms(lib, dets, counts, thr):
    rc, d, c = N.run_host(lib.opd_person_nms_batch, _as_case(dets, counts, thr))
    assert rc == _capi.OPD_OK
    return d, c


def _fields(d):
    return (d.bbox, d.confidence, d.class_id, d.class_name, d.camera_coords, d.floor_coords, d.floor_coords_mm, tuple(d.zone_ids), d.track_id,
            None if d.features is None else np.asarray(d.features).tobytes(), d.appearance_score, d.query_index)


def _same_detections(a, b, what):
    assert [_fields(d) for d in a] == [_fields(d) for d in b], what


# ---- 1. the kernel ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_kernel_equals_host_nms(lib, small, case):
    rc, dets, counts = _device_nms(lib, small[1].model, case)
    assert rc == _capi.OPD_OK, _capi.last_error()
    rc, hd, hc = N.run_host(lib.opd_person_nms_batch, case)
    assert rc == _capi.OPD_OK
    N.assert_same(case["name"], (dets, counts), (hd, hc))
    N.assert_expectations(case, dets, counts)
    for f in np.flatnonzero(case["counts"] < 0):   # the padding slot of an uneven shard is left alone
        assert dets[f].tobytes() == case["dets"][f].tobytes()


def test_refusals(lib, small):
    model = small[1].model
    case = next(c for c in CASES if c["name"] == "batch3_s100")
    host_d, host_c = case["dets"].copy(), case["counts"].copy()
    args = lambda d, c, n=3, stride=100: (C.c_void_p(model), C.c_void_p(d), C.c_void_p(c), n, stride, PERSON, C.c_float(0.4))
    assert lib.opd_detr_nms_records(*args(host_d.ctypes.data, host_c.ctypes.data)) == _capi.OPD_EINVAL       # host pointers
    assert "device-accessible" in _capi.last_error()
    assert host_d.tobytes() == case["dets"].tobytes() and np.array_equal(host_c, case["counts"])
    dev_d = torch.from_numpy(case["dets"].view(np.int32).copy()).cuda()
    dev_c = torch.from_numpy(case["counts"].copy()).cuda()
    assert lib.opd_detr_nms_records(*args(dev_d.data_ptr(), host_c.ctypes.data)) == _capi.OPD_EINVAL         # one of the two on the host
    for stride in (0, 129):
        assert lib.opd_detr_nms_records(*args(dev_d.data_ptr(), dev_c.data_ptr(), stride=stride)) == _capi.OPD_EINVAL
        assert "stride" in _capi.last_error()
    assert lib.opd_detr_nms_records(*args(dev_d.data_ptr(), dev_c.data_ptr(), n=-1)) == _capi.OPD_EINVAL
    assert lib.opd_detr_nms_records(None, C.c_void_p(dev_d.data_ptr()), C.c_void_p(dev_c.data_ptr()), 3, 100, PERSON, C.c_float(0.4)) == _capi.OPD_EINVAL
    torch.cuda.synchronize()
    assert dev_d.cpu().numpy().tobytes() == case["dets"].tobytes() and np.array_equal(dev_c.cpu().numpy(), case["counts"])   # nothing ran
    # a count above the stride: refused after the wait, that frame as it was, the other frames done
    over = dict(case, counts=np.int32([37, 101, 100]))
    rc, dets, counts = _device_nms(lib, model, over)
    assert rc == _capi.OPD_EINVAL and "more records than its slots" in _capi.last_error()
    assert counts[1] == 101 and dets[1].tobytes() == case["dets"][1].tobytes()
    rc, hd, hc = N.run_host(lib.opd_person_nms_batch, dict(case, counts=np.int32([37, -1, 100])))
    assert counts[0] == hc[0] and counts[2] == hc[2] and N.kept_bytes(dets, counts)[0] == N.kept_bytes(hd, hc)[0]
    # ... and the refusal does not stick: the next call is judged on its own records
    rc, dets, counts = _device_nms(lib, model, case)
    assert rc == _capi.OPD_OK
    N.assert_same("after a refusal", (dets, counts), (hd, hc))
    # opd_detr_set_nms
    assert lib.opd_detr_set_nms(C.c_void_p(model), PERSON, C.c_float(float("nan"))) == _capi.OPD_EINVAL and "NaN" in _capi.last_error()
    assert lib.opd_detr_set_nms(None, PERSON, C.c_float(0.4)) == _capi.OPD_EINVAL
    assert lib.opd_detr_nms_records(*args(dev_d.data_ptr(), dev_c.data_ptr(), n=0)) == _capi.OPD_OK


# ---- 2. end to end: the two modes return the same detections -----------------------------------------------------------------------------------
def test_both_modes_return_the_same_detections(lib, small, wide, ext):
    removed = 0
    for (off, on), frames in ((small, _frames(3, 256, 320, seed=41)),
                              (wide, _frames(1, 96, 160, seed=5) * 2 + _frames(1, 96, 160, seed=6)),
                              (wide, _frames(3, 180, 320, seed=41))):
        hw = frames[0].shape[:2]
        assert off._frame_list_target(frames) is not None                # the fused one-call paths are the ones compared
        raw_d, raw_c = _raw(lib, off, frames[:1])
        want = off.detect(frames[0])
        removed += int((raw_d[0, :raw_c[0]]["label"] == PERSON).sum()) - len(want)
        print(f"{hw} -> {on.max_size}: {int(raw_c[0])} records, {len(want)} detections after suppression")
        _same_detections(on.detect(frames[0]), want, f"detect {hw}")
        got_b, want_b = on.detect_batch(frames), off.detect_batch(frames)          # 3 frames, max_batch = 2: two chunks
        assert len(got_b) == len(want_b) == 3
        for g, w in zip(got_b, want_b):
            _same_detections(g, w, f"detect_batch {hw}")
        for kind, kw in (("encoder", {}), ("color", {}), ("reid", {"reid": ext, "reid_slots": 32})):
            (gd, gf), (wd, wf) = on.detect_with_features(frames[0], features=kind, **kw), off.detect_with_features(frames[0], features=kind, **kw)
            _same_detections(gd, wd, f"detect_with_features({kind}) {hw}")
            assert np.asarray(gf).dtype == np.asarray(wf).dtype and np.array_equal(np.asarray(gf), np.asarray(wf)), (kind, hw)
            assert all(d.features is not None for d in gd)
        try:   # the IoU limit at which nothing is suppressed, assigned as callers assign it: order and rows of MANY kept records
            off.nms_threshold = on.nms_threshold = 1.0
            want1 = off.detect(frames[0])
            assert len(want1) > len(want) and len(want1) >= 2
            _same_detections(on.detect(frames[0]), want1, f"detect at 1.0 {hw}")
            for g, w in zip(on.detect_batch(frames), off.detect_batch(frames)):
                _same_detections(g, w, f"detect_batch at 1.0 {hw}")
            for kind, kw in (("encoder", {}), ("color", {}), ("reid", {"reid": ext, "reid_slots": 32})):
                (gd, gf), (wd, wf) = on.detect_with_features(frames[0], features=kind, **kw), off.detect_with_features(frames[0], features=kind, **kw)
                _same_detections(gd, wd, f"detect_with_features({kind}) at 1.0 {hw}")
                assert len(gd) == len(want1) and np.array_equal(np.asarray(gf), np.asarray(wf)), (kind, hw)
        finally:
            off.nms_threshold = on.nms_threshold = 0.4
        rng = np.random.default_rng(9)
        src = np.concatenate([np.array([[0, 0], [hw[1], 0], [0, hw[0]], [hw[1], hw[0]]], float), rng.uniform((10, 10), (hw[1] - 10, hw[0] - 10), (20, 2))])
        dst = np.stack([5.5 * src[:, 0] + 40 + 15 * np.sin(src[:, 1] / 40.0), 7.0 * src[:, 1] + 30 + 10 * np.cos(src[:, 0] / 50.0)], 1)
        mapper = HipFloorMapper.piecewise_affine(src, dst, FM, ZONES)
        try:
            got_f, want_f = on.detect(frames[0], floor_map=mapper), off.detect(frames[0], floor_map=mapper)
            _same_detections(got_f, want_f, f"detect(floor_map) {hw}")
            assert all(d.floor_coords is not None for d in got_f)
            for g, w in zip(on.detect_batch(frames, floor_map=mapper), off.detect_batch(frames, floor_map=mapper)):
                _same_detections(g, w, f"detect_batch(floor_map) {hw}")
            try:
                off.nms_threshold = on.nms_threshold = 1.0
                got_f, want_f = on.detect(frames[0], floor_map=mapper), off.detect(frames[0], floor_map=mapper)
                _same_detections(got_f, want_f, f"detect(floor_map) at 1.0 {hw}")
                assert len(got_f) >= 2 and all(d.floor_coords is not None for d in got_f)
            finally:
                off.nms_threshold = on.nms_threshold = 0.4
        finally:
            mapper.close()
    assert removed >= 1, "host suppression removes nothing on any of these frames: the comparison shows nothing"


# ---- 3. the Re-ID call's counts and slots ----------------------------------------------------------------------------------------------------
def _fused_reid(lib, det, ext, frames, slots):
    B, Q = len(frames), det.num_queries
    dets, counts = np.zeros((B, Q), N.DET), np.zeros(B, np.int32)
    feats, slot_map, n_person = np.zeros((slots, ext.feature_dim), np.float32), np.full(slots, -9, np.int32), C.c_int32(-9)
    ptrs = (C.c_void_p * B)(*[f.ctypes.data for f in frames])
    h, w = frames[0].shape[:2]
    rc = lib.opd_detr_detect_frames_reid(C.c_void_p(det.model), ext._handle, ptrs, B, h, w, 288, 512, THRESHOLD, PERSON, slots,
                                         dets.ctypes.data_as(C.POINTER(_capi.OpdDet)), counts.ctypes.data_as(C.POINTER(C.c_int32)),
                                         feats.ctypes.data, slot_map.ctypes.data, C.byref(n_person))
    _capi.check(rc, "opd_detr_detect_frames_reid")
    return dets, counts, slot_map, int(n_person.value)


def test_reid_slots_go_to_the_kept_records(lib, wide, ext):
    off, on = wide
    Q = on.num_queries
    frames = _frames(1, 180, 320, seed=41) + _frames(1, 180, 320, seed=43)
    raw_d, raw_c = _raw(lib, off, frames)
    persons = int(sum((raw_d[b, :raw_c[b]]["label"] == PERSON).sum() for b in range(2)))
    try:
        for thr in (on.nms_threshold, 1.0):
            on.nms_threshold = thr
            on._sync_nms()
            want_d, want_c = _host_nms(lib, raw_d, raw_c, thr)
            dets, counts, slot_map, n_person = _fused_reid(lib, on, ext, frames, 128)
            N.assert_same(f"fused Re-ID records at {thr}", (dets, counts), (want_d, want_c))
            assert n_person == int(counts.sum())                                        # the kept count
            order = [b * Q + int(q) for b in range(2) for q in dets[b, :counts[b]]["query_index"]]   # score order within each frame
            n = min(n_person, 128)
            assert slot_map[:n].tolist() == order[:n] and (slot_map[n:] == -9).all()
            if thr == 1.0:
                assert n_person == persons                                              # nothing suppressed: every person record
            else:
                assert counts[0] == 1 and n_person < persons                            # the frame where suppression keeps one record
    finally:
        on.nms_threshold = off.nms_threshold
        on._sync_nms()


# ---- 4. the other ways records leave the handle ------------------------------------------------------------------------------------------------
def test_ticketed_submissions_deliver_the_same_records(lib, wide):
    on = wide[1]
    Q, model = on.num_queries, C.c_void_p(on.model)
    frames = _frames(2, 288, 512, seed=47)
    blocking = []
    for f in frames:
        d, c = np.zeros((1, Q), N.DET), np.zeros(1, np.int32)
        _capi.check(lib.opd_detr_detect(model, f.ctypes.data, _capi.OPD_PIXELS_U8_BGR_HWC, _capi.OPD_MEM_HOST, 1, 288, 512, THRESHOLD, None,
                                        d.ctypes.data_as(C.POINTER(_capi.OpdDet)), c.ctypes.data_as(C.POINTER(C.c_int32))), "opd_detr_detect")
        blocking.append((d, c))
    outs, tickets = [], []
    for f in frames:                                                                   # two submissions outstanding at once
        d, c, t = np.zeros((1, Q), N.DET), np.zeros(1, np.int32), C.c_int(-1)
        _capi.check(lib.opd_detr_detect_async(model, f.ctypes.data, _capi.OPD_PIXELS_U8_BGR_HWC, _capi.OPD_MEM_HOST, 1, 288, 512, THRESHOLD, None,
                                              d.ctypes.data_as(C.POINTER(_capi.OpdDet)), c.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(t)), "opd_detr_detect_async")
        outs.append((d, c))
        tickets.append(t.value)
    for t in tickets:
        _capi.check(lib.opd_detr_wait(model, t), "opd_detr_wait")
    for k in range(2):
        N.assert_same(f"ticket {k}", outs[k], blocking[k])
        raw_d, raw_c = _raw(lib, wide[0], [frames[k]])
        N.assert_same(f"blocking {k}", blocking[k], _host_nms(lib, raw_d, raw_c, on.nms_threshold))
    assert sum(int(c[0]) for _, c in blocking) >= 1


def test_device_outputs_hold_the_suppressed_records(lib, wide):
    off, on = wide
    Q = on.num_queries
    frames = _frames(2, 180, 320, seed=41)
    dev_d = torch.full((2, Q, 8), -1, dtype=torch.int32, device="cuda")
    dev_c = torch.full((2,), -5, dtype=torch.int32, device="cuda")
    _raw(lib, on, frames, _capi.OPD_MEM_HOST_PIXELS_DEVICE_OUT, out=(dev_d.data_ptr(), dev_c.data_ptr()))
    torch.cuda.synchronize()
    got = (dev_d.cpu().numpy().reshape(2, Q * 8).view(N.DET), dev_c.cpu().numpy())
    raw_d, raw_c = _raw(lib, off, frames)
    want = _host_nms(lib, raw_d, raw_c, on.nms_threshold)
    N.assert_same("device outputs", got, want)
    assert 0 < int(want[1].sum()) < int(raw_c.sum())
    # the Python surface of the sharded path writes the same buffers
    dev_d.fill_(-1); dev_c.fill_(-5)
    on.detect_records_into(frames, dev_d, dev_c)
    torch.cuda.synchronize()
    N.assert_same("detect_records_into", (dev_d.cpu().numpy().reshape(2, Q * 8).view(N.DET), dev_c.cpu().numpy()), want)


def test_setting_off_restores_unsuppressed_records(lib, wide):
    off, on = wide
    frames = _frames(2, 180, 320, seed=41)
    raw = _raw(lib, off, frames)
    try:
        assert lib.opd_detr_set_nms(C.c_void_p(on.model), PERSON, C.c_float(-1.0)) == _capi.OPD_OK
        got = _raw(lib, on, frames)
        N.assert_same("setting off", got, raw)
        for b in range(2):
            assert (np.diff(got[0][b, :got[1][b]]["query_index"]) > 0).all()            # query order, unsuppressed
    finally:
        on._nms_set = None
        on._sync_nms()
    N.assert_same("setting on again", _raw(lib, on, frames), _host_nms(lib, *raw, on.nms_threshold))
