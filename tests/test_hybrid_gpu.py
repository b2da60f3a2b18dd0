"""Hybrid tracking with one host wait: a run of in-between frames (``opd_lwt_interpolate_sequence``,
``HipLightweightTracker.interpolate_sequence``), detection frames inside the detect call (``opd_detr_detect_frames_hybrid``,
``HipDetrDetector.detect_and_track_hybrid``) and a run of key and in-between frames of one camera (``opd_detr_detect_sequence_hybrid``,
``HipDetrDetector.track_hybrid_batch``).

Every comparison is an equality of bits between a handle that takes the new call and a twin, made alike and fed the same frames, that
takes the per-frame calls ``opd_detr_detect_frames``, ``opd_lwt_update`` and ``opd_lwt_interpolate``: ids, the records of every frame,
every number of every track (``opd_lwt_get``), and the counts of ``opd_lwt_info``.  The per-frame calls are pinned to the reference and to
the numpy restatement by test_lwt_gpu.py; nothing here has a tolerance.  The ingest launch alone is held to its numpy restatement
(lwt_ingest_common.py), which test_hybrid_cpu.py holds to the Python path."""

import ctypes as C
import faulthandler

import numpy as np
import pytest
import torch

import flow_common as FC
import lwt_common as LC
import lwt_ingest_common as LI
import track_common as TC
from office_person_detection_vit_amd import Detection, HipDetrDetector, HipLightweightTracker, _capi
from office_person_detection_vit_amd.frames import structured_frames
from office_person_detection_vit_amd.weights import DetrArch, ensure_weight_file

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
HH, WW, SEED = 97, 131, 501
P_FLOW = dict(max_age=30, iou_threshold=0.3, use_optical_flow=True)


@pytest.fixture(autouse=True)
def _time_limit():
    """Every test runs under its own limit: a hang ends the process (with a traceback) instead of holding the GPU."""
    faulthandler.dump_traceback_later(120, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def lib():
    return _capi.load_library(test_hooks=True)


def _shifted(f):
    """The frame moved by the integer shift (2 rows, 1 column), the flat rectangle painted over it (test_lwt_gpu.py's third frame)."""
    ys, xs = np.clip(np.arange(HH) - 2, 0, HH - 1), np.clip(np.arange(WW) - 1, 0, WW - 1)
    g = f[ys][:, xs].copy()
    y0, y1, x0, x1 = FC.flat_rect(HH, WW)
    g[y0:y1, x0:x1] = FC.FLAT_BGR
    return np.ascontiguousarray(g)


@pytest.fixture(scope="module")
def frames():
    """Four frames: test_lwt_gpu.py's three (a structured frame, each next one the one before moved by an integer shift) and one more shift."""
    f0, f1 = FC.structured_pair(HH, WW, SEED, (2, 1))
    f2 = _shifted(f1)
    out = [np.ascontiguousarray(f0), np.ascontiguousarray(f1), f2, _shifted(f2)]
    for f in out:
        f.setflags(write=False)
    return out


def _boxes_21():
    """test_lwt_gpu.py's 21 boxes: centres on a 7 x 3 grid, the first inside the flat rectangle (a point LK loses)."""
    cx, cy = np.meshgrid(np.linspace(WW * 0.12, WW * 0.88, 7), np.linspace(HH * 0.2, HH * 0.8, 3))
    c = np.round(np.stack([cx.ravel(), cy.ravel()], 1) * 4) / 4
    y0, y1, x0, x1 = FC.flat_rect(HH, WW)
    c[0] = [(x0 + x1) / 2.0, (y0 + y1) / 2.0]
    w, h = 8.0 + 0.5 * (np.arange(21) % 4), 12.0 + 0.25 * (np.arange(21) % 3)
    return np.stack([c[:, 0] - w / 2, c[:, 1] - h / 2, w, h], 1).astype(F32)


def _sequence(lib, h, frames, capacity, F=None):
    """opd_lwt_interpolate_sequence on host arrays, (device pointer, h, w) tuples or None (no frame list); returns (rc, [records per frame])."""
    if frames is None:
        ptrs, kind, fh, fw = None, 0, 0, 0
    else:
        args = [LC._frame_args(f) for f in frames]
        assert len({a[1:] for a in args}) == 1
        ptrs, (_, kind, fh, fw) = (C.c_void_p * len(args))(*[a[0] for a in args]), args[0]
        F = len(args) if F is None else F
    recs, counts = (_capi.OpdLwtRec * (capacity * F))(), (C.c_int32 * F)(*([-7] * F))
    rc = lib.opd_lwt_interpolate_sequence(h, ptrs, kind, F, fh, fw, recs, capacity, counts)
    if rc != 0:
        return rc, None
    return rc, [[(recs[f * capacity + i].track_id, tuple(float(v) for v in recs[f * capacity + i].bbox)) for i in range(counts[f])] for f in range(F)]


def _observe(lib, h):
    """Every number of every track as bytes, and (n_tracks, next_id, n_points)."""
    st = LC.info(lib, _capi, h)
    return [a.tobytes() for a in LC.device_states(lib, _capi, h)], (st.n_tracks, st.next_id, st.n_points)


def _recs_bits(recs):
    return [q[0] for q in recs], np.array([q[1] for q in recs], F64).tobytes()


def _pair(lib, max_tracks=32, **p):
    return tuple(LC.create(lib, _capi, max_tracks=max_tracks, max_dets=32, max_h=HH, max_w=WW, **p) for _ in range(2))


def _start(lib, handles, first, boxes):
    for h in handles:
        rc, ids = LC.device_update(lib, _capi, h, boxes, first)
        assert rc == 0 and ids.tolist() == list(range(1, len(boxes) + 1)), _capi.last_error()


def _run_both(lib, a, b, run, what, launches_per_frame):
    """`run` through the sequence call on a and through the per-frame loop on b: equal records, states and counts; returns b's point counts."""
    rc, got = _sequence(lib, a, run, capacity=64)
    assert rc == 0, _capi.last_error()
    info = LC.info(lib, _capi, a)
    assert info.last_waits == 1 and info.last_launches == launches_per_frame * len(run), (what, info.last_launches)
    points = []
    for f, fr in enumerate(run):
        want = LC.device_interpolate(lib, _capi, b, fr)
        assert LC.info(lib, _capi, b).last_waits == 1
        points.append(LC.info(lib, _capi, b).n_points)
        assert _recs_bits(got[f]) == _recs_bits(want), (what, f)
    assert _observe(lib, a) == _observe(lib, b), what
    return points


# ---- 1. the sequence against the loop -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("on_device", [False, True])
def test_interpolate_sequence_equals_the_per_frame_loop(lib, frames, on_device):
    keep = [torch.from_numpy(np.array(f)).to("cuda") for f in frames] if on_device else None
    torch.cuda.synchronize()
    fr = [(k.data_ptr(), HH, WW) for k in keep] if on_device else frames
    a, b = _pair(lib, **P_FLOW)
    try:
        _start(lib, (a, b), fr[0], _boxes_21())
        points = _run_both(lib, a, b, fr[1:], "three frames", launches_per_frame=5)   # gray, two pyramid levels, LK, the tracks
        lost_total = 21 - points[-1]
        assert 0 < lost_total < 21, points   # what makes this meaningful: LK launches ran for a bound above the count, and points were followed
        assert points[0] < 21 or points[1] < points[0], points   # ... and the bound exceeded the count BEFORE the last frame's launch
        # the call left a usable reference and a complete state: one more per-frame call on both, then a detection frame, then one frame each way
        assert _recs_bits(LC.device_interpolate(lib, _capi, a, fr[2])) == _recs_bits(LC.device_interpolate(lib, _capi, b, fr[2]))
        assert _observe(lib, a) == _observe(lib, b)
        for h in (a, b):
            rc, _ = LC.device_update(lib, _capi, h, _boxes_21() + np.array([1.0, 1.0, 0.0, 0.0], F32), fr[1])
            assert rc == 0, _capi.last_error()
        assert _run_both(lib, a, b, fr[2:3], "one frame", launches_per_frame=5)[0] > 0
    finally:
        for h in (a, b):
            lib.opd_lwt_destroy(h)


def test_no_point_left_in_the_middle_of_a_sequence(lib, frames):
    """Two uniform frames and a structured one behind the three shifted frames.  Against a uniform REFERENCE every window's gradient matrix is
    zero, so LK gives every point up on the second uniform frame at the latest: the last frame meets a device count of zero under a launch
    sized for 21 points, and builds a pyramid the per-frame loop (which skips the frame) does not -- which nothing can observe."""
    flat = np.full((HH, WW, 3), 128, np.uint8)
    run = frames[1:] + [flat, flat.copy(), frames[1]]
    a, b = _pair(lib, max_tracks=64, **P_FLOW)   # (room for the tracks of a second detection frame that matches few of the moved boxes)
    try:
        _start(lib, (a, b), frames[0], _boxes_21())
        points = _run_both(lib, a, b, run, "six frames", launches_per_frame=5)
        assert points[2] > 0 and points[4] == 0 and points[5] == 0, points
        # without points at entry the call reads no frame, as the loop does not: a frame of another size is accepted by both
        other = np.zeros((HH - 1, WW, 3), np.uint8)
        assert _run_both(lib, a, b, [other, other], "no points at entry", launches_per_frame=1) == [0, 0]
        # the next detection frame replaces the reference on both, and both go on alike
        for h in (a, b):
            rc, _ = LC.device_update(lib, _capi, h, _boxes_21(), frames[1])
            assert rc == 0, _capi.last_error()
        assert _observe(lib, a) == _observe(lib, b)
        assert _run_both(lib, a, b, frames[2:], "after the next detection frame", launches_per_frame=5)[-1] > 0
    finally:
        for h in (a, b):
            lib.opd_lwt_destroy(h)


def test_sequence_without_optical_flow_and_without_tracks(lib, frames):
    p = dict(P_FLOW, use_optical_flow=False)
    a, b = _pair(lib, **p)
    c, d = _pair(lib, **P_FLOW)
    try:
        rc, got = _sequence(lib, a, None, capacity=32, F=3)   # a tracker without tracks, no frame list
        assert rc == 0 and got == [[], [], []], _capi.last_error()
        assert LC.info(lib, _capi, a).last_waits == 1 and LC.info(lib, _capi, a).last_launches == 3
        for _ in range(3):
            assert LC.device_interpolate(lib, _capi, b) == []
        assert _observe(lib, a) == _observe(lib, b)
        _start(lib, (a, b), None, _boxes_21())
        for h in (a, b):   # a second detection frame gives the tracks a velocity: every prediction moves the record
            rc, ids = LC.device_update(lib, _capi, h, _boxes_21() + np.array([2.0, 1.0, 0.0, 0.0], F32))
            assert rc == 0 and ids.tolist() == list(range(1, 22)), _capi.last_error()
        rc, got = _sequence(lib, a, None, capacity=32, F=5)   # every track predicted, five times
        assert rc == 0 and LC.info(lib, _capi, a).last_waits == 1 and LC.info(lib, _capi, a).last_launches == 5, _capi.last_error()
        for f in range(5):
            assert _recs_bits(got[f]) == _recs_bits(LC.device_interpolate(lib, _capi, b)), f
        assert len(got[4]) == 21 and got[4] != got[0]
        assert _observe(lib, a) == _observe(lib, b)
        # optical flow, no tracks yet (and no reference frame): the frames are not looked at, as in the per-frame call
        assert _run_both(lib, c, d, frames[:2], "flow, no tracks", launches_per_frame=1) == [0, 0]
    finally:
        for h in (a, b, c, d):
            lib.opd_lwt_destroy(h)


def test_sequence_refusals_change_nothing(lib, frames):
    a, b = _pair(lib, **P_FLOW)
    try:
        _start(lib, (a, b), frames[0], _boxes_21())
        before = _observe(lib, a)

        def refused(text, run, capacity=32, F=None):
            rc, _ = _sequence(lib, a, run, capacity, F)
            assert rc == _capi.OPD_EINVAL and text in _capi.last_error(), (text, _capi.last_error())
            assert _observe(lib, a) == before, text

        refused("max_tracks = 32", frames[1:], capacity=31)
        refused("65 frames", [frames[1]] * 65)
        refused("0 frames", frames[1:], F=0)
        refused("null frame list", None, F=2)
        small = np.zeros((HH - 1, WW, 3), np.uint8)
        refused("the reference has 97 x 131", [small, small])
        big = np.zeros((HH + 1, WW, 3), np.uint8)
        refused("created for up to", [big])
        counts, recs = (C.c_int32 * 2)(), (_capi.OpdLwtRec * 64)()
        ptrs = (C.c_void_p * 2)(C.c_void_p(frames[1].ctypes.data), None)   # the second frame of the list is missing
        assert lib.opd_lwt_interpolate_sequence(a, ptrs, 0, 2, HH, WW, recs, 32, counts) == _capi.OPD_EINVAL and "null frame" in _capi.last_error()
        assert lib.opd_lwt_interpolate_sequence(a, ptrs, 7, 1, HH, WW, recs, 32, counts) == _capi.OPD_EINVAL and "mem_kind" in _capi.last_error()
        host_as_device = (C.c_void_p * 1)(C.c_void_p(frames[1].ctypes.data))   # an ordinary host pointer under OPD_MEM_DEVICE
        assert lib.opd_lwt_interpolate_sequence(a, host_as_device, 1, 1, HH, WW, recs, 32, counts) == _capi.OPD_EINVAL
        assert _observe(lib, a) == before
        _run_both(lib, a, b, frames[1:], "after the refusals", launches_per_frame=5)
    finally:
        for h in (a, b):
            lib.opd_lwt_destroy(h)


# ---- 2. the class ----------------------------------------------------------------------------------------------------------------------------
def _dets(boxes):
    return [Detection(bbox=tuple(float(v) for v in b), confidence=0.9, class_id=1, class_name="person", camera_coords=(0.0, 0.0)) for b in boxes]


@pytest.mark.parametrize("on_device", [False, True])
def test_class_interpolate_sequence_equals_interpolate_in_a_loop(frames, on_device):
    fr = [torch.from_numpy(np.array(f)).to("cuda") for f in frames] if on_device else frames
    a, b = HipLightweightTracker(max_tracks=32), HipLightweightTracker(max_tracks=32)
    try:
        for t in (a, b):
            t.update_with_detections(fr[0], _dets(_boxes_21()))
        got = a.interpolate_sequence(fr[1:])
        assert a.info().last_waits == 1 and 0 < a.info().n_points < 21
        want = [b.interpolate(f) for f in fr[1:]]
        assert got == want and len(got) == 3 and len(got[0]) == 21
        assert all(isinstance(q[0], int) and all(isinstance(v, float) for v in q[1]) for recs in got for q in recs)
        assert [(q.track_id, q.bbox, q.hits, q.time_since_update) for q in a.tracks] == [(q.track_id, q.bbox, q.hits, q.time_since_update) for q in b.tracks]
        assert a.info().n_points == b.info().n_points
        with pytest.raises(ValueError, match="one size"):
            a.interpolate_sequence([fr[1], np.zeros((HH - 1, WW, 3), np.uint8)])
        with pytest.raises(RuntimeError, match="pixels"):
            a.interpolate_sequence([np.zeros((HH - 1, WW, 3), np.uint8)] * 2)   # not the size of the reference frame
    finally:
        a.close()
        b.close()


# ---- 3. the ingest launch alone ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 100, 250, -3])
def test_ingest_alone_equals_the_restatement(lib, n):
    """Counts around the wave's 64 lanes, the full frame, and counts the kernel must clamp."""
    Q = 100
    records = LI.edge_records()
    boxes = np.full((Q, 4), 7.5, F32)
    want = boxes.copy()
    n_want = LI.ingest(records, n, Q, want)
    n_out = np.full(1, -7, np.int32)
    assert lib.opd_lwt_test_ingest(0, TC.ptr(records), n, Q, TC.ptr(boxes), TC.ptr(n_out)) == 0, _capi.last_error()
    assert int(n_out[0]) == n_want
    assert boxes.tobytes() == want.tobytes(), (n, np.argwhere(boxes != want)[:8].tolist())


# ---- 4. detection frames inside the detect call ---------------------------------------------------------------------------------------------
PERSON = 1
DH, DW = 288, 512
FUSED_LAUNCHES = 1 + (1 + 3) + 1   # ingest; gray and the three pyramid levels of 288 x 512; the update


@pytest.fixture(scope="module")
def det(weight_cache):
    """The seeded detector of test_detect_track_gpu.py: at threshold 0.05 all 100 queries are persons with heavily overlapping boxes, so
    suppression at 0.4 keeps ONE record a frame and at 1.0 all 100 (a 100 x 100 greedy match with ties)."""
    path = ensure_weight_file(weight_cache, DetrArch(), 0, 1.0, "r50")
    d = HipDetrDetector(model_path=path, max_batch=2, max_size=(DH, DW), resize=True, confidence_threshold=0.05, device_nms=True)
    d.load_model()
    yield d
    d.close()


@pytest.fixture(scope="module")
def det_frames():
    return [np.ascontiguousarray(f).copy() for f in structured_frames(5, DH, DW, seed=3)]


def _set_nms(det, thr):
    det.device_nms, det.nms_threshold = True, thr
    det._sync_nms()


def _lwt(lib, max_tracks=256, max_dets=128, max_h=DH, max_w=DW, flow=True, iou=0.3):
    return LC.create(lib, _capi, max_tracks=max_tracks, max_dets=max_dets, max_h=max_h, max_w=max_w, max_age=30, iou_threshold=iou, use_optical_flow=flow)


def _no_frame(r):
    """Records without their `frame` field: a frame's index in ITS call, which differs between a batch and a one-frame call."""
    r = r.copy()
    r["frame"] = 0
    return r.tobytes()


def _fused(lib, det, trackers, frames):
    """opd_detr_detect_frames_hybrid: (rc, kept records per frame, ids per frame); ids start as sentinels and must stay so beyond the kept count."""
    B, Q = len(frames), det.num_queries
    recs, counts = (_capi.OpdDet * (B * Q))(), (C.c_int32 * B)()
    ids = np.full((B, Q), -7, np.int32)
    ptrs = (C.c_void_p * B)(*[f.ctypes.data for f in frames])
    hs = (C.c_void_p * B)(*[t.value for t in trackers])
    rc = lib.opd_detr_detect_frames_hybrid(C.c_void_p(det.model), hs, ptrs, B, DH, DW, DH, DW, 0.05, PERSON, recs, counts, ids.ctypes.data)
    raw = np.frombuffer(bytes(recs), LI.DET).reshape(B, Q)
    per = [raw[b, :int(counts[b])].copy() for b in range(B)]
    for b in range(B):
        assert np.all(ids[b, len(per[b]):] == -7), "ids beyond the kept count were written"
    return rc, per, [ids[b, :len(per[b])].copy() for b in range(B)]


def _two_calls(lib, det, tracker, frame):
    """opd_detr_detect_frames on one frame, then opd_lwt_update with the boxes the Python path builds: (rc of the update, records, ids)."""
    Q = det.num_queries
    recs, counts = (_capi.OpdDet * Q)(), (C.c_int32 * 1)()
    ptrs = (C.c_void_p * 1)(frame.ctypes.data)
    _capi.check(lib.opd_detr_detect_frames(C.c_void_p(det.model), ptrs, _capi.OPD_MEM_HOST, 1, DH, DW, DH, DW, 0.05, recs, counts), "opd_detr_detect_frames")
    r = np.frombuffer(bytes(recs), LI.DET)[:int(counts[0])].copy()
    rc, ids = LC.device_update(lib, _capi, tracker, LI.pack(r), frame)
    return rc, r, ids


@pytest.mark.parametrize("nms,kept", [(0.4, 1), (1.0, 100)])
def test_fused_detection_frames_equal_detect_then_update(lib, det, det_frames, nms, kept):
    _set_nms(det, nms)
    a, b = _lwt(lib), _lwt(lib)
    try:
        for f in range(3):
            rc, per, ids = _fused(lib, det, [a], [det_frames[f]])
            assert rc == 0, _capi.last_error()
            rc2, r, ids2 = _two_calls(lib, det, b, det_frames[f])
            assert rc2 == 0, _capi.last_error()
            assert len(r) == kept and per[0].tobytes() == r.tobytes(), f
            assert ids[0].tolist() == ids2.tolist() and _observe(lib, a) == _observe(lib, b), (f, ids[0].tolist(), ids2.tolist())
            info = LC.info(lib, _capi, a)
            assert info.last_waits == 0 and info.last_launches == FUSED_LAUNCHES and info.n_points == kept, (f, info.last_launches, info.n_points)
        if kept == 100:
            assert LC.info(lib, _capi, a).n_tracks >= 100 and min(ids[0]) <= 100   # tracks of the first frame were matched again
        # the fused call left a complete state and a usable reference frame to the handle's own stream: an in-between frame on both
        ra, rb = LC.device_interpolate(lib, _capi, a, det_frames[3]), LC.device_interpolate(lib, _capi, b, det_frames[3])
        assert _recs_bits(ra) == _recs_bits(rb) and _observe(lib, a) == _observe(lib, b)
        assert LC.info(lib, _capi, a).last_waits == 1
    finally:
        for h in (a, b):
            lib.opd_lwt_destroy(h)


def test_fused_detection_frames_of_two_cameras_and_without_optical_flow(lib, det, det_frames):
    _set_nms(det, 1.0)
    a = [_lwt(lib), _lwt(lib, flow=False)]
    b = [_lwt(lib), _lwt(lib, flow=False)]
    try:
        for f in range(2):
            pair = [det_frames[f], det_frames[4 - f]]
            rc, per, ids = _fused(lib, det, a, pair)
            assert rc == 0, _capi.last_error()
            for k in range(2):
                rc2, r, ids2 = _two_calls(lib, det, b[k], pair[k])
                assert rc2 == 0 and _no_frame(per[k]) == _no_frame(r) and ids[k].tolist() == ids2.tolist(), (f, k)
                assert _observe(lib, a[k]) == _observe(lib, b[k]), (f, k)
                info = LC.info(lib, _capi, a[k])
                assert info.last_waits == 0 and info.last_launches == (FUSED_LAUNCHES if k == 0 else 2), (f, k, info.last_launches)
    finally:
        for h in a + b:
            lib.opd_lwt_destroy(h)


def test_fused_detection_frame_refusals(lib, det, det_frames):
    a, small_dets, small_frame = _lwt(lib), _lwt(lib, max_dets=64), _lwt(lib, max_h=97, max_w=131)
    try:
        def refused(text, trackers, frames):
            before = [_observe(lib, t) for t in trackers]
            rc, _, _ = _fused(lib, det, trackers, frames)
            assert rc == _capi.OPD_EINVAL and text in _capi.last_error(), (text, _capi.last_error())
            assert [_observe(lib, t) for t in trackers] == before, text

        det.device_nms = False
        det._sync_nms()
        refused("opd_detr_set_nms is off", [a], det_frames[:1])
        _set_nms(det, 0.4)
        refused("name the same tracker", [a, a], det_frames[:2])
        refused("max_dets = 64", [small_dets], det_frames[:1])
        refused("created for up to 97 x 131", [small_frame], det_frames[:1])
        refused("created for up to 97 x 131", [a, small_frame], det_frames[:2])   # ... before the first tracker sees anything
        assert LC.info(lib, _capi, a).n_tracks == 0
    finally:
        for h in (a, small_dets, small_frame):
            lib.opd_lwt_destroy(h)


def test_fused_new_tracks_that_do_not_fit(lib, det, det_frames):
    """max_tracks = 64 under 100 kept records.  One accepted frame (one record) first, so that there is a state and a reference frame to keep;
    then the refused one beside a tracker with room: records and counts are delivered, the refused tracker's ids are -1 and its state,
    points and reference frame are those of the twin whose per-frame update was refused, the other tracker is committed."""
    a, b = _lwt(lib, max_tracks=64), _lwt(lib, max_tracks=64)
    big, big_twin = _lwt(lib), _lwt(lib)
    try:
        _set_nms(det, 0.4)
        rc, _, ids = _fused(lib, det, [a], det_frames[:1])
        assert rc == 0 and ids[0].tolist() == [1], _capi.last_error()
        assert _two_calls(lib, det, b, det_frames[0])[0] == 0
        before = _observe(lib, a)
        _set_nms(det, 1.0)
        rc, per, ids = _fused(lib, det, [a, big], [det_frames[1], det_frames[1]])
        assert rc == _capi.OPD_EINVAL and "max_tracks = 64" in _capi.last_error(), _capi.last_error()
        assert len(per[0]) == len(per[1]) == 100 and ids[0].tolist() == [-1] * 100
        rc2, r, _ = _two_calls(lib, det, b, det_frames[1])
        assert rc2 == _capi.OPD_EINVAL and _no_frame(per[0]) == _no_frame(r)   # the per-frame update is refused there too: the case is what it claims
        assert _observe(lib, a) == before == _observe(lib, b)
        rc3, r3, ids3 = _two_calls(lib, det, big_twin, det_frames[1])
        assert rc3 == 0 and ids[1].tolist() == ids3.tolist() == list(range(1, 101)) and _observe(lib, big) == _observe(lib, big_twin)
        # the refused tracker still follows its point from the frame of the ACCEPTED call
        ra, rb = LC.device_interpolate(lib, _capi, a, det_frames[1]), LC.device_interpolate(lib, _capi, b, det_frames[1])
        assert _recs_bits(ra) == _recs_bits(rb) and _observe(lib, a) == _observe(lib, b)
    finally:
        for h in (a, b, big, big_twin):
            lib.opd_lwt_destroy(h)


def test_class_detect_and_track_hybrid_equals_detect_then_update(det, det_frames):
    _set_nms(det, 1.0)
    a, b = HipLightweightTracker(max_tracks=256), HipLightweightTracker(max_tracks=256)
    small = HipLightweightTracker(max_tracks=64)
    try:
        for f in range(2):
            got = det.detect_and_track_hybrid(det_frames[f], a)
            assert a.info().last_waits == 0   # the fused path was taken: the wait was the detector's
            want = b.update_with_detections(det_frames[f], det.detect(det_frames[f]))
            assert [(d.track_id, d.bbox, d.confidence, d.query_index) for d in got] == [(d.track_id, d.bbox, d.confidence, d.query_index) for d in want]
            assert len(got) == 100 and all(d.features is None for d in got)
        assert a.interpolate(det_frames[2]) == b.interpolate(det_frames[2])
        assert [(q.track_id, q.bbox, q.hits, q.time_since_update, q.features) for q in a.tracks] == [(q.track_id, q.bbox, q.hits, q.time_since_update, q.features) for q in b.tracks]
        _set_nms(det, 0.4)   # max_tracks below num_queries: the two calls run one after the other
        assert [d.track_id for d in det.detect_and_track_hybrid(det_frames[0], small)] == [1] and small.info().last_waits == 1
    finally:
        for t in (a, b, small):
            t.close()


# ---- 5. a run of frames of one camera: key frames and in-between frames in one call ---------------------------------------------------------
def _seq_hybrid(lib, det, t, frames, keys, capacity):
    """opd_detr_detect_sequence_hybrid: (rc, frames_done, per frame: (kept records, ids) of a key frame or the record list of an in-between frame).
    Ids beyond a key frame's kept count must stay sentinels."""
    F, K, Q = len(frames), sum(keys), det.num_queries
    recs, counts, ids = (_capi.OpdDet * (max(K, 1) * Q))(), (C.c_int32 * max(K, 1))(), np.full((max(K, 1), Q), -7, np.int32)
    lrecs, lcounts, done = (_capi.OpdLwtRec * (max(F - K, 1) * capacity))(), (C.c_int32 * max(F - K, 1))(*([-7] * max(F - K, 1))), C.c_int32(-7)
    ptrs = (C.c_void_p * F)(*[f.ctypes.data for f in frames])
    flags = (C.c_uint8 * F)(*[int(k) for k in keys])
    rc = lib.opd_detr_detect_sequence_hybrid(C.c_void_p(det.model), t, ptrs, flags, F, DH, DW, DH, DW, 0.05, PERSON, recs, counts, ids.ctypes.data,
                                             lrecs, capacity, lcounts, C.byref(done))
    raw = np.frombuffer(bytes(recs), LI.DET).reshape(max(K, 1), Q)
    out, k, j = [], 0, 0
    for f in range(F):
        if keys[f]:
            n = int(counts[k])
            assert np.all(ids[k, n:] == -7), "ids beyond the kept count were written"
            out.append((raw[k, :n].copy(), ids[k, :n].copy()))
            k += 1
        else:
            out.append([(lrecs[j * capacity + i].track_id, tuple(float(v) for v in lrecs[j * capacity + i].bbox)) for i in range(max(lcounts[j], 0))] if lcounts[j] != -7 else None)
            j += 1
    return rc, done.value, out


def _loop(lib, det, t, frames, keys):
    """The per-frame loop of the parent's calls, stopping at the first refused update: (frames applied, outputs as _seq_hybrid's, point counts)."""
    out, points = [], []
    for f, (frame, key) in enumerate(zip(frames, keys)):
        if key:
            rc, r, ids = _two_calls(lib, det, t, frame)
            if rc != 0:
                assert rc == _capi.OPD_EINVAL and "max_tracks" in _capi.last_error(), _capi.last_error()
                return f, out, points, r
            out.append((r, ids))
        else:
            out.append(LC.device_interpolate(lib, _capi, t, frame))
        points.append(LC.info(lib, _capi, t).n_points)
    return len(frames), out, points, None


def _same_outputs(got, want, keys, where):
    for f, key in enumerate(keys[:len(want)]):
        if key:
            assert _no_frame(got[f][0]) == _no_frame(want[f][0]) and got[f][1].tolist() == want[f][1].tolist(), (where, f, got[f][1].tolist(), want[f][1].tolist())
        else:
            assert _recs_bits(got[f]) == _recs_bits(want[f]), (where, f)


@pytest.mark.parametrize("nms", [0.4, 1.0])
def test_sequence_of_key_and_in_between_frames_equals_the_loop(lib, det, det_frames, nms):
    _set_nms(det, nms)
    a, b = _lwt(lib), _lwt(lib)
    keys = [True, False, False, True, False]
    try:
        rc, done, got = _seq_hybrid(lib, det, a, det_frames, keys, capacity=256)
        assert rc == 0 and done == 5, _capi.last_error()
        info = LC.info(lib, _capi, a)
        assert info.last_waits == 0 and info.last_launches == 2 * FUSED_LAUNCHES + 3 * (1 + 3 + 1 + 1), info.last_launches   # in between: gray, three levels, LK, the tracks
        applied, want, points, _ = _loop(lib, det, b, det_frames, keys)
        assert applied == 5, points
        if nms == 1.0:
            assert points[1] > 0, points   # LK really ran on the first in-between frame and followed points
        else:
            assert points[:3] == [1, 0, 0], points   # the one point is lost at once: the second in-between frame meets a device count of zero behind a key frame
        _same_outputs(got, want, keys, "five frames")
        assert _observe(lib, a) == _observe(lib, b)
        # the call left a usable reference: one more per-frame in-between frame on both
        assert _recs_bits(LC.device_interpolate(lib, _capi, a, det_frames[0])) == _recs_bits(LC.device_interpolate(lib, _capi, b, det_frames[0]))
        assert _observe(lib, a) == _observe(lib, b)
        # a run that starts with two in-between frames on a tracker that holds tracks (and, at 0.4, its one point): the first frame need not be a key frame
        run, keys2 = [det_frames[1], det_frames[2], det_frames[3], det_frames[4]], [False, False, True, False]
        rc, done, got = _seq_hybrid(lib, det, a, run, keys2, capacity=256)
        assert rc == 0 and done == 4, _capi.last_error()
        applied, want, points, _ = _loop(lib, det, b, run, keys2)
        assert applied == 4
        _same_outputs(got, want, keys2, "in-between frames first")
        assert _observe(lib, a) == _observe(lib, b)
        # K = 0 is opd_lwt_interpolate_sequence
        rc, done, got = _seq_hybrid(lib, det, a, det_frames[:3], [False] * 3, capacity=256)
        assert rc == 0 and done == 3 and LC.info(lib, _capi, a).last_waits == 1, _capi.last_error()
        ptrs = (C.c_void_p * 3)(*[f.ctypes.data for f in det_frames[:3]])
        recs, counts = (_capi.OpdLwtRec * (3 * 256))(), (C.c_int32 * 3)()
        assert lib.opd_lwt_interpolate_sequence(b, ptrs, 0, 3, DH, DW, recs, 256, counts) == 0, _capi.last_error()
        for f in range(3):
            assert _recs_bits(got[f]) == _recs_bits([(recs[f * 256 + i].track_id, tuple(float(v) for v in recs[f * 256 + i].bbox)) for i in range(counts[f])]), f
        assert _observe(lib, a) == _observe(lib, b) and LC.info(lib, _capi, a).last_launches == LC.info(lib, _capi, b).last_launches
    finally:
        for h in (a, b):
            lib.opd_lwt_destroy(h)


def test_sequence_without_optical_flow_and_its_refusals(lib, det, det_frames):
    _set_nms(det, 1.0)
    a, b = _lwt(lib, flow=False), _lwt(lib, flow=False)
    small = _lwt(lib, max_h=97, max_w=131)
    keys = [False, True, False, True]
    try:
        rc, done, got = _seq_hybrid(lib, det, a, det_frames[:4], keys, capacity=256)
        assert rc == 0 and done == 4 and LC.info(lib, _capi, a).last_launches == 2 * 2 + 2, _capi.last_error()
        applied, want, _, _ = _loop(lib, det, b, det_frames[:4], keys)
        assert applied == 4
        _same_outputs(got, want, keys, "no flow")
        assert _observe(lib, a) == _observe(lib, b)
        before = _observe(lib, a)

        def refused(text, t, frames, keys, capacity=256):
            rc, _, _ = _seq_hybrid(lib, det, t, frames, keys, capacity)
            assert rc == _capi.OPD_EINVAL and text in _capi.last_error(), (text, _capi.last_error())

        refused("max_tracks = 256", a, det_frames[:2], [True, False], capacity=255)
        refused("outside the configured maximum", a, det_frames[:3], [True, True, True])   # three key frames, max_batch = 2
        refused("created for up to 97 x 131", small, det_frames[:2], [True, False])
        det.device_nms = False
        det._sync_nms()
        refused("opd_detr_set_nms is off", a, det_frames[:2], [True, False])
        _set_nms(det, 1.0)
        assert _observe(lib, a) == before
    finally:
        for h in (a, b, small):
            lib.opd_lwt_destroy(h)


def test_sequence_whose_second_key_frame_is_refused(lib, det, det_frames):
    """max_tracks = 128 under 100 kept records, matching at IoU 0.5.  The second key frame is a WHITE image: the seeded detector's boxes on it
    overlap those of the structured frames too little at 0.5 (measured: 96 of 100 start a track), so the new tracks do not fit.  The twin's
    per-frame update of that frame is asserted to be refused, else this proves nothing.  Frame 2 changes nothing and ends the run:
    frames_done = 3, its ids and nothing else of it are delivered as -1, the in-between frame behind it has no records, and the tracker --
    state, points, reference frame -- is that of the loop that stopped."""
    _set_nms(det, 1.0)
    white = np.full((DH, DW, 3), 255, np.uint8)
    run, keys = [det_frames[0], det_frames[1], white, det_frames[2]], [True, False, True, False]
    a, b = _lwt(lib, max_tracks=128, iou=0.5), _lwt(lib, max_tracks=128, iou=0.5)
    try:
        rc, done, got = _seq_hybrid(lib, det, a, run, keys, capacity=128)
        assert rc == _capi.OPD_EINVAL and "max_tracks = 128" in _capi.last_error() and "frame 2" in _capi.last_error(), _capi.last_error()
        assert done == 3
        applied, want, points, refused_records = _loop(lib, det, b, run, keys)
        assert applied == 2 and refused_records is not None and len(refused_records) == 100   # the per-frame update of the white frame is refused there
        assert points[1] > 0                                                                  # ... and LK really ran on the in-between frame before it
        _same_outputs(got, want, keys, "the accepted frames")
        assert _no_frame(got[2][0]) == _no_frame(refused_records) and got[2][1].tolist() == [-1] * 100   # records and counts of ALL key frames are delivered
        assert got[3] == []                                                                              # a later in-between frame: no records
        assert _observe(lib, a) == _observe(lib, b)
        # the reference frame is still the last accepted frame's: both follow their points from it alike, and a later run continues alike
        assert _recs_bits(LC.device_interpolate(lib, _capi, a, det_frames[2])) == _recs_bits(LC.device_interpolate(lib, _capi, b, det_frames[2]))
        assert _observe(lib, a) == _observe(lib, b) and LC.info(lib, _capi, a).n_points > 0
        rc, done, got = _seq_hybrid(lib, det, a, [det_frames[3], det_frames[4]], [False, True], capacity=128)
        applied, want, _, _ = _loop(lib, det, b, [det_frames[3], det_frames[4]], [False, True])
        assert (rc == 0) == (applied == 2) and done == 2   # (accepted or refused at its last frame: both say 2, and both ways the twin agrees)
        _same_outputs(got, want, [False, True], "the next run")
        assert _observe(lib, a) == _observe(lib, b)
    finally:
        for h in (a, b):
            lib.opd_lwt_destroy(h)


def test_class_track_hybrid_batch_equals_the_loop(det, det_frames):
    _set_nms(det, 1.0)
    a, b = HipLightweightTracker(max_tracks=256), HipLightweightTracker(max_tracks=256)
    keys = [True, False, False, True, False]   # max_batch = 2: one native call; a sixth frame would start a second
    try:
        got = det.track_hybrid_batch(det_frames + det_frames[:2], a, keys + [True, False])   # three key frames: two native calls
        assert a.info().last_waits == 0
        want = []
        for f, k in zip(det_frames + det_frames[:2], keys + [True, False]):
            want.append(b.update_with_detections(f, det.detect(f)) if k else b.interpolate(f))
        assert len(got) == len(want) == 7
        for f, (g, w) in enumerate(zip(got, want)):
            if (keys + [True, False])[f]:
                assert [(d.track_id, d.bbox, d.confidence) for d in g] == [(d.track_id, d.bbox, d.confidence) for d in w], f
            else:
                assert g == w and len(g) > 0, f
        assert [(q.track_id, q.bbox, q.hits, q.time_since_update) for q in a.tracks] == [(q.track_id, q.bbox, q.hits, q.time_since_update) for q in b.tracks]
        with pytest.raises(ValueError, match="key flags"):
            det.track_hybrid_batch(det_frames, a, [True])
    finally:
        a.close()
        b.close()
