"""GPU tests of the fused detect + Re-ID call (-m gpu): ``opd_detr_detect_frames_reid`` and ``detect_with_features(features="reid")``.

Everything here is an equality of bits.  The device crop planner evaluates the routines the host instantiates (csrc/opd_crop.h, held
to the staged plan of opd_reid_extract by test_crop_plan_cpu.py), so its records and tables equal the host's; the crops are then read
by the unchanged pre-processing kernels and the forward is batch-independent (test_reid_gpu.py, test_osnet_gpu.py), so every row of the
fused call equals the row opd_reid_extract gives for the same frame and box on the same handle.  The standalone call takes all boxes
of a fused call at once: the same crop-count bucket, although the rows do not depend on it.

The seeded detector (threshold 0.05) labels nearly every one of its 100 queries a person on these frames (counted on the CPU oracle:
87 .. 100 per frame for the seeds used), so one frame overflows a small ``slots`` and two frames overflow 128.  The rows are
``feature_dim`` wide: 512 for OSNet, 128 for the ``tiny`` CLIP set."""

import ctypes as C
import faulthandler

import numpy as np
import pytest

import color_common as CC
import crop_plan_common as P
import reid_common as R
from office_person_detection_vit_amd import HipDetrDetector, HipOSNetReIDExtractor, HipReIDExtractor, _capi
from office_person_detection_vit_amd.frames import structured_frames
from office_person_detection_vit_amd.weights import DetrArch, ensure_clip_weight_file, ensure_osnet_weight_file, ensure_weight_file

pytestmark = pytest.mark.gpu

PERSON = 1
MAX_CROPS = 256
SENTINEL = np.float32(7.5)


@pytest.fixture(autouse=True)
def _time_limit():
    """Every test runs under its own limit: a hang ends the process (with a traceback) instead of holding the GPU."""
    faulthandler.dump_traceback_later(300, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def lib():
    return _capi.load_library(test_hooks=True)


@pytest.fixture(scope="module")
def det(weight_cache):
    path = ensure_weight_file(weight_cache, DetrArch(), 0, 1.0, "r50")
    d = HipDetrDetector(model_path=path, max_batch=2, max_size=(288, 512), resize=True, confidence_threshold=0.05)
    d.load_model()
    yield d
    d.close()


@pytest.fixture(scope="module", params=["clip", "osnet"])
def ext(request, weight_cache):
    if request.param == "clip":
        e = HipReIDExtractor(model_path=ensure_clip_weight_file(weight_cache, "tiny"), max_crops=MAX_CROPS)
    else:
        e = HipOSNetReIDExtractor(model_path=ensure_osnet_weight_file(weight_cache, "half"), max_crops=MAX_CROPS)
    e.load_model()
    yield e
    e.cleanup()


def _frames(n, h, w, seed):
    frames = [np.ascontiguousarray(f).copy() for f in structured_frames(n, h, w, seed=seed)]
    for f in frames:
        f[60:80, 100:130] = CC.UNIFORM_BGR   # (the frames of test_color_features_gpu.py, whose person counts are known)
    return frames


def _tuples(recs, counts, Q):
    return [[(r.x1, r.y1, r.x2, r.y2, r.score, r.label, r.query_index, r.frame) for r in recs[b * Q:b * Q + int(counts[b])]] for b in range(len(counts))]


def _plain(lib, det, frames, threshold=0.05):
    B, Q = len(frames), det.num_queries
    recs, counts = (_capi.OpdDet * (B * Q))(), (C.c_int32 * B)()
    ptrs = (C.c_void_p * B)(*[f.ctypes.data for f in frames])
    h, w = frames[0].shape[:2]
    _capi.check(lib.opd_detr_detect_frames(C.c_void_p(det.model), ptrs, _capi.OPD_MEM_HOST, B, h, w, 288, 512, threshold, recs, counts), "opd_detr_detect_frames")
    return _tuples(recs, counts, Q)


def _fused(lib, det, ext, frames, slots, threshold=0.05):
    """(records per frame, rows [slots][feature_dim], slot_map [slots], n_person); rows and slot_map start as sentinels."""
    B, Q = len(frames), det.num_queries
    recs, counts = (_capi.OpdDet * (B * Q))(), (C.c_int32 * B)()
    feats, slot_map, n_person = np.full((slots, ext.feature_dim), SENTINEL, np.float32), np.full(slots, -9, np.int32), C.c_int32(-9)
    ptrs = (C.c_void_p * B)(*[f.ctypes.data for f in frames])
    h, w = frames[0].shape[:2]
    _capi.check(lib.opd_detr_detect_frames_reid(C.c_void_p(det.model), ext._handle, ptrs, B, h, w, 288, 512, threshold, PERSON, slots, recs, counts,
                                                feats.ctypes.data, slot_map.ctypes.data, C.byref(n_person)), "opd_detr_detect_frames_reid")
    return _tuples(recs, counts, Q), feats, slot_map, int(n_person.value)


def _bbox(r):
    return (float(r[0]), float(r[1]), float(r[2] - r[0]), float(r[3] - r[1]))   # Detection.bbox as the shim derives it


def _check_rows(ext, frames, per_frame, feats, slot_map, n_person, slots, Q):
    """slot_map, n_person and every written row against the records and ONE standalone call on the same handle; returns the persons."""
    persons = [(b, r) for b, recs in enumerate(per_frame) for r in recs if r[5] == PERSON]   # (frame, record index) order
    assert n_person == len(persons)
    n = min(n_person, slots)
    assert list(slot_map[:n]) == [b * Q + r[6] for b, r in persons[:n]]
    assert (slot_map[n:] == -9).all() and (feats[n:] == SENTINEL).all()          # nothing is written behind the last row
    if n:
        want = ext.extract_features_batch(frames, [[_bbox(r) for b, r in persons[:n] if b == f] for f in range(len(frames))])
        assert want.shape == (n, ext.feature_dim) and np.isfinite(want).all()
        bad = np.flatnonzero((feats[:n] != want).any(axis=1))
        assert bad.size == 0, f"rows {bad[:8]} of {n} differ from opd_reid_extract, first record {persons[int(bad[0])]}"
    return persons


# ---- 1. the plan ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", P.FRAMES)
@pytest.mark.parametrize("spec", sorted(P.SPECS))
def test_device_plan_equals_host_plan(lib, spec, hw):
    """crop_plan_kernel against the host instantiation of the routines it evaluates: geometry, record, source address and the four
    tables of every box, bit for bit: up- and down-scaling, the largest tap counts, the 1-pixel-wide box, the degenerate ones, NaN."""
    H, W = hw
    boxes = np.concatenate([np.asarray(R.PIXEL_BOXES, np.float32), P.size_boxes(H, W)])
    dev = P.plan(lib, "device", spec, boxes, H, W)
    host = P.plan(lib, "host", spec, boxes, H, W)
    P.assert_same_plan(dev, host, boxes, f"{spec} {H}x{W}")
    zero = host["meta"][:, 3] == 1
    print(f"{spec} {H}x{W}: {len(boxes)} boxes, {int(zero.sum())} degenerate, taps up to {host['meta'][:, 0].max()} x {host['meta'][:, 1].max()}")
    assert zero.any() and not zero.all()


# ---- 2. fused == standalone ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(288, 512), (180, 320)])   # model resolution (crops read from the model's own input), and resized
def test_fused_call_equals_the_two_calls(lib, det, ext, hw):
    Q = det.num_queries
    total = 0
    for frame in _frames(3, hw[0], hw[1], seed=41):
        assert det._frame_list_target([frame]) == (288, 512)
        per_frame, feats, slot_map, n_person = _fused(lib, det, ext, [frame], 128)
        assert per_frame == _plain(lib, det, [frame])                      # records and counts: what opd_detr_detect_frames gives
        total += len(_check_rows(ext, [frame], per_frame, feats, slot_map, n_person, 128, Q))
        # the Python surface: the detections of the default mode, every row assigned
        dets_r, fr = det.detect_with_features(frame, features="reid", reid=ext, reid_slots=128)
        dets_e, _ = det.detect_with_features(frame)
        sig = lambda ds: [(d.query_index, d.bbox, d.confidence) for d in ds]
        assert sig(dets_r) == sig(dets_e)
        assert fr.shape == (len(dets_r), ext.feature_dim) and fr.dtype == np.float32
        row_of = {int(q): k for k, q in enumerate(slot_map[:n_person])}
        for i, d in enumerate(dets_r):
            assert np.array_equal(d.features, feats[row_of[d.query_index]]) and np.array_equal(fr[i], d.features)
    # a batch of two frames in one call: every row comes from its own frame's pixels
    pair = _frames(2, hw[0], hw[1], seed=43)
    per_frame, feats, slot_map, n_person = _fused(lib, det, ext, pair, MAX_CROPS)
    assert per_frame == _plain(lib, det, pair)
    for b in range(2):
        assert [r[:7] for r in per_frame[b]] == [r[:7] for r in _plain(lib, det, [pair[b]])[0]] and all(r[7] == b for r in per_frame[b])
    persons = _check_rows(ext, pair, per_frame, feats, slot_map, n_person, MAX_CROPS, Q)
    assert {b for b, _ in persons} == {0, 1} and n_person <= MAX_CROPS         # rows of both frames were compared
    first = next(k for k, (b, _) in enumerate(persons) if b == 1)
    swapped = ext.extract_features(pair[0], [_bbox(persons[first][1])])[0]
    assert not np.array_equal(swapped, feats[first])                           # (the other frame's pixels give another row)
    total += len(persons)
    assert total >= 2, f"the test frames give {total} person records at threshold 0.05: nothing to compare"


# ---- 3. fewer slots than persons, the other modes, the fallback ------------------------------------------------------------------------------
def test_slots_smaller_than_the_person_count(lib, det, ext):
    Q = det.num_queries
    frame = _frames(1, 180, 320, seed=41)[0]
    per_frame, feats, slot_map, n_person = _fused(lib, det, ext, [frame], 8)
    assert per_frame == _plain(lib, det, [frame])
    persons = _check_rows(ext, [frame], per_frame, feats, slot_map, n_person, 8, Q)
    assert n_person == len(persons) > 8, "the frame must overflow eight slots"
    # the Python surface still returns every row: the remainder comes from the standalone call.  The boxes of these frames overlap so
    # much that suppression keeps one detection (CPU oracle: query 21, behind the eight slots); with the IoU threshold at 1.0 nothing
    # is suppressed, and the rows come from both sources.
    before_e, fe0 = det.detect_with_features(frame)
    before_c, fc0 = det.detect_with_features(frame, features="color")
    in_slots = {int(q) for q in slot_map[:8]}
    sig = lambda ds: [(d.query_index, d.bbox, d.confidence) for d in ds]
    nms = det.nms_threshold
    try:
        for thr, least in ((nms, 1), (1.0, 9)):
            det.nms_threshold = thr
            dets, rows = det.detect_with_features(frame, features="reid", reid=ext, reid_slots=8)
            plain = det.detect(frame)
            want = ext.extract_features(frame, [d.bbox for d in plain])
            assert sig(dets) == sig(plain) and len(dets) >= least
            assert rows.dtype == np.float32 and rows.shape == want.shape == (len(dets), ext.feature_dim) and np.array_equal(rows, want)
            assert all(np.array_equal(d.features, rows[i]) for i, d in enumerate(dets))
            assert any(d.query_index not in in_slots for d in dets), "no kept detection lies behind the slots: the remainder path did not run"
        assert any(d.query_index in in_slots for d in dets)
        # a frame that cannot go down as a host frame list (not contiguous): detect + extract_features
        view = np.concatenate([frame, frame], axis=1)[:, :frame.shape[1]]
        assert not view.flags.c_contiguous and det._frame_list_target([view]) is None
        dets_v, rows_v = det.detect_with_features(view, features="reid", reid=ext, reid_slots=8)
        plain_v = det.detect(view)
        assert sig(dets_v) == sig(plain_v) and len(dets_v) >= 9
        assert np.array_equal(rows_v, ext.extract_features(view, [d.bbox for d in plain_v]))
    finally:
        det.nms_threshold = nms
    # the other feature modes are what they were
    after_e, fe1 = det.detect_with_features(frame, features="encoder")
    after_c, fc1 = det.detect_with_features(frame, features="color")
    assert sig(before_e) == sig(after_e) and sig(before_c) == sig(after_c)
    assert np.array_equal(np.asarray(fe0), np.asarray(fe1)) and np.array_equal(np.asarray(fc0), np.asarray(fc1))
    assert all(np.array_equal(a.features, b.features) for a, b in zip(before_e, after_e))
    assert all(np.array_equal(a.features, b.features) for a, b in zip(before_c, after_c))
    with pytest.raises(ValueError, match="needs reid="):
        det.detect_with_features(frame, features="reid")
    with pytest.raises(ValueError, match="features must be"):
        det.detect_with_features(frame, features="hog", reid=ext)


def test_no_record_above_the_threshold(lib, det, ext):
    frame = _frames(1, 180, 320, seed=41)[0]
    per_frame, feats, slot_map, n_person = _fused(lib, det, ext, [frame], 16, threshold=0.99)
    assert per_frame == [[]] == _plain(lib, det, [frame], threshold=0.99)
    assert n_person == 0 and (feats == SENTINEL).all() and (slot_map == -9).all()
    # and the handle is as good as before: the next call's rows are right
    per_frame, feats, slot_map, n_person = _fused(lib, det, ext, [frame], 16)
    assert len(_check_rows(ext, [frame], per_frame, feats, slot_map, n_person, 16, det.num_queries)) >= 2


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals(lib, det, ext):
    Q = det.num_queries
    frame = _frames(1, 96, 160, seed=5)[0]
    ptrs = (C.c_void_p * 2)(frame.ctypes.data, frame.ctypes.data)
    recs, counts = (_capi.OpdDet * (3 * Q))(), (C.c_int32 * 3)()
    feats, slot_map, n_person = np.full((8, ext.feature_dim), SENTINEL, np.float32), np.full(8, -9, np.int32), C.c_int32(-9)

    def call(m=det.model, r=ext._handle, frames=ptrs, B=1, h=96, w=160, H=288, W=512, slots=8, out=recs, cnt=counts, f=feats, sm=slot_map, n=n_person):
        return lib.opd_detr_detect_frames_reid(C.c_void_p(m) if m else None, r, frames, B, h, w, H, W, 0.5, PERSON, slots, out, cnt,
                                               f.ctypes.data if f is not None else None, sm.ctypes.data if sm is not None else None,
                                               C.byref(n) if n is not None else None)

    assert call() == _capi.OPD_OK
    for kwargs, text in (
            (dict(m=None), "null model handle"),
            (dict(r=None), "null Re-ID handle"),
            (dict(out=None), "null output buffer"),
            (dict(cnt=None), "null output buffer"),
            (dict(f=None), "null output buffer"),
            (dict(sm=None), "null output buffer"),
            (dict(n=None), "null output buffer"),
            (dict(frames=(C.c_void_p * 1)(None)), "null frame pointer"),
            (dict(slots=0), "outside 1 .. max_crops"),
            (dict(slots=-1), "outside 1 .. max_crops"),
            (dict(slots=MAX_CROPS + 1), "outside 1 .. max_crops"),
            (dict(B=3), "outside the configured maximum"),
            (dict(B=0), "outside the configured maximum"),
            (dict(H=320, W=512), "outside the configured maximum"),
            (dict(H=288, W=16), "outside the configured maximum"),
            (dict(h=0), "source frame size"),
            (dict(w=-4), "source frame size")):
        n_person.value = -9
        assert call(**kwargs) == _capi.OPD_EINVAL, kwargs
        assert text in _capi.last_error(), (kwargs, _capi.last_error())
        assert n_person.value == -9 and (feats[-1] == SENTINEL).all()
    assert call() == _capi.OPD_OK                                        # a refusal leaves both handles usable


# ---- 5. one Re-ID handle, two threads ---------------------------------------------------------------------------------------------------------
def test_two_threads_on_one_reid_handle_take_turns(lib, det, weight_cache):
    """The fused call on one thread and opd_reid_extract on another, on ONE fresh Re-ID handle (so that both also capture their graphs
    while the other runs): each call waits for the other to finish, and every result is what the same call gives alone."""
    import threading
    frame = _frames(1, 180, 320, seed=41)[0]
    boxes = [_bbox(r) for r in _plain(lib, det, [frame])[0] if r[5] == PERSON][20:25]
    one = HipOSNetReIDExtractor(model_path=ensure_osnet_weight_file(weight_cache, "half"), max_crops=32)
    ref = HipOSNetReIDExtractor(model_path=ensure_osnet_weight_file(weight_cache, "half"), max_crops=32)
    one.load_model()
    ref.load_model()
    try:
        want_fused = _fused(lib, det, ref, [frame], 16)
        want_rows = ref.extract_features(frame, boxes)
        got, errors = {"fused": [], "rows": []}, []

        def run(key, call):
            try:
                for _ in range(6):
                    got[key].append(call())
            except Exception as e:   # (reported below, on the main thread)
                errors.append(e)

        threads = [threading.Thread(target=run, args=("fused", lambda: _fused(lib, det, one, [frame], 16))),
                   threading.Thread(target=run, args=("rows", lambda: one.extract_features(frame, boxes)))]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors, errors
        assert len(got["fused"]) == len(got["rows"]) == 6
        for per_frame, feats, slot_map, n_person in got["fused"]:
            assert per_frame == want_fused[0] and n_person == want_fused[3]
            assert np.array_equal(feats, want_fused[1]) and np.array_equal(slot_map, want_fused[2])
        for rows in got["rows"]:
            assert np.array_equal(rows, want_rows)
    finally:
        one.cleanup()
        ref.cleanup()
