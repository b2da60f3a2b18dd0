"""GPU tests of the fused detect-and-track call (-m gpu): ``opd_detr_detect_frames_track`` and ``HipDetrDetector.detect_and_track``.

Everything here is an equality of bits.  The ingest launch writes the float32 numbers the Python path hands to ``opd_track_update``
(tests/track_ingest_common.py, held to that path by test_detect_track_cpu.py), the predict / cost launch is the same kernel on the same
staging image, and the association is the same host routine on the same matrices: a tracker that takes the fused call and a twin that takes
the feature call followed by ``opd_track_update`` must agree in every id and every state bit, ties included.  Where they do not, the
failure shows the cost matrices of both.

The seeded detector (threshold 0.05) labels all 100 queries a person on these frames, with scores between 0.30 and 0.67 and boxes that
overlap heavily and hardly move from frame to frame (counted on the device): suppression at 0.4 keeps ONE record a frame, at 1.0 all 100,
so the two thresholds give a 1 x 1 and a 100 x 100 association.  ``high_conf_threshold`` = 0.5 lies inside the score range: both the
high- and the low-confidence stages of the association see records.  Re-ID slots can lie below the kept count only where more than
one record is kept, so that frame is demanded at 1.0 alone."""

import ctypes as C
import faulthandler

import numpy as np
import pytest

import color_common as CC
import track_common as TC
import track_ingest_common as TI
from office_person_detection_vit_amd import HipDetrDetector, HipOSNetReIDExtractor, HipReIDExtractor, HipTracker, _capi
from office_person_detection_vit_amd.frames import structured_frames
from office_person_detection_vit_amd.weights import DetrArch, ensure_clip_weight_file, ensure_osnet_weight_file, ensure_weight_file

pytestmark = pytest.mark.gpu

PERSON = 1
NONE, ENCODER, COLOR, REID = _capi.OPD_TRACK_FEAT_NONE, _capi.OPD_TRACK_FEAT_ENCODER, _capi.OPD_TRACK_FEAT_COLOR, _capi.OPD_TRACK_FEAT_REID
TRACKER = dict(max_tracks=128, max_dets=128, min_hits=1, high_conf_threshold=0.5)
ABOVE_EVERY_SCORE = 1.5
H, W = 288, 512


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
    d = HipDetrDetector(model_path=path, max_batch=2, max_size=(H, W), resize=True, confidence_threshold=0.05, device_nms=True)
    d.load_model()
    yield d
    d.close()


@pytest.fixture(scope="module")
def exts(weight_cache):
    made = {}

    def get(name):
        if name not in made:
            e = (HipReIDExtractor(model_path=ensure_clip_weight_file(weight_cache, "tiny"), max_crops=64) if name == "clip"
                 else HipOSNetReIDExtractor(model_path=ensure_osnet_weight_file(weight_cache, "half"), max_crops=64))
            e.load_model()
            made[name] = e
        return made[name]

    yield get
    for e in made.values():
        e.cleanup()


@pytest.fixture(scope="module")
def frames():
    out = [np.ascontiguousarray(f).copy() for f in structured_frames(5, H, W, seed=3)]
    for f in out:
        f[60:80, 100:130] = CC.UNIFORM_BGR
    return out


def _set_nms(det, thr):
    det.device_nms, det.nms_threshold = True, thr
    det._sync_nms()


def _dim(det, kind, ext):
    return {NONE: 64, ENCODER: 256, COLOR: 256, REID: ext.feature_dim if ext is not None else 0}[kind]


def _recs_of(recs, counts, Q):
    """Per frame: the kept records as a TI.DET array."""
    raw = np.frombuffer(bytes(recs), TI.DET).reshape(len(counts), Q)
    return [raw[b, :int(counts[b])].copy() for b in range(len(counts))]


def _fused(lib, det, trackers, frames, kind, ext=None, slots=0, threshold=0.05):
    """(rc, records per frame, ids per frame, n_featured); ids start as sentinels and must stay so beyond the kept count."""
    B, Q = len(frames), det.num_queries
    recs, counts = (_capi.OpdDet * (B * Q))(), (C.c_int32 * B)()
    ids, nf = np.full((B, Q), -7, np.int32), np.full(B, -7, np.int32)
    ptrs = (C.c_void_p * B)(*[f.ctypes.data for f in frames])
    hs = (C.c_void_p * B)(*[t.value for t in trackers])
    rc = lib.opd_detr_detect_frames_track(C.c_void_p(det.model), ext._handle if ext is not None else None, hs, ptrs, B, H, W, H, W, threshold, PERSON, kind, slots,
                                          recs, counts, ids.ctypes.data, nf.ctypes.data)
    per = _recs_of(recs, counts, Q)
    for b in range(B):
        assert np.all(ids[b, len(per[b]):] == -7), "ids beyond the kept count were written"
    return rc, per, [ids[b, :len(per[b])].copy() for b in range(B)], nf


def _two_calls(lib, det, tracker, frame, kind, ext=None, slots=0, threshold=0.05):
    """The feature call of `kind` on one frame, then opd_track_update with the rows it returned: (rc, records, ids, number of rows)."""
    Q = det.num_queries
    recs, counts = (_capi.OpdDet * Q)(), (C.c_int32 * 1)()
    ptrs = (C.c_void_p * 1)(frame.ctypes.data)
    m = C.c_void_p(det.model)
    feats = has = None
    if kind == NONE:
        _capi.check(lib.opd_detr_detect_frames(m, ptrs, _capi.OPD_MEM_HOST, 1, H, W, H, W, threshold, recs, counts), "opd_detr_detect_frames")
        r = _recs_of(recs, counts, Q)[0]
    elif kind in (ENCODER, COLOR):
        name = "opd_detr_detect_frames_color" if kind == COLOR else "opd_detr_detect_frames_features"
        rows = np.zeros((1, Q, 256), np.float32)
        _capi.check(getattr(lib, name)(m, ptrs, 1, H, W, H, W, threshold, PERSON, recs, counts, rows.ctypes.data_as(C.POINTER(C.c_float))), name)
        r = _recs_of(recs, counts, Q)[0]
        feats, has = rows[0, r["query_index"]].reshape(len(r), 256), np.ones(len(r), np.uint8)
    else:
        E = ext.feature_dim
        rows, slot_map, n_person = np.zeros((slots, E), np.float32), np.full(slots, -9, np.int32), C.c_int32(-9)
        _capi.check(lib.opd_detr_detect_frames_reid(m, ext._handle, ptrs, 1, H, W, H, W, threshold, PERSON, slots, recs, counts, rows.ctypes.data,
                                                    slot_map.ctypes.data, C.byref(n_person)), "opd_detr_detect_frames_reid")
        r = _recs_of(recs, counts, Q)[0]
        row_of = {int(q): k for k, q in enumerate(slot_map[:min(n_person.value, slots)])}
        feats, has = np.zeros((len(r), E), np.float32), np.zeros(len(r), np.uint8)
        for i, q in enumerate(r["query_index"].tolist()):
            if q in row_of:
                feats[i], has[i] = rows[row_of[q]], 1
    boxes, foot = TI.pack(r)
    rc, ids = TC.device_update(lib, _capi, tracker, boxes, foot, r["score"], feats, has)
    return rc, r, ids, 0 if has is None else int(has.sum())


def _info(lib, h):
    info = _capi.OpdTrackStatus()
    _capi.check(lib.opd_track_info(h, C.byref(info)), "opd_track_info")
    return info


def _state(lib, h):
    recs = TC.device_tracks(lib, _capi, h)
    info = _info(lib, h)
    return b"".join(bytes(r) for r in recs), info.n_tracks, info.next_id


def _assert_twins(lib, a, b, ids_a, ids_b, where):
    if ids_a.tolist() != ids_b.tolist() or _state(lib, a) != _state(lib, b):
        ma, mb = TC.device_matrices(lib, _capi, a), TC.device_matrices(lib, _capi, b)
        names = ("app", "iou", "comb")
        diff = [(n, x.shape, y.shape, np.argwhere(x.view(np.uint32) != y.view(np.uint32))[:8].tolist() if x.shape == y.shape else "shapes differ")
                for n, x, y in zip(names, ma, mb)]
        raise AssertionError((where, "ids", ids_a.tolist(), ids_b.tolist(), "matrices (name, shapes, first differing entries)", diff,
                              [m[:4, :8] for m in ma], [m[:4, :8] for m in mb]))


def _assert_launches(lib, h, T_before, ids, where):
    info = _info(lib, h)
    want = 1 + (1 if T_before > 0 else 0) + (1 if (np.asarray(ids) >= 0).any() else 0)
    assert info.last_waits == 0 and 1 <= info.last_launches <= 3 and info.last_launches == want, (where, info.last_launches, want, info.last_waits)


# ---- the ingest launch alone ----------------------------------------------------------------------------------------------------------
def _run_ingest(lib, records, n, Q, D, frame, kind, rows, slot_map, n_person, slots):
    boxes, foot, has, feat = np.full((Q, 4), 7.5, np.float32), np.full((Q, 2), 7.5, np.float32), np.full(Q, 9, np.uint8), np.full((Q, D), 7.5, np.float32)
    want = [a.copy() for a in (boxes, foot, has, feat)]
    n_want = TI.ingest(records, n, Q, D, frame, kind, rows, slot_map, n_person, slots, *want)
    n_out = np.full(1, -7, np.int32)
    p = TC.ptr
    rc = lib.opd_track_test_ingest(0, p(records), n, Q, D, frame, kind, p(rows), 0 if rows is None else len(rows), p(slot_map), n_person, slots, Q,
                                   p(boxes), p(foot), p(has), p(feat), p(n_out))
    assert rc == 0, _capi.last_error()
    assert int(n_out[0]) == n_want
    for name, got, w in zip(("boxes", "foot", "has", "feat"), (boxes, foot, has, feat), want):
        assert got.tobytes() == w.tobytes(), (name, n, D, kind, np.argwhere(got != w)[:8].tolist())


@pytest.mark.parametrize("D", [1, 128, 256, 512])
@pytest.mark.parametrize("n", [0, 1, 100])
def test_ingest_alone_equals_the_restatement(lib, n, D):
    Q = 100
    base = TI.hard_records()
    records = np.zeros(Q, TI.DET)
    records[:len(base)] = base
    records[len(base):] = base[:Q - len(base)]
    records["query_index"] = np.random.default_rng(5).permutation(Q).astype(np.int32)
    rows = np.random.default_rng(n * 1000 + D).standard_normal((2 * Q, D)).astype(np.float32)
    _run_ingest(lib, records, n, Q, D, 0, TI.ROWS_NONE, None, None, 0, 0)
    for frame in (0, 1):
        _run_ingest(lib, records, n, Q, D, frame, TI.ROWS_BY_QUERY, rows, None, 0, 0)
    q = records["query_index"]
    every = (Q + q).astype(np.int32)                          # frame 1: a slot for every record
    some = np.ascontiguousarray(every[::3][:20])              # ... for every third of the first sixty
    other = (q + 0).astype(np.int32)                          # slots of frame 0 only: none for frame 1
    for slot_map, n_person in ((every, Q), (some, 77), (other, Q), (every, 0), (every, 5)):
        _run_ingest(lib, records, n, Q, D, 1, TI.ROWS_BY_SLOT, rows, slot_map, n_person, len(slot_map))


# ---- equality with the two-call path ---------------------------------------------------------------------------------------------------
CASES = [(NONE, None), (ENCODER, None), (COLOR, None), (REID, "clip"), (REID, "osnet")]


@pytest.mark.parametrize("nms", [0.4, 1.0])
@pytest.mark.parametrize("kind,model", CASES, ids=["none", "encoder", "color", "reid-clip", "reid-osnet"])
def test_fused_call_equals_the_two_calls(lib, det, exts, frames, kind, model, nms):
    ext = exts(model) if model else None
    slots = 16 if kind == REID else 0
    _set_nms(det, nms)
    D = _dim(det, kind, ext)
    a, b = TC.create(lib, _capi, D, **TRACKER), TC.create(lib, _capi, D, **TRACKER)
    try:
        saw_empty = saw_overflowing_slots = saw_three = False
        for f, frame in enumerate(frames):
            threshold = ABOVE_EVERY_SCORE if f == 2 else 0.05
            T = _info(lib, a).n_tracks
            assert (f == 0) == (T == 0), "the first frame, and only it, meets no track"
            rc, per, ids, nf = _fused(lib, det, [a], [frame], kind, ext, slots, threshold)
            assert rc == 0, _capi.last_error()
            rc2, r2, ids2, n_rows = _two_calls(lib, det, b, frame, kind, ext, slots, threshold)
            assert rc2 == 0, _capi.last_error()
            assert per[0].tobytes() == r2.tobytes(), (f, "records")
            assert int(nf[0]) == n_rows == {NONE: 0, ENCODER: len(r2), COLOR: len(r2), REID: min(len(r2), slots)}[kind], (f, nf, n_rows)
            _assert_twins(lib, a, b, ids[0], ids2, (kind, model, nms, f))
            _assert_launches(lib, a, T, ids[0], f)
            if f == 2:
                assert len(r2) == 0 and _info(lib, a).last_launches == 2   # ingest and predict: tracks age, nothing to commit
                saw_empty = True
            saw_overflowing_slots |= kind == REID and len(r2) > slots
            print(f"{kind} {model} nms {nms} frame {f}: {T} tracks before, {len(r2)} kept, {n_rows} rows, {int((ids[0] >= 0).sum())} ids, {_info(lib, a).n_tracks} tracks after")
            saw_three |= _info(lib, a).last_launches == 3
        assert saw_empty and saw_three and (kind != REID or nms < 1.0 or saw_overflowing_slots)
        assert _info(lib, a).n_tracks > 0
    finally:
        lib.opd_track_destroy(a)
        lib.opd_track_destroy(b)


def test_two_frames_two_trackers(lib, det, frames):
    _set_nms(det, 0.4)
    pair, single = [TC.create(lib, _capi, 256, **TRACKER) for _ in range(2)], [TC.create(lib, _capi, 256, **TRACKER) for _ in range(2)]
    try:
        for f in range(3):
            two = [frames[f], frames[4 - f]]
            T = [_info(lib, h).n_tracks for h in pair]
            rc, per, ids, nf = _fused(lib, det, pair, two, COLOR)
            assert rc == 0, _capi.last_error()
            for b in range(2):
                rc1, per1, ids1, nf1 = _fused(lib, det, [single[b]], [two[b]], COLOR)
                assert rc1 == 0, _capi.last_error()
                got, want = per[b].copy(), per1[0].copy()
                assert got["frame"].tolist() == [b] * len(got)
                got["frame"] = 0
                assert got.tobytes() == want.tobytes(), (f, b, "records")
                assert int(nf[b]) == int(nf1[0]) == len(want)
                _assert_twins(lib, pair[b], single[b], ids[b], ids1[0], (f, b))
                _assert_launches(lib, pair[b], T[b], ids[b], (f, b))
    finally:
        for h in pair + single:
            lib.opd_track_destroy(h)


def test_fused_and_standalone_updates_interleave(lib, det, frames):
    _set_nms(det, 0.4)
    a, b = TC.create(lib, _capi, 256, **TRACKER), TC.create(lib, _capi, 256, **TRACKER)
    try:
        for f in range(4):
            if f % 2 == 0:
                rc, per, ids, _ = _fused(lib, det, [a], [frames[f]], ENCODER)
                ids_a = ids[0]
            else:
                rc, _, ids_a, _ = _two_calls(lib, det, a, frames[f], ENCODER)
                assert _info(lib, a).last_waits == 1
            assert rc == 0, _capi.last_error()
            rc2, _, ids_b, _ = _two_calls(lib, det, b, frames[f], ENCODER)
            assert rc2 == 0, _capi.last_error()
            _assert_twins(lib, a, b, ids_a, ids_b, f)
    finally:
        lib.opd_track_destroy(a)
        lib.opd_track_destroy(b)


def test_a_tracker_out_of_slots(lib, det, frames):
    _set_nms(det, 1.0)
    small = dict(TRACKER, max_tracks=4, high_conf_threshold=0.06)   # (every record may start a track)
    a, b, other = TC.create(lib, _capi, 256, **small), TC.create(lib, _capi, 256, **small), TC.create(lib, _capi, 256, **TRACKER)
    try:
        rc, per, ids, nf = _fused(lib, det, [a, other], [frames[0], frames[1]], COLOR)
        assert rc == _capi.OPD_EINVAL and "exceed max_tracks = 4" in _capi.last_error() and "counted as one without detections" in _capi.last_error()
        assert len(per[0]) > 4 and int(nf[0]) == len(per[0]) and ids[0].tolist() == [-1] * len(per[0])
        assert (ids[1] >= 0).any() and _info(lib, other).n_tracks > 0, "the other tracker of the batch was not committed"
        rc2, r2, ids2, _ = _two_calls(lib, det, b, frames[0], COLOR)
        assert rc2 == _capi.OPD_EINVAL and "exceed max_tracks = 4" in _capi.last_error()
        assert per[0].tobytes() == r2.tobytes()
        _assert_twins(lib, a, b, ids[0], ids2, "overflow")
        # the same frame again, above all but its four best scores: at most four records, which fit
        threshold = float(np.sort(r2["score"])[-4]) - 1e-7
        rc, per, ids, nf = _fused(lib, det, [a], [frames[0]], COLOR, threshold=threshold)
        assert rc == 0, _capi.last_error()
        rc2, r2, ids2, _ = _two_calls(lib, det, b, frames[0], COLOR, threshold=threshold)
        assert rc2 == 0, _capi.last_error()
        assert 1 <= len(r2) <= 4 and per[0].tobytes() == r2.tobytes() and (ids[0] >= 0).all()
        _assert_twins(lib, a, b, ids[0], ids2, "after the overflow")
    finally:
        for h in (a, b, other):
            lib.opd_track_destroy(h)


def test_refusals_that_read_a_handle(lib, det, exts, frames):
    ext = exts("clip")
    Q = det.num_queries
    good = TC.create(lib, _capi, 256, **TRACKER)
    narrow = TC.create(lib, _capi, 256, **dict(TRACKER, max_dets=Q - 1))
    wide = TC.create(lib, _capi, 512, **TRACKER)
    try:
        def refused(text, trackers=None, two=False, kind=COLOR, e=None, slots=0, label=PERSON):
            fr = [frames[0], frames[1]] if two else [frames[0]]
            before = _state(lib, good)
            B = len(fr)
            recs, counts = (_capi.OpdDet * (B * Q))(), (C.c_int32 * B)()
            ids, nf = np.full((B, Q), -7, np.int32), np.full(B, -7, np.int32)
            ptrs = (C.c_void_p * B)(*[f.ctypes.data for f in fr])
            hs = (C.c_void_p * B)(*[t.value if t is not None else None for t in (trackers or [good])])
            rc = lib.opd_detr_detect_frames_track(C.c_void_p(det.model), e._handle if e is not None else None, hs, ptrs, B, H, W, H, W, 0.05, label, kind, slots,
                                                  recs, counts, ids.ctypes.data, nf.ctypes.data)
            assert rc == _capi.OPD_EINVAL and text in _capi.last_error(), (text, _capi.last_error())
            assert np.all(ids == -7) and _state(lib, good) == before

        _set_nms(det, 0.4)
        refused("label 1, the call asks for label 2", label=2)
        refused("null tracker handle", trackers=[None])
        refused("name the same tracker", trackers=[good, good], two=True)
        refused("max_dets = %d" % (Q - 1), trackers=[narrow])
        refused("feature_dim = 512", trackers=[wide])
        refused("feature_dim = 256", kind=REID, e=ext, slots=8)   # (the tiny CLIP set has 128 numbers a row)
        refused("slots = 0 outside 1 .. max_crops", kind=REID, e=ext, slots=0, trackers=[good])
        refused("slots = 65 outside 1 .. max_crops", kind=REID, e=ext, slots=65)
        det.device_nms = False
        det._sync_nms()
        refused("opd_detr_set_nms is off")
        # nothing above left a mark: the handle still tracks
        _set_nms(det, 0.4)
        rc, per, ids, nf = _fused(lib, det, [good], [frames[0]], COLOR)
        assert rc == 0 and len(per[0]) > 0 and (ids[0] >= 0).any(), _capi.last_error()
    finally:
        for h in (good, narrow, wide):
            lib.opd_track_destroy(h)


# ---- the Python surface ------------------------------------------------------------------------------------------------------------------
def _mirror(tracker):
    return [(t.track_id, t.age, t.hits, t.time_since_update, list(t.trajectory), t.get_state()) for t in tracker.get_confirmed_tracks()]


@pytest.mark.parametrize("features", ["color", None])
@pytest.mark.parametrize("device_nms", [True, False])
def test_detect_and_track_equals_detect_then_update(det, frames, features, device_nms):
    det.device_nms, det.nms_threshold = device_nms, 0.4
    D = 256 if features else 64
    a, b = (HipTracker(feature_dim=D, max_tracks=128, max_dets=128, min_hits=1) for _ in range(2))
    try:
        for f, frame in enumerate(frames[:4]):
            got = det.detect_and_track(frame, a, features=features)
            dets = det.detect_with_features(frame, features=features)[0] if features else det.detect(frame)
            want = b.update(dets)
            assert all(d.features is None for d in got) or not device_nms
            assert [(d.track_id, d.bbox, d.confidence, d.query_index) for d in got] == [(d.track_id, d.bbox, d.confidence, d.query_index) for d in want], f
            assert len(got) > 0 and _mirror(a) == _mirror(b) and a.next_id == b.next_id, f
            info = _capi.OpdTrackStatus()
            _capi.check(a._lib.opd_track_info(a._h, C.byref(info)), "opd_track_info")
            assert info.last_waits == (0 if device_nms else 1), "the fused call was not taken" if device_nms else "the fallback was not taken"
    finally:
        a.close()
        b.close()
        det.device_nms = True
