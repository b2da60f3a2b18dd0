"""GPU tests of the sequence calls (-m gpu): ``track_assoc_kernel`` alone, ``opd_track_update_sequence``, ``opd_detr_detect_sequence_track``,
``HipTracker.update_sequence`` and ``HipDetrDetector.detect_and_track_batch``.

Everything here is an equality.  The association kernel is the host's ``associate()`` pair for pair (the same stages, the same solver picking
the same column at every step, ties included), the predict / cost and commit launches are the per-frame ones reading their sizes from the
device table, so a tracker that takes a run of frames in one call and a twin that takes them one call per frame must agree in every id,
every counter and every state bit."""

import ctypes as C
import faulthandler

import numpy as np
import pytest
import torch

import color_common as CC
import track_common as TC
import track_ingest_common as TI
from office_person_detection_vit_amd import HipDetrDetector, HipReIDExtractor, HipTracker, _capi
from office_person_detection_vit_amd.data_models import Detection
from office_person_detection_vit_amd.frames import structured_frames
from office_person_detection_vit_amd.weights import DetrArch, ensure_clip_weight_file, ensure_weight_file

pytestmark = pytest.mark.gpu

F32 = np.float32
PERSON = 1
NONE, ENCODER, COLOR, REID = _capi.OPD_TRACK_FEAT_NONE, _capi.OPD_TRACK_FEAT_ENCODER, _capi.OPD_TRACK_FEAT_COLOR, _capi.OPD_TRACK_FEAT_REID
TRACKER = dict(max_tracks=128, max_dets=128, min_hits=1, high_conf_threshold=0.5)
H, W = 288, 512
B = 5


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
def golden():
    return np.load(TC.GOLDEN)


def _info(lib, h):
    info = _capi.OpdTrackStatus()
    _capi.check(lib.opd_track_info(h, C.byref(info)), "opd_track_info")
    return info


def _state(lib, h):
    recs = TC.device_tracks(lib, _capi, h)
    info = _info(lib, h)
    return b"".join(bytes(r) for r in recs), info.n_tracks, info.next_id


# ---- the association kernel alone ------------------------------------------------------------------------------------------------------
def _assoc(lib, app, iou, comb, hits, conf, min_hits, high_conf, n_free):
    """(kernel, host): each (matches [(track, detection)] in order, new detections, unmatched tracks)."""
    T, N = len(hits), len(conf)
    app, iou, comb = (np.ascontiguousarray(m, F32).reshape(T, N) for m in (app, iou, comb))
    hits, conf = np.ascontiguousarray(hits, np.int32), np.ascontiguousarray(conf, F32)
    sides = []
    for _ in range(2):
        sides.append([np.full((max(min(T, N), 1), 2), -7, np.int32), np.full(1, -7, np.int32), np.full(max(N, 1), -7, np.int32), np.full(1, -7, np.int32),
                      np.full(max(T, 1), -7, np.int32), np.full(1, -7, np.int32)])
    rc = lib.opd_track_test_assoc(0, TC.ptr(app), TC.ptr(iou), TC.ptr(comb), T, N, TC.ptr(hits), TC.ptr(conf), min_hits, high_conf, n_free,
                                  *[TC.ptr(a) for side in sides for a in side])
    assert rc == 0, _capi.last_error()
    return tuple(([tuple(p) for p in m[:nm[0]].tolist()], new[:nn[0]].tolist(), un[:nu[0]].tolist()) for m, nm, new, nn, un, nu in sides)


def _draw(kind, T, N, rng):
    if kind == "ties":
        mats = [rng.choice(np.array([0.25, 0.5, 1.0], F32), size=(T, N)) for _ in range(3)]
    else:
        mats = [rng.random((T, N), dtype=F32) for _ in range(3)]
    if kind == "nonfinite":
        for m in mats:
            r = rng.random((T, N))
            m[r < 0.1] = np.nan
            m[(r >= 0.1) & (r < 0.2)] = np.inf
    hits = rng.integers(0, 6, T).astype(np.int32)                 # either side of min_hits = 3
    conf = rng.uniform(0.2, 0.9, N).astype(F32)                   # either side of high_conf = 0.5
    if N:
        conf[rng.integers(0, N)] = 0.5                            # ... and one exactly on it
    return mats, hits, conf


# across the 64-lane boundary in both orientations; the last two take the solver's instantiations for up to 256 and for more columns
SHAPES = [(1, 1), (1, 5), (5, 1), (7, 7), (3, 64), (64, 65), (65, 64), (130, 70), (3, 300), (300, 2)]


@pytest.mark.parametrize("kind", ["uniform", "ties", "nonfinite", "no_free_slots"])
def test_association_kernel_equals_the_host(lib, kind):
    rng = np.random.default_rng({"uniform": 1, "ties": 2, "nonfinite": 3, "no_free_slots": 4}[kind])
    matched = created = dropped = 0
    for T, N in SHAPES:
        for rep in range(3 if T * N <= 64 * 65 else 1):
            mats, hits, conf = _draw(kind, T, N, rng)
            n_free = 0 if kind == "no_free_slots" else N
            got, want = _assoc(lib, *mats, hits, conf, 3, 0.5, n_free)
            assert got == want, (kind, T, N, rep, [(a, b) for a, b in zip(got[0], want[0]) if a != b][:4], got[1][:8], want[1][:8], got[2][:8], want[2][:8])
            matched += len(want[0])
            created += len(want[1])
            dropped += kind == "no_free_slots" and want[0] == [] and len(want[2]) < T
    assert matched > 0 and (created > 0 or kind == "no_free_slots") and (dropped > 0 or kind != "no_free_slots")


def test_association_kernel_without_tracks_or_detections(lib):
    rng = np.random.default_rng(5)
    for T, N in ((0, 5), (0, 70), (5, 0), (70, 0), (0, 0)):
        mats, hits, conf = _draw("uniform", T, N, rng)
        got, want = _assoc(lib, *mats, hits, conf, 3, 0.5, 128 - T)
        assert got == want, (T, N, got, want)
        assert want[0] == [] and want[2] == list(range(T)) and want[1] == [j for j in range(N) if conf[j] >= 0.5]
    mats, hits, conf = _draw("uniform", 0, 5, rng)
    got, want = _assoc(lib, *mats, hits, np.full(5, 0.9, F32), 3, 0.5, 4)   # five new tracks, four slots
    assert got == want == ([], [], [])


# ---- opd_track_update_sequence against the per-frame loop -------------------------------------------------------------------------------
def _pack(frames):
    """frames of TC.sequence -> the packed arrays of opd_track_update_sequence."""
    counts = np.array([len(fr[2]) for fr in frames], np.int32)
    cat = lambda k, tail: np.ascontiguousarray(np.concatenate([np.asarray(fr[k], F32).reshape((-1,) + tail) for fr in frames]))   # noqa: E731
    use = frames[0][3] is not None
    feats = cat(3, (np.asarray(frames[0][3]).shape[1],)) if use else None
    has = np.ascontiguousarray(np.concatenate([np.asarray(fr[4], np.uint8) for fr in frames])) if use else None
    return cat(0, (4,)), cat(1, (2,)), cat(2, ()), feats, has, counts


def _sequence(lib, h, frames, feat_ptr=None):
    """(rc, ids per frame, frames_done); ids start as sentinels."""
    boxes, foot, conf, feats, has, counts = _pack(frames)
    ids, done = np.full(max(int(counts.sum()), 1), -7, np.int32), np.full(1, -7, np.int32)
    if feat_ptr is not None:
        rc = lib.opd_track_update_sequence(h, TC.ptr(boxes), TC.ptr(foot), TC.ptr(conf), C.c_void_p(feat_ptr), TC.ptr(has), _capi.OPD_MEM_DEVICE, TC.ptr(counts),
                                           len(frames), TC.ptr(ids), TC.ptr(done))
    else:
        rc = lib.opd_track_update_sequence(h, TC.ptr(boxes), TC.ptr(foot), TC.ptr(conf), TC.ptr(feats), TC.ptr(has), _capi.OPD_MEM_HOST, TC.ptr(counts),
                                           len(frames), TC.ptr(ids), TC.ptr(done))
    off = np.concatenate([[0], np.cumsum(counts)])
    return rc, [ids[off[f]:off[f + 1]].tolist() for f in range(len(frames))], int(done[0])


def _loop(lib, h, frames):
    """The twin: one opd_track_update per frame, stopping at the first error.  (rc, ids per frame applied, frames applied)."""
    out = []
    for boxes, foot, conf, feats, has, *_ in frames:
        rc, ids = TC.device_update(lib, _capi, h, boxes, foot, conf, feats, has)
        out.append(ids.tolist())
        if rc != 0:
            return rc, out, len(out)
    return 0, out, len(out)


@pytest.mark.parametrize("name", TC.sequence_names(np.load(TC.GOLDEN)))
def test_recorded_sequences_in_one_call(lib, golden, name):
    params, D, frames = TC.sequence(golden, name)
    a, b = (TC.create(lib, _capi, D, max_tracks=12, max_dets=16, **params) for _ in range(2))
    try:
        rc, ids, done = _sequence(lib, a, frames)
        assert rc == 0 and done == len(frames), _capi.last_error()
        info = _info(lib, a)
        assert info.last_waits == 1 and len(frames) <= info.last_launches <= 3 * len(frames)
        rc2, ids2, _ = _loop(lib, b, frames)
        assert rc2 == 0, _capi.last_error()
        for f, fr in enumerate(frames):
            assert ids[f] == ids2[f] == fr[5].tolist(), (name, f, ids[f], ids2[f], fr[5].tolist())
        assert _state(lib, a) == _state(lib, b)
        got = np.array([[r.track_id, r.age, r.hits, r.time_since_update] for r in TC.device_tracks(lib, _capi, a)], np.int32).reshape(-1, 4)
        assert np.array_equal(got, golden[f"{name}_counters"])
        # the adopted table: one more per-frame update on both
        boxes, foot, conf, feats, has, _ = frames[len(frames) // 2]
        rc, one = TC.device_update(lib, _capi, a, boxes, foot, conf, feats, has)
        rc2, two = TC.device_update(lib, _capi, b, boxes, foot, conf, feats, has)
        assert rc == rc2 == 0 and one.tolist() == two.tolist() and _state(lib, a) == _state(lib, b)
        assert _info(lib, a).last_waits == 1 and _info(lib, a).last_launches <= 2
    finally:
        lib.opd_track_destroy(a)
        lib.opd_track_destroy(b)


def test_sequence_and_per_frame_calls_interleave(lib, golden):
    name = TC.sequence_names(golden)[0]
    params, D, frames = TC.sequence(golden, name)
    assert len(frames) >= 7
    third = len(frames) // 3
    a, b = (TC.create(lib, _capi, D, max_tracks=12, max_dets=16, **params) for _ in range(2))
    try:
        rc, ids, _ = _sequence(lib, a, frames[:third])
        assert rc == 0, _capi.last_error()
        rc, more, _ = _loop(lib, a, frames[third:2 * third])
        assert rc == 0, _capi.last_error()
        rc, last, done = _sequence(lib, a, frames[2 * third:])
        assert rc == 0 and done == len(frames) - 2 * third, _capi.last_error()
        rc2, ids2, _ = _loop(lib, b, frames)
        assert rc2 == 0 and ids + more + last == ids2 == [fr[5].tolist() for fr in frames]
        assert _state(lib, a) == _state(lib, b)
        # one frame in a sequence call is opd_track_update; so is a frame without detections among others
        empty = (np.zeros((0, 4), F32), np.zeros((0, 2), F32), np.zeros(0, F32), None if frames[0][3] is None else np.zeros((0, D), F32),
                 None if frames[0][3] is None else np.zeros(0, bool), np.zeros(0, np.int32))
        for run in ([frames[1]], [frames[2], empty, frames[3]], [empty]):
            rc, ids, done = _sequence(lib, a, run)
            rc2, ids2, _ = _loop(lib, b, run)
            assert rc == rc2 == 0 and done == len(run) and ids == ids2 and _state(lib, a) == _state(lib, b), _capi.last_error()
            assert _info(lib, a).last_waits == 1
    finally:
        lib.opd_track_destroy(a)
        lib.opd_track_destroy(b)


def _walkers(n, f, D, rng):
    """n well-separated high-confidence detections on frame f, each with its own feature."""
    boxes = np.array([[100.0 + 200.0 * k + 2.0 * f, 300.0 + f, 50.0, 120.0] for k in range(n)], F32).reshape(-1, 4)
    foot = np.stack([boxes[:, 0] + boxes[:, 2] / F32(2), boxes[:, 1] + boxes[:, 3]], 1).astype(F32).reshape(-1, 2)
    feats = np.eye(max(n, 1), D, dtype=F32)[:n]
    return boxes, foot, np.full(n, 0.9, F32), feats, np.ones(n, bool), None


def test_out_of_slots_in_the_middle_of_a_sequence(lib):
    D = 16
    rng = np.random.default_rng(7)
    frames = [_walkers(n, f, D, rng) for f, n in enumerate((2, 3, 5, 3, 2))]   # frame 2 brings two more tracks than the four slots hold
    a, b = (TC.create(lib, _capi, D, max_tracks=4, max_dets=8, min_hits=1) for _ in range(2))
    try:
        rc, ids, done = _sequence(lib, a, frames)
        assert rc == _capi.OPD_EINVAL and "exceed max_tracks = 4" in _capi.last_error() and "counted as one without detections" in _capi.last_error()
        assert "opd_track_update_sequence: 3 live tracks and 2 new ones" in _capi.last_error()
        rc2, ids2, applied = _loop(lib, b, frames)
        assert rc2 == _capi.OPD_EINVAL and applied == done == 3
        assert ids[:3] == ids2 and ids[0] == [1, 2] and ids[1] == [1, 2, 3] and ids[2] == [-1] * 5
        assert ids[3] == [-1] * 3 and ids[4] == [-1] * 2, "frames behind the out-of-slots one were applied"
        assert _state(lib, a) == _state(lib, b)
        assert [(r.track_id, r.time_since_update) for r in TC.device_tracks(lib, _capi, a)] == [(1, 1), (2, 1), (3, 1)]
        rc, ids, done = _sequence(lib, a, frames[3:])   # the next call works
        rc2, ids2, _ = _loop(lib, b, frames[3:])
        assert rc == rc2 == 0 and done == 2 and ids == ids2 == [[1, 2, 3], [1, 2]] and _state(lib, a) == _state(lib, b), _capi.last_error()
    finally:
        lib.opd_track_destroy(a)
        lib.opd_track_destroy(b)


def test_refusals_that_read_the_handle_and_device_features(lib):
    D = 16
    rng = np.random.default_rng(8)
    frames = [_walkers(3, f, D, rng) for f in range(4)]
    a, b = (TC.create(lib, _capi, D, max_tracks=8, max_dets=4, min_hits=1) for _ in range(2))
    try:
        rc, ids, done = _sequence(lib, a, frames[:2])
        rc2, ids2, _ = _loop(lib, b, frames[:2])
        assert rc == rc2 == 0 and ids == ids2
        before = _state(lib, a)
        rc, ids, done = _sequence(lib, a, [frames[2], _walkers(5, 3, D, rng)])
        assert rc == _capi.OPD_EINVAL and "5 detections in frame 1" in _capi.last_error() and "max_dets = 4" in _capi.last_error()
        assert done == -7 and ids == [[-7] * 3, [-7] * 5] and _state(lib, a) == before
        feats = np.concatenate([fr[3] for fr in frames[2:]])
        rc, ids, done = _sequence(lib, a, frames[2:], feat_ptr=feats.ctypes.data)   # pageable host memory called device memory
        assert rc == _capi.OPD_EINVAL and "not device-accessible" in _capi.last_error() and _state(lib, a) == before
        dev = torch.from_numpy(feats).to("cuda")
        torch.cuda.synchronize()
        rc, ids, done = _sequence(lib, a, frames[2:], feat_ptr=dev.data_ptr())
        rc2, ids2, _ = _loop(lib, b, frames[2:])
        assert rc == rc2 == 0 and done == 2 and ids == ids2 == [[1, 2, 3]] * 2 and _state(lib, a) == _state(lib, b), _capi.last_error()
    finally:
        lib.opd_track_destroy(a)
        lib.opd_track_destroy(b)


# ---- HipTracker.update_sequence ----------------------------------------------------------------------------------------------------------
def _detections(frame):
    boxes, foot, conf, feats, has = frame[:5]
    return [Detection(bbox=tuple(float(v) for v in boxes[j]), confidence=float(conf[j]), class_id=1, class_name="person",
                      camera_coords=(float(foot[j, 0]), float(foot[j, 1])), features=feats[j] if feats is not None and has[j] else None)
            for j in range(len(conf))]


def _mirror(tracker):
    return [(t.track_id, t.age, t.hits, t.time_since_update, list(t.trajectory), t.get_state()) for t in tracker.get_tracks()]


def test_hip_tracker_update_sequence_equals_the_loop(golden):
    name = TC.sequence_names(golden)[-1]
    params, D, frames = TC.sequence(golden, name)
    a, b = (HipTracker(feature_dim=D, max_tracks=12, max_dets=16, **params) for _ in range(2))
    try:
        half = len(frames) // 2
        for run in (frames[:half], frames[half:]):
            da, db = [_detections(fr) for fr in run], [_detections(fr) for fr in run]
            got = a.update_sequence(da)
            want = [b.update(d) for d in db]
            assert [[(d.track_id, d.bbox) for d in f] for f in got] == [[(d.track_id, d.bbox) for d in f] for f in want]
            assert [[d.track_id if d.track_id is not None else -1 for d in f] for f in da] == [fr[5].tolist() for fr in run]
            assert _mirror(a) == _mirror(b) and a.next_id == b.next_id
        assert a.update_sequence([]) == []
    finally:
        a.close()
        b.close()
    D = 16
    rng = np.random.default_rng(9)
    frames = [_walkers(n, f, D, rng) for f, n in enumerate((2, 3, 5, 3))]
    a, b = (HipTracker(feature_dim=D, max_tracks=4, max_dets=8, min_hits=1) for _ in range(2))
    try:
        with pytest.raises(RuntimeError, match="counted as one without detections"):
            a.update_sequence([_detections(fr) for fr in frames])
        with pytest.raises(RuntimeError, match="counted as one without detections"):
            for fr in frames:
                b.update(_detections(fr))
        assert _mirror(a) == _mirror(b) and len(a.tracks) == 3 and a.next_id == b.next_id == 4
        assert [[d.track_id for d in f] for f in a.update_sequence([_detections(frames[3])])] == [[1, 2, 3]]
    finally:
        a.close()
        b.close()


# ---- opd_detr_detect_sequence_track --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def det(weight_cache):
    path = ensure_weight_file(weight_cache, DetrArch(), 0, 1.0, "r50")
    d = HipDetrDetector(model_path=path, max_batch=B, max_size=(H, W), resize=True, confidence_threshold=0.05, device_nms=True)
    d.load_model()
    yield d
    d.close()


@pytest.fixture(scope="module")
def clip(weight_cache):
    e = HipReIDExtractor(model_path=ensure_clip_weight_file(weight_cache, "tiny"), max_crops=512)   # (a slot for every kept person of a call, also with the suppression at 1.0)
    e.load_model()
    yield e
    e.cleanup()


@pytest.fixture(scope="module")
def frames():
    out = [np.ascontiguousarray(f).copy() for f in structured_frames(2 * B, H, W, seed=3)]
    for f in out:
        f[60:80, 100:130] = CC.UNIFORM_BGR
    return out


def _set_nms(det, thr):
    det.device_nms, det.nms_threshold = True, thr
    det._sync_nms()


def _recs_of(recs, counts, Q):
    raw = np.frombuffer(bytes(recs), TI.DET).reshape(len(counts), Q)
    return [raw[b, :int(counts[b])].copy() for b in range(len(counts))]


def _call(lib, det, name, tracker, fr, kind, ext=None, slots=0, label=PERSON):
    """opd_detr_detect_sequence_track (`tracker`: one handle) or opd_detr_detect_frames_track (`tracker`: a list).  (rc, records, ids, n_featured, frames_done)"""
    n, Q = len(fr), det.num_queries
    recs, counts = (_capi.OpdDet * (n * Q))(), (C.c_int32 * n)()
    ids, nf, done = np.full((n, Q), -7, np.int32), np.full(n, -7, np.int32), np.full(1, -7, np.int32)
    ptrs = (C.c_void_p * n)(*[f.ctypes.data for f in fr])
    m, e = C.c_void_p(det.model), ext._handle if ext is not None else None
    if name == "sequence":
        rc = lib.opd_detr_detect_sequence_track(m, e, tracker, ptrs, n, H, W, H, W, 0.05, label, kind, slots, recs, counts, ids.ctypes.data, nf.ctypes.data, done.ctypes.data)
    else:
        hs = (C.c_void_p * n)(*[t.value for t in tracker])
        rc = lib.opd_detr_detect_frames_track(m, e, hs, ptrs, n, H, W, H, W, 0.05, label, kind, slots, recs, counts, ids.ctypes.data, nf.ctypes.data)
    per = _recs_of(recs, counts, Q)
    for b in range(n):
        assert np.all(ids[b, len(per[b]):] == -7), "ids beyond the kept count were written"
    return rc, per, [ids[b, :len(per[b])].tolist() for b in range(n)], nf.tolist(), int(done[0])


@pytest.mark.parametrize("nms", [0.4, 1.0])
@pytest.mark.parametrize("kind", [NONE, ENCODER, COLOR, REID], ids=["none", "encoder", "color", "reid-clip"])
def test_detect_sequence_equals_five_single_frame_calls(lib, det, clip, frames, kind, nms):
    ext = clip if kind == REID else None
    _set_nms(det, nms)
    D = {NONE: 64, ENCODER: 256, COLOR: 256, REID: clip.feature_dim}[kind]
    slots = 512 if kind == REID else 0
    a, b = TC.create(lib, _capi, D, **TRACKER), TC.create(lib, _capi, D, **TRACKER)
    try:
        for run in (frames[:B], frames[B:]):   # the second call continues the first
            T = _info(lib, a).n_tracks
            rc, per, ids, nf, done = _call(lib, det, "sequence", a, run, kind, ext, slots)
            assert rc == 0 and done == B, _capi.last_error()
            info = _info(lib, a)
            assert info.last_waits == 0 and info.last_launches == 3 * B + (B - 1 if T == 0 else B)   # ingest, association, commit; predict / cost where a track may be alive
            kept = 0
            for f, frame in enumerate(run):
                rc1, per1, ids1, nf1, _ = _call(lib, det, "frames", [b], [frame], kind, ext, slots)
                assert rc1 == 0, _capi.last_error()
                got, want = per[f].copy(), per1[0].copy()
                assert got["frame"].tolist() == [f] * len(got)
                got["frame"] = 0
                assert got.tobytes() == want.tobytes(), (f, "records")
                assert ids[f] == ids1[0] and nf[f] == nf1[0], (kind, nms, f, ids[f], ids1[0], nf[f], nf1[0])
                kept += len(want)
            assert kind != REID or kept <= slots, "every kept person needs a crop slot for the twins to see the same rows"
            assert kept >= B and any(i >= 0 for f in ids for i in f)
            assert _state(lib, a) == _state(lib, b)
            print(f"kind {kind} nms {nms}: {T} tracks before, {kept} records kept, {_info(lib, a).n_tracks} tracks after, {info.last_launches} launches")
    finally:
        lib.opd_track_destroy(a)
        lib.opd_track_destroy(b)


def test_detect_sequence_out_of_slots_and_refusals(lib, det, clip, frames):
    Q = det.num_queries
    _set_nms(det, 1.0)
    small = dict(TRACKER, max_tracks=4, high_conf_threshold=0.06)   # (every record may start a track)
    a, b = TC.create(lib, _capi, 256, **small), TC.create(lib, _capi, 256, **small)
    good, narrow, wide = TC.create(lib, _capi, 256, **TRACKER), TC.create(lib, _capi, 256, **dict(TRACKER, max_dets=Q - 1)), TC.create(lib, _capi, 512, **TRACKER)
    try:
        rc, per, ids, nf, done = _call(lib, det, "sequence", a, frames[:3], COLOR)
        assert rc == _capi.OPD_EINVAL and "opd_detr_detect_sequence_track" in _capi.last_error() and "exceed max_tracks = 4" in _capi.last_error()
        assert "counted as one without detections" in _capi.last_error() and done == 1
        rc1, per1, ids1, _, _ = _call(lib, det, "frames", [b], [frames[0]], COLOR)
        assert rc1 == _capi.OPD_EINVAL and "exceed max_tracks = 4" in _capi.last_error()
        assert all(len(p) > 4 for p in per) and per[0].tobytes() == per1[0].tobytes(), "records and counts of all frames are delivered"
        assert ids == [[-1] * len(p) for p in per] and nf == [len(p) for p in per]
        assert _state(lib, a) == _state(lib, b)

        def refused(text, t=good, kind=COLOR, e=None, slots=0, label=PERSON):
            before = _state(lib, good)
            rc, _, ids, _, done = _call(lib, det, "sequence", t, frames[:2], kind, e, slots, label)
            assert rc == _capi.OPD_EINVAL and text in _capi.last_error() and "opd_detr_detect_sequence_track" in _capi.last_error(), (text, _capi.last_error())
            assert done == -7 and _state(lib, good) == before

        _set_nms(det, 0.4)
        refused("label 1, the call asks for label 2", label=2)
        refused("null tracker handle", t=None)
        refused("max_dets = %d" % (Q - 1), t=narrow)
        refused("feature_dim = 512", t=wide)
        refused("feature_dim = 256", kind=REID, e=clip, slots=8)   # (the tiny CLIP set has 128 numbers a row)
        refused("slots = 0 outside 1 .. max_crops", kind=REID, e=clip, slots=0)
        refused("slots = 513 outside 1 .. max_crops", kind=REID, e=clip, slots=513)
        det.device_nms = False
        det._sync_nms()
        refused("opd_detr_set_nms is off")
        _set_nms(det, 0.4)
        rc, per, ids, nf, done = _call(lib, det, "sequence", good, frames[:2], COLOR)   # nothing above left a mark: the handle still tracks
        assert rc == 0 and done == 2 and all(len(p) > 0 for p in per) and any(i >= 0 for f in ids for i in f), _capi.last_error()
    finally:
        for h in (a, b, good, narrow, wide):
            lib.opd_track_destroy(h)


@pytest.mark.parametrize("features", ["color", None])
@pytest.mark.parametrize("device_nms", [True, False])
def test_detect_and_track_batch_equals_the_loop(det, frames, features, device_nms):
    det.device_nms, det.nms_threshold = device_nms, 0.4
    D = 256 if features else 64
    a, b = (HipTracker(feature_dim=D, max_tracks=128, max_dets=128, min_hits=1) for _ in range(2))
    try:
        run = frames[:B + 2]   # one full chunk and a short one
        got = det.detect_and_track_batch(run, a, features=features)
        info = _capi.OpdTrackStatus()
        _capi.check(a._lib.opd_track_info(a._h, C.byref(info)), "opd_track_info")
        assert info.last_waits == (0 if device_nms else 1), "the sequence call was not taken" if device_nms else "the fallback was not taken"
        want = [det.detect_and_track(f, b, features=features) for f in run]
        key = lambda d: (d.track_id, d.bbox, d.confidence, d.query_index)   # noqa: E731
        assert [[key(d) for d in f] for f in got] == [[key(d) for d in f] for f in want]
        assert len(got) == len(run) and all(len(f) > 0 for f in got) and _mirror(a) == _mirror(b) and a.next_id == b.next_id
        assert det.detect_and_track_batch([], a, features=features) == []
    finally:
        a.close()
        b.close()
        det.device_nms = True
