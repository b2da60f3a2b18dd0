"""GPU tests of the streams calls (-m gpu): ``track_assoc_multi_kernel`` on cameras of different sizes in one launch, ``opd_track_update_streams``,
``opd_detr_detect_streams_track``, ``HipTracker.update_streams`` and ``HipDetrDetector.detect_and_track_streams``.

Everything here is an equality.  The camera-batched kernels run the one-tracker kernels' code on the block of blockIdx.y's camera, and cameras share
no memory, so C trackers that take their frames side by side in one call and twins that take them in one sequence call (or one per-frame call) each
must agree in every id, every counter and every state bit, whatever the interleaving and whatever the other cameras of the call do."""

import ctypes as C
import faulthandler

import numpy as np
import pytest

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
NONE, COLOR, REID = _capi.OPD_TRACK_FEAT_NONE, _capi.OPD_TRACK_FEAT_COLOR, _capi.OPD_TRACK_FEAT_REID
TRACKER = dict(max_tracks=128, max_dets=128, min_hits=1, high_conf_threshold=0.5)
H, W = 288, 512
B = 6
CAMERA_OF = [0, 1, 0, 2, 2, 0]
SLOTS = 640


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


# ---- 1. the association kernel, cameras of different sizes in ONE launch -----------------------------------------------------------------------
# blocks that fit the LDS cache and (400 x 400: about 200 confirmed tracks x 230 high-confidence detections, more than its 28672 floats) one that is read from
# global memory, the four columns-per-lane instantiations (<= 64, <= 128, <= 256, more), a camera with no tracks and one with no detections, side by side
SHAPES = [(1, 1), (130, 70), (3, 300), (0, 5), (5, 0), (64, 65), (400, 400)]


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


def _assoc_multi(lib, cams, n_free):
    """cams: [(mats, hits, conf)]; (kernel, host), each a list per camera of (matches, new detections, unmatched tracks)."""
    T = np.array([len(c[1]) for c in cams], np.int32)
    N = np.array([len(c[2]) for c in cams], np.int32)
    cat = lambda parts, dt: np.ascontiguousarray(np.concatenate([np.asarray(p, dt).reshape(-1) for p in parts]))   # noqa: E731
    app, iou, comb = (cat([c[0][k] for c in cams], F32) for k in range(3))
    hits, conf = cat([c[1] for c in cams], np.int32), cat([c[2] for c in cams], F32)
    rows_m, rows_n, rows_t = np.maximum(np.minimum(T, N), 1), np.maximum(N, 1), np.maximum(T, 1)
    sides = [[np.full((rows_m.sum(), 2), -7, np.int32), np.full(len(cams), -7, np.int32), np.full(rows_n.sum(), -7, np.int32), np.full(len(cams), -7, np.int32),
              np.full(rows_t.sum(), -7, np.int32), np.full(len(cams), -7, np.int32)] for _ in range(2)]
    rc = lib.opd_track_test_assoc_multi(0, len(cams), TC.ptr(T), TC.ptr(N), TC.ptr(np.asarray(n_free, np.int32)), TC.ptr(app), TC.ptr(iou), TC.ptr(comb), TC.ptr(hits),
                                        TC.ptr(conf), 3, 0.5, *[TC.ptr(a) for side in sides for a in side])
    assert rc == 0, _capi.last_error()
    om, on, ot = (np.concatenate([[0], np.cumsum(r)]) for r in (rows_m, rows_n, rows_t))
    return tuple([([tuple(p) for p in m[om[c]:om[c] + nm[c]].tolist()], new[on[c]:on[c] + nn[c]].tolist(), un[ot[c]:ot[c] + nu[c]].tolist()) for c in range(len(cams))]
                 for m, nm, new, nn, un, nu in sides)


@pytest.mark.parametrize("kind", ["uniform", "ties", "nonfinite", "one_camera_without_free_slots"])
def test_association_kernel_cameras_of_different_sizes_in_one_launch(lib, kind):
    rng = np.random.default_rng({"uniform": 21, "ties": 22, "nonfinite": 23, "one_camera_without_free_slots": 24}[kind])
    cams = [_draw("uniform" if kind.startswith("one") else kind, T, N, rng) for T, N in SHAPES]
    n_free = [N for _, N in SHAPES]
    if kind.startswith("one"):
        n_free[2] = 0   # the 3 x 300 camera: its matches and new tracks are dropped, the cameras beside it keep theirs
    got, want = _assoc_multi(lib, cams, n_free)
    for c, (T, N) in enumerate(SHAPES):
        assert got[c] == want[c], (kind, c, T, N, [(a, b) for a, b in zip(got[c][0], want[c][0]) if a != b][:4], got[c][1][:8], want[c][1][:8], got[c][2][:8], want[c][2][:8])
    assert sum(len(w[0]) for w in want) > 0 and want[3] == ([], [j for j in range(5) if cams[3][2][j] >= 0.5], []) and want[4] == ([], [], list(range(5)))
    if kind.startswith("one"):
        assert want[2][0] == [] and want[2][1] == [] and all(len(want[c][0]) > 0 for c in (1, 5, 6))
    else:
        assert all(len(want[c][1]) > 0 for c in (2, 3))


# ---- opd_track_update_streams --------------------------------------------------------------------------------------------------------------------
def _round_robin(lengths, order=None):
    """camera_of for cameras of `lengths` frames, one frame of each in turn (`order`: the turn order) while it has one."""
    order = list(range(len(lengths))) if order is None else order
    return [c for k in range(max(lengths)) for c in order if k < lengths[c]]


def _streams(lib, handles, cams, camera_of):
    """cams: per camera the frames of TC.sequence; camera_of: the call order.  (rc, ids per camera per frame, frames_done per camera); ids start as sentinels."""
    at, frames = [0] * len(cams), []
    for c in camera_of:
        frames.append(cams[c][at[c]])
        at[c] += 1
    assert at == [len(cam) for cam in cams]
    widths = [int(np.asarray(cam[0][3]).shape[1]) if cam[0][3] is not None else None for cam in cams]
    any_feats = any(w is not None for w in widths)
    counts = np.array([len(fr[2]) for fr in frames], np.int32)
    cat = lambda k, tail: np.ascontiguousarray(np.concatenate([np.asarray(fr[k], F32).reshape((-1,) + tail) for fr in frames]))   # noqa: E731
    feats = has = None
    if any_feats:   # ragged by frame: a row is as wide as its own tracker's feature_dim; a camera without features sends has = 0 and rows that are never read
        dims = [int(_info(lib, handles[c]).feature_dim) for c in range(len(cams))]
        feats = np.ascontiguousarray(np.concatenate([np.asarray(fr[3], F32).reshape(-1) if fr[3] is not None else np.zeros(len(fr[2]) * dims[c], F32)
                                                     for c, fr in zip(camera_of, frames)] + [np.zeros(1, F32)]))
        has = np.ascontiguousarray(np.concatenate([np.asarray(fr[4], np.uint8) if fr[4] is not None else np.zeros(len(fr[2]), np.uint8) for fr in frames] + [np.zeros(1, np.uint8)]))
    ids, done = np.full(max(int(counts.sum()), 1), -7, np.int32), np.full(len(cams), -7, np.int32)
    hs = (C.c_void_p * len(cams))(*[h.value for h in handles])
    cam = np.asarray(camera_of, np.int32)
    rc = lib.opd_track_update_streams(hs, len(cams), TC.ptr(cam), len(frames), TC.ptr(cat(0, (4,))), TC.ptr(cat(1, (2,))), TC.ptr(cat(2, ())), TC.ptr(feats), TC.ptr(has),
                                      _capi.OPD_MEM_HOST, TC.ptr(counts), TC.ptr(ids), TC.ptr(done))
    off = np.concatenate([[0], np.cumsum(counts)])
    per = [[] for _ in cams]
    for f, c in enumerate(camera_of):
        per[c].append(ids[off[f]:off[f + 1]].tolist())
    return rc, per, done.tolist()


def _pack(frames):
    counts = np.array([len(fr[2]) for fr in frames], np.int32)
    cat = lambda k, tail: np.ascontiguousarray(np.concatenate([np.asarray(fr[k], F32).reshape((-1,) + tail) for fr in frames]))   # noqa: E731
    use = frames[0][3] is not None
    feats = cat(3, (np.asarray(frames[0][3]).shape[1],)) if use else None
    has = np.ascontiguousarray(np.concatenate([np.asarray(fr[4], np.uint8) for fr in frames])) if use else None
    return cat(0, (4,)), cat(1, (2,)), cat(2, ()), feats, has, counts


def _sequence(lib, h, frames):
    """One opd_track_update_sequence: (rc, ids per frame, frames_done)."""
    boxes, foot, conf, feats, has, counts = _pack(frames)
    ids, done = np.full(max(int(counts.sum()), 1), -7, np.int32), np.full(1, -7, np.int32)
    rc = lib.opd_track_update_sequence(h, TC.ptr(boxes), TC.ptr(foot), TC.ptr(conf), TC.ptr(feats), TC.ptr(has), _capi.OPD_MEM_HOST, TC.ptr(counts), len(frames), TC.ptr(ids), TC.ptr(done))
    off = np.concatenate([[0], np.cumsum(counts)])
    return rc, [ids[off[f]:off[f + 1]].tolist() for f in range(len(frames))], int(done[0])


def _loop(lib, h, frames):
    """One opd_track_update per frame, stopping at the first error: (rc, ids per frame applied, frames applied)."""
    out = []
    for boxes, foot, conf, feats, has, *_ in frames:
        rc, ids = TC.device_update(lib, _capi, h, boxes, foot, conf, feats, has)
        out.append(ids.tolist())
        if rc != 0:
            return rc, out, len(out)
    return 0, out, len(out)


def _make(lib, golden, names):
    """Per recorded sequence its frames and two trackers, every pair with its own configuration."""
    cams, a, b = [], [], []
    for c, name in enumerate(names):
        params, D, frames = TC.sequence(golden, name)
        cams.append(frames)
        for side in (a, b):
            side.append(TC.create(lib, _capi, D, max_tracks=12 + c % 3, max_dets=16 + c % 5, **params))
    return cams, a, b


def test_all_recorded_sequences_as_cameras_of_one_call(lib, golden):
    names = TC.sequence_names(golden)
    cams, a, b = _make(lib, golden, names)
    try:
        lengths = [len(cam) for cam in cams]
        assert len(names) == 27 and min(lengths) == 8 and max(lengths) == 30
        assert {int(_info(lib, h).feature_dim) for h in a} == {37, 256, 512} and {int(_info(lib, h).max_age) for h in a} == {3, 30}
        rc, ids, done = _streams(lib, a, cams, _round_robin(lengths))
        assert rc == 0 and done == lengths, _capi.last_error()
        launches = {_info(lib, h).last_launches for h in a}
        assert len(launches) == 1 and 30 <= launches.pop() <= 4 * 30
        assert [_info(lib, h).last_waits for h in a] == [1] + [0] * 26
        for c, name in enumerate(names):
            rc2, ids2, done2 = _sequence(lib, b[c], cams[c])
            assert rc2 == 0 and done2 == lengths[c], _capi.last_error()
            assert ids[c] == ids2 == [fr[5].tolist() for fr in cams[c]], (name, ids[c], ids2)
            assert _state(lib, a[c]) == _state(lib, b[c]), name
    finally:
        for h in a + b:
            lib.opd_track_destroy(h)


def test_a_camera_does_not_depend_on_its_neighbours_or_the_interleaving(lib, golden):
    names = [n for n in TC.sequence_names(golden)][:3]
    cams, a, b = _make(lib, golden, names)
    cams2, a2, b2 = _make(lib, golden, names)
    try:
        lengths = [len(cam) for cam in cams]
        rc, ids, done = _streams(lib, a, cams, _round_robin(lengths))
        assert rc == 0 and done == lengths, _capi.last_error()
        # the cameras in order (2, 0, 1), camera after camera instead of round robin
        order = [2, 0, 1]
        moved = [c for c in range(3) for _ in cams[order[c]]]
        rc, ids_m, done_m = _streams(lib, [a2[c] for c in order], [cams[c] for c in order], moved)
        assert rc == 0 and done_m == [lengths[c] for c in order], _capi.last_error()
        for c in range(3):
            rc1, ids1, _ = _sequence(lib, b[c], cams[c])
            assert rc1 == 0 and ids[c] == ids_m[order.index(c)] == ids1
            assert _state(lib, a[c]) == _state(lib, a2[c]) == _state(lib, b[c])
    finally:
        for h in a + b + a2 + b2:
            lib.opd_track_destroy(h)


def _walkers(n, f, D, shift=0.0):
    """n well-separated high-confidence detections on frame f, each with its own feature."""
    boxes = np.array([[100.0 + 200.0 * k + 2.0 * f + shift, 300.0 + f, 50.0, 120.0] for k in range(n)], F32).reshape(-1, 4)
    foot = np.stack([boxes[:, 0] + boxes[:, 2] / F32(2), boxes[:, 1] + boxes[:, 3]], 1).astype(F32).reshape(-1, 2)
    feats = np.eye(max(n, 1), D, dtype=F32)[:n]
    return boxes, foot, np.full(n, 0.9, F32), feats, np.ones(n, bool), None


def test_out_of_slots_in_one_camera_in_the_middle(lib):
    dims = (16, 24, 16)
    cams = [[_walkers(n, f, dims[0]) for f, n in enumerate((2, 2, 3, 3, 2, 2))],
            [_walkers(n, f, dims[1]) for f, n in enumerate((2, 3, 5, 3, 2))],   # frame 2 brings two more tracks than the four slots hold
            [_walkers(n, f, dims[2], 7.0) for f, n in enumerate((1, 4, 4))]]
    a, b = ([TC.create(lib, _capi, dims[c], max_tracks=(8, 4, 8)[c], max_dets=8, min_hits=1) for c in range(3)] for _ in range(2))
    try:
        lengths = [len(cam) for cam in cams]
        rc, ids, done = _streams(lib, a, cams, _round_robin(lengths))
        err = _capi.last_error()
        assert rc == _capi.OPD_EINVAL and "opd_track_update_streams: camera 1: 3 live tracks and 2 new ones exceed max_tracks = 4" in err, err
        assert "counted as one without detections" in err and "cameras out of slots: 1" in err
        assert done == [6, 3, 3]
        rc1, ids1, applied = _loop(lib, b[1], cams[1])
        assert rc1 == _capi.OPD_EINVAL and applied == 3
        assert ids[1][:3] == ids1 and ids[1][2] == [-1] * 5 and ids[1][3] == [-1] * 3 and ids[1][4] == [-1] * 2, "frames behind the out-of-slots one were applied"
        assert _state(lib, a[1]) == _state(lib, b[1])
        for c in (0, 2):   # the other two cameras finish
            rc2, ids2, n2 = _loop(lib, b[c], cams[c])
            assert rc2 == 0 and n2 == lengths[c] and ids[c] == ids2 and all(i >= 0 for f in ids[c] for i in f)
            assert _state(lib, a[c]) == _state(lib, b[c])
        # a following streams call and a following per-frame call both work
        more = [[cams[0][5]], cams[1][3:], [cams[2][2]]]
        rc, ids, done = _streams(lib, a, more, _round_robin([1, 2, 1]))
        assert rc == 0 and done == [1, 2, 1], _capi.last_error()
        for c in range(3):
            rc2, ids2, _ = _loop(lib, b[c], more[c])
            assert rc2 == 0 and ids[c] == ids2 and _state(lib, a[c]) == _state(lib, b[c])
        assert ids[1] == [[1, 2, 3], [1, 2]]
        for c in range(3):
            fr = cams[c][1]
            rc1, one = TC.device_update(lib, _capi, a[c], *fr[:5])
            rc2, two = TC.device_update(lib, _capi, b[c], *fr[:5])
            assert rc1 == rc2 == 0 and one.tolist() == two.tolist() and _state(lib, a[c]) == _state(lib, b[c])
    finally:
        for h in a + b:
            lib.opd_track_destroy(h)


def test_streams_per_frame_and_sequence_calls_interleave(lib, golden):
    names = TC.sequence_names(golden)
    names = [names[0], names[len(names) // 2], names[-1]]
    cams, a, b = _make(lib, golden, names)
    try:
        cut = [(len(cam) // 4, len(cam) // 2, 3 * len(cam) // 4) for cam in cams]
        part = lambda k: [cam[([0] + list(cut[c]))[k]:(list(cut[c]) + [len(cam)])[k]] for c, cam in enumerate(cams)]   # noqa: E731
        got = [[] for _ in cams]
        rc, ids, _ = _streams(lib, a, part(0), _round_robin([len(p) for p in part(0)]))
        assert rc == 0, _capi.last_error()
        for c in range(3):
            got[c] += ids[c]
            rc, ids1, _ = _loop(lib, a[c], part(1)[c]) if c != 1 else _sequence(lib, a[c], part(1)[c])
            assert rc == 0, _capi.last_error()
            got[c] += ids1
        rc, ids, _ = _streams(lib, [a[2], a[0]], [part(2)[2], part(2)[0]], _round_robin([len(part(2)[2]), len(part(2)[0])]))   # two of the three, the other way round
        assert rc == 0, _capi.last_error()
        got[2] += ids[0]
        got[0] += ids[1]
        rc, ids1, _ = _sequence(lib, a[1], part(2)[1])
        got[1] += ids1
        rc, ids, done = _streams(lib, a, part(3), _round_robin([len(p) for p in part(3)], [1, 2, 0]))
        assert rc == 0 and done == [len(p) for p in part(3)], _capi.last_error()
        for c in range(3):
            got[c] += ids[c]
            rc2, ids2, _ = _loop(lib, b[c], cams[c])
            assert rc2 == 0 and got[c] == ids2 == [fr[5].tolist() for fr in cams[c]]
            assert _state(lib, a[c]) == _state(lib, b[c])
    finally:
        for h in a + b:
            lib.opd_track_destroy(h)


def test_refusals_that_read_the_handles(lib):
    D = 16
    frames = [_walkers(3, f, D) for f in range(4)]
    a = [TC.create(lib, _capi, D, max_tracks=8, max_dets=4, min_hits=1) for _ in range(2)]
    try:
        rc, ids, done = _streams(lib, a, [frames[:2], frames[:2]], [0, 1, 0, 1])
        assert rc == 0 and done == [2, 2]
        before = [_state(lib, h) for h in a]
        rc, ids, done = _streams(lib, a, [[frames[2]], [_walkers(5, 3, D)]], [0, 1])
        assert rc == _capi.OPD_EINVAL and "5 detections in frame 1" in _capi.last_error() and "camera 1 was made for max_dets = 4" in _capi.last_error()
        assert done == [-7, -7] and ids == [[[-7] * 3], [[-7] * 5]] and [_state(lib, h) for h in a] == before
        rc, ids, done = _streams(lib, [a[0], a[0]], [[frames[2]], [frames[3]]], [0, 1])
        assert rc == _capi.OPD_EINVAL and "name the same tracker" in _capi.last_error() and done == [-7, -7] and [_state(lib, h) for h in a] == before
        rc, ids, done = _streams(lib, a, [[frames[2]], [frames[3]]], [1, 0])   # nothing above left a mark
        assert rc == 0 and done == [1, 1] and ids == [[[1, 2, 3]], [[1, 2, 3]]], _capi.last_error()
    finally:
        for h in a:
            lib.opd_track_destroy(h)


# ---- HipTracker.update_streams -----------------------------------------------------------------------------------------------------------------------
def _detections(frame):
    boxes, foot, conf, feats, has = frame[:5]
    return [Detection(bbox=tuple(float(v) for v in boxes[j]), confidence=float(conf[j]), class_id=1, class_name="person",
                      camera_coords=(float(foot[j, 0]), float(foot[j, 1])), features=feats[j] if feats is not None and has[j] else None)
            for j in range(len(conf))]


def _mirror(tracker):
    return [(t.track_id, t.age, t.hits, t.time_since_update, list(t.trajectory), t.get_state()) for t in tracker.get_tracks()]


def test_hip_tracker_update_streams_equals_update_sequence(golden):
    names = TC.sequence_names(golden)
    names = [names[0], names[len(names) // 2], names[-1]]
    seqs = [TC.sequence(golden, n) for n in names]
    a, b = ([HipTracker(feature_dim=D, max_tracks=12, max_dets=16, **params) for params, D, _ in seqs] for _ in range(2))
    try:
        for lo, hi in ((0.0, 0.5), (0.5, 1.0)):
            runs = [frames[int(lo * len(frames)):int(hi * len(frames))] for _, _, frames in seqs]
            da, db = [[_detections(fr) for fr in run] for run in runs], [[_detections(fr) for fr in run] for run in runs]
            got = HipTracker.update_streams(a, da)
            want = [t.update_sequence(d) for t, d in zip(b, db)]
            key = lambda cams: [[[(d.track_id, d.bbox) for d in f] for f in cam] for cam in cams]   # noqa: E731
            assert key(got) == key(want)
            assert [[[d.track_id if d.track_id is not None else -1 for d in f] for f in cam] for cam in da] == [[fr[5].tolist() for fr in run] for run in runs]
            assert [_mirror(t) for t in a] == [_mirror(t) for t in b] and [t.next_id for t in a] == [t.next_id for t in b]
        assert HipTracker.update_streams(a, [[], [], []]) == [[], [], []]
    finally:
        for t in a + b:
            t.close()
    D = 16
    cams = [[_walkers(n, f, D) for f, n in enumerate((2, 3, 5, 3))], [_walkers(n, f, D) for f, n in enumerate((1, 2, 2, 2, 1))]]
    a, b = ([HipTracker(feature_dim=D, max_tracks=4, max_dets=8, min_hits=1) for _ in range(2)] for _ in range(2))
    try:
        with pytest.raises(RuntimeError, match="counted as one without detections"):
            HipTracker.update_streams(a, [[_detections(fr) for fr in cam] for cam in cams])
        with pytest.raises(RuntimeError, match="counted as one without detections"):
            b[0].update_sequence([_detections(fr) for fr in cams[0]])
        b[1].update_sequence([_detections(fr) for fr in cams[1]])
        assert [_mirror(t) for t in a] == [_mirror(t) for t in b] and len(a[0].tracks) == 3 and len(a[1].tracks) == 2
        got = HipTracker.update_streams(a, [[_detections(cams[0][3])], [_detections(cams[1][4])]])
        assert [[[d.track_id for d in f] for f in cam] for cam in got] == [[[1, 2, 3]], [[1]]]
    finally:
        for t in a + b:
            t.close()


# ---- opd_detr_detect_streams_track -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def det(weight_cache):
    path = ensure_weight_file(weight_cache, DetrArch(), 0, 1.0, "r50")
    d = HipDetrDetector(model_path=path, max_batch=B, max_size=(H, W), resize=True, confidence_threshold=0.05, device_nms=True)
    d.load_model()
    yield d
    d.close()


@pytest.fixture(scope="module")
def clip(weight_cache):
    # a slot for every kept person of a call, also with the suppression at 1.0: six frames keep up to 6 x 100 records, more than the 512 slots that
    # cover the five-frame calls of test_track_sequence_gpu.py, and a camera's twin call, with fewer frames, would then see rows this call has no slot for
    e = HipReIDExtractor(model_path=ensure_clip_weight_file(weight_cache, "tiny"), max_crops=SLOTS)
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


def _call(lib, det, trackers, fr, kind, ext=None, slots=0, label=PERSON, camera_of=None):
    """opd_detr_detect_streams_track (`trackers`: a list, with camera_of) or opd_detr_detect_sequence_track (`trackers`: one handle).
    (rc, records, ids, n_featured, frames_done)"""
    n, Q = len(fr), det.num_queries
    recs, counts = (_capi.OpdDet * (n * Q))(), (C.c_int32 * n)()
    ids, nf = np.full((n, Q), -7, np.int32), np.full(n, -7, np.int32)
    ptrs = (C.c_void_p * n)(*[f.ctypes.data for f in fr])
    m, e = C.c_void_p(det.model), ext._handle if ext is not None else None
    if camera_of is None:
        done = np.full(1, -7, np.int32)
        rc = lib.opd_detr_detect_sequence_track(m, e, trackers, ptrs, n, H, W, H, W, 0.05, label, kind, slots, recs, counts, ids.ctypes.data, nf.ctypes.data, done.ctypes.data)
    else:
        done = np.full(len(trackers), -7, np.int32)
        hs = (C.c_void_p * len(trackers))(*[None if t is None else t.value for t in trackers])
        cam = np.asarray(camera_of, np.int32)
        rc = lib.opd_detr_detect_streams_track(m, e, hs, len(trackers), TC.ptr(cam), ptrs, n, H, W, H, W, 0.05, label, kind, slots, recs, counts, ids.ctypes.data,
                                               nf.ctypes.data, done.ctypes.data)
    per = _recs_of(recs, counts, Q)
    for b in range(n):
        assert np.all(ids[b, len(per[b]):] == -7), "ids beyond the kept count were written"
    return rc, per, [ids[b, :len(per[b])].tolist() for b in range(n)], nf.tolist(), done.tolist()


@pytest.mark.parametrize("nms", [0.4, 1.0])
@pytest.mark.parametrize("kind", [NONE, COLOR, REID], ids=["none", "color", "reid-clip"])
def test_detect_streams_equals_a_sequence_call_per_camera(lib, det, clip, frames, kind, nms):
    ext = clip if kind == REID else None
    _set_nms(det, nms)
    D = {NONE: 64, COLOR: 256, REID: clip.feature_dim}[kind]
    slots = SLOTS if kind == REID else 0
    a, b = ([TC.create(lib, _capi, D, **dict(TRACKER, max_tracks=128 - 8 * c)) for c in range(3)] for _ in range(2))
    try:
        for run in (frames[:B], frames[B:]):   # the second call continues the first
            rc, per, ids, nf, done = _call(lib, det, a, run, kind, ext, slots, camera_of=CAMERA_OF)
            assert rc == 0 and done == [3, 1, 2], _capi.last_error()
            infos = [_info(lib, h) for h in a]
            assert all(i.last_waits == 0 for i in infos) and len({i.last_launches for i in infos}) == 1 and 3 * 3 <= infos[0].last_launches <= 4 * 3
            kept = 0
            for c in range(3):
                mine = [f for f in range(B) if CAMERA_OF[f] == c]
                rc1, per1, ids1, nf1, done1 = _call(lib, det, b[c], [run[f] for f in mine], kind, ext, slots)
                assert rc1 == 0 and done1 == [len(mine)], _capi.last_error()
                for k, f in enumerate(mine):
                    got, want = per[f].copy(), per1[k].copy()
                    assert got["frame"].tolist() == [f] * len(got) and want["frame"].tolist() == [k] * len(want)
                    got["frame"] = want["frame"] = 0
                    assert got.tobytes() == want.tobytes(), (c, f, "records")
                    assert ids[f] == ids1[k] and nf[f] == nf1[k], (kind, nms, c, f, ids[f], ids1[k], nf[f], nf1[k])
                    kept += len(want)
                assert _state(lib, a[c]) == _state(lib, b[c]), c
            assert kind != REID or kept <= slots, "every kept person needs a crop slot for the twins to see the same rows"
            assert all(len(p) >= 1 for p in per) and any(i >= 0 for f in ids for i in f)
            print(f"kind {kind} nms {nms}: {kept} records kept, {[_info(lib, h).n_tracks for h in a]} tracks after, {infos[0].last_launches} launches")
    finally:
        for h in a + b:
            lib.opd_track_destroy(h)


def test_detect_streams_out_of_slots_in_one_camera_and_refusals(lib, det, clip, frames):
    Q = det.num_queries
    _set_nms(det, 1.0)
    small = dict(TRACKER, max_tracks=4, high_conf_threshold=0.06)   # (every record may start a track)
    a, b = ([TC.create(lib, _capi, 256, **(small if c == 1 else TRACKER)) for c in range(2)] for _ in range(2))
    good, narrow, wide = (TC.create(lib, _capi, 256, **TRACKER), TC.create(lib, _capi, 256, **dict(TRACKER, max_dets=Q - 1)), TC.create(lib, _capi, 512, **TRACKER))
    try:
        cam = [0, 1, 1, 0, 0]
        rc, per, ids, nf, done = _call(lib, det, a, frames[:5], COLOR, camera_of=cam)
        err = _capi.last_error()
        assert rc == _capi.OPD_EINVAL and "opd_detr_detect_streams_track: camera 1:" in err and "exceed max_tracks = 4" in err and "cameras out of slots: 1" in err, err
        assert "counted as one without detections" in err and done == [3, 1]
        assert all(len(p) > 4 for p in per), "records and counts of all frames are delivered"
        rc0, per0, ids0, nf0, done0 = _call(lib, det, b[0], [frames[0], frames[3], frames[4]], COLOR)
        assert rc0 == 0 and done0 == [3], _capi.last_error()
        rc1, per1, ids1, nf1, done1 = _call(lib, det, b[1], [frames[1], frames[2]], COLOR)
        assert rc1 == _capi.OPD_EINVAL and done1 == [1]
        assert [ids[0], ids[3], ids[4]] == ids0 and any(i >= 0 for f in ids0 for i in f) and [ids[1], ids[2]] == ids1 == [[-1] * len(per[1]), [-1] * len(per[2])]
        assert nf == [len(p) for p in per] and [_state(lib, h) for h in a] == [_state(lib, h) for h in b]

        def refused(text, t, kind=COLOR, e=None, slots=0, label=PERSON, camera_of=(0, 1)):
            before = _state(lib, good)
            rc, _, ids, _, done = _call(lib, det, t, frames[:2], kind, e, slots, label, camera_of=list(camera_of))
            assert rc == _capi.OPD_EINVAL and text in _capi.last_error() and "opd_detr_detect_streams_track" in _capi.last_error(), (text, _capi.last_error())
            assert done == [-7] * len(t) and _state(lib, good) == before

        _set_nms(det, 0.4)
        refused("label 1, the call asks for label 2", [good, a[0]], label=2)
        refused("null tracker handle", [good, None])
        refused("max_dets = %d" % (Q - 1), [good, narrow])
        refused("feature_dim = 512", [good, wide])
        refused("feature_dim = 256", [good, a[0]], kind=REID, e=clip, slots=8)   # (the tiny CLIP set has 128 numbers a row)
        refused("camera_of[1] = 2 outside", [good, a[0]], camera_of=(0, 2))
        refused("name the same tracker", [good, good])
        refused("camera 1 gets no frame", [good, a[0]], camera_of=(0, 0))
        det.device_nms = False
        det._sync_nms()
        refused("opd_detr_set_nms is off", [good, a[0]])
        _set_nms(det, 0.4)
        rc, per, ids, nf, done = _call(lib, det, [good, a[0]], frames[:2], COLOR, camera_of=[1, 0])   # nothing above left a mark: the handles still track
        assert rc == 0 and done == [1, 1] and all(len(p) > 0 for p in per) and any(i >= 0 for f in ids for i in f), _capi.last_error()
    finally:
        for h in a + b + [good, narrow, wide]:
            lib.opd_track_destroy(h)


@pytest.mark.parametrize("device_nms", [True, False])
def test_detect_and_track_streams_equals_detect_and_track_batch_per_camera(det, frames, device_nms):
    det.device_nms, det.nms_threshold = device_nms, 0.4
    a, b = ([HipTracker(feature_dim=256, max_tracks=128, max_dets=128, min_hits=1) for _ in range(3)] for _ in range(2))
    try:
        per_camera = [frames[:5], frames[5:6], frames[6:9]]   # 9 frames at max_batch 6: two calls, the cut inside camera 0's run
        got = det.detect_and_track_streams(per_camera, a, features="color")
        info = _capi.OpdTrackStatus()
        _capi.check(a[0]._lib.opd_track_info(a[0]._h, C.byref(info)), "opd_track_info")
        assert info.last_waits == (0 if device_nms else 1), "the streams call was not taken" if device_nms else "the fallback was not taken"
        want = [det.detect_and_track_batch(f, t, features="color") for f, t in zip(per_camera, b)]
        key = lambda d: (d.track_id, d.bbox, d.confidence, d.query_index)   # noqa: E731
        assert [[[key(d) for d in f] for f in cam] for cam in got] == [[[key(d) for d in f] for f in cam] for cam in want]
        assert [len(cam) for cam in got] == [5, 1, 3] and all(len(f) > 0 for cam in got for f in cam)
        assert [_mirror(t) for t in a] == [_mirror(t) for t in b] and [t.next_id for t in a] == [t.next_id for t in b]
        assert det.detect_and_track_streams([[], []], a[:2], features="color") == [[], []]
    finally:
        for t in a + b:
            t.close()
        det.device_nms = True
