"""GPU tests of the hybrid tracker inside a tiled call (-m gpu; ``opd_detr_detect_tiled_hybrid``, ``opd_detr_detect_tiled_sequence_hybrid``,
``HipDetrDetector.detect_tiled_hybrid`` / ``track_tiled_hybrid_batch``, ``TiledDetector.detect_and_track_hybrid`` / ``track_hybrid_batch``).

Every comparison is an equality of bits between handles that take the new call and twins, made alike and fed the same frames, that take the
separate calls ``opd_detr_detect_tiled`` (a mixed grid: ``opd_detr_detect_tiled_ragged``), ``opd_lwt_update`` with the boxes the Python path builds
from the merged detections, and ``opd_lwt_interpolate``: merged records and counts, ids, every number of every track (``opd_lwt_get``), the counts
of ``opd_lwt_info``, and -- through one more in-between frame on both -- flow points and reference frame.  The ingest launch alone is held to its
numpy restatement (tile_hybrid_common.py), which test_tile_hybrid_cpu.py holds to the Python path.  Nothing here has a tolerance."""

import ctypes as C
import faulthandler

import numpy as np
import pytest

import flow_common as FC
import lwt_common as LC
import tile_hybrid_common as TH
import tile_stages_common as TS
import track_common as TC
from office_person_detection_vit_amd import HipDetrDetector, HipFloorMapper, HipLightweightTracker, TiledDetector, _capi
from office_person_detection_vit_amd.detector import model_input_size
from office_person_detection_vit_amd.frames import structured_frames
from office_person_detection_vit_amd.tiling import split_tiles, tile_grid
from office_person_detection_vit_amd.weights import DetrArch, ensure_weight_file
from tile_common import TILE_DET

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64

THRESHOLD = 0.05
FRAME_HW = (192, 256)
SEEDS = (5, 6, 7)
GRID = tile_grid(192, 256, 2, 2, 0.125)
ODD_HW, ODD = (193, 256), tile_grid(193, 256, 2, 2, 0.125)
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


def _detector(weight_cache, **kw):
    d = HipDetrDetector(model_path=ensure_weight_file(weight_cache, DetrArch(), 0, 2.0, "r50"), max_batch=8, max_size=(256, 320), resize=True,
                        confidence_threshold=THRESHOLD, **kw)
    d.load_model()
    return d


@pytest.fixture(scope="module")
def sharp(weight_cache, lib):
    """tests/test_tile_stages_gpu.py's `sharp` detector: the seeded weights with attention gain 2, on which the seam merge absorbs boxes."""
    d = _detector(weight_cache)
    yield d
    d.close()


@pytest.fixture(scope="module")
def mapper(lib):
    h, w = FRAME_HW
    rng = np.random.default_rng(9)
    src = np.concatenate([np.array([[0, 0], [w, 0], [0, h], [w, h]], float), rng.uniform((10, 10), (w - 10, h - 10), (20, 2))])
    dst = np.stack([5.5 * src[:, 0] + 40 + 15 * np.sin(src[:, 1] / 40.0), 7.0 * src[:, 1] + 30 + 10 * np.cos(src[:, 0] / 50.0)], 1)
    m = HipFloorMapper.piecewise_affine(src, dst, FM, ZONES, device=0)
    yield m
    m.close()


def _frames(hw):
    return [np.ascontiguousarray(structured_frames(1, hw[0], hw[1], seed=s)[0]).copy() for s in SEEDS]


@pytest.fixture(scope="module")
def frames():
    return _frames(FRAME_HW)


# ---- the calls through ctypes ----------------------------------------------------------------------------------------------------------------------
def _lwt(lib, max_tracks=512, max_dets=512, hw=FRAME_HW, flow=True, iou=0.3):
    return LC.create(lib, _capi, max_tracks=max_tracks, max_dets=max_dets, max_h=hw[0], max_w=hw[1], max_age=30, iou_threshold=iou, use_optical_flow=flow)


def _observe(lib, h):
    """Every number of every track as bytes, and (n_tracks, next_id, n_points)."""
    st = LC.info(lib, _capi, h)
    return [a.tobytes() for a in LC.device_states(lib, _capi, h)], (st.n_tracks, st.next_id, st.n_points)


def _recs_bits(recs):
    return [q[0] for q in recs], np.array([q[1] for q in recs], F64).tobytes()


def _geometry(det, grid):
    """(windows, H, W, tile_HW or None) as the tiled entries take them."""
    win = np.asarray(grid, np.int32).reshape(-1, 4)
    sizes = det.tile_model_sizes(grid)
    if len({(t[2], t[3]) for t in grid}) == 1:
        return win, sizes[0][0], sizes[0][1], None
    return win, 0, 0, np.asarray(sizes, np.int32).reshape(-1, 2)


def _params(det):
    return _capi.OpdTileParams(struct_size=C.sizeof(_capi.OpdTileParams), person_label=1, tile_nms_threshold=float(det.nms_threshold), merge_nms_threshold=0.4,
                               merge_threshold=0.5, edge_tolerance=0.01)


def _hwp(hw):
    return None if hw is None else hw.ctypes.data_as(C.c_void_p)


def _fused(lib, det, trackers, frames, grid=GRID, floor_map=None):
    """opd_detr_detect_tiled_hybrid: (rc, merged records per frame, ids per frame, raw counts, floor rows); ids start as sentinels and must stay so
    beyond the kept count."""
    n, T = len(frames), len(grid)
    S = T * det.num_queries
    h, w = frames[0].shape[:2]
    win, H, W, hw = _geometry(det, grid)
    p = _params(det)
    out, counts, ids = np.zeros((n, S), TILE_DET), np.full(n, -9, np.int32), np.full((n, S), -7, np.int32)
    ptrs = (C.c_void_p * n)(*[f.ctypes.data for f in frames])
    hs = (C.c_void_p * n)(*[t.value if t is not None else None for t in trackers])
    hy = _capi.OpdTileHybrid(struct_size=C.sizeof(_capi.OpdTileHybrid), trackers=C.addressof(hs), track_ids=ids.ctypes.data)
    floor = None
    if floor_map is not None:
        floor = np.zeros(n * S, floor_map.REC_DTYPE)
        hy.floor, hy.floor_out = floor_map._require().value, floor.ctypes.data
    rc = lib.opd_detr_detect_tiled_hybrid(C.c_void_p(det.model), ptrs, n, h, w, win.ctypes.data_as(C.c_void_p), T, H, W, _hwp(hw), THRESHOLD, C.byref(p), C.byref(hy),
                                          out.ctypes.data_as(C.POINTER(_capi.OpdTileDet)), counts.ctypes.data_as(C.POINTER(C.c_int32)))
    per = [out[b, :max(int(counts[b]), 0)].copy() for b in range(n)]
    for b in range(n):
        if counts[b] >= 0:
            assert np.all(ids[b, len(per[b]):] == -7), "ids beyond the kept count were written"
    return rc, per, [ids[b, :len(per[b])].copy() for b in range(n)], counts, floor


def _plain(lib, det, frame, grid=GRID):
    """opd_detr_detect_tiled (a mixed grid: opd_detr_detect_tiled_ragged) on one frame: its merged records."""
    T = len(grid)
    S = T * det.num_queries
    h, w = frame.shape[:2]
    win, H, W, hw = _geometry(det, grid)
    p = _params(det)
    out, counts = np.zeros((1, S), TILE_DET), np.full(1, -9, np.int32)
    ptrs = (C.c_void_p * 1)(frame.ctypes.data)
    tail = (C.byref(p), out.ctypes.data_as(C.POINTER(_capi.OpdTileDet)), counts.ctypes.data_as(C.POINTER(C.c_int32)))
    if hw is None:
        rc = lib.opd_detr_detect_tiled(C.c_void_p(det.model), ptrs, 1, h, w, win.ctypes.data_as(C.c_void_p), T, H, W, THRESHOLD, *tail)
    else:
        rc = lib.opd_detr_detect_tiled_ragged(C.c_void_p(det.model), ptrs, 1, h, w, win.ctypes.data_as(C.c_void_p), T, _hwp(hw), THRESHOLD, tail[0], None, *tail[1:])
    assert rc == 0, _capi.last_error()
    return out[0, :int(counts[0])].copy()


def _boxes(recs):
    """What HipLightweightTracker.update_with_detections builds from the merged Detections of these records."""
    bbox = [(float(r["x"]), float(r["y"]), float(r["w"]), float(r["h"])) for r in recs]   # Detection.bbox of HipDetrDetector.detect_tiled
    return np.array(bbox, F32).reshape(len(bbox), 4)


def _two_calls(lib, det, tracker, frame, grid=GRID):
    """The plain tiled call on one frame, then opd_lwt_update with the boxes the Python path builds: (rc of the update, merged records, ids)."""
    r = _plain(lib, det, frame, grid)
    rc, ids = LC.device_update(lib, _capi, tracker, _boxes(r), frame)
    return rc, r, ids


def _same_after_one_more_frame(lib, a, b, frame):
    """Flow points and reference frame: one more in-between frame on both, from the frame each holds as its reference."""
    assert _recs_bits(LC.device_interpolate(lib, _capi, a, frame)) == _recs_bits(LC.device_interpolate(lib, _capi, b, frame))
    assert _observe(lib, a) == _observe(lib, b)


# ---- 1. the ingest launch alone --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,n", [(400, 0), (400, 1), (400, 63), (400, 64), (400, 65), (400, 400), (400, 401), (400, -3), (1024, 1024)])
def test_ingest_of_merged_records_equals_the_restatement(lib, S, n):
    """Counts around the wave's 64-lane stride, the full stride, the widest stride there is, and counts the kernel must clamp."""
    merged = TH.edge_merged(S)
    boxes = np.full((S, 4), 7.5, F32)
    want = boxes.copy()
    n_want = TH.ingest_merged(merged, n, S, want)
    n_out = np.full(1, -7, np.int32)
    assert lib.opd_lwt_test_ingest_merged(0, TC.ptr(merged), n, S, TC.ptr(boxes), TC.ptr(n_out)) == 0, _capi.last_error()
    assert int(n_out[0]) == n_want == max(0, min(n, S))
    assert boxes.tobytes() == want.tobytes(), (n, np.argwhere(boxes != want)[:8].tolist())
    assert boxes[:n_want].tobytes() == _boxes(merged[:n_want]).tobytes()   # ... which is the Python path's array


def test_ingest_hook_refusals(lib):
    merged, boxes, n_out = TH.edge_merged(8), np.zeros((8, 4), F32), np.zeros(1, np.int32)
    for S in (0, 1025):
        assert lib.opd_lwt_test_ingest_merged(0, TC.ptr(merged), 1, S, TC.ptr(boxes), TC.ptr(n_out)) == _capi.OPD_EINVAL
    assert lib.opd_lwt_test_ingest_merged(0, None, 1, 8, TC.ptr(boxes), TC.ptr(n_out)) == _capi.OPD_EINVAL


# ---- 2. detection frames ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flow", [True, False], ids=["optical_flow", "no_flow"])
def test_three_consecutive_calls_on_one_tracker_equal_the_separate_calls(lib, sharp, frames, flow):
    a, b = _lwt(lib, flow=flow), _lwt(lib, flow=flow)
    per_tile_widest = max(d.bbox[2] for f in frames for t in sharp.detect_batch(split_tiles(f, 2, 2, 0.125)[0]) for d in t)
    grown, matched = False, []
    try:
        for k, f in enumerate(frames):
            before = LC.info(lib, _capi, b).next_id
            rc, per, ids, counts, _ = _fused(lib, sharp, [a], [f])
            assert rc == 0, _capi.last_error()
            rc2, r, ids2 = _two_calls(lib, sharp, b, f)
            assert rc2 == 0, _capi.last_error()
            assert per[0].tobytes() == r.tobytes() and int(counts[0]) == len(r), k
            assert ids[0].tolist() == ids2.tolist() and _observe(lib, a) == _observe(lib, b), (k, ids[0].tolist(), ids2.tolist())
            info = LC.info(lib, _capi, a)
            assert info.last_waits == 0 and info.n_points == (len(r) if flow else 0), (k, info.n_points)   # the wait was the detector's
            # what keeps this from passing vacuously, asserted on the twin
            assert len(r) >= 2, (k, len(r))
            grown = grown or bool((r["w"] > per_tile_widest + 1.0).any())
            matched.append(int((ids2 < before).sum()))
            if k == 0:
                assert LC.info(lib, _capi, b).n_tracks >= 2 and ids2.tolist() == list(range(1, len(r) + 1))   # the first frame opens tracks
        assert grown, "no kept box has grown: the seam merge itself never happened"
        assert matched[1] >= 1, matched   # the second frame matches a track of the first
        st = LC.device_states(lib, _capi, b)[4]
        assert (st[:, 3] > 0).any() or matched[2] >= 1, "neither ageing nor a later match occurred"
        if flow:
            _same_after_one_more_frame(lib, a, b, frames[0])
            assert LC.info(lib, _capi, a).last_waits == 1
    finally:
        for h in (a, b):
            lib.opd_lwt_destroy(h)


def test_two_frames_into_two_trackers_equal_two_one_frame_calls(lib, sharp, frames):
    a = [_lwt(lib), _lwt(lib, flow=False)]
    b = [_lwt(lib), _lwt(lib, flow=False)]
    c = [_lwt(lib), _lwt(lib, flow=False)]
    try:
        for pair in (frames[:2], frames[1:]):
            rc, per, ids, _, _ = _fused(lib, sharp, a, pair)
            assert rc == 0, _capi.last_error()
            for k in range(2):
                rc1, per1, ids1, _, _ = _fused(lib, sharp, [b[k]], [pair[k]])
                rc2, r, ids2 = _two_calls(lib, sharp, c[k], pair[k])
                assert rc1 == 0 and rc2 == 0, _capi.last_error()
                assert per[k].tobytes() == per1[0].tobytes() == r.tobytes() and ids[k].tolist() == ids1[0].tolist() == ids2.tolist(), k
                assert _observe(lib, a[k]) == _observe(lib, b[k]) == _observe(lib, c[k]), k
                assert LC.info(lib, _capi, a[k]).last_waits == 0
        _same_after_one_more_frame(lib, a[0], c[0], frames[0])
    finally:
        for h in a + b + c:
            lib.opd_lwt_destroy(h)


def test_with_a_floor_map_the_rows_equal_the_staged_call(lib, sharp, frames, mapper):
    a, b = _lwt(lib), _lwt(lib)
    try:
        rc, per, ids, counts, floor = _fused(lib, sharp, [a], frames[:1], floor_map=mapper)
        assert rc == 0, _capi.last_error()
        rc2, r, ids2 = _two_calls(lib, sharp, b, frames[0])
        assert per[0].tobytes() == r.tobytes() and ids[0].tolist() == ids2.tolist() and _observe(lib, a) == _observe(lib, b)
        want = sharp.detect_tiled(frames[:1], GRID)[0]
        mapper.apply(want)
        got = sharp.detect_tiled(frames[:1], GRID)[0]
        for k, d in enumerate(got):
            mapper._fill(d, floor[k])
        TS.same([got], [want], "floor rows by position")
        assert any(d.floor_coords is not None for d in want)
    finally:
        for h in (a, b):
            lib.opd_lwt_destroy(h)


# ---- 3. a mixed grid -------------------------------------------------------------------------------------------------------------------------------
def test_a_mixed_grid_equals_the_ragged_call_and_the_update(lib, sharp):
    frames = _frames(ODD_HW)
    assert len({(t[2], t[3]) for t in ODD}) > 1
    a, b = _lwt(lib, hw=ODD_HW), _lwt(lib, hw=ODD_HW)
    try:
        for k, f in enumerate(frames):
            rc, per, ids, _, _ = _fused(lib, sharp, [a], [f], grid=ODD)
            assert rc == 0, _capi.last_error()
            rc2, r, ids2 = _two_calls(lib, sharp, b, f, grid=ODD)
            assert rc2 == 0 and len(r) >= 2 and per[0].tobytes() == r.tobytes() and ids[0].tolist() == ids2.tolist(), k
            assert _observe(lib, a) == _observe(lib, b), k
        assert LC.info(lib, _capi, b).n_tracks >= 2
        _same_after_one_more_frame(lib, a, b, frames[0])
    finally:
        for h in (a, b):
            lib.opd_lwt_destroy(h)


# ---- 4. a run of frames ----------------------------------------------------------------------------------------------------------------------------
def _shifted(f):
    """The frame moved by the integer shift (2 rows, 1 column), the flat rectangle painted over it (test_hybrid_gpu.py's construction)."""
    hh, ww = f.shape[:2]
    ys, xs = np.clip(np.arange(hh) - 2, 0, hh - 1), np.clip(np.arange(ww) - 1, 0, ww - 1)
    g = f[ys][:, xs].copy()
    y0, y1, x0, x1 = FC.flat_rect(hh, ww)
    g[y0:y1, x0:x1] = FC.FLAT_BGR
    return np.ascontiguousarray(g)


@pytest.fixture(scope="module")
def run_frames():
    """A structured 192 x 256 frame, then each next one the one before shifted by (2, 1) with the flat rectangle painted over it."""
    f0, f1 = FC.structured_pair(FRAME_HW[0], FRAME_HW[1], 501, (2, 1))
    out = [np.ascontiguousarray(f0), np.ascontiguousarray(f1)]
    while len(out) < 5:
        out.append(_shifted(out[-1]))
    for f in out:
        f.setflags(write=False)
    return out


def _seq(lib, det, t, frames, keys, capacity, grid=GRID):
    """opd_detr_detect_tiled_sequence_hybrid: (rc, frames_done, per frame: (merged records, ids) of a key frame or the record list of an in-between frame)."""
    F, K, T = len(frames), sum(keys), len(grid)
    S = T * det.num_queries
    h, w = frames[0].shape[:2]
    win, H, W, hw = _geometry(det, grid)
    p = _params(det)
    out, counts, ids = np.zeros((max(K, 1), S), TILE_DET), np.full(max(K, 1), -9, np.int32), np.full((max(K, 1), S), -7, np.int32)
    lrecs, lcounts, done = (_capi.OpdLwtRec * (max(F - K, 1) * capacity))(), (C.c_int32 * max(F - K, 1))(*([-7] * max(F - K, 1))), C.c_int32(-7)
    ptrs = (C.c_void_p * F)(*[f.ctypes.data for f in frames])
    flags = (C.c_uint8 * F)(*[int(k) for k in keys])
    rc = lib.opd_detr_detect_tiled_sequence_hybrid(C.c_void_p(det.model), t, ptrs, flags, F, h, w, win.ctypes.data_as(C.c_void_p), T, H, W, _hwp(hw), THRESHOLD, C.byref(p),
                                                   out.ctypes.data_as(C.POINTER(_capi.OpdTileDet)), counts.ctypes.data_as(C.POINTER(C.c_int32)), ids.ctypes.data, lrecs, capacity,
                                                   lcounts, C.byref(done))
    res, k, j = [], 0, 0
    for f in range(F):
        if keys[f]:
            n = max(int(counts[k]), 0)
            if counts[k] >= 0:
                assert np.all(ids[k, n:] == -7), "ids beyond the kept count were written"
            res.append((out[k, :n].copy(), ids[k, :n].copy()))
            k += 1
        else:
            res.append([(lrecs[j * capacity + i].track_id, tuple(float(v) for v in lrecs[j * capacity + i].bbox)) for i in range(max(lcounts[j], 0))] if lcounts[j] != -7 else None)
            j += 1
    return rc, done.value, res


def _loop(lib, det, t, frames, keys, grid=GRID):
    """The per-frame loop of the separate calls, stopping at the first refused update: (frames applied, outputs as _seq's, point counts, refused records)."""
    out, points = [], []
    for f, (frame, key) in enumerate(zip(frames, keys)):
        if key:
            rc, r, ids = _two_calls(lib, det, t, frame, grid)
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
            assert got[f][0].tobytes() == want[f][0].tobytes() and got[f][1].tolist() == want[f][1].tolist(), (where, f, got[f][1].tolist(), want[f][1].tolist())
        else:
            assert _recs_bits(got[f]) == _recs_bits(want[f]), (where, f)


def test_a_run_of_key_and_in_between_frames_equals_the_loop(lib, sharp, run_frames):
    a, b = _lwt(lib), _lwt(lib)
    keys = [True, False, False, True, False]   # 2 key frames x 4 tiles = max_batch
    try:
        rc, done, got = _seq(lib, sharp, a, run_frames, keys, capacity=512)
        assert rc == 0 and done == 5, _capi.last_error()
        assert LC.info(lib, _capi, a).last_waits == 0
        applied, want, points, _ = _loop(lib, sharp, b, run_frames, keys)
        assert applied == 5, points
        tracks = LC.info(lib, _capi, b).n_tracks
        assert len(want[0][0]) >= 2 and 0 < points[2] < len(want[0][0]), (points, len(want[0][0]), tracks)   # LK followed some points and lost some
        _same_outputs(got, want, keys, "five frames")
        assert _observe(lib, a) == _observe(lib, b)
        _same_after_one_more_frame(lib, a, b, run_frames[0])
        # a run that starts in between, on a tracker that holds tracks and points
        run, keys2 = [run_frames[1], run_frames[2], run_frames[3], run_frames[4]], [False, False, True, False]
        rc, done, got = _seq(lib, sharp, a, run, keys2, capacity=512)
        assert rc == 0 and done == 4, _capi.last_error()
        applied, want, points, _ = _loop(lib, sharp, b, run, keys2)
        assert applied == 4
        _same_outputs(got, want, keys2, "in-between frames first")
        assert _observe(lib, a) == _observe(lib, b)
        # K = 0 is opd_lwt_interpolate_sequence
        rc, done, got = _seq(lib, sharp, a, run_frames[:3], [False] * 3, capacity=512)
        assert rc == 0 and done == 3 and LC.info(lib, _capi, a).last_waits == 1, _capi.last_error()
        ptrs = (C.c_void_p * 3)(*[f.ctypes.data for f in run_frames[:3]])
        recs, counts = (_capi.OpdLwtRec * (3 * 512))(), (C.c_int32 * 3)()
        assert lib.opd_lwt_interpolate_sequence(b, ptrs, 0, 3, FRAME_HW[0], FRAME_HW[1], recs, 512, counts) == 0, _capi.last_error()
        for f in range(3):
            assert _recs_bits(got[f]) == _recs_bits([(recs[f * 512 + i].track_id, tuple(float(v) for v in recs[f * 512 + i].bbox)) for i in range(counts[f])]), f
        assert _observe(lib, a) == _observe(lib, b) and LC.info(lib, _capi, a).last_launches == LC.info(lib, _capi, b).last_launches
    finally:
        for h in (a, b):
            lib.opd_lwt_destroy(h)


def test_a_run_whose_second_key_frame_is_refused(lib, sharp, run_frames, frames):
    """max_tracks = the first key frame's kept count, matching at IoU 0.95: the second key frame (another scene) opens a track, which does not fit.
    The twin's per-frame update of that frame is asserted to be refused, else this proves nothing."""
    n0 = len(_plain(lib, sharp, run_frames[0]))
    assert n0 >= 2
    run, keys = [run_frames[0], run_frames[1], frames[1], run_frames[2]], [True, False, True, False]
    a, b = _lwt(lib, max_tracks=n0, iou=0.95), _lwt(lib, max_tracks=n0, iou=0.95)
    try:
        rc, done, got = _seq(lib, sharp, a, run, keys, capacity=n0)
        assert rc == _capi.OPD_EINVAL and f"max_tracks = {n0}" in _capi.last_error() and "frame 2" in _capi.last_error(), _capi.last_error()
        assert done == 3
        applied, want, points, refused_records = _loop(lib, sharp, b, run, keys)
        assert applied == 2 and refused_records is not None   # the per-frame update of that frame is refused there too
        _same_outputs(got, want, keys, "the accepted frames")
        assert got[2][0].tobytes() == refused_records.tobytes() and got[2][1].tolist() == [-1] * len(refused_records)   # records and counts of ALL key frames are delivered
        assert got[3] == []                                                                                              # a later in-between frame: no records
        assert _observe(lib, a) == _observe(lib, b)
        _same_after_one_more_frame(lib, a, b, run_frames[2])   # the reference frame is still the last accepted frame's
    finally:
        for h in (a, b):
            lib.opd_lwt_destroy(h)


# ---- 5. refusals with handles ------------------------------------------------------------------------------------------------------------------------
def test_refusals_with_handles_change_nothing(lib, sharp, frames, run_frames):
    good, small_dets, small_frame, no_room = _lwt(lib), _lwt(lib, max_dets=399), _lwt(lib, hw=(97, 131)), _lwt(lib, max_tracks=1, iou=0.95)
    try:
        rc, _, ids, _, _ = _fused(lib, sharp, [good], frames[:1])
        assert rc == 0 and len(ids[0]) >= 2, _capi.last_error()
        plain_before = _plain(lib, sharp, frames[0]).tobytes()

        def refused(text, trackers, fr, me="opd_detr_detect_tiled_hybrid"):
            before = [_observe(lib, t) for t in trackers if t is not None]
            rc = _fused(lib, sharp, trackers, fr)[0]
            assert rc == _capi.OPD_EINVAL and text in _capi.last_error() and _capi.last_error().startswith(me + ":"), (text, _capi.last_error())
            assert [_observe(lib, t) for t in trackers if t is not None] == before, text

        refused("created for up to 97 x 131", [small_frame], frames[:1])
        refused("created for up to 97 x 131", [good, small_frame], frames[:2])   # ... before the first tracker sees anything
        refused("max_dets = 399", [small_dets], frames[:1])
        refused("name the same tracker", [good, good], frames[:2])
        refused("null tracker handle", [None], frames[:1])
        refused("3 frames x 4 tiles", [good, small_dets, small_frame], frames)
        # new tracks that do not fit: records and counts are delivered, that tracker's ids are -1 and it is left as it was, the other is committed
        twin = _lwt(lib)
        try:
            assert _two_calls(lib, sharp, twin, frames[0])[0] == 0
            before = _observe(lib, no_room)
            rc, per, ids, _, _ = _fused(lib, sharp, [no_room, good], [frames[1], frames[1]])
            assert rc == _capi.OPD_EINVAL and "max_tracks = 1" in _capi.last_error(), _capi.last_error()
            rc2, r, ids2 = _two_calls(lib, sharp, twin, frames[1])
            assert rc2 == 0 and per[0].tobytes() == per[1].tobytes() == r.tobytes() and len(r) >= 2
            assert ids[0].tolist() == [-1] * len(r) and ids[1].tolist() == ids2.tolist()
            assert _observe(lib, no_room) == before and _observe(lib, good) == _observe(lib, twin)
        finally:
            lib.opd_lwt_destroy(twin)

        def seq_refused(text, t, fr, keys, capacity=512):
            before = _observe(lib, t)
            rc, _, _ = _seq(lib, sharp, t, fr, keys, capacity)
            assert rc == _capi.OPD_EINVAL and text in _capi.last_error(), (text, _capi.last_error())
            assert _observe(lib, t) == before, text

        seq_refused("3 frames x 4 tiles", good, run_frames[:3], [True, True, True])   # K x n_tiles > max_batch
        seq_refused("max_tracks = 512", good, run_frames[:2], [True, False], capacity=511)
        seq_refused("max_dets = 399", small_dets, run_frames[:2], [True, False])
        seq_refused("created for up to 97 x 131", small_frame, run_frames[:2], [True, False])
        assert _plain(lib, sharp, frames[0]).tobytes() == plain_before   # the detector is as it was
    finally:
        for h in (good, small_dets, small_frame, no_room):
            lib.opd_lwt_destroy(h)


# ---- 6. Python ---------------------------------------------------------------------------------------------------------------------------------------
def _track_fields(t):
    return [(q.track_id, q.bbox, tuple(q.center), q.age, q.hits, q.time_since_update) for q in t.tracks]


def _status(t):
    s = t.info()
    return (s.n_tracks, s.next_id, s.n_points)


def test_class_detect_tiled_hybrid_equals_its_fallback_loop(sharp, frames, mapper):
    a, b, c, d = (HipLightweightTracker(max_tracks=512) for _ in range(4))
    small, small_twin = HipLightweightTracker(max_tracks=64), HipLightweightTracker(max_tracks=64)
    try:
        for pair in (frames[:2], frames[1:]):
            got = sharp.detect_tiled_hybrid(pair, GRID, [a, b], floor_map=mapper)
            assert a.info().last_waits == 0 and b.info().last_waits == 0   # the fused path was taken: the wait was the detector's
            want = sharp.detect_tiled(pair, GRID)
            for t, f, dets in zip((c, d), pair, want):
                t.update_with_detections(f, dets)
                mapper.apply(dets)
            TS.same(got, want, "detect_tiled_hybrid")
            assert all(x.track_id is not None for dets in got for x in dets) and min(len(x) for x in got) >= 2
            assert _track_fields(a) == _track_fields(c) and _track_fields(b) == _track_fields(d)
            assert _status(a) == _status(c) and _status(b) == _status(d)
        assert a.interpolate(frames[0]) == c.interpolate(frames[0])
        # max_tracks below tiles x queries: the separate calls run one after the other, with the same lists
        got = sharp.detect_tiled_hybrid(frames[:1], GRID, [small])
        want = sharp.detect_tiled(frames[:1], GRID)
        small_twin.update_with_detections(frames[0], want[0])
        TS.same(got, want, "fallback")
        assert small.info().last_waits == 1 and _track_fields(small) == _track_fields(small_twin)
        # a mixed grid through the same method
        odd = _frames(ODD_HW)[:1]
        e, f = HipLightweightTracker(max_tracks=512), HipLightweightTracker(max_tracks=512)
        try:
            got = sharp.detect_tiled_hybrid(odd, ODD, [e])
            want = sharp.detect_tiled_ragged(odd, ODD)
            f.update_with_detections(odd[0], want[0])
            TS.same(got, want, "mixed grid")
            assert e.info().last_waits == 0 and _track_fields(e) == _track_fields(f)
        finally:
            e.close()
            f.close()
    finally:
        for t in (a, b, c, d, small, small_twin):
            t.close()


def test_class_track_tiled_hybrid_batch_equals_the_loop(sharp, run_frames):
    a, b = HipLightweightTracker(max_tracks=512), HipLightweightTracker(max_tracks=512)
    seq = [np.array(f) for f in run_frames] + [np.array(run_frames[0]), np.array(run_frames[1])]
    keys = [True, False, False, True, False, True, False]   # three key frames: two native calls (max_batch // 4 = 2 key frames each)
    try:
        got = sharp.track_tiled_hybrid_batch(seq, GRID, a, keys)
        assert a.info().last_waits == 0
        want = [b.update_with_detections(f, sharp.detect_tiled([f], GRID)[0]) if k else b.interpolate(f) for f, k in zip(seq, keys)]
        assert len(got) == len(want) == 7
        for f, (g, w) in enumerate(zip(got, want)):
            if keys[f]:
                TS.same([g], [w], f"key frame {f}")
            else:
                assert g == w and len(g) > 0, f
        assert _track_fields(a) == _track_fields(b) and _status(a) == _status(b)
    finally:
        a.close()
        b.close()


def test_tiled_detector_methods_equal_their_fallback_loops(sharp, frames, run_frames, monkeypatch):
    calls = []
    real_one, real_run = sharp.detect_tiled_hybrid, sharp.track_tiled_hybrid_batch
    monkeypatch.setattr(sharp, "detect_tiled_hybrid", lambda *a, **kw: (calls.append("detect_tiled_hybrid"), real_one(*a, **kw))[1])
    monkeypatch.setattr(sharp, "track_tiled_hybrid_batch", lambda *a, **kw: (calls.append("track_tiled_hybrid_batch"), real_run(*a, **kw))[1])
    native, host = TiledDetector(sharp, native=True), TiledDetector(sharp, native=True)
    a, b = HipLightweightTracker(max_tracks=512), HipLightweightTracker(max_tracks=512)
    seq, keys = [np.array(f) for f in run_frames[:4]], [True, False, True, False]
    try:
        got = native.detect_and_track_hybrid(frames[0], a)
        want = b.update_with_detections(frames[0], host.detect(frames[0]))
        TS.same([got], [want], "detect_and_track_hybrid")
        assert a.info().last_waits == 0 and len(got) >= 2
        got = native.track_hybrid_batch(seq, a, keys)
        want = [b.update_with_detections(f, host.detect(f)) if k else b.interpolate(f) for f, k in zip(seq, keys)]
        for f, (g, w) in enumerate(zip(got, want)):
            if keys[f]:
                TS.same([g], [w], f"key frame {f}")
            else:
                assert g == w, f
        assert calls == ["detect_tiled_hybrid", "track_tiled_hybrid_batch"]
        assert _track_fields(a) == _track_fields(b) and _status(a) == _status(b)
    finally:
        a.close()
        b.close()


# ---- 7. no leak into the existing calls --------------------------------------------------------------------------------------------------------------
def test_existing_calls_after_the_new_ones_equal_a_fresh_handle(weight_cache, lib, frames, run_frames):
    used, fresh = _detector(weight_cache, device_nms=True), _detector(weight_cache, device_nms=True)
    t = [HipLightweightTracker(max_tracks=512) for _ in range(4)]
    try:
        used.detect_tiled_hybrid(frames[:2], GRID, t[:2])
        used.track_tiled_hybrid_batch([np.array(f) for f in run_frames[:3]], GRID, t[0], [True, False, True])
        used.detect_tiled_hybrid(_frames(ODD_HW)[:1], ODD, [HipLightweightTracker(max_tracks=512)])

        def existing(det, lwt):
            tiled = [[TS.fields(d) for d in w] for w in det.detect_tiled(frames, GRID)]
            hybrid = [TS.fields(d) for d in det.detect_and_track_hybrid(frames[0], lwt)]
            assert lwt.info().last_waits == 0   # the frame-list hybrid entry itself
            return tiled, hybrid, _track_fields(lwt)

        got, want = existing(used, t[2]), existing(fresh, t[3])
        assert got == want and len(got[0][0]) >= 2 and len(got[1]) >= 1
    finally:
        for x in t:
            x.close()
        used.close()
        fresh.close()
