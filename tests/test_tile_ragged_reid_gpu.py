"""GPU tests of the Re-ID rows inside a tiled call whose tiles DIFFER in size (-m gpu; ``opd_detr_detect_tiled_ragged_reid``,
``HipDetrDetector.detect_tiled_ragged_reid``, ``TiledDetector(native=True, mixed_sizes=True)`` with ``features="reid"``): the fused call end to end
against ``detect_tiled_ragged`` + ``reid.extract_features`` (+ ``floor_map.apply``, + ``tracker.update``) on the same handles, a grid of one size
against ``opd_detr_detect_tiled_reid`` byte for byte, and the refusals.  Everything here is an equality."""

import ctypes as C
import faulthandler

import numpy as np
import pytest

import tile_stages_common as TS
from office_person_detection_vit_amd import HipDetrDetector, HipFloorMapper, HipOSNetReIDExtractor, HipTracker, TiledDetector, _capi
from office_person_detection_vit_amd.detector import model_input_size
from office_person_detection_vit_amd.frames import structured_frames
from office_person_detection_vit_amd.tiling import tile_grid
from office_person_detection_vit_amd.weights import DetrArch, ensure_osnet_weight_file, ensure_weight_file
from tile_common import TILE_DET

pytestmark = pytest.mark.gpu

THRESHOLD = 0.05
MAX_CROPS = 64
SEEDS = (5, 6, 7)
ODD_HW, ODD = (193, 256), tile_grid(193, 256, 2, 2, 0.125)      # a side that does not divide
STRIP_HW, STRIP = (96, 384), tile_grid(96, 384, 1, 3, 0.125)    # an interior tile
EVEN_HW, EVEN = (192, 256), tile_grid(192, 256, 2, 2, 0.125)    # one size
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


@pytest.fixture(scope="module")
def sharp(weight_cache, lib):
    """tests/test_tile_stages_gpu.py's `sharp` detector: the seeded weights with attention gain 2, on which the seam merge absorbs boxes."""
    d = HipDetrDetector(model_path=ensure_weight_file(weight_cache, DetrArch(), 0, 2.0, "r50"), max_batch=8, max_size=(256, 320), resize=True,
                        confidence_threshold=THRESHOLD)
    d.load_model()
    yield d
    d.close()


@pytest.fixture(scope="module")
def ext(weight_cache, lib):
    e = HipOSNetReIDExtractor(model_path=ensure_osnet_weight_file(weight_cache, "half"), max_crops=MAX_CROPS)
    e.load_model()
    yield e
    e.cleanup()


@pytest.fixture(scope="module")
def mapper(lib):
    h, w = ODD_HW
    rng = np.random.default_rng(9)
    src = np.concatenate([np.array([[0, 0], [w, 0], [0, h], [w, h]], float), rng.uniform((10, 10), (w - 10, h - 10), (20, 2))])
    dst = np.stack([5.5 * src[:, 0] + 40 + 15 * np.sin(src[:, 1] / 40.0), 7.0 * src[:, 1] + 30 + 10 * np.cos(src[:, 0] / 50.0)], 1)
    m = HipFloorMapper.piecewise_affine(src, dst, FM, ZONES, device=0)
    yield m
    m.close()


def _frames(hw):
    return [np.ascontiguousarray(structured_frames(1, hw[0], hw[1], seed=s)[0]).copy() for s in SEEDS]


@pytest.fixture(scope="module")
def odd_frames():
    return _frames(ODD_HW)


def _separate(det, ext, frames, grid, floor_map=None):
    """The separate calls on the same handles: detect_tiled_ragged, then reid.extract_features and floor_map.apply per frame."""
    out = det.detect_tiled_ragged(frames, grid)
    for f, dets in zip(frames, out):
        for d, row in zip(dets, ext.extract_features(f, [d.bbox for d in dets])):
            d.features = row
        if floor_map is not None:
            floor_map.apply(dets)
    return out


@pytest.fixture(scope="module")
def reference(sharp, ext, odd_frames, mapper):
    out = _separate(sharp, ext, odd_frames, ODD, mapper)
    HIGH_CONF[:] = [float(np.median([d.confidence for dets in out for d in dets]))]
    return out


HIGH_CONF = []


def _tracker(ext, **kw):
    return HipTracker(max_dets=kw.pop("max_dets", 512), feature_dim=kw.pop("feature_dim", int(ext.feature_dim)), min_hits=1,
                      high_conf_threshold=HIGH_CONF[0] if HIGH_CONF else 0.5, **kw)


def _track_rows(t):
    return [bytes(r) for r in t._records()]


def _raw(lib, det, ext, frames, grid, slots, entry="opd_detr_detect_tiled_ragged_reid", features=True, trackers=None, struct_size=None, sizes=None):
    """One call of either Re-ID tiled entry through ctypes: (rc, merged records, counts, rows, slot_map, n_person, ids, n_featured)."""
    n, T, Q = len(frames), len(grid), det.num_queries
    S = T * Q
    h, w = frames[0].shape[:2]
    p = _capi.OpdTileParams(struct_size=C.sizeof(_capi.OpdTileParams), person_label=1, tile_nms_threshold=float(det.nms_threshold), merge_nms_threshold=0.4,
                            merge_threshold=0.5, edge_tolerance=0.01)
    out, counts = np.zeros((n, S), TILE_DET), np.full(n, -9, np.int32)
    win = np.asarray(grid, np.int32).reshape(-1, 4)
    ptrs = (C.c_void_p * n)(*[f.ctypes.data for f in frames])
    E, size = int(ext.feature_dim), max(slots, 1)
    rows, slot_map, n_person = np.full((size, E), -3.0, np.float32), np.full(size, -5, np.int32), np.full(1, -5, np.int32)
    st = _capi.OpdTileReidStages(struct_size=C.sizeof(_capi.OpdTileReidStages) if struct_size is None else struct_size, slots=slots, reid=ext._handle.value,
                                 slot_map=slot_map.ctypes.data, n_person=n_person.ctypes.data)
    if features:
        st.features = rows.ctypes.data
    ids = n_featured = keep = None
    if trackers is not None:
        keep = (C.c_void_p * len(trackers))(*[t._h.value if t is not None else None for t in trackers])
        ids, n_featured = np.full(n * S, -1, np.int32), np.full(n, -9, np.int32)
        st.trackers, st.track_ids, st.n_featured = C.addressof(keep), ids.ctypes.data, n_featured.ctypes.data
    tile_hw = np.asarray(det.tile_model_sizes(grid) if sizes is None else sizes, np.int32).reshape(T, 2)
    if entry == "opd_detr_detect_tiled_reid":
        H, W = model_input_size(grid[0][2], grid[0][3], det.max_size[0], det.max_size[1])
        size_args = (H, W)
    else:
        size_args = (tile_hw.ctypes.data_as(C.c_void_p),)
    rc = getattr(lib, entry)(C.c_void_p(det.model), ptrs, n, h, w, win.ctypes.data_as(C.c_void_p), T, *size_args, THRESHOLD, C.byref(p), C.byref(st),
                             out.ctypes.data_as(C.POINTER(_capi.OpdTileDet)), counts.ctypes.data_as(C.POINTER(C.c_int32)))
    return rc, out, counts, rows, slot_map, n_person, ids, n_featured


def test_the_grids_are_mixed_and_the_reference_has_records(reference):
    assert len({(t[2], t[3]) for t in ODD}) > 1 and len({(t[2], t[3]) for t in STRIP}) > 1 and len({(t[2], t[3]) for t in EVEN}) == 1
    assert all(len(w) >= 2 for w in reference), [len(w) for w in reference]
    assert all(d.features is not None and d.floor_coords is not None for w in reference for d in w)


def test_slots_rows_and_slot_list_of_a_two_frame_call(lib, sharp, ext, odd_frames, reference):
    """The C-ABI call itself at slots below, at and above the person count on two frames: the slot list in (frame, position) order, rows bit for bit
    the standalone rows."""
    cnts = [len(d) for d in reference[:2]]
    n, S = sum(cnts), len(ODD) * sharp.num_queries
    want_rows = np.concatenate([np.stack([d.features for d in dets]) for dets in reference[:2]])
    keys = [f * S + k for f in range(2) for k in range(cnts[f])]
    for slots in (1, n - 1, n, n + 3):
        rc, out, counts, rows, slot_map, n_person, *_ = _raw(lib, sharp, ext, odd_frames[:2], ODD, slots)
        assert rc == _capi.OPD_OK, _capi.last_error()
        filled = min(n, slots)
        assert counts.tolist() == cnts and int(n_person[0]) == n
        assert slot_map[:filled].tolist() == keys[:filled] and (slot_map[filled:] == -5).all()
        assert rows[:filled].tobytes() == want_rows[:filled].tobytes() and (rows[filled:] == -3.0).all(), f"slots = {slots}"
        for f in range(2):
            assert [(r["x"], r["y"], r["w"], r["h"]) for r in out[f, :cnts[f]]] == [d.bbox for d in reference[f]]


@pytest.mark.parametrize("n", [1, 3], ids=["one_frame", "three_frames_two_chunks"])
def test_fused_features_and_floor_equal_the_separate_calls(sharp, ext, odd_frames, mapper, reference, n):
    per = min(n, 2)
    first = sum(len(d) for d in reference[:per])   # the records of the first call (chunks of max_batch // 4 = 2 frames)
    plain = _separate(sharp, ext, odd_frames[:n], ODD)
    for target in (first - 1, first + 3):
        reid_slots = max(1, -(-target // per))
        got = sharp.detect_tiled_ragged_reid(odd_frames[:n], ODD, ext, reid_slots=reid_slots, floor_map=mapper)
        TS.same(got, reference[:n], f"fused against the separate calls, reid_slots = {reid_slots}")
        TS.same(sharp.detect_tiled_ragged_reid(odd_frames[:n], ODD, ext, reid_slots=reid_slots), plain, f"rows alone, reid_slots = {reid_slots}")


def test_a_1x3_strip_equals_the_separate_calls(sharp, ext):
    frames = _frames(STRIP_HW)[:2]
    want = _separate(sharp, ext, frames, STRIP)
    assert all(len(w) >= 1 for w in want)
    TS.same(sharp.detect_tiled_ragged_reid(frames, STRIP, ext, reid_slots=16), want, "1 x 3 strip, two frames in one call")


def test_fused_tracking_equals_the_separate_calls_with_a_record_beyond_the_slots(lib, sharp, ext, odd_frames, reference):
    fused, twin = _tracker(ext), _tracker(ext)
    try:
        for k, f in enumerate(odd_frames):   # three consecutive calls on one tracker; on the odd ones the last record gets no slot
            n = len(reference[k])
            slots = n - (k % 2)
            got = sharp.detect_tiled_ragged_reid([f], ODD, ext, reid_slots=slots, trackers=[fused])[0]
            want = _separate(sharp, ext, [f], ODD)[0]
            for d in want[slots:]:
                d.features = None   # a record beyond the slots enters the tracker without a feature
            twin.update(want)
            assert [d.track_id for d in got] == [d.track_id for d in want], f"ids of frame {k}"
            assert any(d.track_id is not None for d in got) and all(d.features is None for d in got)
            TS.same([got], [want], f"frame {k}", skip_features=True)
            assert _track_rows(fused) == _track_rows(twin), f"track rows after frame {k}"
        # n_featured of the C-ABI call itself
        raw = _tracker(ext)
        raw._ensure()
        n = len(reference[0])
        try:
            for slots, featured in ((n - 1, n - 1), (n + 3, n)):
                rc, _, counts, rows, slot_map, n_person, ids, n_featured = _raw(lib, sharp, ext, odd_frames[:1], ODD, slots, features=False, trackers=[raw])
                assert rc == _capi.OPD_OK, _capi.last_error()
                assert n_featured.tolist() == [featured] and int(n_person[0]) == n and (rows == -3.0).all()
        finally:
            raw.close()
    finally:
        fused.close()
        twin.close()


def test_a_grid_of_one_size_equals_the_uniform_entry_byte_for_byte(lib, sharp, ext):
    frames = _frames(EVEN_HW)[:2]
    for slots in (3, 40):
        a = _raw(lib, sharp, ext, frames, EVEN, slots, entry="opd_detr_detect_tiled_reid")
        b = _raw(lib, sharp, ext, frames, EVEN, slots)
        assert a[0] == b[0] == _capi.OPD_OK, _capi.last_error()
        assert a[2].tolist() == b[2].tolist() and min(a[2]) >= 2
        for x, y in zip(a[1:6], b[1:6]):   # records (decoy slots included), counts, rows, slot list, person count
            assert x.tobytes() == y.tobytes()


def test_refusals_with_handles(lib, sharp, ext, odd_frames, reference):
    S = len(ODD) * sharp.num_queries
    small, narrow, good = _tracker(ext, max_dets=S - 1), _tracker(ext, feature_dim=int(ext.feature_dim) // 2), _tracker(ext)
    for t in (small, narrow, good):
        t._ensure()

    def refused(text, slots=4, **kw):
        rc = _raw(lib, sharp, ext, kw.pop("fr", odd_frames[:1]), ODD, slots, **kw)[0]
        assert rc == _capi.OPD_EINVAL and text in _capi.last_error(), (text, _capi.last_error())
        assert _capi.last_error().startswith("opd_detr_detect_tiled_ragged_reid:")

    try:
        refused("struct_size", struct_size=56)
        refused("slots = 65 outside 1 .. max_crops = 64", slots=MAX_CROPS + 1)
        refused("features is null while no trackers are given", features=False)
        refused("trackers[0] was made for max_dets", trackers=[small])
        refused("trackers[0] was made for feature_dim", trackers=[narrow])
        refused("trackers[1] is trackers[0] too", fr=odd_frames[:2], trackers=[good, good])
        refused("3 frames x 4 tiles", fr=odd_frames[:3])
        rc = _raw(lib, sharp, ext, odd_frames[:1], ODD, 4, sizes=[(400, 400)] * 4)[0]   # a canvas the handle was not made for (worded by the shape check all entries share)
        assert rc == _capi.OPD_EINVAL and "outside the configured maximum" in _capi.last_error(), _capi.last_error()
        info = _capi.OpdTrackStatus()
        assert lib.opd_track_info(good._h, C.byref(info)) == 0 and info.n_tracks == 0 and info.last_launches == 0   # no refused call reached a tracker
        TS.same(sharp.detect_tiled_ragged_reid(odd_frames[:1], ODD, ext), _separate(sharp, ext, odd_frames[:1], ODD), "after the refusals")
        with pytest.raises(ValueError, match="None or 'color'"):
            sharp.detect_tiled_ragged(odd_frames[:1], ODD, features="reid")
    finally:
        for t in (small, narrow, good):
            t.close()


def test_tiled_detector_forwards_reid_on_a_mixed_grid(sharp, ext, odd_frames, reference, monkeypatch):
    calls = []
    real = sharp.detect_tiled_ragged_reid
    monkeypatch.setattr(sharp, "detect_tiled_ragged_reid", lambda *a, **kw: (calls.append(kw), real(*a, **kw))[1])
    td = TiledDetector(sharp, native=True, mixed_sizes=True)
    dets, rows = td.detect_with_features(odd_frames[0], features="reid", reid=ext, reid_slots=2)
    TS.same([dets], _separate(sharp, ext, odd_frames[:1], ODD), "detect_with_features")
    assert rows.tobytes() == np.stack([d.features for d in reference[0]]).tobytes()
    fused, twin = _tracker(ext), _tracker(ext)
    try:
        got = td.detect_and_track(odd_frames[0], fused, features="reid", reid=ext)
        want = twin.update(_separate(sharp, ext, odd_frames[:1], ODD)[0])
        TS.same([got], [want], "detect_and_track", skip_features=True)
        assert _track_rows(fused) == _track_rows(twin)
    finally:
        fused.close()
        twin.close()
    assert calls == [{"reid_slots": 2}, {"reid_slots": 32, "trackers": [fused]}]
    # where the fused conditions fail (no room in the tracker) the separate calls give the same lists
    small, small_twin = _tracker(ext, max_dets=128), _tracker(ext, max_dets=128)
    try:
        got = sharp.detect_tiled_ragged_reid(odd_frames[:1], ODD, ext, trackers=[small])
        want = _separate(sharp, ext, odd_frames[:1], ODD)
        small_twin.update(want[0])
        TS.same(got, want, "fallback")
        assert _track_rows(small) == _track_rows(small_twin)
    finally:
        small.close()
        small_twin.close()
