"""GPU tests of the Re-ID stage of a tiled call (-m gpu; ``opd_detr_detect_tiled_reid``, ``HipDetrDetector.detect_tiled_reid``,
``TiledDetector(native=True)`` with ``features="reid"``): the merged-record readers of the two crop kernels and the rows-by-slot reader of the merged
ingest on hand-made records against the public standalone calls, the fused call end to end against ``detect_tiled`` + ``reid.extract_features`` +
``floor_map.apply`` + ``tracker.update`` on the same handles, the handles afterwards, the refusals that need handles and the Python fallbacks.
Everything here is an equality."""

import ctypes as C
import faulthandler

import numpy as np
import pytest

import crop_plan_common as CP
import tile_stages_common as TS
from office_person_detection_vit_amd import HipDetrDetector, HipFloorMapper, HipOSNetReIDExtractor, HipReIDExtractor, HipTracker, TiledDetector, _capi
from office_person_detection_vit_amd.detector import model_input_size
from office_person_detection_vit_amd.frames import structured_frames
from office_person_detection_vit_amd.tiling import tile_grid
from office_person_detection_vit_amd.weights import DetrArch, ensure_clip_weight_file, ensure_osnet_weight_file, ensure_weight_file
from tile_common import TILE_DET

pytestmark = pytest.mark.gpu

THRESHOLD = 0.05
FRAME_HW = (192, 256)
SEEDS = (5, 6, 7)
GRID = tile_grid(192, 256, 2, 2, 0.125)
MAX_CROPS = 64
FM = (1878, 1369, 28.1926406926406, 28.241430700447)
ZONES = [{"id": "zone_1", "polygon": [[859, 912], [1095, 912], [1095, 1350], [859, 1350]], "priority": 1},
         {"id": "zone_2", "polygon": [[1095, 912], [1331, 912], [1331, 1350], [1095, 1350]], "priority": 2},
         {"id": "zone_3", "polygon": [[1331, 912], [1567, 912], [1567, 1350], [1331, 1350]], "priority": 3}]


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


@pytest.fixture(scope="module", params=["osnet", "clip"])
def ext(request, weight_cache, lib):
    if request.param == "clip":
        e = HipReIDExtractor(model_path=ensure_clip_weight_file(weight_cache, "tiny"), max_crops=MAX_CROPS)
    else:
        e = HipOSNetReIDExtractor(model_path=ensure_osnet_weight_file(weight_cache, "half"), max_crops=MAX_CROPS)
    e.load_model()
    e.spec = request.param
    yield e
    e.cleanup()


@pytest.fixture(scope="module")
def mapper(lib):
    h, w = FRAME_HW
    rng = np.random.default_rng(9)
    src = np.concatenate([np.array([[0, 0], [w, 0], [0, h], [w, h]], float), rng.uniform((10, 10), (w - 10, h - 10), (20, 2))])
    dst = np.stack([5.5 * src[:, 0] + 40 + 15 * np.sin(src[:, 1] / 40.0), 7.0 * src[:, 1] + 30 + 10 * np.cos(src[:, 0] / 50.0)], 1)
    m = HipFloorMapper.piecewise_affine(src, dst, FM, ZONES, device=0)
    yield m
    m.close()


@pytest.fixture(scope="module")
def frames():
    return [np.ascontiguousarray(structured_frames(1, FRAME_HW[0], FRAME_HW[1], seed=s)[0]).copy() for s in SEEDS]


def _separate(det, ext, frames, floor_map=None):
    """The separate calls on the same handles: detect_tiled, then reid.extract_features and floor_map.apply per frame."""
    out = det.detect_tiled(frames, GRID)
    for f, dets in zip(frames, out):
        for d, row in zip(dets, ext.extract_features(f, [d.bbox for d in dets])):
            d.features = row
        if floor_map is not None:
            floor_map.apply(dets)
    return out


@pytest.fixture(scope="module")
def reference(sharp, ext, frames, mapper):
    """The separate calls, once per model: per frame the detections with Re-ID rows and floor fields."""
    out = _separate(sharp, ext, frames, mapper)
    HIGH_CONF[:] = [float(np.median([d.confidence for dets in out for d in dets]))]
    return out


HIGH_CONF = []   # the median score of the reference records (set by `reference`): both stages of the association see records


def _tracker(ext, **kw):
    return HipTracker(max_dets=kw.pop("max_dets", 512), feature_dim=kw.pop("feature_dim", int(ext.feature_dim)), min_hits=1,
                      high_conf_threshold=HIGH_CONF[0] if HIGH_CONF else 0.5, **kw)


def _track_rows(t):
    return [bytes(r) for r in t._records()]


def _counts(reference, n):
    return [len(d) for d in reference[:n]]


# ---- 1. the stage kernels on hand-made merged records ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hand_rows(ext):
    """The standalone rows of every hand-made box on both hand-made frames, once per model: rows[f][j] of TS.BOXES[j] on frame f."""
    fr = TS.frames()
    rows = ext.extract_features_batch([fr[0], fr[1]], [TS.BOXES, TS.BOXES])
    return rows.reshape(2, len(TS.BOXES), -1)


@pytest.mark.parametrize("slots", [1, 4, 8, 11])
@pytest.mark.parametrize("counts", TS.RUNS, ids=["counts_5_0", "counts_8_3"])
def test_stage_kernels_equal_the_standalone_calls(lib, ext, hand_rows, counts, slots):
    h, w = TS.FRAME_HW
    S, E = TS.S, int(ext.feature_dim)
    frames = TS.frames()
    variants = [TS.merged(counts)]
    if slots == 4:   # a record of another label inside the count: no slot, no row, and it still enters the staging image
        other = TS.merged(counts)
        other[0, 1]["label"] = 0
        variants.append(other)
    for recs in variants:
        persons = [f * S + k for f in range(2) for k in range(counts[f]) if recs[f, k]["label"] == 1]
        slot_map, rec, n_person = np.full(slots, -5, np.int32), np.full(slots, -5, np.int32), np.full(1, -5, np.int32)
        geom, rows = np.full((slots, 13), -7, np.int32), np.full((slots, E), -3.0, np.float32)
        boxes, foot = np.full((2, S, 4), -3.0, np.float32), np.full((2, S, 2), -3.0, np.float32)
        has, feat, n_out = np.full((2, S), 7, np.uint8), np.full((2, S, E), -3.0, np.float32), np.full(2, -9, np.int32)
        cnt = np.asarray(counts, np.int32)
        rc = lib.opd_test_tile_reid(0, ext._handle, frames.ctypes.data, 2, h, w, recs.ctypes.data, cnt.ctypes.data, S, slots, slot_map.ctypes.data, rec.ctypes.data,
                                    n_person.ctypes.data, geom.ctypes.data, rows.ctypes.data, boxes.ctypes.data, foot.ctypes.data, has.ctypes.data, feat.ctypes.data,
                                    n_out.ctypes.data)
        assert rc == _capi.OPD_OK, _capi.last_error()
        filled = min(len(persons), slots)
        assert int(n_person[0]) == len(persons) and (len(persons) == sum(counts) or recs is not variants[0])
        assert slot_map[:filled].tolist() == persons[:filled] and rec[:filled].tolist() == persons[:filled]
        # nothing is written behind min(n_person, slots)
        assert (slot_map[filled:] == -5).all() and (rec[filled:] == -5).all() and (geom[filled:] == -7).all() and (rows[filled:] == -3.0).all()
        assert n_out.tolist() == list(counts)
        # the plan and the rows of the selected records: the float32 box of each, on its frame
        flat = recs.reshape(-1)
        sel = [flat[p] for p in persons[:filled]]
        b32 = np.asarray([(r["x"], r["y"], r["w"], r["h"]) for r in sel], np.float32).reshape(-1, 4)
        if filled:
            assert geom[:filled].tobytes() == CP.plan(lib, "host", ext.spec, b32, h, w)["geom"].tobytes(), "geometry words"
            order = [range(len(TS.BOXES)), range(len(TS.BOXES) - 1, -1, -1)]   # frame 1 holds BOXES reversed
            want_rows = np.stack([hand_rows[p // S, order[p // S][p % S]] for p in persons[:filled]])
            assert rows[:filled].tobytes() == want_rows.tobytes(), "rows against extract_features_batch on the same handle"
        row_of = {p: k for k, p in enumerate(persons[:filled])}
        for f in range(2):
            n = counts[f]
            _, want_b, want_foot, conf = TS.host_arrays(recs[f], n)
            assert conf.tobytes() == np.ascontiguousarray(recs[f, :n]["score"]).tobytes()
            assert (boxes[f, n:] == -3.0).all() and (foot[f, n:] == -3.0).all() and (has[f, n:] == 7).all() and (feat[f, n:] == -3.0).all()
            assert boxes[f, :n].tobytes() == want_b.tobytes(), f"staged boxes of frame {f}"
            assert foot[f, :n].tobytes() == want_foot.tobytes(), f"staged foot points of frame {f}"
            assert has[f, :n].tolist() == [int(f * S + k in row_of) for k in range(n)], f"has of frame {f}"
            for k in range(n):
                if f * S + k in row_of:
                    assert feat[f, k].tobytes() == rows[row_of[f * S + k]].tobytes(), f"staged row of record {k} of frame {f}"
                else:
                    assert (feat[f, k] == -3.0).all()


# ---- 2. end to end ---------------------------------------------------------------------------------------------------------------------------
def _raw(lib, det, ext, frames, slots, features=True, floor_map=None, trackers=None, struct_size=None):
    """One opd_detr_detect_tiled_reid call through ctypes: (rc, per-frame merged records, rows, slot_map, n_person, floor, ids, n_featured)."""
    n, T, Q = len(frames), len(GRID), det.num_queries
    S = T * Q
    th, tw = GRID[0][2], GRID[0][3]
    H, W = model_input_size(th, tw, det.max_size[0], det.max_size[1])
    p = _capi.OpdTileParams(struct_size=C.sizeof(_capi.OpdTileParams), person_label=1, tile_nms_threshold=float(det.nms_threshold), merge_nms_threshold=0.4,
                            merge_threshold=0.5, edge_tolerance=0.01)
    out, counts = np.zeros((n, S), TILE_DET), np.full(n, -9, np.int32)
    win = np.asarray(GRID, np.int32).reshape(-1, 4)
    ptrs = (C.c_void_p * n)(*[f.ctypes.data for f in frames])
    E = int(ext.feature_dim)
    size = max(slots, 1)
    rows, slot_map, n_person = np.full((size, E), -3.0, np.float32), np.full(size, -5, np.int32), np.full(1, -5, np.int32)
    st = _capi.OpdTileReidStages(struct_size=C.sizeof(_capi.OpdTileReidStages) if struct_size is None else struct_size, slots=slots, reid=ext._handle.value,
                                 slot_map=slot_map.ctypes.data, n_person=n_person.ctypes.data)
    if features:
        st.features = rows.ctypes.data
    floor = ids = n_featured = keep = None
    if floor_map is not None:
        floor = np.zeros(n * S, floor_map.REC_DTYPE)
        st.floor, st.floor_out = floor_map._require().value, floor.ctypes.data
    if trackers is not None:
        keep = (C.c_void_p * len(trackers))(*[t._h.value if t is not None else None for t in trackers])
        ids, n_featured = np.full(n * S, -1, np.int32), np.full(n, -9, np.int32)
        st.trackers, st.track_ids, st.n_featured = C.addressof(keep), ids.ctypes.data, n_featured.ctypes.data
    rc = lib.opd_detr_detect_tiled_reid(C.c_void_p(det.model), ptrs, n, FRAME_HW[0], FRAME_HW[1], win.ctypes.data_as(C.c_void_p), T, H, W, THRESHOLD, C.byref(p), C.byref(st),
                                        out.ctypes.data_as(C.POINTER(_capi.OpdTileDet)), counts.ctypes.data_as(C.POINTER(C.c_int32)))
    return rc, out, counts, rows, slot_map, n_person, floor, ids, n_featured


def test_the_reference_lists_have_records(sharp, ext, frames, reference):
    assert all(len(w) > 0 for w in reference) and sum(_counts(reference, 2)) >= 3, [len(w) for w in reference]
    assert all(d.features is not None and d.floor_coords is not None for w in reference for d in w)


def test_slots_rows_and_slot_list_of_a_two_frame_call(lib, sharp, ext, frames, reference):
    """The C-ABI call itself at slots = 1, n - 1, n, n + 3 on two frames: the slot list in (frame, position) order, rows bit for bit the standalone rows."""
    cnts = _counts(reference, 2)
    n, S = sum(cnts), len(GRID) * sharp.num_queries
    assert n >= 3
    want_rows = np.concatenate([np.stack([d.features for d in dets]) for dets in reference[:2]])
    keys = [f * S + k for f in range(2) for k in range(cnts[f])]
    for slots in (1, n - 1, n, n + 3):
        rc, out, counts, rows, slot_map, n_person, *_ = _raw(lib, sharp, ext, frames[:2], slots)
        assert rc == _capi.OPD_OK, _capi.last_error()
        filled = min(n, slots)
        assert counts.tolist() == cnts and int(n_person[0]) == n
        assert slot_map[:filled].tolist() == keys[:filled] and (slot_map[filled:] == -5).all()
        assert rows[:filled].tobytes() == want_rows[:filled].tobytes() and (rows[filled:] == -3.0).all(), f"slots = {slots}"
        for f in range(2):
            assert [(r["x"], r["y"], r["w"], r["h"]) for r in out[f, :cnts[f]]] == [d.bbox for d in reference[f]]


@pytest.mark.parametrize("n", [1, 2, 3], ids=["one_frame", "two_frames_one_call", "three_frames_two_chunks"])
def test_fused_features_and_floor_equal_the_separate_calls(sharp, ext, frames, mapper, reference, n):
    first = sum(_counts(reference, min(n, 2)))   # the records of the first call (chunks of max_batch // 4 = 2 frames)
    per = min(n, 2)
    plain = _separate(sharp, ext, frames[:n])
    for target in (1, first - 1, first, first + 3):
        reid_slots = max(1, -(-target // per))   # the call's slots: reid_slots x the frames of the chunk
        got = sharp.detect_tiled_reid(frames[:n], GRID, ext, reid_slots=reid_slots, floor_map=mapper)
        TS.same(got, reference[:n], f"fused against the separate calls, reid_slots = {reid_slots}")
        TS.same(sharp.detect_tiled_reid(frames[:n], GRID, ext, reid_slots=reid_slots), plain, f"rows alone, reid_slots = {reid_slots}")


def test_fused_tracking_equals_the_separate_calls(lib, sharp, ext, frames, reference):
    fused, twin = _tracker(ext), _tracker(ext)
    try:
        for k, f in enumerate(frames):   # three consecutive calls on one tracker
            got = sharp.detect_tiled_reid([f], GRID, ext, reid_slots=len(reference[k]) + (k % 2), trackers=[fused])[0]
            want = _separate(sharp, ext, [f])[0]
            twin.update(want)
            assert [d.track_id for d in got] == [d.track_id for d in want], f"ids of frame {k}"
            assert any(d.track_id is not None for d in got)
            TS.same([got], [want], f"frame {k}", skip_features=True)
            assert all(d.features is None for d in got)
            assert _track_rows(fused) == _track_rows(twin), f"track rows after frame {k}"
            assert [(t.track_id, t.age, t.hits, t.time_since_update) for t in fused.tracks] == [(t.track_id, t.age, t.hits, t.time_since_update) for t in twin.tracks]
    finally:
        fused.close()
        twin.close()


def test_a_record_beyond_the_slots_enters_without_a_feature(lib, sharp, ext, frames, reference):
    n = len(reference[0])
    assert n >= 2
    fused, twin, raw, raw_twin = _tracker(ext), _tracker(ext), _tracker(ext), _tracker(ext)
    try:
        for k in range(2):   # the second call matches against tracks of which the last never got a row
            got = sharp.detect_tiled_reid(frames[:1], GRID, ext, reid_slots=n - 1, trackers=[fused])[0]
            want = _separate(sharp, ext, frames[:1])[0]
            want[-1].features = None
            twin.update(want)
            TS.same([got], [[d for d in want]], f"call {k}", skip_features=True)
            assert _track_rows(fused) == _track_rows(twin), f"track rows after call {k}"
        # n_featured and the slot list of the C-ABI call itself; with `features` NULL no row leaves the device
        for t in (raw, raw_twin):
            t._ensure()
        for slots, featured in ((n - 1, n - 1), (n + 3, n)):
            rc, out, counts, rows, slot_map, n_person, _, ids, n_featured = _raw(lib, sharp, ext, frames[:1], slots, features=False, trackers=[raw])
            assert rc == _capi.OPD_OK, _capi.last_error()
            assert n_featured.tolist() == [featured] and int(n_person[0]) == n and slot_map[:featured].tolist() == list(range(featured))
            assert (rows == -3.0).all() and (slot_map[featured:] == -5).all()
            want = _separate(sharp, ext, frames[:1])[0]
            for d in want[featured:]:
                d.features = None
            raw_twin.update(want)
            assert ids[:n].tolist() == [-1 if d.track_id is None else d.track_id for d in want] and _track_rows(raw) == _track_rows(raw_twin)
    finally:
        for t in (fused, twin, raw, raw_twin):
            t.close()


def test_two_frames_with_two_trackers_equal_two_single_frame_calls(sharp, ext, frames, mapper, reference):
    a, b, a1, b1 = (_tracker(ext) for _ in range(4))
    try:
        for pair in (frames[:2], frames[1:]):
            both = sharp.detect_tiled_reid(pair, GRID, ext, floor_map=mapper, trackers=[a, b])
            one = [sharp.detect_tiled_reid([pair[0]], GRID, ext, floor_map=mapper, trackers=[a1])[0],
                   sharp.detect_tiled_reid([pair[1]], GRID, ext, floor_map=mapper, trackers=[b1])[0]]
            TS.same(both, one, "two trackers in one call")
            assert any(d.track_id is not None for dets in both for d in dets)
            assert _track_rows(a) == _track_rows(a1) and _track_rows(b) == _track_rows(b1)
    finally:
        for t in (a, b, a1, b1):
            t.close()


def test_tiled_detector_forwards_to_the_fused_call(sharp, ext, frames, reference, monkeypatch):
    calls = []
    real = sharp.detect_tiled_reid
    monkeypatch.setattr(sharp, "detect_tiled_reid", lambda *a, **kw: (calls.append(kw), real(*a, **kw))[1])
    td = TiledDetector(sharp, native=True)
    dets, rows = td.detect_with_features(frames[0], features="reid", reid=ext, reid_slots=2)
    TS.same([dets], _separate(sharp, ext, frames[:1]), "detect_with_features")
    assert rows.tobytes() == np.stack([d.features for d in reference[0]]).tobytes()
    fused, twin = _tracker(ext), _tracker(ext)
    try:
        got = td.detect_and_track(frames[0], fused, features="reid", reid=ext)
        want = twin.update(_separate(sharp, ext, frames[:1])[0])
        TS.same([got], [want], "detect_and_track", skip_features=True)
        assert _track_rows(fused) == _track_rows(twin)
    finally:
        fused.close()
        twin.close()
    assert calls == [{"reid_slots": 2}, {"reid_slots": 32, "trackers": [fused]}]


# ---- 3. the handles afterwards ---------------------------------------------------------------------------------------------------------------
def test_a_tiled_reid_call_leaves_the_handles_as_they_were(sharp, ext, frames, mapper, reference):
    small = np.ascontiguousarray(structured_frames(1, 192, 256, seed=11)[0]).copy()

    def plain():
        dets, rows = sharp.detect_with_features(small, features="reid", reid=ext)
        boxes = [d.bbox for d in reference[0]]
        return ([TS.fields(d) for d in sharp.detect_tiled(frames[:2], GRID)[1]], [[TS.fields(d) for d in w] for w in sharp.detect_batch([small, frames[0]])],
                [TS.fields(d) for d in dets], rows.tobytes(), ext.extract_features(frames[0], boxes).tobytes())

    def tiled(t):
        return ([[TS.fields(d) for d in w] for w in sharp.detect_tiled_reid(frames[:2], GRID, ext, reid_slots=2, floor_map=mapper)],
                [TS.fields(d) for d in sharp.detect_tiled_reid(frames[:1], GRID, ext, trackers=[t])[0]], _track_rows(t))

    trackers = [_tracker(ext) for _ in range(2)]
    try:
        before = plain()
        tiled_before = tiled(trackers[0])
        after = plain()
        tiled_after = tiled(trackers[1])
        assert len(before[0]) > 0 and len(before[2]) > 0 and len(tiled_before[0][0]) > 0
        assert after == before, "detect_tiled / detect_batch / detect_with_features / extract_features after a tiled Re-ID call"
        assert tiled_after == tiled_before, "a tiled Re-ID call after the plain calls"
    finally:
        for t in trackers:
            t.close()


# ---- 4. refusals that need handles, and the Python fallbacks ---------------------------------------------------------------------------------
def test_refusals_with_handles(lib, sharp, ext, frames, reference):
    S = len(GRID) * sharp.num_queries
    small, narrow, good = _tracker(ext, max_dets=S - 1), _tracker(ext, feature_dim=int(ext.feature_dim) // 2), _tracker(ext)
    for t in (small, narrow, good):
        t._ensure()
    before = ext.extract_features(frames[0], [d.bbox for d in reference[0]]).tobytes()

    def refused(text, slots=4, **kw):
        rc = _raw(lib, sharp, ext, kw.pop("fr", frames[:1]), slots, **kw)[0]
        assert rc == _capi.OPD_EINVAL and text in _capi.last_error(), (text, _capi.last_error())
        assert _capi.last_error().startswith("opd_detr_detect_tiled_reid:")

    try:
        refused("struct_size", struct_size=56)
        refused("slots = 65 outside 1 .. max_crops = 64", slots=MAX_CROPS + 1)
        refused("slots = 0 outside 1 .. max_crops = 64", slots=0)
        refused("features is null while no trackers are given", features=False)
        refused("trackers[0] was made for max_dets", trackers=[small])
        refused(f"trackers[0] was made for feature_dim = {int(ext.feature_dim) // 2}, the rows of the Re-ID model have {int(ext.feature_dim)}", trackers=[narrow])
        refused("trackers[1] is trackers[0] too", fr=frames[:2], trackers=[good, good])
        refused("trackers[0] is null", trackers=[None])
        refused("3 frames x 4 tiles", fr=frames[:3])
        info = _capi.OpdTrackStatus()
        assert lib.opd_track_info(good._h, C.byref(info)) == 0 and info.n_tracks == 0 and info.last_launches == 0   # no refused call reached a tracker
        # the handles stay usable
        assert ext.extract_features(frames[0], [d.bbox for d in reference[0]]).tobytes() == before
        TS.same(sharp.detect_tiled_reid(frames[:1], GRID, ext), _separate(sharp, ext, frames[:1]), "after the refusals")
    finally:
        for t in (small, narrow, good):
            t.close()


def test_python_fallbacks_equal_the_fused_path(sharp, ext, frames, mapper, reference, monkeypatch):
    S = len(GRID) * sharp.num_queries
    fused_t = _tracker(ext)
    try:
        fused = sharp.detect_tiled_reid(frames[:1], GRID, ext, floor_map=mapper, trackers=[fused_t])
        rows = _track_rows(fused_t)
    finally:
        fused_t.close()
    calls = []

    class Spy:   # the library with the fused entry counted
        def __getattr__(self, name):
            if name == "opd_detr_detect_tiled_reid":
                calls.append(name)
            return getattr(sharp_lib, name)

    sharp_lib = sharp._lib
    monkeypatch.setattr(sharp, "_lib", Spy())

    def fallback(what, prepare=lambda t: None, with_tracker=True, **kw):
        t = _tracker(ext, **kw)
        try:
            del calls[:]
            prepare(t)
            got = sharp.detect_tiled_reid(frames[:1], GRID, ext, floor_map=mapper, trackers=[t] if with_tracker else None)
            assert calls == [], f"{what}: the fused entry was called"
            if with_tracker:
                TS.same(got, fused, what, skip_features=True)
                assert _track_rows(t) == rows, what
            else:
                TS.same(got, reference[:1], what)
        finally:
            t.close()

    fallback("max_dets < S", max_dets=S - 1)

    def elsewhere(t):   # (seen by the condition only: made on the detector's GPU, the separate update runs there)
        t.device_ordinal = sharp.device_ordinal + 1
        monkeypatch.setattr(t, "_ensure", lambda real=t._ensure: (setattr(t, "device_ordinal", sharp.device_ordinal), real()))

    fallback("a tracker on another GPU", prepare=elsewhere)
    with monkeypatch.context() as mp:
        mp.setattr(ext, "_ordinal", lambda: sharp.device_ordinal + 1)
        fallback("the Re-ID model on another GPU")
        fallback("the Re-ID model on another GPU, rows to the caller", with_tracker=False)
    with monkeypatch.context() as mp:
        mp.setattr(mapper, "device", int(mapper.device) + 1)
        fallback("a floor map on another GPU")

    class HostOnly:   # an extractor without a native handle: the separate calls
        feature_dim, max_crops, is_loaded = ext.feature_dim, ext.max_crops, True

        def extract_features(self, frame, bboxes):
            return ext.extract_features(frame, bboxes)

    del calls[:]
    TS.same(sharp.detect_tiled_reid(frames[:1], GRID, HostOnly(), floor_map=mapper), reference[:1], "no native handle")
    assert calls == []
    # a wrong feature_dim: the separate update refuses the rows, as it does without tiling
    narrow = _tracker(ext, feature_dim=int(ext.feature_dim) // 2)
    try:
        with pytest.raises(ValueError, match="feature of width"):
            sharp.detect_tiled_reid(frames[:1], GRID, ext, trackers=[narrow])
        assert calls == []
    finally:
        narrow.close()
    sharp.detect_tiled_reid(frames[:1], GRID, ext)
    assert calls == ["opd_detr_detect_tiled_reid"]
