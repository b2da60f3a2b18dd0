"""GPU tests of the feature, floor and track stages of a tiled call (-m gpu; ``opd_detr_detect_tiled_stages``,
``HipDetrDetector.detect_tiled_stages(features=, floor_map=, trackers=)``, ``TiledDetector(native=True)``'s new methods): the merged-record readers of
the three kernels on hand-made records against the public standalone calls, the fused call end to end against ``detect_tiled`` +
``extract_color_features`` + ``floor_map.apply`` + ``tracker.update`` on the same handle, the handle afterwards, the refusals that need a handle and
the Python fallbacks.  Everything here is an equality."""

import ctypes as C
import faulthandler

import numpy as np
import pytest

import tile_stages_common as TS
from office_person_detection_vit_amd import HipDetrDetector, HipFloorMapper, HipTracker, TiledDetector, _capi
from office_person_detection_vit_amd.frames import structured_frames
from office_person_detection_vit_amd.tiling import split_tiles, tile_grid
from office_person_detection_vit_amd.weights import DetrArch, ensure_weight_file

pytestmark = pytest.mark.gpu

THRESHOLD = 0.05
FRAME_HW = (192, 256)
SEEDS = (5, 6, 7)
GRID = tile_grid(192, 256, 2, 2, 0.125)
FM = (1878, 1369, 28.1926406926406, 28.241430700447)
ZONES = [{"id": "zone_1", "polygon": [[859, 912], [1095, 912], [1095, 1350], [859, 1350]], "priority": 1},
         {"id": "zone_2", "polygon": [[1095, 912], [1331, 912], [1331, 1350], [1095, 1350]], "priority": 2},
         {"id": "zone_3", "polygon": [[1331, 912], [1567, 912], [1567, 1350], [1331, 1350]], "priority": 3}]
H = [[-0.8795888447, -2.8974379541, 417.8510123786], [-1.5459702925, -3.4570021203, 1054.0107447082], [-0.0011928509, -0.0035480452, 1.0]]


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
    """tests/test_tile_gpu.py's `sharp` detector: the seeded weights with attention gain 2, on which the seam merge absorbs boxes."""
    d = _detector(weight_cache)
    yield d
    d.close()


def _pwa(hw, device=0):
    """A piecewise-affine map over an h x w camera frame onto the zones' floor map (tests/test_floor_gpu.py's construction)."""
    h, w = hw
    rng = np.random.default_rng(9)
    src = np.concatenate([np.array([[0, 0], [w, 0], [0, h], [w, h]], float), rng.uniform((10, 10), (w - 10, h - 10), (20, 2))])
    dst = np.stack([5.5 * src[:, 0] + 40 + 15 * np.sin(src[:, 1] / 40.0), 7.0 * src[:, 1] + 30 + 10 * np.cos(src[:, 0] / 50.0)], 1)
    return HipFloorMapper.piecewise_affine(src, dst, FM, ZONES, device=device)


@pytest.fixture(scope="module")
def mapper(lib):
    m = _pwa(FRAME_HW)
    yield m
    m.close()


@pytest.fixture(scope="module")
def frames():
    return [np.ascontiguousarray(structured_frames(1, FRAME_HW[0], FRAME_HW[1], seed=s)[0]).copy() for s in SEEDS]


def _separate(det, frames, features=None, floor_map=None):
    """The separate calls on the same handle: detect_tiled, then extract_color_features and floor_map.apply per frame."""
    out = det.detect_tiled(frames, GRID)
    for f, dets in zip(frames, out):
        if features == "color":
            for d, row in zip(dets, det.extract_color_features(f, dets)):
                d.features = row
        if floor_map is not None:
            floor_map.apply(dets)
    return out


@pytest.fixture(scope="module")
def reference(sharp, frames, mapper):
    """The separate calls, once: per frame the detections with colour rows and floor fields."""
    out = _separate(sharp, frames, "color", mapper)
    HIGH_CONF[:] = [float(np.median([d.confidence for dets in out for d in dets]))]
    return out


HIGH_CONF = []   # the median score of the reference records (set by `reference`): the high- and the low-confidence stages of the association both see records


def _tracker(**kw):
    return HipTracker(max_dets=kw.pop("max_dets", 512), feature_dim=kw.pop("feature_dim", 256), min_hits=1, high_conf_threshold=HIGH_CONF[0] if HIGH_CONF else 0.5, **kw)


def _track_rows(t):
    return [bytes(r) for r in t._records()]


# ---- 1. the stage kernels on hand-made merged records ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("counts", TS.RUNS, ids=["counts_5_0", "counts_8_3"])
@pytest.mark.parametrize("method", ["homography", "piecewise_affine"])
def test_stage_kernels_equal_the_standalone_calls(lib, counts, method):
    h, w = TS.FRAME_HW
    S = TS.S
    frames = TS.frames()
    recs = TS.merged(counts)
    fmap = HipFloorMapper.homography(H, FM, ZONES) if method == "homography" else _pwa(TS.FRAME_HW)
    try:
        for with_rows in (1, 0):
            color = np.full((2 * S, 256), -3.0, np.float32)
            floor = np.frombuffer(bytearray(b"\xa5" * (2 * S * 48)), HipFloorMapper.REC_DTYPE).copy()
            boxes, foot = np.full((2, S, 4), -3.0, np.float32), np.full((2, S, 2), -3.0, np.float32)
            has, feat, n_out = np.full((2, S), 7, np.uint8), np.full((2, S, 256), -3.0, np.float32), np.full(2, -9, np.int32)
            cnt = np.asarray(counts, np.int32)
            rc = lib.opd_test_tile_stages(0, frames.ctypes.data, 2, h, w, recs.ctypes.data, cnt.ctypes.data, S, fmap._require(), with_rows, color.ctypes.data,
                                          floor.ctypes.data, boxes.ctypes.data, foot.ctypes.data, has.ctypes.data, feat.ctypes.data, n_out.ctypes.data)
            assert rc == _capi.OPD_OK, _capi.last_error()
            assert n_out.tolist() == list(counts)
            for f in range(2):
                n = counts[f]
                bbox, b32, foot32, conf = TS.host_arrays(recs[f], n)
                assert conf.tobytes() == np.ascontiguousarray(recs[f, :n]["score"]).tobytes()
                # rows at and behind the count were not written by any stage
                assert (color[f * S + n:(f + 1) * S] == -3.0).all() and (boxes[f, n:] == -3.0).all() and (foot[f, n:] == -3.0).all() and (has[f, n:] == 7).all()
                assert floor[f * S + n:(f + 1) * S].tobytes() == b"\xa5" * ((S - n) * 48)
                if n == 0:
                    continue
                want_color = np.empty((n, 256), np.float32)
                ptrs, hw = (C.c_void_p * 1)(frames[f].ctypes.data), np.array([h, w], np.int32)
                rc = lib.opd_color_features(0, ptrs, hw.ctypes.data_as(C.c_void_p), 1, _capi.OPD_MEM_HOST, b32.ctypes.data_as(C.c_void_p), None, n,
                                            want_color.ctypes.data_as(C.c_void_p))
                assert rc == _capi.OPD_OK, _capi.last_error()
                assert color[f * S:f * S + n].tobytes() == want_color.tobytes(), f"colour rows of frame {f}"
                assert floor[f * S:f * S + n].tobytes() == fmap.transform_records(bbox).tobytes(), f"floor rows of frame {f} ({method})"
                assert boxes[f, :n].tobytes() == b32.tobytes(), f"staged boxes of frame {f}"
                assert foot[f, :n].tobytes() == foot32.tobytes(), f"staged foot points of frame {f}"
                assert has[f, :n].tolist() == [with_rows] * n
                if with_rows:
                    assert feat[f, :n].tobytes() == want_color.tobytes(), f"staged rows of frame {f}"
                else:
                    assert (feat[f] == -3.0).all()
    finally:
        fmap.close()


# ---- 2. end to end ---------------------------------------------------------------------------------------------------------------------------
def test_reference_lists_show_a_box_the_seam_merge_grew(sharp, frames, reference):
    per_tile = [sharp.detect_batch(split_tiles(f, 2, 2, 0.125)[0]) for f in frames]
    assert all(len(w) > 0 for w in reference)
    widest = max(d.bbox[2] for p in per_tile for t in p for d in t)
    assert any(d.bbox[2] > widest + 1.0 for w in reference for d in w), "no kept box has grown: the seam merge itself never happened"
    assert all(d.features is not None and d.floor_coords is not None for w in reference for d in w)


@pytest.mark.parametrize("n", [1, 2, 3], ids=["one_frame", "two_frames_one_call", "three_frames_two_chunks"])
def test_fused_features_and_floor_equal_the_separate_calls(sharp, frames, mapper, reference, n):
    got = sharp.detect_tiled_stages(frames[:n], GRID, features="color", floor_map=mapper)
    TS.same(got, reference[:n], "fused against the separate calls")
    TS.same(sharp.detect_tiled_stages(frames[:n], GRID, features="color"), _separate(sharp, frames[:n], "color"), "colour rows alone")
    TS.same(sharp.detect_tiled_stages(frames[:n], GRID, floor_map=mapper), _separate(sharp, frames[:n], None, mapper), "floor fields alone")


@pytest.mark.parametrize("features", ["color", None], ids=["colour_rows", "motion_only"])
def test_fused_tracking_equals_the_separate_calls(sharp, frames, reference, features):
    fused, twin = _tracker(), _tracker()
    try:
        for k, f in enumerate(frames + frames[:1]):
            got = sharp.detect_tiled_stages([f], GRID, features=features, trackers=[fused])[0]
            want = _separate(sharp, [f], features)[0]
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


def test_two_frames_with_two_trackers_equal_two_single_frame_calls(sharp, frames, mapper, reference):
    a, b, a1, b1 = _tracker(), _tracker(), _tracker(), _tracker()
    try:
        for pair in (frames[:2], frames[1:]):
            both = sharp.detect_tiled_stages(pair, GRID, features="color", floor_map=mapper, trackers=[a, b])
            one = [sharp.detect_tiled_stages([pair[0]], GRID, features="color", floor_map=mapper, trackers=[a1])[0],
                   sharp.detect_tiled_stages([pair[1]], GRID, features="color", floor_map=mapper, trackers=[b1])[0]]
            TS.same(both, one, "two trackers in one call")
            assert _track_rows(a) == _track_rows(a1) and _track_rows(b) == _track_rows(b1)
    finally:
        for t in (a, b, a1, b1):
            t.close()


def test_tiled_detector_forwards_to_the_fused_call(sharp, frames, mapper, reference):
    td = TiledDetector(sharp, native=True)
    TS.same(td.detect_batch(frames, floor_map=mapper), _separate(sharp, frames, None, mapper), "detect_batch(floor_map=)")
    TS.same([td.detect(frames[0], floor_map=mapper)], _separate(sharp, frames[:1], None, mapper), "detect(floor_map=)")
    dets, rows = td.detect_with_features(frames[0], features="color")
    TS.same([dets], _separate(sharp, frames[:1], "color"), "detect_with_features")
    assert rows.tobytes() == np.stack([d.features for d in reference[0]]).tobytes()
    fused, twin = _tracker(), _tracker()
    try:
        got = td.detect_and_track(frames[0], fused, features="color")
        want = twin.update(_separate(sharp, frames[:1], "color")[0])
        TS.same([got], [want], "detect_and_track", skip_features=True)
        assert _track_rows(fused) == _track_rows(twin)
    finally:
        fused.close()
        twin.close()
    with pytest.raises(ValueError, match="encoder"):
        td.detect_with_features(frames[0], features="encoder")
    with pytest.raises(ValueError, match="encoder"):
        sharp.detect_tiled_stages(frames[:1], GRID, features="encoder")
    # native=False: the host composition of the same calls
    host = TiledDetector(sharp, native=False)
    hd, hrows = host.detect_with_features(frames[0], features="color")
    want = host.detect(frames[0])
    assert hrows.tobytes() == sharp.extract_color_features(frames[0], want).tobytes() and [d.bbox for d in hd] == [d.bbox for d in want]


# ---- 3. the handle afterwards ----------------------------------------------------------------------------------------------------------------
def test_a_staged_tiled_call_leaves_the_handle_as_it_was(sharp, frames, mapper, reference):
    small = np.ascontiguousarray(structured_frames(1, 192, 256, seed=11)[0]).copy()
    sharp.device_nms = True
    trackers = [_tracker() for _ in range(4)]
    try:
        def plain(t):
            dets, rows = sharp.detect_with_features(small, features="color")
            tracked = sharp.detect_and_track(small, t, features="color")
            return [TS.fields(d) for d in dets], rows.tobytes(), [TS.fields(d) for d in tracked], _track_rows(t)

        def staged(t):
            return [TS.fields(d) for d in sharp.detect_tiled_stages(frames[:2], GRID, features="color", floor_map=mapper)[0]], \
                   [TS.fields(d) for d in sharp.detect_tiled_stages(frames[:1], GRID, features="color", trackers=[t])[0]], _track_rows(t)

        before = plain(trackers[0])
        tiled_before = staged(trackers[1])
        after = plain(trackers[2])
        tiled_after = staged(trackers[3])
        assert len(before[0]) > 0 and len(tiled_before[0]) > 0
        assert after == before, "detect_with_features / detect_and_track after a staged tiled call"
        assert tiled_after == tiled_before, "a staged tiled call after detect_with_features / detect_and_track"
    finally:
        sharp.device_nms = False
        for t in trackers:
            t.close()


@pytest.mark.parametrize("poison", [0x00, 0xFF], ids=["poison_00", "poison_ff"])
def test_a_staged_tiled_call_does_not_depend_on_memory_it_has_not_written(lib, weight_cache, frames, mapper, reference, poison):
    """The handle AND the buffers its first staged call allocates (colour sums, floor rows, merged records) are filled with the byte."""
    t, twin = _tracker(), _tracker()
    lib.opd_test_set_alloc_poison(poison)
    try:
        det = _detector(weight_cache)
        try:
            got = det.detect_tiled_stages(frames[:2], GRID, features="color", floor_map=mapper)
            tracked = det.detect_tiled_stages(frames[:1], GRID, features="color", trackers=[t])[0]
        finally:
            lib.opd_test_set_alloc_poison(-1)
        TS.same(got, reference[:2], f"poison {poison:#x}")
        want = _separate(det, frames[:1], "color")[0]
        twin.update(want)
        assert [d.track_id for d in tracked] == [d.track_id for d in want] and _track_rows(t) == _track_rows(twin)
        bad = lib.opd_test_check_redzones(C.c_void_p(det.model))
        assert bad == 0, f"{bad} buffers with a damaged red zone; first: {_capi.last_error()}"
        det.close()
    finally:
        lib.opd_test_set_alloc_poison(-1)
        t.close()
        twin.close()


# ---- 4. refusals that need a handle, and the Python fallbacks --------------------------------------------------------------------------------
def test_refusals_with_a_handle(lib, sharp, frames, mapper, reference):
    S = len(GRID) * sharp.num_queries
    p = _capi.OpdTileParams(struct_size=C.sizeof(_capi.OpdTileParams), person_label=1, tile_nms_threshold=0.4, merge_nms_threshold=0.4, merge_threshold=0.5,
                            edge_tolerance=0.01)
    out, counts = (_capi.OpdTileDet * S)(), (C.c_int32 * 1)()
    win = np.asarray(GRID, np.int32).reshape(-1, 4)
    ptrs = (C.c_void_p * 1)(frames[0].ctypes.data)
    ids, nf, floor = np.zeros(S, np.int32), np.zeros(1, np.int32), np.zeros(S, HipFloorMapper.REC_DTYPE)
    small, narrow, good = _tracker(max_dets=S - 1), _tracker(feature_dim=128), _tracker()
    for t in (small, narrow, good):
        t._ensure()

    def refused(text, n_frames=1, **kw):
        st = _capi.OpdTileStages(struct_size=kw.pop("struct_size", C.sizeof(_capi.OpdTileStages)), **kw)
        rc = lib.opd_detr_detect_tiled_stages(C.c_void_p(sharp.model), ptrs, n_frames, 192, 256, win.ctypes.data_as(C.c_void_p), 4, 240, 320, THRESHOLD, C.byref(p), C.byref(st),
                                              out, counts)
        assert rc == _capi.OPD_EINVAL and text in _capi.last_error(), (text, _capi.last_error())

    def handles(*ts):
        arr = (C.c_void_p * len(ts))(*[t._h.value if t is not None else None for t in ts])
        return arr, C.addressof(arr)

    try:
        refused("struct_size", struct_size=48)
        refused("feature_kind", feature_kind=_capi.OPD_TRACK_FEAT_ENCODER)
        refused("feature_kind", feature_kind=_capi.OPD_TRACK_FEAT_REID)
        refused("features given", features=floor.ctypes.data)
        refused("floor_out", floor=mapper._require().value)
        keep, ptr = handles(good)
        refused("track_ids or n_featured", trackers=ptr, n_featured=nf.ctypes.data)
        refused("track_ids or n_featured", trackers=ptr, track_ids=ids.ctypes.data)
        keep, ptr = handles(small)
        refused("trackers[0] was made for max_dets", trackers=ptr, track_ids=ids.ctypes.data, n_featured=nf.ctypes.data)
        keep, ptr = handles(narrow)
        refused("trackers[0] was made for feature_dim = 128", feature_kind=_capi.OPD_TRACK_FEAT_COLOR, trackers=ptr, track_ids=ids.ctypes.data, n_featured=nf.ctypes.data)
        keep, ptr = handles(None)
        refused("trackers[0] is null", trackers=ptr, track_ids=ids.ctypes.data, n_featured=nf.ctypes.data)
        # what opd_detr_detect_tiled refuses is refused here too, in its own name
        refused("opd_detr_detect_tiled_stages: 3 frames x 4 tiles", n_frames=3)
        rc = lib.opd_detr_detect_tiled_stages(C.c_void_p(sharp.model), ptrs, 1, 192, 256, win.ctypes.data_as(C.c_void_p), 4, 240, 320, THRESHOLD, C.byref(p), None, out, counts)
        assert rc == _capi.OPD_EINVAL and "stages" in _capi.last_error()
        info = _capi.OpdTrackStatus()
        assert lib.opd_track_info(good._h, C.byref(info)) == 0 and info.n_tracks == 0 and info.last_launches == 0   # no refused call reached a tracker
    finally:
        for t in (small, narrow, good):
            t.close()


def test_python_fallbacks_equal_the_fused_path(sharp, frames, mapper, reference, monkeypatch):
    S = len(GRID) * sharp.num_queries
    fused_t = _tracker()
    try:
        fused = sharp.detect_tiled_stages(frames[:1], GRID, features="color", floor_map=mapper, trackers=[fused_t])
        rows = _track_rows(fused_t)
    finally:
        fused_t.close()
    calls = []
    real = sharp._lib.opd_detr_detect_tiled_stages

    class Spy:   # the library with the fused entry counted
        def __getattr__(self, name):
            if name == "opd_detr_detect_tiled_stages":
                calls.append(name)
            return getattr(sharp_lib, name)

    sharp_lib = sharp._lib
    monkeypatch.setattr(sharp, "_lib", Spy())
    assert real is not None

    def fallback(what, features="color", skip_features=True, **kw):
        t = _tracker(**kw)
        try:
            del calls[:]
            got = sharp.detect_tiled_stages(frames[:1], GRID, features=features, floor_map=mapper, trackers=[t])
            assert calls == [], f"{what}: the fused entry was called"
            TS.same(got, fused, what, skip_features=skip_features)
            if features == "color" and t.feature_dim == 256:
                assert _track_rows(t) == rows, what
        finally:
            t.close()

    fallback("max_dets < S", max_dets=S - 1)
    t = _tracker()
    t.device_ordinal = sharp.device_ordinal + 1   # (seen by the condition only: made on the detector's GPU, the separate update runs there)
    try:
        del calls[:]
        monkeypatch.setattr(t, "_ensure", lambda real=t._ensure: (setattr(t, "device_ordinal", sharp.device_ordinal), real()))
        TS.same(sharp.detect_tiled_stages(frames[:1], GRID, features="color", floor_map=mapper, trackers=[t]), fused, "a tracker on another GPU", skip_features=True)
        assert calls == [] and _track_rows(t) == rows
    finally:
        t.close()
    # a side above 4096 with colour features: the condition alone (a 4097-pixel frame is not needed to take the branch)
    assert sharp._tiled_stages_fused(192, 256, S, "color", mapper, None) and not sharp._tiled_stages_fused(4097, 256, S, "color", mapper, None)
    assert sharp._tiled_stages_fused(4097, 256, S, None, mapper, None)
    # a wrong feature_dim with colour features: the separate update refuses the 256-wide rows, as it does without tiling
    narrow = _tracker(feature_dim=128)
    try:
        del calls[:]
        with pytest.raises(ValueError, match="feature of width 256"):
            sharp.detect_tiled_stages(frames[:1], GRID, features="color", trackers=[narrow])
        assert calls == []
    finally:
        narrow.close()
    del calls[:]
    sharp.detect_tiled_stages(frames[:1], GRID, features="color")
    assert calls == ["opd_detr_detect_tiled_stages"]
