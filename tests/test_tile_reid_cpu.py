"""CPU tests of the Re-ID stage of a tiled call: the declarations of ``opd_detr_detect_tiled_reid`` against the header, every refusal that needs no
handle (before any device call: a null handle is the LAST thing reported), the two older tiled entries as they were, and the Python surface
(``HipDetrDetector.detect_tiled_reid``, ``TiledDetector``'s forwarding and the fallback composition) on stubs."""

import ctypes as C
import os
import re

import numpy as np
import pytest

from office_person_detection_vit_amd import HipDetrDetector, HipOSNetReIDExtractor, HipReIDExtractor, TiledDetector, _capi
from office_person_detection_vit_amd.data_models import Detection
from office_person_detection_vit_amd.tiling import tile_grid

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "opd_detr.h")
ME = "opd_detr_detect_tiled_reid"


@pytest.fixture(scope="module")
def lib():
    return _capi.load_library(test_hooks=True)


def test_declarations_match_the_header():
    text = open(HEADER).read()
    body = re.search(r"typedef struct opd_tile_reid_stages \{(.*?)\} opd_tile_reid_stages;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decls = [decl.strip() for decl in body.split(";") if decl.strip()]
    names = [re.split(r"[\s\*]+", d)[-1] for d in decls]
    St = _capi.OpdTileReidStages
    assert names == [f[0] for f in St._fields_]
    # the offsets the header's types give on this ABI: two int32, then pointers
    want, off = {}, 0
    for d, name in zip(decls, names):
        size = 8 if "*" in d else 4
        assert "*" in d or d.startswith("int32_t"), d
        off = (off + size - 1) // size * size
        want[name] = off
        off += size
    assert {n: getattr(St, n).offset for n in names} == want
    assert C.sizeof(St) == off == 80 and St.slots.offset == 4 and St.reid.offset == 8 and St.n_featured.offset == 72
    assert C.sizeof(_capi.OpdTileStages) == 56   # the older block is as it was
    proto = re.search(r"OPD_API int " + ME + r"\((.*?)\);", text, re.S).group(1)
    assert len(proto.split(",")) == len(_capi.API[ME][1]) == 14
    assert "opd_test_tile_reid" in _capi.TEST_API and "opd_test_tile_reid" not in text
    assert "Re-ID is a call of its own" not in text


def test_arguments_are_refused_before_any_device_call(lib):
    grid = np.asarray(tile_grid(40, 52, 2, 2, 0.125), np.int32)
    p = _capi.OpdTileParams(struct_size=C.sizeof(_capi.OpdTileParams), person_label=1, tile_nms_threshold=0.4, merge_nms_threshold=0.4, merge_threshold=0.5,
                            edge_tolerance=0.01)
    frame = np.zeros((40, 52, 3), np.uint8)
    ptrs = (C.c_void_p * 1)(frame.ctypes.data)
    out, counts = (_capi.OpdTileDet * 400)(), (C.c_int32 * 1)()
    buf = np.zeros(64, np.int32)
    dummy = buf.ctypes.data   # stands for a handle or an output: never dereferenced before the refusal
    full = dict(slots=4, reid=dummy, features=dummy, slot_map=dummy, n_person=dummy)

    def refused(text, stages=True, h=40, w=52, tiles=grid, params=p, o=out, fr=ptrs, struct_size=C.sizeof(_capi.OpdTileReidStages), drop=(), **kw):
        fields = {k: v for k, v in {**full, **kw}.items() if k not in drop}
        st = _capi.OpdTileReidStages(struct_size=struct_size, **fields)
        rc = lib.opd_detr_detect_tiled_reid(None, fr, 1, h, w, tiles.ctypes.data_as(C.c_void_p), 4, 32, 40, 0.05, None if params is None else C.byref(params),
                                            C.byref(st) if stages else None, o, counts)
        assert rc == _capi.OPD_EINVAL and text in _capi.last_error(), (text, _capi.last_error())
        assert _capi.last_error().startswith(ME + ":") or text == "null model handle"

    # a complete block: the null model handle is what is left to report
    refused("null model handle")
    refused("null model handle", floor=dummy, floor_out=dummy, trackers=dummy, track_ids=dummy, n_featured=dummy)
    refused("null model handle", drop=("features",), trackers=dummy, track_ids=dummy, n_featured=dummy)   # no rows to the caller: the trackers take them
    for slots in (0, -1, 1 << 20):   # (the range needs the Re-ID handle, which is not read before the model handle)
        refused("null model handle", slots=slots)
    refused("stages", stages=False)
    refused("opd_tile_reid_stages.struct_size", struct_size=56)
    refused("opd_tile_reid_stages.struct_size", struct_size=0)
    refused("null Re-ID handle", drop=("reid",))
    refused("slot_map or n_person is null", drop=("slot_map",))
    refused("slot_map or n_person is null", drop=("n_person",))
    refused("features is null while no trackers are given", drop=("features",))
    refused("floor_out is null", floor=dummy)
    refused("track_ids or n_featured is null", trackers=dummy)
    refused("track_ids or n_featured is null", trackers=dummy, track_ids=dummy)
    refused("track_ids or n_featured is null", trackers=dummy, n_featured=dummy)
    # what opd_detr_detect_tiled refuses, in this entry's name
    refused("null argument", o=None)
    refused("null argument", fr=None)
    refused("null argument", params=None)
    outside = grid.copy(); outside[3, 1] += 1
    refused("lies outside the 40 x 52 frame", tiles=outside)
    refused("more than one size", tiles=np.asarray(tile_grid(41, 52, 2, 2, 0.125), np.int32), h=41)
    refused("tile_nms_threshold", params=_capi.OpdTileParams(struct_size=C.sizeof(_capi.OpdTileParams), person_label=1, tile_nms_threshold=float("nan")))
    refused("opd_tile_params.struct_size", params=_capi.OpdTileParams(struct_size=8, person_label=1, tile_nms_threshold=0.4))
    wide = np.asarray(tile_grid(40, 4098, 2, 2, 0.125), np.int32)
    refused("null model handle", w=4098, tiles=wide)   # (the colour kernel's 4096 limit is no limit of the Re-ID crop)

    # the two older entries word and refuse as before
    rc = lib.opd_detr_detect_tiled(None, ptrs, 1, 40, 52, grid.ctypes.data_as(C.c_void_p), 4, 32, 40, 0.05, C.byref(p), None, counts)
    assert rc == _capi.OPD_EINVAL and _capi.last_error() == "opd_detr_detect_tiled: null argument"
    rc = lib.opd_detr_detect_tiled(None, ptrs, 1, 40, 52, grid.ctypes.data_as(C.c_void_p), 4, 32, 40, 0.05, C.byref(p), out, counts)
    assert rc == _capi.OPD_EINVAL and _capi.last_error() == "null model handle"

    def stages_refused(text, **kw):
        st = _capi.OpdTileStages(struct_size=C.sizeof(_capi.OpdTileStages), **kw)
        rc = lib.opd_detr_detect_tiled_stages(None, ptrs, 1, 40, 52, grid.ctypes.data_as(C.c_void_p), 4, 32, 40, 0.05, C.byref(p), C.byref(st), out, counts)
        assert rc == _capi.OPD_EINVAL and text in _capi.last_error(), (text, _capi.last_error())
        assert _capi.last_error().startswith("opd_detr_detect_tiled_stages:") or text == "null model handle"

    stages_refused("null model handle")
    for kind in (_capi.OPD_TRACK_FEAT_ENCODER, _capi.OPD_TRACK_FEAT_REID, 7, -1):
        stages_refused("feature_kind " + str(kind), feature_kind=kind)
    stages_refused("feature_kind 3", feature_kind=_capi.OPD_TRACK_FEAT_REID, features=dummy, trackers=dummy, track_ids=dummy, n_featured=dummy)
    stages_refused("features given with feature_kind OPD_TRACK_FEAT_NONE", features=dummy)
    stages_refused("floor_out is null", floor=dummy)
    stages_refused("track_ids or n_featured is null", trackers=dummy)


def _det(k, **kw):
    return Detection(bbox=(10.0 * k, 5.0, 20.0, 40.0), confidence=0.9 - 0.1 * k, class_id=1, class_name="person", camera_coords=(10.0 * k + 10.0, 45.0), query_index=k, **kw)


def test_detect_tiled_reid_argument_errors_come_before_any_library_call():
    frame = np.zeros((40, 52, 3), np.uint8)
    grid = tile_grid(40, 52, 2, 2, 0.125)
    det = HipDetrDetector(model_path="unused", max_batch=8)
    det.model = 1   # (never dereferenced: every check below comes before the library call)

    class NoLibrary:
        def __getattr__(self, name):
            raise AssertionError(f"the library was called: {name}")

    det._lib = NoLibrary()
    reid = object()
    try:
        with pytest.raises(ValueError, match="needs reid="):
            det.detect_tiled_reid([frame], grid, None)
        with pytest.raises(ValueError, match="1 trackers for 2 frames"):
            det.detect_tiled_reid([frame, frame], grid, reid, trackers=[object()])
        t = object()
        with pytest.raises(ValueError, match="named twice"):
            det.detect_tiled_reid([frame, frame], grid, reid, trackers=[t, t])
        with pytest.raises(ValueError, match="more than one size"):
            det.detect_tiled_reid([frame], [(0, 0, 20, 26), (0, 26, 20, 25)], reid)
        with pytest.raises(ValueError, match="non-empty list"):
            det.detect_tiled_reid([frame], [], reid)
        with pytest.raises(ValueError, match="exceed max_batch"):
            det.detect_tiled_reid([frame], [(0, 0, 8, 8)] * 9, reid)
        unloaded = HipOSNetReIDExtractor(model_path="unused")
        with pytest.raises(RuntimeError, match="not loaded"):
            det.detect_tiled_reid([frame], grid, unloaded)
        with pytest.raises(ValueError, match="contiguous uint8"):
            det.detect_tiled_reid([frame.astype(np.float32)], grid, reid)
        assert det.detect_tiled_reid([], grid, reid, trackers=[]) == []
        with pytest.raises(ValueError, match="None or 'color'"):   # the staged method keeps refusing the kind
            det.detect_tiled_stages([frame], grid, features="reid")
    finally:
        det.model = None


def test_fallback_composition_order_on_stubs():
    """Where the fused conditions fail: detect_tiled, then per frame extract_features, floor_map.apply, tracker.update."""
    frame = np.zeros((40, 52, 3), np.uint8)
    grid = tile_grid(40, 52, 2, 2, 0.125)
    det = HipDetrDetector(model_path="unused", max_batch=8)
    det.model = 1
    calls = []

    class Info:
        num_queries = 100

    det._info = Info()
    det.detect_tiled = lambda frames, tiles, a, b, c: (calls.append(("detect_tiled", len(frames), tiles, a, b, c)), [[_det(0), _det(1)] for _ in frames])[1]

    class Reid:   # no native handle: the first fused condition fails
        feature_dim = 512

        def extract_features(self, image, bboxes):
            calls.append(("extract_features", len(bboxes)))
            return np.full((len(bboxes), 512), 2.0, np.float32)

    class Floor:
        def apply(self, dets):
            calls.append(("apply", len(dets)))
            for d in dets:
                d.zone_ids = ["z"]

    class Tracker:
        def update(self, dets):
            calls.append(("update", len(dets), all(d.features is not None for d in dets)))
            for d in dets:
                d.track_id = 9
            return list(dets)

    try:
        out = det.detect_tiled_reid([frame, frame], grid, Reid(), 0.3, 0.6, 0.02, floor_map=Floor(), trackers=[Tracker(), Tracker()])
    finally:
        det.model = None
    assert calls == [("detect_tiled", 2, [tuple(t) for t in grid], 0.3, 0.6, 0.02)] + [("extract_features", 2), ("apply", 2), ("update", 2, True)] * 2
    assert all(d.track_id == 9 and d.zone_ids == ["z"] and d.features[0] == 2.0 for dets in out for d in dets)
    del calls[:]
    det.model = 1
    try:
        out = det.detect_tiled_reid([frame], grid, Reid())
    finally:
        det.model = None
    assert [c[0] for c in calls] == ["detect_tiled", "extract_features"] and out[0][1].features.shape == (512,)


def test_tiled_detector_forwards_under_the_three_conditions_only():
    frame = np.zeros((40, 52, 3), np.uint8)
    grid = tile_grid(40, 52, 2, 2, 0.125)
    calls = []

    class Staged:   # detect_tiled and detect_tiled_stages, no detect_tiled_reid
        def detect_tiled(self, frames, tiles, nms_threshold, merge_threshold):
            calls.append(("detect_tiled", len(frames), tiles, nms_threshold, merge_threshold))
            return [[_det(0), _det(1)] for _ in frames]

        def detect_tiled_stages(self, frames, tiles, nms_threshold, merge_threshold, **kw):
            calls.append(("detect_tiled_stages", kw))
            return [[_det(0), _det(1)] for _ in frames]

    class Native(Staged):
        def detect_tiled_reid(self, frames, tiles, reid, nms_threshold, merge_threshold, **kw):
            calls.append(("detect_tiled_reid", len(frames), tiles, reid, nms_threshold, merge_threshold, kw))
            dets = [_det(0, features=None if kw.get("trackers") else np.ones(512, np.float32)), _det(1, features=None if kw.get("trackers") else np.zeros(512, np.float32))]
            if kw.get("trackers"):
                dets[0].track_id = 4
            return [dets for _ in frames]

    class StubReid:   # anything that is no HipReIDExtractor: the separate call
        def extract_features(self, frame, bboxes):
            calls.append(("extract_features", len(bboxes)))
            return np.full((len(bboxes), 512), 2.0, np.float32)

    class Tracker:
        def update(self, dets):
            calls.append(("update", len(dets)))
            for d in dets:
                d.track_id = 9
            return list(dets)

    loaded = [HipOSNetReIDExtractor(model_path="unused"), HipReIDExtractor(model_path="unused")]
    unloaded = HipOSNetReIDExtractor(model_path="unused")
    def not_forwarded(frame, bboxes):
        raise AssertionError("the separate Re-ID call ran where the fused method should have been called")

    for ext in loaded:
        ext._handle = C.c_void_p(1)   # "loaded" for the condition; never handed to the library
        ext.extract_features = not_forwarded
    try:
        assert all(e.is_loaded for e in loaded) and not unloaded.is_loaded
        td = TiledDetector(Native(), native=True, nms_threshold=0.3, merge_threshold=0.6)
        tracker = Tracker()
        for ext in loaded:
            del calls[:]
            dets, rows = td.detect_with_features(frame, features="reid", reid=ext)
            assert rows.shape == (2, 512) and rows[0, 0] == 1.0 and dets[0].features[0] == 1.0
            td.detect_with_features(frame, features="reid", reid=ext, reid_slots=7)
            tracked = td.detect_and_track(frame, tracker, features="reid", reid=ext)
            assert [d.track_id for d in tracked] == [4]
            td.detect_and_track(frame, tracker, features="reid", reid=ext, reid_slots=5)
            assert calls == [("detect_tiled_reid", 1, grid, ext, 0.3, 0.6, {"reid_slots": 32}), ("detect_tiled_reid", 1, grid, ext, 0.3, 0.6, {"reid_slots": 7}),
                             ("detect_tiled_reid", 1, grid, ext, 0.3, 0.6, {"reid_slots": 32, "trackers": [tracker]}),
                             ("detect_tiled_reid", 1, grid, ext, 0.3, 0.6, {"reid_slots": 5, "trackers": [tracker]})]

        def present_sequence(td, ext):
            """What the two methods do today: detect_tiled (or the host tiles), then the Re-ID call, then the update."""
            del calls[:]
            dets, rows = td.detect_with_features(frame, features="reid", reid=ext)
            assert rows.shape == (2, 512) and dets[1].features[0] == 2.0
            assert calls == [("detect_tiled", 1, grid, 0.3, 0.6), ("extract_features", 2)]
            del calls[:]
            tracked = td.detect_and_track(frame, tracker, features="reid", reid=ext)
            assert [d.track_id for d in tracked] == [9, 9] and tracked[0].features[0] == 2.0
            assert calls == [("detect_tiled", 1, grid, 0.3, 0.6), ("extract_features", 2), ("update", 2)]

        # 1. reid is no loaded extractor of the package
        present_sequence(td, StubReid())
        unloaded.extract_features = StubReid().extract_features
        present_sequence(td, unloaded)
        # 2. the wrapped detector has no detect_tiled_reid
        loaded[0].extract_features = StubReid().extract_features
        present_sequence(TiledDetector(Staged(), native=True, nms_threshold=0.3, merge_threshold=0.6), loaded[0])
        loaded[0].extract_features = not_forwarded
        # 3. native=False: the host composition, the fused method is not touched

        class Host(Native):
            def detect_batch(self, tiles):
                calls.append(("detect_batch", len(tiles)))
                return [[_det(0)] if i == 0 else [] for i in range(len(tiles))]

        loaded[0].extract_features = StubReid().extract_features
        del calls[:]
        host = TiledDetector(Host(), native=False)
        dets, rows = host.detect_with_features(frame, features="reid", reid=loaded[0])
        host.detect_and_track(frame, tracker, features="reid", reid=loaded[0])
        assert calls == [("detect_batch", 4), ("extract_features", 1), ("detect_batch", 4), ("extract_features", 1), ("update", 1)] and rows.shape == (1, 512)
        # the other kinds go where they went
        del calls[:]
        td.detect_with_features(frame, features="color")
        td.detect_and_track(frame, tracker, features=None)
        assert calls == [("detect_tiled_stages", {"features": "color"}), ("detect_tiled_stages", {"features": None, "trackers": [tracker]})]
        with pytest.raises(ValueError, match="needs reid="):
            td.detect_with_features(frame, features="reid")
        with pytest.raises(ValueError, match="needs reid="):
            td.detect_and_track(frame, tracker, features="reid")
    finally:
        for ext in loaded:
            ext._handle = None   # (nothing to destroy)
