"""CPU tests of hybrid tracking inside a tiled call and of the Re-ID rows for a grid whose tiles differ in size: the declarations of
``opd_detr_detect_tiled_hybrid``, ``opd_detr_detect_tiled_sequence_hybrid`` and ``opd_detr_detect_tiled_ragged_reid`` against the header, every refusal
that needs no handle (before any device call: a null handle is the LAST thing reported), the numpy restatement of the ingest of MERGED records against
the boxes the Python path builds, and the Python surface (``HipDetrDetector``'s three methods, ``TiledDetector``'s routing) on stubs."""

import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import tile_common as TC
import tile_hybrid_common as TH
from office_person_detection_vit_amd import HipDetrDetector, HipOSNetReIDExtractor, TiledDetector, _capi
from office_person_detection_vit_amd.data_models import Detection
from office_person_detection_vit_amd.tiling import tile_grid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "opd_detr.h")
A, B, R = "opd_detr_detect_tiled_hybrid", "opd_detr_detect_tiled_sequence_hybrid", "opd_detr_detect_tiled_ragged_reid"


@pytest.fixture(scope="module")
def lib():
    return _capi.load_library(test_hooks=True)


# ---- 1. exports, bindings, struct sizes ---------------------------------------------------------------------------------------------------------
def test_declarations_match_the_header(lib):
    text = open(HEADER).read()
    body = re.search(r"typedef struct opd_tile_hybrid \{(.*?)\} opd_tile_hybrid;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in [d.strip() for d in body.split(";") if d.strip()]:
        names += [re.split(r"[\s\*]+", part.strip())[-1] for part in decl.split(",")]
    St = _capi.OpdTileHybrid
    assert names == [f[0] for f in St._fields_] == ["struct_size", "reserved", "trackers", "track_ids", "floor", "floor_out"]
    assert C.sizeof(St) == 40 and [getattr(St, n).offset for n in names] == [0, 4, 8, 16, 24, 32]
    assert C.sizeof(_capi.OpdTileStages) == 56 and C.sizeof(_capi.OpdTileReidStages) == 80   # the older blocks are as they were
    for name, n_args in ((A, 15), (B, 21), (R, 13)):
        proto = re.search(r"OPD_API int " + name + r"\((.*?)\);", text, re.S).group(1)
        assert len(proto.split(",")) == len(_capi.API[name][1]) == n_args, name
        assert getattr(lib, name) is not None
        product = C.CDLL(_capi.LIB_PATH)   # exported from the product library, not only from the test build
        assert hasattr(product, name), name
    assert "opd_lwt_test_ingest_merged" in _capi.TEST_API and "opd_lwt_test_ingest_merged" not in text
    assert hasattr(lib, "opd_lwt_test_ingest_merged") and not hasattr(C.CDLL(_capi.LIB_PATH), "opd_lwt_test_ingest_merged")
    assert "Re-ID rows are not offered" not in text and "opd_detr_detect_tiled_ragged_reid below" in text
    src = open(os.path.join(ROOT, "office_person_detection_vit_amd", "csrc", "build.py")).read()
    assert src.count("opd_lwt_ingest_merged_test_api.cpp") == 2   # a source, and TEST_ONLY


# ---- 2. refusals that need no handle --------------------------------------------------------------------------------------------------------------
GRID = np.asarray(tile_grid(40, 52, 2, 2, 0.125), np.int32)
MIXED = np.asarray(tile_grid(41, 52, 2, 2, 0.125), np.int32)


def _params(**kw):
    return _capi.OpdTileParams(**{**dict(struct_size=C.sizeof(_capi.OpdTileParams), person_label=1, tile_nms_threshold=0.4, merge_nms_threshold=0.4, merge_threshold=0.5,
                                         edge_tolerance=0.01), **kw})


def _last(rc, text, me):
    assert rc == _capi.OPD_EINVAL and text in _capi.last_error(), (text, _capi.last_error())
    assert _capi.last_error().startswith(me + ":") or text == "null model handle"


def test_detection_frame_arguments_are_refused_before_any_device_call(lib):
    p = _params()
    frame = np.zeros((41, 52, 3), np.uint8)
    ptrs = (C.c_void_p * 1)(frame.ctypes.data)
    out, counts = (_capi.OpdTileDet * 400)(), (C.c_int32 * 1)()
    buf = np.zeros(64, np.int32)
    dummy = buf.ctypes.data   # stands for a handle or an output: never dereferenced before the refusal
    hw = np.asarray([[32, 40]] * 4, np.int32)

    def refused(text, block=True, h=40, tiles=GRID, tile_hw=None, params=p, o=out, fr=ptrs, struct_size=C.sizeof(_capi.OpdTileHybrid), drop=(), **kw):
        fields = {k: v for k, v in {**dict(trackers=dummy, track_ids=dummy), **kw}.items() if k not in drop}
        hy = _capi.OpdTileHybrid(struct_size=struct_size, **fields)
        rc = lib.opd_detr_detect_tiled_hybrid(None, fr, 1, h, 52, tiles.ctypes.data_as(C.c_void_p), 4, 32, 40, None if tile_hw is None else tile_hw.ctypes.data_as(C.c_void_p),
                                              0.05, None if params is None else C.byref(params), C.byref(hy) if block else None, o, counts)
        _last(rc, text, A)

    refused("null model handle")   # a complete block: the null model handle is what is left to report
    refused("null model handle", floor=dummy, floor_out=dummy)
    refused("null model handle", tiles=MIXED, h=41, tile_hw=hw)   # windows of several sizes pass with tile_HW
    refused("null argument (hy)", block=False)
    refused("opd_tile_hybrid.struct_size", struct_size=56)
    refused("opd_tile_hybrid.struct_size", struct_size=0)
    refused("trackers or track_ids is null", drop=("trackers",))
    refused("trackers or track_ids is null", drop=("track_ids",))
    refused("floor_out is null", floor=dummy)
    # what the plain tiled entries refuse, in this entry's name
    refused("null argument", o=None)
    refused("null argument", fr=None)
    refused("null argument", params=None)
    outside = GRID.copy(); outside[3, 1] += 1
    refused("lies outside the 40 x 52 frame", tiles=outside)
    refused("more than one size", tiles=MIXED, h=41)   # ... without tile_HW
    refused("below 1", tiles=MIXED, h=41, tile_hw=np.asarray([[32, 40], [0, 40], [32, 40], [32, 40]], np.int32))
    refused("tile_nms_threshold", params=_params(tile_nms_threshold=float("nan")))
    refused("opd_tile_params.struct_size", params=_params(struct_size=8))


def test_sequence_arguments_are_refused_before_any_device_call(lib):
    p = _params()
    frame = np.zeros((40, 52, 3), np.uint8)
    out, counts, ids = (_capi.OpdTileDet * 800)(), (C.c_int32 * 2)(), np.zeros(800, np.int32)
    lrecs, lcounts = (_capi.OpdLwtRec * 64)(), (C.c_int32 * 2)()
    buf = np.zeros(64, np.int32)
    dummy = C.c_void_p(buf.ctypes.data)

    def refused(text, keys=(1, 0), F=2, capacity=32, fr=True, flags=True, done=True, o=out, cn=counts, ti=ids.ctypes.data, lr=lrecs, lc=lcounts, t=dummy, tiles=GRID,
                params=p):
        ptrs = (C.c_void_p * 65)(*([frame.ctypes.data] * 65))
        ks = (C.c_uint8 * 65)(*(list(keys) + [0] * (65 - len(keys))))
        d = C.c_int32(-7)
        rc = lib.opd_detr_detect_tiled_sequence_hybrid(None, t, ptrs if fr else None, ks if flags else None, F, 40, 52, tiles.ctypes.data_as(C.c_void_p), 4, 32, 40, None, 0.05,
                                                       None if params is None else C.byref(params), o, cn, ti, lr, capacity, lc, C.byref(d) if done else None)
        _last(rc, text, B)
        assert d.value == -7   # frames_done is not written by a refusal in front of the device

    refused("null model handle")
    refused("null model handle", keys=(0, 0), o=None, cn=None, ti=None)   # K = 0: no key-frame output is needed
    refused("null model handle", keys=(1, 1), lr=None, lc=None)         # K = F: no in-between output is needed
    refused("0 frames", F=0)
    refused("65 frames", F=65)
    refused("capacity 0", capacity=0)
    refused("null argument", fr=False)
    refused("null argument", flags=False)
    refused("null argument", done=False)
    refused("null output of the key frames", o=None)
    refused("null output of the key frames", ti=None)
    refused("null output of the in-between frames", lr=None)
    refused("null output of the in-between frames", lc=None)
    refused("null argument", params=None)
    refused("more than one size", tiles=np.asarray([[0, 0, 20, 26], [0, 26, 20, 25], [20, 0, 20, 26], [20, 26, 20, 26]], np.int32))


def test_ragged_reid_arguments_are_refused_before_any_device_call(lib):
    p = _params()
    frame = np.zeros((41, 52, 3), np.uint8)
    ptrs = (C.c_void_p * 1)(frame.ctypes.data)
    out, counts = (_capi.OpdTileDet * 400)(), (C.c_int32 * 1)()
    buf = np.zeros(64, np.int32)
    dummy = buf.ctypes.data
    hw = np.asarray([[32, 40]] * 4, np.int32)
    full = dict(slots=4, reid=dummy, features=dummy, slot_map=dummy, n_person=dummy)

    def refused(text, stages=True, tiles=MIXED, tile_hw=hw, struct_size=C.sizeof(_capi.OpdTileReidStages), drop=(), o=out, **kw):
        st = _capi.OpdTileReidStages(struct_size=struct_size, **{k: v for k, v in {**full, **kw}.items() if k not in drop})
        rc = lib.opd_detr_detect_tiled_ragged_reid(None, ptrs, 1, 41, 52, tiles.ctypes.data_as(C.c_void_p), 4, None if tile_hw is None else tile_hw.ctypes.data_as(C.c_void_p), 0.05,
                                                   C.byref(p), C.byref(st) if stages else None, o, counts)
        _last(rc, text, R)

    refused("null model handle")   # windows of several sizes and a complete block
    refused("null model handle", drop=("features",), trackers=dummy, track_ids=dummy, n_featured=dummy)
    refused("stages", stages=False)
    refused("opd_tile_reid_stages.struct_size", struct_size=56)
    refused("null Re-ID handle", drop=("reid",))
    refused("slot_map or n_person is null", drop=("slot_map",))
    refused("features is null while no trackers are given", drop=("features",))
    refused("floor_out is null", floor=dummy)
    refused("track_ids or n_featured is null", trackers=dummy)
    refused("null argument", o=None)
    refused("tile_HW", tile_hw=None)
    outside = MIXED.copy(); outside[3, 1] += 1
    refused("lies outside the 41 x 52 frame", tiles=outside)
    # opd_detr_detect_tiled_ragged keeps refusing the kind
    st = _capi.OpdTileStages(struct_size=C.sizeof(_capi.OpdTileStages), feature_kind=_capi.OPD_TRACK_FEAT_REID)
    rc = lib.opd_detr_detect_tiled_ragged(None, ptrs, 1, 41, 52, MIXED.ctypes.data_as(C.c_void_p), 4, hw.ctypes.data_as(C.c_void_p), 0.05, C.byref(p), C.byref(st), out, counts)
    _last(rc, "feature_kind 3", "opd_detr_detect_tiled_ragged")


# ---- 3. the restatement of the merged ingest against the boxes of the Python path -----------------------------------------------------------------
CASES = TC.cases()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_merged_ingest_restatement_equals_the_python_boxes(case):
    S = len(case["tiles"]) * case["stride"]
    for dets in TH.merged_detections(case):
        n = len(dets)
        recs = TH.as_merged(dets, S)
        boxes = np.full((S, 4), 7.5, np.float32)
        assert TH.ingest_merged(recs, n, S, boxes) == n
        assert boxes[:n].tobytes() == TH.python_boxes(dets).tobytes(), case["name"]
        assert (boxes[n:] == 7.5).all()


def test_the_cases_and_the_edge_records_cover_what_they_claim():
    dets = [d for c in CASES for frame in TH.merged_detections(c) for d in frame]
    boxes = np.array([d.bbox for d in dets], np.float64)
    assert len(dets) > 300
    assert (boxes[:, 2] <= 0).any() and (boxes[:, 3] == 0).any()                  # degenerate boxes survive the merge and reach the tracker
    assert (boxes[:, 0] == 0).any() and (boxes[:, 1] == 0).any()                  # boxes touching 0 ...
    assert any(d.bbox[0] + d.bbox[2] == c["frame"][1] for c in CASES for frame in TH.merged_detections(c) for d in frame)   # ... and the frame edge
    # a width that is NOT the difference of the rounded corners: rounding each of the four once is not re-deriving
    x, w = boxes[:, 0], boxes[:, 2]
    assert ((x + w).astype(np.float32) != x.astype(np.float32) + w.astype(np.float32)).any()
    recs = TH.edge_merged(400)
    for name in ("x", "y", "w", "h"):
        assert (recs[name].astype(np.float32).astype(np.float64) != recs[name]).mean() > 0.9   # nearly every value rounds
    # the clamps of the count
    boxes = np.full((400, 4), 7.5, np.float32)
    assert TH.ingest_merged(recs, 401, 400, boxes) == 400 and (boxes != 7.5).all()
    boxes[:] = 7.5
    assert TH.ingest_merged(recs, -3, 400, boxes) == 0 and (boxes == 7.5).all()


# ---- 4. the Python surface --------------------------------------------------------------------------------------------------------------------------
def test_signatures():
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(HipDetrDetector.detect_tiled_hybrid) == ["self", "frames", "tiles", "lwts", "nms_threshold", "merge_threshold", "edge_tolerance", "floor_map"]
    assert sig(HipDetrDetector.track_tiled_hybrid_batch)[:5] == ["self", "frames", "tiles", "lwt", "key_frames"]
    assert sig(HipDetrDetector.detect_tiled_ragged_reid) == sig(HipDetrDetector.detect_tiled_reid)
    d = inspect.signature(HipDetrDetector.detect_tiled_hybrid).parameters
    assert (d["nms_threshold"].default, d["merge_threshold"].default, d["edge_tolerance"].default, d["floor_map"].default) == (0.4, 0.5, 0.01, None)
    assert sig(TiledDetector.detect_and_track_hybrid) == ["self", "frame", "lwt"] and sig(TiledDetector.track_hybrid_batch) == ["self", "frames", "lwt", "key_frames"]
    # the existing methods keep their parameter lists
    assert sig(HipDetrDetector.detect_tiled) == ["self", "frames", "tiles", "nms_threshold", "merge_threshold", "edge_tolerance"]
    assert sig(HipDetrDetector.detect_tiled_ragged) == ["self", "frames", "tiles", "nms_threshold", "merge_threshold", "edge_tolerance", "features", "floor_map", "trackers"]
    assert sig(HipDetrDetector.detect_and_track_hybrid) == ["self", "frame", "lwt"] and sig(HipDetrDetector.track_hybrid_batch) == ["self", "frames", "lwt", "key_frames"]


class NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the library was called: {name}")


def _stub_detector():
    det = HipDetrDetector(model_path="unused", max_batch=8)
    det.model = 1   # (never dereferenced: every check below comes before the library call)
    det._lib = NoLibrary()

    class Info:
        num_queries = 100

    det._info = Info()
    return det


def test_argument_errors_come_before_any_library_call():
    frame = np.zeros((40, 52, 3), np.uint8)
    grid = tile_grid(40, 52, 2, 2, 0.125)
    det = _stub_detector()
    t = object()
    try:
        with pytest.raises(ValueError, match="1 trackers for 2 frames"):
            det.detect_tiled_hybrid([frame, frame], grid, [t])
        with pytest.raises(ValueError, match="named twice"):
            det.detect_tiled_hybrid([frame, frame], grid, [t, t])
        with pytest.raises(ValueError, match="non-empty list"):
            det.detect_tiled_hybrid([frame], [], [t])
        with pytest.raises(ValueError, match="exceed max_batch"):
            det.detect_tiled_hybrid([frame], [(0, 0, 8, 8)] * 9, [t])
        with pytest.raises(ValueError, match="at least 1"):
            det.detect_tiled_hybrid([frame], [(0, 0, 0, 8)], [t])
        with pytest.raises(ValueError, match="contiguous uint8"):
            det.detect_tiled_hybrid([frame.astype(np.float32)], grid, [t])
        assert det.detect_tiled_hybrid([], grid, []) == []
        with pytest.raises(ValueError, match="2 frames, 1 key flags"):
            det.track_tiled_hybrid_batch([frame, frame], grid, t, [True])
        with pytest.raises(ValueError, match="contiguous uint8"):
            det.track_tiled_hybrid_batch([frame[:, ::2]], grid, t, [True])
        assert det.track_tiled_hybrid_batch([], grid, t, []) == []
        with pytest.raises(ValueError, match="needs reid="):
            det.detect_tiled_ragged_reid([frame], grid, None)
        with pytest.raises(ValueError, match="named twice"):
            det.detect_tiled_ragged_reid([frame, frame], grid, object(), trackers=[t, t])
        with pytest.raises(RuntimeError, match="not loaded"):
            det.detect_tiled_ragged_reid([frame], grid, HipOSNetReIDExtractor(model_path="unused"))
        assert det.detect_tiled_ragged_reid([], grid, object()) == []
        with pytest.raises(ValueError, match="None or 'color'"):   # the existing methods keep their refusals
            det.detect_tiled_ragged([frame], grid, features="reid")
        with pytest.raises(ValueError, match="more than one size"):
            det.detect_tiled_reid([frame], [(0, 0, 20, 26), (0, 26, 20, 25)], object())
    finally:
        det.model = None


def _det(k, **kw):
    return Detection(bbox=(10.0 * k, 5.0, 20.0, 40.0), confidence=0.9 - 0.1 * k, class_id=1, class_name="person", camera_coords=(10.0 * k + 10.0, 45.0), query_index=k, **kw)


class StubLwt:
    """Records what reaches it; `max_tracks` below 400 fails the fused condition of a 2 x 2 grid under 100 queries."""

    SEQUENCE_MAX = 64

    def __init__(self, calls, device=0, max_tracks=64):
        self.calls, self.device, self.max_tracks, self._h = calls, device, max_tracks, None

    def update_with_detections(self, frame, dets):
        self.calls.append(("update_with_detections", len(dets)))
        for k, d in enumerate(dets):
            d.track_id = k + 1
        return dets

    def interpolate(self, frame):
        self.calls.append(("interpolate",))
        return [(1, (0.0, 0.0, 1.0, 1.0))]


def test_detector_fallback_composition_on_stubs():
    """Where the fused conditions fail: the plain tiled call of the grid's kind, then update_with_detections (and floor_map.apply) per frame."""
    frame, odd = np.zeros((40, 52, 3), np.uint8), np.zeros((41, 52, 3), np.uint8)
    grid, mixed = tile_grid(40, 52, 2, 2, 0.125), tile_grid(41, 52, 2, 2, 0.125)
    det = _stub_detector()
    calls = []
    det.detect_tiled = lambda frames, tiles, a, b, c: (calls.append(("detect_tiled", len(frames), a, b, c)), [[_det(0), _det(1)] for _ in frames])[1]
    det.detect_tiled_ragged = lambda frames, tiles, a, b, c: (calls.append(("detect_tiled_ragged", len(frames), a, b, c)), [[_det(0)] for _ in frames])[1]

    class Floor:
        device = 0

        def apply(self, dets):
            calls.append(("apply", len(dets)))

    try:
        det.device = "hip:0"
        small = [StubLwt(calls), StubLwt(calls)]
        out = det.detect_tiled_hybrid([frame, frame], grid, small, 0.3, 0.6, 0.02, floor_map=Floor())
        assert calls == [("detect_tiled", 2, 0.3, 0.6, 0.02), ("update_with_detections", 2), ("apply", 2), ("update_with_detections", 2), ("apply", 2)]
        assert [[d.track_id for d in dets] for dets in out] == [[1, 2], [1, 2]]
        del calls[:]
        det.detect_tiled_hybrid([odd], mixed, [StubLwt(calls)])
        assert calls == [("detect_tiled_ragged", 1, 0.4, 0.5, 0.01), ("update_with_detections", 1)]
        del calls[:]
        other_gpu = StubLwt(calls, device=1, max_tracks=1024)   # room, but on another device
        det.detect_tiled_hybrid([frame], grid, [other_gpu])
        assert calls == [("detect_tiled", 1, 0.4, 0.5, 0.01), ("update_with_detections", 2)]
        del calls[:]
        got = det.track_tiled_hybrid_batch([frame] * 3, grid, StubLwt(calls), [False, True, False])
        assert calls == [("interpolate",), ("detect_tiled", 1, 0.4, 0.5, 0.01), ("update_with_detections", 2), ("interpolate",)]
        assert got[0] == [(1, (0.0, 0.0, 1.0, 1.0))] and [d.track_id for d in got[1]] == [1, 2]
    finally:
        det.model = None


def test_tiled_detector_routes():
    frame, odd = np.zeros((40, 52, 3), np.uint8), np.zeros((41, 52, 3), np.uint8)
    grid, mixed = tile_grid(40, 52, 2, 2, 0.125), tile_grid(41, 52, 2, 2, 0.125)
    assert len({(t[2], t[3]) for t in grid}) == 1 and len({(t[2], t[3]) for t in mixed}) > 1
    calls = []

    class Plain:   # the tiled calls of the parent: no hybrid method, no ragged Re-ID
        num_queries, device_ordinal = 100, 0

        def detect_tiled(self, frames, tiles, nms_threshold, merge_threshold):
            calls.append(("detect_tiled", len(frames), tiles))
            return [[_det(0), _det(1)] for _ in frames]

        def detect_tiled_ragged(self, frames, tiles, nms_threshold, merge_threshold, **kw):
            calls.append(("detect_tiled_ragged", len(frames), tiles, kw))
            return [[_det(0)] for _ in frames]

        def detect_tiled_reid(self, frames, tiles, reid, nms_threshold, merge_threshold, **kw):
            calls.append(("detect_tiled_reid", tiles, kw))
            return [[_det(0, features=np.ones(512, np.float32))] for _ in frames]

    class Native(Plain):
        def detect_tiled_hybrid(self, frames, tiles, lwts, nms_threshold, merge_threshold):
            calls.append(("detect_tiled_hybrid", len(frames), tiles, lwts, nms_threshold, merge_threshold))
            return [[_det(0, track_id=7)] for _ in frames]

        def track_tiled_hybrid_batch(self, frames, tiles, lwt, key_frames, nms_threshold, merge_threshold):
            calls.append(("track_tiled_hybrid_batch", len(frames), tiles, lwt, key_frames, nms_threshold, merge_threshold))
            return [[_det(0, track_id=7)] if k else [(7, (0.0, 0.0, 1.0, 1.0))] for k in key_frames]

        def detect_tiled_ragged_reid(self, frames, tiles, reid, nms_threshold, merge_threshold, **kw):
            calls.append(("detect_tiled_ragged_reid", tiles, reid, nms_threshold, merge_threshold, kw))
            dets = [_det(0, features=None if kw.get("trackers") else np.ones(512, np.float32))]
            if kw.get("trackers"):
                dets[0].track_id = 4
            return [dets for _ in frames]

    big = StubLwt(calls, max_tracks=512)
    # native: one call of the wrapped detector's method
    td = TiledDetector(Native(), native=True, nms_threshold=0.3, merge_threshold=0.6)
    assert [d.track_id for d in td.detect_and_track_hybrid(frame, big)] == [7]
    out = td.track_hybrid_batch([frame, frame], big, [1, 0])
    assert calls == [("detect_tiled_hybrid", 1, grid, [big], 0.3, 0.6), ("track_tiled_hybrid_batch", 2, grid, big, [True, False], 0.3, 0.6)]
    assert out[1] == [(7, (0.0, 0.0, 1.0, 1.0))]
    with pytest.raises(ValueError, match="key flags"):
        td.track_hybrid_batch([frame], big, [1, 0])

    def fallback(td, lwt, fr=frame, first="detect_tiled"):
        del calls[:]
        td.detect_and_track_hybrid(fr, lwt)
        td.track_hybrid_batch([fr, fr], lwt, [False, True])
        assert [c[0] for c in calls] == [first, "update_with_detections", "interpolate", first, "update_with_detections"], calls

    fallback(td, StubLwt(calls, max_tracks=399))                 # no room for S = 400 records
    fallback(td, StubLwt(calls, device=1, max_tracks=512))       # another device
    fallback(TiledDetector(Plain(), native=True), big)           # the wrapped detector has no such method

    class Host(Native):
        def detect_batch(self, tiles):
            calls.append(("detect_batch", len(tiles)))
            return [[] for _ in tiles]

    del calls[:]
    TiledDetector(Host(), native=False).detect_and_track_hybrid(frame, big)   # native=False: the host tiles, then the tracker
    assert calls == [("detect_batch", 4), ("update_with_detections", 0)]
    # a mixed grid: native under mixed_sizes=True; without the keyword the loop, whose detect refuses the grid as it always did
    del calls[:]
    tm = TiledDetector(Native(), native=True, mixed_sizes=True)
    tm.detect_and_track_hybrid(odd, big)
    tm.track_hybrid_batch([odd], big, [True])
    assert [c[0] for c in calls] == ["detect_tiled_hybrid", "track_tiled_hybrid_batch"] and calls[0][2] == mixed

    class Refusing(Native):
        def detect_tiled(self, frames, tiles, nms_threshold, merge_threshold):
            raise ValueError("tiles of more than one size: one forward has one model size")

    del calls[:]
    with pytest.raises(ValueError, match="more than one size"):
        TiledDetector(Refusing(), native=True).detect_and_track_hybrid(odd, big)
    assert calls == []

    # features="reid" on a mixed grid
    ext = HipOSNetReIDExtractor(model_path="unused")
    ext._handle = C.c_void_p(1)   # "loaded" for the condition; never handed to the library
    rows = []
    ext.extract_features = lambda image, bboxes: (rows.append(len(bboxes)), np.full((len(bboxes), 512), 2.0, np.float32))[1]

    class Tracker:
        def update(self, dets):
            calls.append(("update", len(dets)))
            return list(dets)

    tracker = Tracker()
    try:
        del calls[:]
        dets, feats = tm.detect_with_features(odd, features="reid", reid=ext, reid_slots=7)
        assert feats.shape == (1, 512) and feats[0, 0] == 1.0
        assert [d.track_id for d in tm.detect_and_track(odd, tracker, features="reid", reid=ext)] == [4]
        assert calls == [("detect_tiled_ragged_reid", mixed, ext, 0.4, 0.5, {"reid_slots": 7}), ("detect_tiled_ragged_reid", mixed, ext, 0.4, 0.5, {"reid_slots": 32, "trackers": [tracker]})]
        assert rows == []
        # a detector without the method: the separate Re-ID call on the merged detections, as before
        del calls[:]
        dets, feats = TiledDetector(Plain(), native=True, mixed_sizes=True).detect_with_features(odd, features="reid", reid=ext)
        assert [c[0] for c in calls] == ["detect_tiled_ragged"] and rows == [1] and feats[0, 0] == 2.0
        # a grid of one size goes where it went
        del calls[:]
        tm.detect_with_features(frame, features="reid", reid=ext)
        assert [c[0] for c in calls] == ["detect_tiled_reid"]
    finally:
        ext._handle = None
