"""CPU tests of the stages of a tiled call: the declarations of ``opd_detr_detect_tiled_stages`` against the header, every refusal that needs no
handle (before any device call: a null handle is the LAST thing reported), the Python surface and its forwarding on stubbed detectors, and the
hand-made records of tests/tile_stages_common.py themselves."""

import ctypes as C
import os
import re

import numpy as np
import pytest

import tile_stages_common as TS
from office_person_detection_vit_amd import HipDetrDetector, TiledDetector, _capi
from office_person_detection_vit_amd.data_models import Detection
from office_person_detection_vit_amd.tiling import tile_grid

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "opd_detr.h")


@pytest.fixture(scope="module")
def lib():
    return _capi.load_library(test_hooks=True)


def test_declarations_match_the_header():
    text = open(HEADER).read()
    body = re.search(r"typedef struct opd_tile_stages \{(.*?)\} opd_tile_stages;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.split(r"[\s\*]+", decl.strip())[-1] for decl in body.split(";") if decl.strip()]
    assert names == [f[0] for f in _capi.OpdTileStages._fields_]
    assert C.sizeof(_capi.OpdTileStages) == 56 and _capi.OpdTileStages.features.offset == 8 and _capi.OpdTileStages.n_featured.offset == 48
    proto = re.search(r"OPD_API int opd_detr_detect_tiled_stages\((.*?)\);", text, re.S).group(1)
    assert len(proto.split(",")) == len(_capi.API["opd_detr_detect_tiled_stages"][1]) == 14
    assert "opd_test_tile_stages" in _capi.TEST_API and "opd_test_tile_stages" not in text


def test_hand_made_records_hold_the_cases():
    recs = TS.merged([8, 3])
    assert recs.shape == (2, TS.S) and recs.dtype.itemsize == 48
    x, y, w, h = recs[0, :8]["x"], recs[0, :8]["y"], recs[0, :8]["w"], recs[0, :8]["h"]
    assert (x % 1 != 0).any() and (w == 0).any() and (x < 0).any() and (x > TS.FRAME_HW[1]).any() and ((x + w > TS.FRAME_HW[1]) & (x < TS.FRAME_HW[1])).any()
    assert (recs[1, 3:]["query_index"] == -7).all() and len(set(recs[0]["query_index"].tolist())) < TS.S   # decoys; query numbers repeat
    _, boxes, foot, conf = TS.host_arrays(recs[0], 8)
    assert boxes.dtype == foot.dtype == conf.dtype == np.float32 and boxes[2, 0] == 16.0
    rounded = np.float32(boxes[:, 0].astype(np.float64) + boxes[:, 2].astype(np.float64) / 2.0)
    assert (rounded != foot[:, 0]).any(), "no record tells the float64 foot point from the foot point of the rounded box"


def test_arguments_are_refused_before_any_device_call(lib):
    grid = np.asarray(tile_grid(40, 52, 2, 2, 0.125), np.int32)
    p = _capi.OpdTileParams(struct_size=C.sizeof(_capi.OpdTileParams), person_label=1, tile_nms_threshold=0.4, merge_nms_threshold=0.4, merge_threshold=0.5,
                            edge_tolerance=0.01)
    frame = np.zeros((40, 52, 3), np.uint8)
    ptrs = (C.c_void_p * 1)(frame.ctypes.data)
    out, counts = (_capi.OpdTileDet * 400)(), (C.c_int32 * 1)()
    buf = np.zeros(64, np.int32)
    dummy = buf.ctypes.data   # stands for a handle or an output: never dereferenced before the refusal

    def refused(text, stages=True, h=40, w=52, tiles=grid, params=p, o=out, struct_size=C.sizeof(_capi.OpdTileStages), **kw):
        st = _capi.OpdTileStages(struct_size=struct_size, **kw)
        rc = lib.opd_detr_detect_tiled_stages(None, ptrs, 1, h, w, tiles.ctypes.data_as(C.c_void_p), 4, 32, 40, 0.05, None if params is None else C.byref(params),
                                              C.byref(st) if stages else None, o, counts)
        assert rc == _capi.OPD_EINVAL and text in _capi.last_error(), (text, _capi.last_error())
        assert _capi.last_error().startswith("opd_detr_detect_tiled_stages") or text == "null model handle"

    refused("null model handle")
    refused("null model handle", feature_kind=_capi.OPD_TRACK_FEAT_COLOR, features=dummy, floor=dummy, floor_out=dummy, trackers=dummy, track_ids=dummy, n_featured=dummy)
    refused("stages", stages=False)
    refused("opd_tile_stages.struct_size", struct_size=48)
    refused("opd_tile_stages.struct_size", struct_size=0)
    for kind in (_capi.OPD_TRACK_FEAT_ENCODER, _capi.OPD_TRACK_FEAT_REID, 7, -1):
        refused("feature_kind", feature_kind=kind)
    refused("features given with feature_kind OPD_TRACK_FEAT_NONE", features=dummy)
    refused("floor_out is null", floor=dummy)
    refused("track_ids or n_featured is null", trackers=dummy)
    refused("track_ids or n_featured is null", trackers=dummy, track_ids=dummy)
    refused("track_ids or n_featured is null", trackers=dummy, n_featured=dummy)
    # colour features above the colour kernel's 4096 limit (the windows are checked first: they must lie on the frame)
    wide = np.asarray(tile_grid(40, 4098, 2, 2, 0.125), np.int32)
    refused("feature_kind OPD_TRACK_FEAT_COLOR on frames of 40 x 4098", feature_kind=_capi.OPD_TRACK_FEAT_COLOR, w=4098, tiles=wide)
    refused("null model handle", w=4098, tiles=wide)   # (without colour features the size is no refusal)
    # what opd_detr_detect_tiled refuses, in this entry's name
    refused("null argument", o=None)
    refused("null argument", params=None)
    outside = grid.copy(); outside[3, 1] += 1
    refused("lies outside the 40 x 52 frame", tiles=outside)
    refused("more than one size", tiles=np.asarray(tile_grid(41, 52, 2, 2, 0.125), np.int32), h=41)
    refused("tile_nms_threshold", params=_capi.OpdTileParams(struct_size=C.sizeof(_capi.OpdTileParams), person_label=1, tile_nms_threshold=float("nan")))
    # and the plain entry still words its refusals in its own name
    rc = lib.opd_detr_detect_tiled(None, ptrs, 1, 40, 52, grid.ctypes.data_as(C.c_void_p), 4, 32, 40, 0.05, C.byref(p), None, counts)
    assert rc == _capi.OPD_EINVAL and _capi.last_error() == "opd_detr_detect_tiled: null argument"


def _det(k, **kw):
    return Detection(bbox=(10.0 * k, 5.0, 20.0, 40.0), confidence=0.9 - 0.1 * k, class_id=1, class_name="person", camera_coords=(10.0 * k + 10.0, 45.0), query_index=k, **kw)


def test_python_surface_on_stubs():
    frame = np.zeros((40, 52, 3), np.uint8)
    grid = tile_grid(40, 52, 2, 2, 0.125)
    det = HipDetrDetector(model_path="unused", max_batch=8)
    det.model = 1   # (never dereferenced: every check below comes before the library call)
    try:
        with pytest.raises(ValueError, match="encoder"):
            det.detect_tiled_stages([frame], grid, features="encoder")
        with pytest.raises(ValueError, match="None or 'color'"):
            det.detect_tiled_stages([frame], grid, features="reid")
        with pytest.raises(ValueError, match="1 trackers for 2 frames"):
            det.detect_tiled_stages([frame, frame], grid, trackers=[object()])
        t = object()
        with pytest.raises(ValueError, match="named twice"):
            det.detect_tiled_stages([frame, frame], grid, trackers=[t, t])
        assert det.detect_tiled_stages([], grid, features="color", trackers=[]) == []
    finally:
        det.model = None

    calls = []

    class Native:   # a detector with detect_tiled and detect_tiled_stages: what TiledDetector(native=True) forwards
        def detect_tiled(self, frames, tiles, nms_threshold, merge_threshold):
            return self.detect_tiled_stages(frames, tiles, nms_threshold, merge_threshold)

        def detect_tiled_stages(self, frames, tiles, nms_threshold, merge_threshold, **kw):
            calls.append((len(frames), tiles, nms_threshold, merge_threshold, kw))
            dets = [_det(0, features=np.ones(256, np.float32) if kw.get("features") else None), _det(1, features=np.zeros(256, np.float32) if kw.get("features") else None)]
            if kw.get("trackers"):
                dets[0].track_id = 4
            return [dets for _ in frames]

    td = TiledDetector(Native(), native=True, nms_threshold=0.3, merge_threshold=0.6)
    fm, tracker = object(), object()
    td.detect_batch([frame])
    td.detect(frame, floor_map=fm)
    dets, rows = td.detect_with_features(frame)
    assert rows.shape == (2, 256) and rows[0, 0] == 1.0
    tracked = td.detect_and_track(frame, tracker)
    assert [d.track_id for d in tracked] == [4]
    td.detect_and_track(frame, tracker, features=None)
    assert [c[4] for c in calls] == [{}, {"floor_map": fm}, {"features": "color"}, {"features": "color", "trackers": [tracker]}, {"features": None, "trackers": [tracker]}]
    assert all(c[:4] == (1, grid, 0.3, 0.6) for c in calls)
    for bad in ("encoder",):
        with pytest.raises(ValueError, match="encoder"):
            td.detect_with_features(frame, features=bad)
        with pytest.raises(ValueError, match="encoder"):
            td.detect_and_track(frame, tracker, features=bad)
    with pytest.raises(ValueError, match="needs reid="):
        td.detect_with_features(frame, features="reid")
    with pytest.raises(ValueError, match="features must be"):
        td.detect_with_features(frame, features=None)

    class Reid:
        def extract_features(self, frame, bboxes):
            return np.full((len(bboxes), 512), 2.0, np.float32)

    del calls[:]
    dets, rows = td.detect_with_features(frame, features="reid", reid=Reid())   # detect_tiled, then the Re-ID call
    assert calls[0][4] == {} and rows.shape == (2, 512) and dets[1].features[0] == 2.0

    class Host:   # native=False: the host composition of the same calls
        def detect_batch(self, tiles):
            return [[_det(0)] if i == 0 else [] for i in range(len(tiles))]

        def extract_color_features(self, frame, dets):
            return np.full((len(dets), 256), 3.0, np.float32)

    class Floor:
        def apply(self, dets):
            for d in dets:
                d.zone_ids = ["z"]

    class Tracker:
        def update(self, dets):
            for d in dets:
                d.track_id = 9
            return list(dets)

    host = TiledDetector(Host(), native=False)
    assert [d.zone_ids for d in host.detect(frame, floor_map=Floor())] == [["z"]]
    assert host.detect(frame)[0].zone_ids in (None, [])
    dets, rows = host.detect_with_features(frame)
    assert rows.shape == (1, 256) and dets[0].features[0] == 3.0
    tracked = host.detect_and_track(frame, Tracker(), features="color")
    assert tracked[0].track_id == 9 and tracked[0].features[0] == 3.0
    assert host.detect_and_track(frame, Tracker(), features=None)[0].features is None


def test_native_needs_detect_tiled():
    class Plain:
        def detect_batch(self, frames):
            return [[] for _ in frames]

    frame = np.zeros((40, 52, 3), np.uint8)
    td = TiledDetector(Plain(), native=True)

    class Half(Plain):   # the plain tiled call alone: the staged methods are refused, there is no silent host composition
        def detect_tiled(self, frames, tiles, nms_threshold, merge_threshold):
            return [[] for _ in frames]

    half = TiledDetector(Half(), native=True)
    assert half.detect_batch([frame]) == [[]]
    for call in (lambda: half.detect(frame, floor_map=object()), lambda: half.detect_with_features(frame), lambda: half.detect_and_track(frame, object())):
        with pytest.raises(ValueError, match="detect_tiled"):
            call()
    for call in (lambda: td.detect_batch([frame]), lambda: td.detect(frame, floor_map=object()), lambda: td.detect_with_features(frame),
                 lambda: td.detect_and_track(frame, object())):
        with pytest.raises(ValueError, match="detect_tiled"):
            call()
