"""CPU characterization of the Python call path of the tiled methods of ``HipDetrDetector``: what each of the seven native tiled entries is handed
(argument count, model size, stage block, frame pointers per chunk) and what is made of what it writes (detections, feature rows by position or by
slot, floor rows, tracker mirrors, the out-of-slots rule, the runs of the hybrid sequences, the separate-calls fallbacks).  The library is a recording
fake and the tracker, floor-map and Re-ID objects are stubs: no GPU call is made."""

import ctypes as C

import numpy as np
import pytest

from office_person_detection_vit_amd import HipDetrDetector, _capi
from office_person_detection_vit_amd.data_models import Detection
from office_person_detection_vit_amd.tiling import tile_grid

Q, T = 100, 4
S = T * Q
E = 8   # feature width of the stub Re-ID model
GRID, MIXED = tile_grid(40, 52, 2, 2, 0.125), tile_grid(41, 52, 2, 2, 0.125)
FLOOR_DTYPE = np.dtype([("v", np.float64), ("tag", np.int64)])
OUT_OF_SLOTS = "tracker 0 is out of slots: the frame is counted as one without detections"

_HEAD = ["model", "frames", "n", "h", "w", "win", "T"]
_TAIL = ["recs", "counts"]
LAYOUT = {
    "opd_detr_detect_tiled": _HEAD + ["H", "W", "thr", "params"] + _TAIL,
    "opd_detr_detect_tiled_stages": _HEAD + ["H", "W", "thr", "params", "block"] + _TAIL,
    "opd_detr_detect_tiled_reid": _HEAD + ["H", "W", "thr", "params", "block"] + _TAIL,
    "opd_detr_detect_tiled_ragged": _HEAD + ["tile_hw", "thr", "params", "block"] + _TAIL,
    "opd_detr_detect_tiled_ragged_reid": _HEAD + ["tile_hw", "thr", "params", "block"] + _TAIL,
    "opd_detr_detect_tiled_hybrid": _HEAD + ["H", "W", "tile_hw", "thr", "params", "block"] + _TAIL,
    "opd_detr_detect_tiled_sequence_hybrid": ["model", "lwt", "frames", "flags", "F", "h", "w", "win", "T", "H", "W", "tile_hw", "thr", "params", "recs", "counts", "ids",
                                              "lrecs", "cap", "lcounts", "done"],
    "opd_detr_detect_sequence_hybrid": ["model", "lwt", "frames", "flags", "F", "h", "w", "H", "W", "thr", "label", "recs", "counts", "ids", "lrecs", "cap", "lcounts", "done"],
}


def _addr(x):
    """Address in whatever form a ctypes argument was given: None, int, c_void_p, a cast pointer or an array."""
    if x is None:
        return 0
    if isinstance(x, int):
        return x
    if isinstance(x, C.c_void_p):
        return x.value or 0
    if isinstance(x, C.Array):
        return C.addressof(x)
    return C.cast(x, C.c_void_p).value or 0


def _obj(x):
    """The structure behind ``C.byref(s)`` / ``C.pointer(s)`` / ``s``; None stays None."""
    if x is None:
        return None
    if hasattr(x, "_obj"):
        return x._obj
    return x.contents if hasattr(x, "contents") else x


def _i32(addr, n):
    return np.ctypeslib.as_array((C.c_int32 * n).from_address(addr))


def n_records(g):
    """How many merged records the fake gives frame number ``g`` of a call sequence (2, 3, 1, 2, 3, ...)."""
    return (g + 1) % 3 + 1


def record(g, k):
    return dict(x=100.0 * g + k + 0.25, y=k + 0.5, w=10.0 + k, h=20.0 + g, score=np.float32(0.9 - 0.01 * k), label=1, query_index=7 * k + g, tile=k % T)


class FakeLib:
    """Stands for libopd_hip.so: every tiled entry records what it was handed and fills the caller's buffers with known values."""

    def __init__(self, frames, rc=0):
        self.index = {f.ctypes.data: g for g, f in enumerate(frames)}   # frame pointer -> number of the frame in the whole call
        self.calls, self.rc = [], rc

    def __getattr__(self, name):
        if name not in LAYOUT:
            raise AssertionError(f"an entry the test does not expect was called: {name}")
        return lambda *args: self._call(name, args)

    def _call(self, name, args):
        assert len(args) == len(_capi.API[name][1]) == len(LAYOUT[name]), name
        a = dict(zip(LAYOUT[name], args))
        n = a["F"] if "F" in a else a["n"]
        gs = [self.index[p] for p in list(a["frames"])[:n]]
        assert len(a["frames"]) == n
        params = _obj(a["params"]) if "params" in a else None
        seen = dict(name=name, frames=gs, h=a["h"], w=a["w"], H=a.get("H"), W=a.get("W"), thr=a["thr"], model=_addr(a["model"]))
        if "win" in a:
            seen.update(T=a["T"], win=_i32(_addr(a["win"]), 4 * a["T"]).reshape(-1, 4).tolist())
            seen["tile_hw"] = _i32(_addr(a["tile_hw"]), 2 * a["T"]).reshape(-1, 2).tolist() if _addr(a.get("tile_hw")) else None
            seen["params"] = {f[0]: getattr(params, f[0]) for f in params._fields_}
        self.calls.append(seen)
        if "flags" in a:
            return self._sequence(name, a, gs, seen)
        block = _obj(a.get("block"))
        seen["block"] = None if block is None else {f[0]: getattr(block, f[0]) for f in block._fields_}
        seen["block_type"] = type(block).__name__ if block is not None else None
        total = 0
        for b, g in enumerate(gs):
            a["counts"][b] = n_records(g)
            for k in range(n_records(g)):
                for key, v in record(g, k).items():
                    setattr(a["recs"][b * S + k], key, v)
            total += n_records(g)
        if block is None:
            return self.rc
        positions = [(b, g, k) for b, g in enumerate(gs) for k in range(n_records(g))]
        if getattr(block, "floor_out", None):
            assert block.floor
            floor = np.ctypeslib.as_array((C.c_uint8 * (n * S * FLOOR_DTYPE.itemsize)).from_address(block.floor_out)).view(FLOOR_DTYPE)
            assert not floor.view(np.uint8).any()   # handed over zeroed
            for b, g, k in positions:
                floor[b * S + k] = (10.0 * g + k, 1)
        if getattr(block, "trackers", None):
            seen["handles"] = [int(v) for v in (C.c_void_p * n).from_address(block.trackers)]
            ids = _i32(block.track_ids, n * S)
            assert (ids == -1).all()
            for b, g, k in positions:
                ids[b * S + k] = 1000 * g + k
            if hasattr(block, "n_featured"):
                _i32(block.n_featured, n)[:] = [n_records(g) for g in gs]
        if isinstance(block, _capi.OpdTileStages) and block.features:
            feats = np.ctypeslib.as_array((C.c_float * (n * S * 256)).from_address(block.features)).reshape(n, S, 256)
            for b, g, k in positions:
                feats[b, k] = 1000.0 * g + k
        if isinstance(block, _capi.OpdTileReidStages):
            slots = block.slots
            slot_map = _i32(block.slot_map, slots)
            assert (slot_map == -1).all()
            _i32(block.n_person, 1)[0] = total   # (may pass the slots: the caller clamps)
            for r, (b, g, k) in enumerate(positions[:slots]):
                slot_map[r] = b * S + k
                if block.features:
                    np.ctypeslib.as_array((C.c_float * (slots * E)).from_address(block.features)).reshape(slots, E)[r] = 1000.0 * g + k
        return self.rc

    def _sequence(self, name, a, gs, seen):
        F = a["F"]
        keys = [bool(v) for v in (C.c_uint8 * F).from_address(_addr(a["flags"]))]
        seen.update(keys=keys, cap=a["cap"], lwt=_addr(a["lwt"]))
        stride = S if "win" in a else Q
        ids = _i32(_addr(a["ids"]), max(sum(keys), 1) * stride)
        k = j = 0
        for g, key in zip(gs, keys):
            if key:
                a["counts"][k] = n_records(g)
                for i in range(n_records(g)):
                    r = record(g, i)
                    if "win" in a:
                        for field, v in r.items():
                            setattr(a["recs"][k * stride + i], field, v)
                    else:
                        rec = a["recs"][k * stride + i]
                        rec.x1, rec.y1, rec.x2, rec.y2, rec.score, rec.label, rec.query_index, rec.frame = r["x"], r["y"], r["x"] + r["w"], r["y"] + r["h"], r["score"], 1, r["query_index"], k
                    ids[k * stride + i] = 1000 * g + i
                k += 1
            else:
                a["lcounts"][j] = 1 + g % 2
                for i in range(1 + g % 2):
                    rec = a["lrecs"][j * a["cap"] + i]
                    rec.track_id = 1000 * g + i
                    rec.bbox[:] = [g + 0.5, i + 0.25, 3.0, 4.0]
                j += 1
        _obj(a["done"]).value = F
        return self.rc


class Info:
    num_queries, d_model = Q, 256


def make_detector(lib):
    det = HipDetrDetector(model_path="unused", max_batch=8, confidence_threshold=0.625)
    det.model, det._lib, det._info = 1234, lib, Info()
    det.nms_threshold = 0.375
    return det


class StubTracker:
    device_ordinal, max_dets = 0, S

    def __init__(self, number, log, feature_dim=256, max_dets=S):
        self.number, self.log, self.feature_dim, self.max_dets, self._h = number, log, feature_dim, max_dets, None

    def _ensure(self):
        self._h = C.c_void_p(5000 + self.number)

    def _apply(self, dets, ids):
        assert isinstance(ids, np.ndarray)
        self.log.append(("_apply", self.number, len(dets), [int(v) for v in ids]))
        for d, v in zip(dets, ids):
            d.track_id = int(v)

    def update(self, dets):
        self.log.append(("update", self.number, len(dets)))
        return list(dets)


class StubLwt:
    SEQUENCE_MAX = 64
    device = 0

    def __init__(self, number, log, max_tracks=S, handle=False):
        self.number, self.log, self.max_tracks = number, log, max_tracks
        self._h = C.c_void_p(6000 + number) if handle else None

    def _ensure(self, h, w):
        self.log.append(("_ensure", self.number, h, w))
        self._h = C.c_void_p(6000 + self.number)

    def _adopt(self, dets, ids):
        assert isinstance(ids, list) and all(isinstance(v, int) for v in ids)
        self.log.append(("_adopt", self.number, len(dets), ids))
        for d, v in zip(dets, ids):
            d.track_id = v
        return dets

    def update_with_detections(self, frame, dets):
        self.log.append(("update_with_detections", self.number, len(dets)))
        return dets

    def interpolate(self, frame):
        self.log.append(("interpolate", self.number))
        return [(1, (0.0, 0.0, 1.0, 1.0))]


class StubFloor:
    device, REC_DTYPE = 0, FLOOR_DTYPE

    def __init__(self, log):
        self.log = log

    def _require(self):
        return C.c_void_p(7777)

    def _fill(self, det, row):
        assert int(row["tag"]) == 1
        det.floor_coords = (float(row["v"]), 0.0)

    def apply(self, dets):
        self.log.append(("apply", len(dets)))


class StubReid:
    is_loaded, feature_dim, max_crops = True, E, 64

    def __init__(self, log, handle=True):
        self.log = log
        self._handle = C.c_void_p(8888) if handle else None

    def _ordinal(self):
        return 0

    def extract_features_batch(self, frames, boxes):
        self.log.append(("extract_features_batch", [f.ctypes.data for f in frames], [list(b) for b in boxes]))
        return np.asarray([[-(bb[0])] * E for b in boxes for bb in b], np.float32).reshape(-1, E)

    def extract_features(self, frame, boxes):
        self.log.append(("extract_features", len(boxes)))
        return np.full((len(boxes), E), 3.0, np.float32)


def frames_of(mixed, count):
    return [np.full((41 if mixed else 40, 52, 3), g, np.uint8) for g in range(count)]


def expected(g, k, **kw):
    r = record(g, k)
    bbox = (r["x"], r["y"], r["w"], r["h"])
    return Detection(bbox=bbox, confidence=float(r["score"]), class_id=1, class_name="person", camera_coords=(bbox[0] + bbox[2] / 2, bbox[1] + bbox[3]),
                     query_index=r["query_index"], **kw)


def same(got, want):
    """Field for field, feature rows by value."""
    assert len(got) == len(want)
    for a, b in zip(got, want):
        fa, fb = a.features, b.features
        assert (fa is None) == (fb is None) and (fa is None or (fa.dtype == np.float32 and np.array_equal(fa, fb)))
        assert {**vars(a), "features": None} == {**vars(b), "features": None}
        assert type(a.class_id) is int and type(a.query_index) is int and type(a.confidence) is float


PLAIN = dict(merge_nms_threshold=0.25, merge_threshold=0.75, edge_tolerance=0.03125)


def check_call_set_up(det, lib, mixed, n_frames, spelling):
    """Chunks of 2 then 1 frames, every pointer once and in order, the windows, the parameter block and the model size in the entry's spelling."""
    grid = MIXED if mixed else GRID
    assert [c["frames"] for c in lib.calls] == [list(range(i, min(i + 2, n_frames))) for i in range(0, n_frames, 2)]
    sizes = det.tile_model_sizes(grid)
    assert (len(set(sizes)) == 1) == (not mixed)
    for c in lib.calls:
        assert (c["h"], c["w"], c["T"], c["win"], c["model"]) == (41 if mixed else 40, 52, T, [list(t) for t in grid], 1234)
        assert c["thr"] == 0.625
        assert c["params"] == dict(struct_size=C.sizeof(_capi.OpdTileParams), person_label=1, tile_nms_threshold=0.375, pad=0.0, **PLAIN)
        if spelling == "HW":
            assert (c["H"], c["W"]) == sizes[0] and c["tile_hw"] is None
        elif spelling == "tile_hw":
            assert c["H"] is None and c["tile_hw"] == [list(s) for s in sizes]
        else:   # (H, W, tile_HW or NULL)
            assert ((c["H"], c["W"]), c["tile_hw"]) == (((0, 0), [list(s) for s in sizes]) if mixed else (sizes[0], None))
    assert det._last_orig == [(41 if mixed else 40, 52)] * n_frames


# ---- the plain calls ------------------------------------------------------------------------------------------------------------------------------
def test_detect_tiled_chunks_and_decodes():
    frames = frames_of(False, 3)
    lib = FakeLib(frames)
    det = make_detector(lib)
    out = det.detect_tiled(frames, GRID, 0.25, 0.75, 0.03125)
    assert [c["name"] for c in lib.calls] == ["opd_detr_detect_tiled"] * 2
    check_call_set_up(det, lib, False, 3, "HW")
    for g, dets in enumerate(out):
        same(dets, [expected(g, k) for k in range(n_records(g))])


@pytest.mark.parametrize("mixed", [False, True])
def test_detect_tiled_ragged_without_stages_hands_a_null_block(mixed):
    frames = frames_of(mixed, 3)
    lib = FakeLib(frames)
    det = make_detector(lib)
    out = det.detect_tiled_ragged(frames, MIXED if mixed else GRID, 0.25, 0.75, 0.03125)
    assert [c["name"] for c in lib.calls] == ["opd_detr_detect_tiled_ragged"] * 2 and all(c["block"] is None for c in lib.calls)
    check_call_set_up(det, lib, mixed, 3, "tile_hw")
    for g, dets in enumerate(out):
        same(dets, [expected(g, k) for k in range(n_records(g))])


def test_detect_tiled_stages_without_stages_is_detect_tiled():
    frames = frames_of(False, 1)
    lib = FakeLib(frames)
    det = make_detector(lib)
    seen = []
    det.detect_tiled = lambda *a: (seen.append(a), "result")[1]
    assert det.detect_tiled_stages(frames, GRID, 0.25, 0.75, 0.03125) == "result"
    assert seen == [(frames, GRID, 0.25, 0.75, 0.03125)] and lib.calls == []


# ---- the stage block of opd_detr_detect_tiled_stages / _ragged ---------------------------------------------------------------------------------------
STAGED = [("detect_tiled_stages", "opd_detr_detect_tiled_stages", False, "HW"), ("detect_tiled_ragged", "opd_detr_detect_tiled_ragged", False, "tile_hw"),
          ("detect_tiled_ragged", "opd_detr_detect_tiled_ragged", True, "tile_hw")]


@pytest.mark.parametrize("method,entry,mixed,spelling", STAGED)
@pytest.mark.parametrize("features,with_floor,with_trackers", [("color", False, False), (None, True, False), ("color", True, True), (None, False, True)])
def test_stages_block_and_rows_by_position(method, entry, mixed, spelling, features, with_floor, with_trackers):
    frames = frames_of(mixed, 3)
    lib, log = FakeLib(frames), []
    det = make_detector(lib)
    trackers = [StubTracker(g, log) for g in range(3)] if with_trackers else None
    out = getattr(det, method)(frames, MIXED if mixed else GRID, 0.25, 0.75, 0.03125, features=features, floor_map=StubFloor(log) if with_floor else None, trackers=trackers)
    assert [c["name"] for c in lib.calls] == [entry] * 2
    check_call_set_up(det, lib, mixed, 3, spelling)
    for c in lib.calls:
        blk = c["block"]
        assert c["block_type"] == "OpdTileStages" and blk["struct_size"] == C.sizeof(_capi.OpdTileStages) == 56
        assert blk["feature_kind"] == (_capi.OPD_TRACK_FEAT_COLOR if features == "color" else _capi.OPD_TRACK_FEAT_NONE)
        assert bool(blk["features"]) == (features == "color" and not with_trackers)
        assert (bool(blk["floor"]), bool(blk["floor_out"])) == (with_floor, with_floor) and (not with_floor or blk["floor"] == 7777)
        assert (bool(blk["trackers"]), bool(blk["track_ids"]), bool(blk["n_featured"])) == (with_trackers,) * 3
        if with_trackers:
            assert c["handles"] == [5000 + g for g in c["frames"]]
    for g, dets in enumerate(out):
        want = [expected(g, k, floor_coords=(10.0 * g + k, 0.0) if with_floor else None, track_id=1000 * g + k if with_trackers else None,
                         features=np.full(256, 1000.0 * g + k, np.float32) if features == "color" and not with_trackers else None) for k in range(n_records(g))]
        same(dets, want)
    assert log == ([("_apply", g, n_records(g), [1000 * g + k for k in range(n_records(g))]) for g in range(3)] if with_trackers else [])


# ---- the Re-ID block and rows by slot -------------------------------------------------------------------------------------------------------------------
REID = [("detect_tiled_reid", "opd_detr_detect_tiled_reid", False, "HW"), ("detect_tiled_ragged_reid", "opd_detr_detect_tiled_ragged_reid", False, "tile_hw"),
        ("detect_tiled_ragged_reid", "opd_detr_detect_tiled_ragged_reid", True, "tile_hw")]


@pytest.mark.parametrize("method,entry,mixed,spelling", REID)
@pytest.mark.parametrize("with_floor,with_trackers", [(False, False), (True, False), (True, True)])
def test_reid_block_and_rows_by_slot(method, entry, mixed, spelling, with_floor, with_trackers):
    frames = frames_of(mixed, 3)
    lib, log = FakeLib(frames), []
    det = make_detector(lib)
    reid = StubReid(log)
    trackers = [StubTracker(g, log, feature_dim=E) for g in range(3)] if with_trackers else None
    # 2 slots per frame: the chunk of frames 0, 1 (2 + 3 records) has 4 slots, the chunk of frame 2 (1 record) has 2
    out = getattr(det, method)(frames, MIXED if mixed else GRID, reid, 0.25, 0.75, 0.03125, reid_slots=2, floor_map=StubFloor(log) if with_floor else None, trackers=trackers)
    assert [c["name"] for c in lib.calls] == [entry] * 2
    check_call_set_up(det, lib, mixed, 3, spelling)
    for c, slots in zip(lib.calls, (4, 2)):
        blk = c["block"]
        assert c["block_type"] == "OpdTileReidStages" and blk["struct_size"] == C.sizeof(_capi.OpdTileReidStages) == 80
        assert (blk["slots"], blk["reid"]) == (slots, 8888) and blk["slot_map"] and blk["n_person"]
        assert bool(blk["features"]) == (not with_trackers)
        assert (bool(blk["floor"]), bool(blk["floor_out"])) == (with_floor, with_floor)
        assert (bool(blk["trackers"]), bool(blk["track_ids"]), bool(blk["n_featured"])) == (with_trackers,) * 3
        if with_trackers:
            assert c["handles"] == [5000 + g for g in c["frames"]]
    beyond = {(1, 2)}   # the fifth record of the first chunk has no slot
    for g, dets in enumerate(out):
        want = []
        for k in range(n_records(g)):
            row = None if with_trackers else np.full(E, -record(g, k)["x"] if (g, k) in beyond else 1000.0 * g + k, np.float32)
            want.append(expected(g, k, floor_coords=(10.0 * g + k, 0.0) if with_floor else None, track_id=1000 * g + k if with_trackers else None, features=row))
        same(dets, want)
    applies = [("_apply", g, n_records(g), [1000 * g + k for k in range(n_records(g))]) for g in range(3)]
    r = record(1, 2)
    fetch = ("extract_features_batch", [frames[0].ctypes.data, frames[1].ctypes.data], [[], [(r["x"], r["y"], r["w"], r["h"])]])
    assert log == (applies if with_trackers else [fetch])   # ONE standalone call, for the one chunk that ran out of slots, boxes per frame


# ---- out of slots: the mirrors follow, then the error with the message of the call -------------------------------------------------------------------
@pytest.mark.parametrize("method,entry,mixed", [(m, e, x) for m, e, x, _ in STAGED + REID])
def test_out_of_slots_applies_every_mirror_of_the_chunk_then_raises(method, entry, mixed, monkeypatch):
    frames = frames_of(mixed, 3)
    lib, log = FakeLib(frames, rc=_capi.OPD_EINVAL), []
    det = make_detector(lib)
    text = [f"{entry}: {OUT_OF_SLOTS}"]
    monkeypatch.setattr(_capi, "last_error", lambda: text[0])
    reid = "reid" in method
    trackers = [StubTracker(g, log, feature_dim=E if reid else 256) for g in range(3)]
    first_apply = trackers[0]._apply
    trackers[0]._apply = lambda dets, ids: (first_apply(dets, ids), text.__setitem__(0, "a later call of the library replaced the message"))[0]
    args = (frames, MIXED if mixed else GRID) + ((StubReid(log),) if reid else ())
    with pytest.raises(RuntimeError) as err:
        getattr(det, method)(*args, trackers=trackers)
    assert str(err.value) == f"{entry} failed (code {_capi.OPD_EINVAL}): {entry}: {OUT_OF_SLOTS}"
    assert len(lib.calls) == 1   # the first chunk: its two mirrors were applied, the second chunk never ran
    assert log == [("_apply", g, n_records(g), [1000 * g + k for k in range(n_records(g))]) for g in range(2)]


def test_another_failure_is_raised_at_once(monkeypatch):
    frames = frames_of(False, 2)
    lib, log = FakeLib(frames, rc=_capi.OPD_EINVAL), []
    det = make_detector(lib)
    monkeypatch.setattr(_capi, "last_error", lambda: "opd_detr_detect_tiled_stages: something else")
    with pytest.raises(RuntimeError, match=r"opd_detr_detect_tiled_stages failed \(code -?\d+\): opd_detr_detect_tiled_stages: something else"):
        det.detect_tiled_stages(frames, GRID, trackers=[StubTracker(g, log) for g in range(2)])
    assert log == []
    with pytest.raises(RuntimeError, match="something else"):   # without trackers the out-of-slots text is no exception either
        det.detect_tiled_stages(frames, GRID, features="color")


# ---- the hybrid block -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("with_floor", [False, True])
def test_hybrid_block_and_adopt(mixed, with_floor):
    frames = frames_of(mixed, 3)
    lib, log = FakeLib(frames), []
    det = make_detector(lib)
    lwts = [StubLwt(g, log) for g in range(3)]
    out = det.detect_tiled_hybrid(frames, MIXED if mixed else GRID, lwts, 0.25, 0.75, 0.03125, floor_map=StubFloor(log) if with_floor else None)
    assert [c["name"] for c in lib.calls] == ["opd_detr_detect_tiled_hybrid"] * 2
    check_call_set_up(det, lib, mixed, 3, "both")
    for c in lib.calls:
        blk = c["block"]
        assert c["block_type"] == "OpdTileHybrid" and blk["struct_size"] == C.sizeof(_capi.OpdTileHybrid) == 40 and blk["reserved"] == 0
        assert blk["trackers"] and blk["track_ids"] and c["handles"] == [6000 + g for g in c["frames"]]
        assert (bool(blk["floor"]), bool(blk["floor_out"])) == (with_floor, with_floor)
    h = 41 if mixed else 40
    assert log == [("_ensure", 0, h, 52), ("_ensure", 1, h, 52), ("_adopt", 0, 2, [0, 1]), ("_adopt", 1, 3, [1000, 1001, 1002]), ("_ensure", 2, h, 52), ("_adopt", 2, 1, [2000])]
    for g, dets in enumerate(out):
        same(dets, [expected(g, k, floor_coords=(10.0 * g + k, 0.0) if with_floor else None, track_id=1000 * g + k) for k in range(n_records(g))])


# ---- the hybrid sequences: runs, interleaving, the no-handle rule -------------------------------------------------------------------------------------------
def in_between(g):
    return [(1000 * g + i, (g + 0.5, i + 0.25, 3.0, 4.0)) for i in range(1 + g % 2)]


@pytest.mark.parametrize("mixed", [False, True])
def test_tiled_sequence_runs(mixed):
    frames = frames_of(mixed, 70)
    keys = [g in (0, 1, 2, 30, 68) for g in range(70)]
    lib, log = FakeLib(frames), []
    det = make_detector(lib)
    lwt = StubLwt(0, log, max_tracks=S + 3)
    out = det.track_tiled_hybrid_batch(frames, MIXED if mixed else GRID, lwt, keys, 0.25, 0.75, 0.03125)
    # per = 2 key frames cut the first run in front of the third key frame, 64 frames cut the second, the rest is the third
    assert [c["frames"] for c in lib.calls] == [[0, 1], list(range(2, 66)), list(range(66, 70))]
    sizes = det.tile_model_sizes(MIXED if mixed else GRID)
    for c in lib.calls:
        assert c["name"] == "opd_detr_detect_tiled_sequence_hybrid" and c["keys"] == [keys[g] for g in c["frames"]]
        assert (c["cap"], c["lwt"], c["T"], c["win"], c["thr"]) == (S + 3, 6000, T, [list(t) for t in (MIXED if mixed else GRID)], 0.625)
        assert ((c["H"], c["W"]), c["tile_hw"]) == (((0, 0), [list(s) for s in sizes]) if mixed else (sizes[0], None))
        assert c["params"] == dict(struct_size=C.sizeof(_capi.OpdTileParams), person_label=1, tile_nms_threshold=0.375, pad=0.0, **PLAIN)
    assert len(out) == 70
    for g in range(70):
        if keys[g]:
            same(out[g], [expected(g, k, track_id=1000 * g + k) for k in range(n_records(g))])
        else:
            assert out[g] == in_between(g)
    assert [e for e in log if e[0] == "_adopt"] == [("_adopt", 0, n_records(g), [1000 * g + k for k in range(n_records(g))]) for g in (0, 1, 2, 30, 68)]
    assert det._last_orig == [(41 if mixed else 40, 52)]   # the key frames of the last run


def test_tiled_sequence_without_handle_and_key_frame_interpolates_per_frame():
    frames = frames_of(False, 3)
    lib, log = FakeLib(frames), []
    det = make_detector(lib)
    out = det.track_tiled_hybrid_batch(frames, GRID, StubLwt(0, log), [False] * 3)
    assert lib.calls == [] and log == [("interpolate", 0)] * 3 and out == [[(1, (0.0, 0.0, 1.0, 1.0))]] * 3
    # with a handle the run is one call without key frames
    lwt = StubLwt(1, log, handle=True)
    out = det.track_tiled_hybrid_batch(frames, GRID, lwt, [False] * 3)
    assert [c["frames"] for c in lib.calls] == [[0, 1, 2]] and out == [in_between(g) for g in range(3)]


def test_frame_list_sequence_runs():
    frames = frames_of(False, 80)
    keys = [g < 9 or g == 75 for g in range(80)]
    lib, log = FakeLib(frames), []
    det = make_detector(lib)
    det.resize = False
    det.device_nms, det._nms_set = True, det.nms_threshold   # suppression on the device: the condition of the fused call
    lwt = StubLwt(0, log, max_tracks=Q)
    out = det.track_hybrid_batch(frames, lwt, keys)
    # max_batch = 8 key frames cut the first run in front of the ninth, 64 frames cut the second, the rest is the third
    assert [c["frames"] for c in lib.calls] == [list(range(8)), list(range(8, 72)), list(range(72, 80))]
    for c in lib.calls:
        assert c["name"] == "opd_detr_detect_sequence_hybrid" and c["keys"] == [keys[g] for g in c["frames"]]
        assert (c["cap"], c["lwt"], c["h"], c["w"], c["H"], c["W"], c["thr"]) == (Q, 6000, 40, 52, 40, 52, 0.625)
    for g in range(80):
        if keys[g]:
            want = []
            for k in range(n_records(g)):
                r = record(g, k)
                bbox = (float(np.float32(r["x"])), float(np.float32(r["y"])), float(np.float32(r["x"] + r["w"]) - np.float32(r["x"])),
                        float(np.float32(r["y"] + r["h"]) - np.float32(r["y"])))
                want.append(Detection(bbox=bbox, confidence=float(r["score"]), class_id=1, class_name="person", camera_coords=(bbox[0] + bbox[2] / 2, bbox[1] + bbox[3]),
                                      query_index=r["query_index"], track_id=1000 * g + k))
            same(out[g], want)
        else:
            assert out[g] == in_between(g)
    assert [e for e in log if e[0] == "_adopt"] == [("_adopt", 0, n_records(g), [1000 * g + k for k in range(n_records(g))]) for g in list(range(9)) + [75]]
    assert det._last_orig == [(40, 52)]

    del lib.calls[:], log[:]
    out = det.track_hybrid_batch(frames[:3], StubLwt(1, log), [False] * 3)   # no handle, no key frame: nothing to interpolate from inside a call
    assert lib.calls == [] and log == [("interpolate", 1)] * 3


# ---- the separate-calls fallbacks: the order of calls per frame -----------------------------------------------------------------------------------------------
def _det(k):
    return Detection(bbox=(10.0 * k, 5.0, 20.0, 40.0), confidence=0.9 - 0.1 * k, class_id=1, class_name="person", camera_coords=(10.0 * k + 10.0, 45.0), query_index=k)


class NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the library was called: {name}")


def _fallback_detector(calls):
    det = make_detector(NoLibrary())
    det.detect_tiled = lambda frames, tiles, a, b, c: (calls.append(("detect_tiled", len(frames), a, b, c)), [[_det(0), _det(1)] for _ in frames])[1]
    det.detect_tiled_ragged = lambda frames, tiles, a, b, c: (calls.append(("detect_tiled_ragged", len(frames), a, b, c)), [[_det(0)] for _ in frames])[1]
    det.extract_color_features = lambda frame, dets: (calls.append(("extract_color_features", len(dets))), np.full((len(dets), 256), 2.0, np.float32))[1]
    return det


def test_stages_fallback_composition_on_stubs():
    """Where the fused conditions fail: the plain tiled call of the method's kind, then per frame the colour rows, floor_map.apply and tracker.update."""
    calls = []
    det = _fallback_detector(calls)
    small = [StubTracker(g, calls, max_dets=S - 1) for g in range(2)]   # no room for tiles x queries records
    frames, odd = frames_of(False, 2), frames_of(True, 1)
    out = det.detect_tiled_stages(frames, GRID, 0.3, 0.6, 0.02, features="color", floor_map=StubFloor(calls), trackers=small)
    per_frame = lambda g, n: [("extract_color_features", n), ("apply", n), ("update", g, n)]
    assert calls == [("detect_tiled", 2, 0.3, 0.6, 0.02)] + per_frame(0, 2) + per_frame(1, 2)
    assert all(d.features.shape == (256,) and d.features[0] == 2.0 for dets in out for d in dets)
    del calls[:]
    HipDetrDetector.detect_tiled_ragged(det, odd, MIXED, features="color", trackers=small[:1])   # (the method itself: the attribute is the stub it falls back to)
    assert calls == [("detect_tiled_ragged", 1, 0.4, 0.5, 0.01), ("extract_color_features", 1), ("update", 0, 1)]
    del calls[:]

    class Elsewhere(StubFloor):
        device = 1

    det.detect_tiled_stages(frames[:1], GRID, floor_map=Elsewhere(calls))
    assert calls == [("detect_tiled", 1, 0.4, 0.5, 0.01), ("apply", 2)]


def test_reid_fallback_composition_on_stubs():
    """The same for the Re-ID methods: reid.extract_features on the merged boxes, floor_map.apply, tracker.update."""
    calls = []
    det = _fallback_detector(calls)
    frames, odd = frames_of(False, 2), frames_of(True, 1)
    host_only = StubReid(calls, handle=False)   # no native handle: the rows are a separate call
    trackers = [StubTracker(g, calls, feature_dim=E) for g in range(2)]
    out = det.detect_tiled_reid(frames, GRID, host_only, 0.3, 0.6, 0.02, floor_map=StubFloor(calls), trackers=trackers)
    per_frame = lambda g, n: [("extract_features", n), ("apply", n), ("update", g, n)]
    assert calls == [("detect_tiled", 2, 0.3, 0.6, 0.02)] + per_frame(0, 2) + per_frame(1, 2)
    assert all(d.features.shape == (E,) and d.features[0] == 3.0 for dets in out for d in dets)
    del calls[:]
    det.detect_tiled_ragged_reid(odd, MIXED, host_only)
    assert calls == [("detect_tiled_ragged", 1, 0.4, 0.5, 0.01), ("extract_features", 1)]
    del calls[:]
    det.detect_tiled_reid(frames[:1], GRID, StubReid(calls), trackers=[StubTracker(0, calls, feature_dim=E + 1)])   # a tracker of another feature width
    assert calls == [("detect_tiled", 1, 0.4, 0.5, 0.01), ("extract_features", 2), ("update", 0, 2)]


# ---- one fault, one message, from every method -------------------------------------------------------------------------------------------------------
def _callers(det, reid, log):
    """Every public tiled method as ``f(frames, tiles)``, and whether it takes grids of one size only."""
    n = lambda frames: [StubTracker(g, log) for g in range(len(frames))]
    return {
        "detect_tiled": (lambda fr, t: det.detect_tiled(fr, t), True),
        "detect_tiled_stages": (lambda fr, t: det.detect_tiled_stages(fr, t, trackers=n(fr)), True),
        "detect_tiled_reid": (lambda fr, t: det.detect_tiled_reid(fr, t, reid, trackers=n(fr)), True),
        "detect_tiled_ragged": (lambda fr, t: det.detect_tiled_ragged(fr, t, trackers=n(fr)), False),
        "detect_tiled_ragged_reid": (lambda fr, t: det.detect_tiled_ragged_reid(fr, t, reid, trackers=n(fr)), False),
        "detect_tiled_hybrid": (lambda fr, t: det.detect_tiled_hybrid(fr, t, [StubLwt(g, log) for g in range(len(fr))]), False),
        "track_tiled_hybrid_batch": (lambda fr, t: det.track_tiled_hybrid_batch(fr, t, StubLwt(0, log), [True] * len(fr)), False),
    }


@pytest.mark.parametrize("name", ["detect_tiled", "detect_tiled_stages", "detect_tiled_reid", "detect_tiled_ragged", "detect_tiled_ragged_reid", "detect_tiled_hybrid",
                                  "track_tiled_hybrid_batch"])
def test_single_faults_raise_the_same_message_from_every_method(name):
    log = []
    det = make_detector(NoLibrary())
    call, one_size = _callers(det, StubReid(log), log)[name]
    frame = np.zeros((40, 52, 3), np.uint8)
    with pytest.raises(ValueError, match=r"^tiles must be a non-empty list of \(y0, x0, h, w\)$"):
        call([frame], [])
    with pytest.raises(ValueError, match=r"^tiles must be a non-empty list of \(y0, x0, h, w\)$"):
        call([frame], [(0, 0, 8)])
    with pytest.raises(ValueError, match=r"^the 9 tiles of one frame exceed max_batch = 8$"):
        call([frame], [(0, 0, 8, 8)] * 9)
    for bad in ([frame, np.zeros((40, 50, 3), np.uint8)], [frame[:, ::2]], [frame.astype(np.float32)], [frame[:, :, :2]], ["frame"]):
        with pytest.raises(ValueError, match=r"^frames must be contiguous uint8 numpy arrays of shape \(H, W, 3\) in BGR order, all of one size$"):
            call(bad, GRID)
    if one_size:
        with pytest.raises(ValueError, match=r"^tiles of more than one size: one forward has one model size$"):
            call([np.zeros((41, 52, 3), np.uint8)], MIXED)
    else:
        with pytest.raises(ValueError, match=r"^tiles must have a height and a width of at least 1$"):
            call([frame], [(0, 0, 0, 8)])
        det.resize = False   # (the model sizes are the windows themselves: their canvas is refused in front of the library)
        with pytest.raises(ValueError, match=r"^ragged batch canvas 2000x1400 exceeds the configured maximum \(800, 1333\) \(either orientation\)$"):
            call([frame], [(0, 0, 2000, 8), (0, 0, 8, 1400)])
    assert call([], GRID) == [] and log == []


def test_tracker_list_faults_keep_both_wordings():
    log = []
    det = make_detector(NoLibrary())
    frame = np.zeros((40, 52, 3), np.uint8)
    t, reid = StubTracker(0, log), StubReid(log)
    for call in (lambda tr: det.detect_tiled_stages([frame, frame], GRID, trackers=tr), lambda tr: det.detect_tiled_ragged([frame, frame], GRID, trackers=tr),
                 lambda tr: det.detect_tiled_reid([frame, frame], GRID, reid, trackers=tr), lambda tr: det.detect_tiled_ragged_reid([frame, frame], GRID, reid, trackers=tr)):
        with pytest.raises(ValueError, match=r"^1 trackers for 2 frames: frame f enters trackers\[f\]$"):
            call([t])
        with pytest.raises(ValueError, match=r"^a tracker is named twice: a tracker takes one frame per call$"):
            call([t, t])
    with pytest.raises(ValueError, match=r"^1 trackers for 2 frames: frame f enters lwts\[f\]$"):
        det.detect_tiled_hybrid([frame, frame], GRID, [t])
    with pytest.raises(ValueError, match=r"^a tracker is named twice: a tracker takes one frame per call$"):
        det.detect_tiled_hybrid([frame, frame], GRID, [t, t])
    for method in (det.detect_tiled_stages, det.detect_tiled_ragged):
        with pytest.raises(ValueError, match=r"^features='encoder' does not exist for tiled detection"):
            method([frame], GRID, features="encoder")
        with pytest.raises(ValueError, match=r"^features must be None or 'color', got 'reid'$"):
            method([frame], GRID, features="reid")
    with pytest.raises(ValueError, match=r"^detect_tiled_reid needs reid= a loaded"):
        det.detect_tiled_reid([frame], GRID, None)
    with pytest.raises(ValueError, match=r"^detect_tiled_ragged_reid needs reid= a loaded"):
        det.detect_tiled_ragged_reid([frame], GRID, None)

    class Unloaded(StubReid):
        is_loaded = False

    for method in (det.detect_tiled_reid, det.detect_tiled_ragged_reid):
        with pytest.raises(RuntimeError, match=r"^Re-ID model is not loaded: call load_model\(\) first$"):
            method([frame], GRID, Unloaded(log))
