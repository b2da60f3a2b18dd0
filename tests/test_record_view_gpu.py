"""What each sink stage takes from the records of a detect call, and the row each record's output lands in (-m gpu): the rules the readers of
csrc/opd_records.h share, pinned on the hand-made records of tests/record_view_common.py (two records of another label in both forms; in the
post-process form one ``query_index`` at the stride and one below zero).  Outputs are poisoned first; every comparison is an equality with the host
twins the other tests already use.

  merged records (a tiled call): colour, floor and ingest take EVERY record below the count, whatever its label, into the row of its POSITION
      (opd_test_tile_stages); the crop selection gives a slot to the records labelled with the stage label alone, named by position, and a record
      without a slot still enters the tracker's staging image, with has = 0 (opd_test_tile_reid).
  post-process records: the ingest takes every record below the count; a feature row goes by ``query_index``, and a record whose ``query_index`` is
      no row of the frame enters with has = 0 (opd_track_test_ingest).  Colour and floor take the records labelled with the stage label alone, into
      the row ``query_index`` names; a negative stage label takes none (opd_detr_detect_frames_color / _floor on a seeded model: no hook feeds these
      two kernels hand-made post-process records, and the hooks of the tiled stages fix the stage label at 1).
  a negative ``person_label`` in the tiled calls (opd_detr_detect_tiled_stages, opd_detr_detect_tiled_reid on a seeded model): colour and floor still
      take every merged record, by position; the crop selection finds no record of that label, so no slot, no row, and trackers that see motion alone.

NOT pinned here, for want of a hook that hands ``floor_kernel`` or the colour kernels hand-made post-process records (the seeded model never emits a
``query_index`` outside its frame): the floor stage's ``(unsigned)key < stride`` test on post-process records, and that the colour stage has none."""

import ctypes as C
import faulthandler

import numpy as np
import pytest

import color_common as CC
import crop_plan_common as CP
import record_view_common as RV
import tile_stages_common as TS
import track_common as TC
import track_ingest_common as TI
from office_person_detection_vit_amd import HipDetrDetector, HipFloorMapper, HipOSNetReIDExtractor, _capi
from office_person_detection_vit_amd.frames import structured_frames
from office_person_detection_vit_amd.weights import DetrArch, ensure_osnet_weight_file, ensure_weight_file

pytestmark = pytest.mark.gpu

COUNTS = [8, 3]
S = RV.S
FM = (1878, 1369, 28.1926406926406, 28.241430700447)
ZONES = [{"id": "zone_1", "polygon": [[859, 912], [1095, 912], [1095, 1350], [859, 1350]], "priority": 1},
         {"id": "zone_2", "polygon": [[1095, 912], [1331, 912], [1331, 1350], [1095, 1350]], "priority": 2}]
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


def test_the_records_separate_the_rules():
    recs, dets = RV.merged(COUNTS), RV.dets(COUNTS)
    for f, k, label in RV.OTHER:
        assert k < COUNTS[f] and label != RV.LABEL and recs[f, k]["label"] == dets[f, k]["label"] == label
    assert len(set(recs[0, :COUNTS[0]]["query_index"].tolist())) < COUNTS[0], "the merged records repeat query numbers: only the position names a row"
    assert dets[0, 4]["query_index"] == S and dets[1, 1]["query_index"] == -1


def test_merged_records_every_label_rows_by_position(lib):
    h, w = TS.FRAME_HW
    frames, recs, cnt = TS.frames(), RV.merged(COUNTS), np.asarray(COUNTS, np.int32)
    fmap = HipFloorMapper.homography(H, FM, ZONES)
    try:
        color = np.full((2 * S, 256), -3.0, np.float32)
        floor = np.frombuffer(bytearray(b"\xa5" * (2 * S * 48)), HipFloorMapper.REC_DTYPE).copy()
        boxes, foot = np.full((2, S, 4), -3.0, np.float32), np.full((2, S, 2), -3.0, np.float32)
        has, feat, n_out = np.full((2, S), 7, np.uint8), np.full((2, S, 256), -3.0, np.float32), np.full(2, -9, np.int32)
        rc = lib.opd_test_tile_stages(0, frames.ctypes.data, 2, h, w, recs.ctypes.data, cnt.ctypes.data, S, fmap._require(), 1, color.ctypes.data, floor.ctypes.data,
                                      boxes.ctypes.data, foot.ctypes.data, has.ctypes.data, feat.ctypes.data, n_out.ctypes.data)
        assert rc == _capi.OPD_OK, _capi.last_error()
        assert n_out.tolist() == COUNTS
        for f in range(2):
            n = COUNTS[f]
            bbox, b32, foot32, _ = TS.host_arrays(recs[f], n)
            want_color = CC.device_color_features(lib, [frames[f]], b32)
            # every record below the count, the two of another label among them, in the row of its position
            assert color[f * S:f * S + n].tobytes() == want_color.tobytes(), f"colour rows of frame {f}"
            assert floor[f * S:f * S + n].tobytes() == fmap.transform_records(bbox).tobytes(), f"floor rows of frame {f}"
            assert boxes[f, :n].tobytes() == b32.tobytes() and foot[f, :n].tobytes() == foot32.tobytes(), f"staging image of frame {f}"
            assert has[f, :n].tolist() == [1] * n and feat[f, :n].tobytes() == want_color.tobytes(), f"staged rows of frame {f}"
            # ... and nothing at or behind it
            assert (color[f * S + n:(f + 1) * S] == -3.0).all() and floor[f * S + n:(f + 1) * S].tobytes() == b"\xa5" * ((S - n) * 48)
            assert (boxes[f, n:] == -3.0).all() and (foot[f, n:] == -3.0).all() and (has[f, n:] == 7).all() and (feat[f, n:] == -3.0).all()
    finally:
        fmap.close()


def test_merged_records_slots_for_the_stage_label_by_position(lib, weight_cache):
    h, w = TS.FRAME_HW
    ext = HipOSNetReIDExtractor(model_path=ensure_osnet_weight_file(weight_cache, "half"), max_crops=16)
    ext.load_model()
    try:
        E, slots = int(ext.feature_dim), S + 2
        frames, recs, cnt = TS.frames(), RV.merged(COUNTS), np.asarray(COUNTS, np.int32)
        persons = [f * S + k for f in range(2) for k in range(COUNTS[f]) if (f, k) not in {(a, b) for a, b, _ in RV.OTHER}]
        assert len(persons) == sum(COUNTS) - len(RV.OTHER) <= slots
        slot_map, rec, n_person = np.full(slots, -5, np.int32), np.full(slots, -5, np.int32), np.full(1, -5, np.int32)
        geom, rows = np.full((slots, 13), -7, np.int32), np.full((slots, E), -3.0, np.float32)
        boxes, foot = np.full((2, S, 4), -3.0, np.float32), np.full((2, S, 2), -3.0, np.float32)
        has, feat, n_out = np.full((2, S), 7, np.uint8), np.full((2, S, E), -3.0, np.float32), np.full(2, -9, np.int32)
        rc = lib.opd_test_tile_reid(0, ext._handle, frames.ctypes.data, 2, h, w, recs.ctypes.data, cnt.ctypes.data, S, slots, slot_map.ctypes.data, rec.ctypes.data,
                                    n_person.ctypes.data, geom.ctypes.data, rows.ctypes.data, boxes.ctypes.data, foot.ctypes.data, has.ctypes.data, feat.ctypes.data,
                                    n_out.ctypes.data)
        assert rc == _capi.OPD_OK, _capi.last_error()
        filled = len(persons)
        assert int(n_person[0]) == filled and slot_map[:filled].tolist() == persons and rec[:filled].tolist() == persons
        assert (slot_map[filled:] == -5).all() and (rec[filled:] == -5).all() and (geom[filled:] == -7).all() and (rows[filled:] == -3.0).all()
        flat = recs.reshape(-1)
        b32 = RV.box64(flat[persons]).astype(np.float32)
        assert geom[:filled].tobytes() == CP.plan(lib, "host", "osnet", b32, h, w)["geom"].tobytes(), "the plan of the float32 box of each selected record"
        for f in range(2):
            mine = [p for p in persons if p // S == f]
            want = ext.extract_features(frames[f], [tuple(float(v) for v in RV.box64(flat[p])) for p in mine])
            assert rows[[persons.index(p) for p in mine]].tobytes() == np.asarray(want, np.float32).tobytes(), f"rows of frame {f}"
            n = COUNTS[f]
            _, want_b, want_foot, _ = TS.host_arrays(recs[f], n)
            assert boxes[f, :n].tobytes() == want_b.tobytes() and foot[f, :n].tobytes() == want_foot.tobytes()   # every record, whatever its label
            assert has[f, :n].tolist() == [int(f * S + k in persons) for k in range(n)]
            for k in range(n):
                p = f * S + k
                assert feat[f, k].tobytes() == (rows[persons.index(p)] if p in persons else np.full(E, -3.0, np.float32)).tobytes()
            assert (boxes[f, n:] == -3.0).all() and (has[f, n:] == 7).all() and (feat[f, n:] == -3.0).all()
        assert n_out.tolist() == COUNTS
    finally:
        ext.cleanup()


@pytest.mark.parametrize("frame", [0, 1])
def test_post_process_records_ingest_rows_by_query_index(lib, frame):
    D = 256
    records = np.ascontiguousarray(RV.dets(COUNTS)[frame])
    n = COUNTS[frame]
    rows = np.random.default_rng(3).standard_normal((2 * S, D)).astype(np.float32)
    q = records["query_index"]
    unnamed = [i for i in range(n) if not 0 <= q[i] < S]
    assert len(unnamed) == 1
    slot_map = np.asarray([frame * S + int(v) for v in q[:n]], np.int32)   # a slot per record below the count; the unnamed one's names no row of this frame
    for kind, sm, n_person in ((TI.ROWS_NONE, None, 0), (TI.ROWS_BY_QUERY, None, 0), (TI.ROWS_BY_SLOT, slot_map, len(slot_map))):
        boxes, foot, has, feat = np.full((S, 4), 7.5, np.float32), np.full((S, 2), 7.5, np.float32), np.full(S, 9, np.uint8), np.full((S, D), 7.5, np.float32)
        want = [a.copy() for a in (boxes, foot, has, feat)]
        n_want = TI.ingest(records, n, S, D, frame, kind, rows, sm, n_person, 0 if sm is None else len(sm), *want)
        n_out = np.full(1, -7, np.int32)
        p = TC.ptr
        rc = lib.opd_track_test_ingest(0, p(records), n, S, D, frame, kind, p(rows if kind != TI.ROWS_NONE else None), 0 if kind == TI.ROWS_NONE else len(rows), p(sm), n_person,
                                       0 if sm is None else len(sm), S, p(boxes), p(foot), p(has), p(feat), p(n_out))
        assert rc == 0, _capi.last_error()
        assert int(n_out[0]) == n_want == n
        for name, got, w in zip(("boxes", "foot", "has", "feat"), (boxes, foot, has, feat), want):
            assert got.tobytes() == w.tobytes(), (name, kind)
        # every record below the count enters, whatever its label; the one no row is named for has none; nothing behind the count
        assert boxes[:n].tobytes() == RV.box64(records[:n]).astype(np.float32).tobytes()
        assert has[:n].tolist() == [int(kind != TI.ROWS_NONE and i not in unnamed) for i in range(n)]
        assert (feat[unnamed] == 7.5).all() and (boxes[n:] == 7.5).all() and (has[n:] == 9).all() and (feat[n:] == 7.5).all()
        if kind == TI.ROWS_BY_QUERY:
            assert all(feat[i].tobytes() == rows[frame * S + q[i]].tobytes() for i in range(n) if i not in unnamed)


def test_post_process_records_colour_and_floor_take_the_stage_label(lib, weight_cache):
    hw = (180, 320)
    det = HipDetrDetector(model_path=ensure_weight_file(weight_cache, DetrArch(), 0, 1.0, "r50"), max_batch=2, max_size=(288, 512), resize=True, confidence_threshold=0.05)
    det.load_model()
    fmap = HipFloorMapper.homography(H, FM, ZONES)
    try:
        Q = det.num_queries
        pair = [np.ascontiguousarray(f).copy() for f in structured_frames(2, hw[0], hw[1], seed=43)]
        ptrs = (C.c_void_p * 2)(*[f.ctypes.data for f in pair])
        plain, pcounts = (_capi.OpdDet * (2 * Q))(), (C.c_int32 * 2)()
        _capi.check(lib.opd_detr_detect_frames(C.c_void_p(det.model), ptrs, _capi.OPD_MEM_HOST, 2, hw[0], hw[1], 288, 512, 0.05, plain, pcounts), "detect_frames")
        kept = [(b, r) for b in range(2) for r in plain[b * Q:b * Q + int(pcounts[b])]]
        labels = [r.label for _, r in kept]
        assert labels, "the test frames give no record at threshold 0.05: nothing to compare"
        common = max(set(labels), key=labels.count)
        absent = min(set(range(len(labels) + 1)) - set(labels))   # a class no record has (the seeded weights may give records of one class only)
        recs, counts = (_capi.OpdDet * (2 * Q))(), (C.c_int32 * 2)()

        def rows(fn, label):
            """The [2 * Q][256] feature area as a fused call of stage label `label` brings it back: the rows the call wrote, and the rest as it lay there."""
            out = np.full((2 * Q, 256), -3.0, np.float32)
            _capi.check(fn(C.c_void_p(det.model), ptrs, 2, hw[0], hw[1], 288, 512, 0.05, label, recs, counts, out.ctypes.data_as(C.POINTER(C.c_float))), "fused call")
            assert list(counts) == list(pcounts) and bytes(recs) == bytes(plain)
            return out

        for label in (common, absent, -1):
            mine = [(b, r) for b, r in kept if r.label == label]
            assert (len(mine) > 0) == (label == common)
            rows_of = sorted(b * Q + r.query_index for b, r in mine)
            rest = np.setdiff1d(np.arange(2 * Q), rows_of)
            # the colour rows travel back as one block with whatever else lies in the handle's feature area: fill the rows of the common label with
            # the encoder's first, so that a row the colour stage writes differs from what lay there
            before = rows(lib.opd_detr_detect_frames_features, common)
            feats = rows(lib.opd_detr_detect_frames_color, label)
            assert feats[rest].tobytes() == before[rest].tobytes(), f"label {label}: a colour row of another record was written"
            assert all(feats[k].tobytes() != before[k].tobytes() for k in rows_of)
            feats = feats.reshape(2, Q, 256)
            floor = np.frombuffer(bytearray(b"\xa5" * (2 * Q * 48)), HipFloorMapper.REC_DTYPE)
            _capi.check(lib.opd_detr_detect_frames_floor(C.c_void_p(det.model), fmap._require(), ptrs, 2, hw[0], hw[1], 288, 512, 0.05, label, recs, counts,
                                                         floor.ctypes.data), "opd_detr_detect_frames_floor")
            assert list(counts) == list(pcounts) and bytes(recs) == bytes(plain)
            for b, r in mine:
                bbox = (float(r.x1), float(r.y1), float(r.x2 - r.x1), float(r.y2 - r.y1))   # Detection.bbox as the shim derives it
                assert feats[b, r.query_index].tobytes() == CC.device_color_features(lib, [pair[b]], [bbox])[0].tobytes(), (label, b, r.query_index)
                assert floor[b * Q + r.query_index].tobytes() == fmap.transform_records([bbox])[0].tobytes(), (label, b, r.query_index)
            assert floor[rest].tobytes() == b"\xa5" * (len(rest) * 48), f"label {label}: a floor row of another record was written"
    finally:
        fmap.close()
        det.close()


# ---- a negative person_label in the tiled calls: every class through the tiles' suppression, and the stages' rules on the merged records ------------------
TILED_HW = (192, 256)


def _tiled(lib, det, frames, grid, entry, stages, label):
    """One call of a tiled entry through ctypes with person_label = `label`: ([n][S] merged records, counts)."""
    from office_person_detection_vit_amd.detector import model_input_size
    from tile_common import TILE_DET
    n, T = len(frames), len(grid)
    Hm, Wm = model_input_size(grid[0][2], grid[0][3], det.max_size[0], det.max_size[1])
    p = _capi.OpdTileParams(struct_size=C.sizeof(_capi.OpdTileParams), person_label=label, tile_nms_threshold=0.4, merge_nms_threshold=0.4, merge_threshold=0.5,
                            edge_tolerance=0.01)
    out, counts = np.zeros((n, T * det.num_queries), TILE_DET), np.full(n, -9, np.int32)
    win = np.asarray(grid, np.int32).reshape(-1, 4)
    ptrs = (C.c_void_p * n)(*[f.ctypes.data for f in frames])
    args = [C.c_void_p(det.model), ptrs, n, TILED_HW[0], TILED_HW[1], win.ctypes.data_as(C.c_void_p), T, Hm, Wm, 0.05, C.byref(p)]
    if stages is not None:
        args.append(C.byref(stages))
    rc = getattr(lib, entry)(*args, out.ctypes.data_as(C.POINTER(_capi.OpdTileDet)), counts.ctypes.data_as(C.POINTER(C.c_int32)))
    assert rc == _capi.OPD_OK, _capi.last_error()
    return out, counts


def test_tiled_calls_with_a_negative_person_label(lib, weight_cache):
    """person_label = -1: the colour and floor stages still take EVERY merged record, by position; the crop selection looks for the label itself and finds
    none, so no record gets a slot or a row and the trackers see motion alone."""
    from office_person_detection_vit_amd import HipTracker
    from office_person_detection_vit_amd.tiling import tile_grid
    grid = tile_grid(TILED_HW[0], TILED_HW[1], 2, 2, 0.125)
    frames = [np.ascontiguousarray(structured_frames(1, TILED_HW[0], TILED_HW[1], seed=s)[0]).copy() for s in (5, 6)]
    det = HipDetrDetector(model_path=ensure_weight_file(weight_cache, DetrArch(), 0, 2.0, "r50"), max_batch=8, max_size=(256, 320), resize=True, confidence_threshold=0.05)
    det.load_model()
    ext = HipOSNetReIDExtractor(model_path=ensure_osnet_weight_file(weight_cache, "half"), max_crops=16)
    ext.load_model()
    fmap = HipFloorMapper.homography(H, FM, ZONES)
    E = int(ext.feature_dim)
    trackers = [HipTracker(max_dets=512, feature_dim=E, min_hits=1) for _ in range(4)]
    try:
        for t in trackers:
            t._ensure()
        Sd = len(grid) * det.num_queries
        plain, pcounts = _tiled(lib, det, frames, grid, "opd_detr_detect_tiled", None, -1)
        assert (pcounts > 0).all() and (pcounts <= Sd).all()

        def twins(out, floor):
            for f in range(2):
                n = int(pcounts[f])
                bbox = [tuple(float(v) for v in b) for b in RV.box64(out[f, :n])]
                assert floor[f * Sd:f * Sd + n].tobytes() == fmap.transform_records(bbox).tobytes(), f"floor rows of frame {f}"
                assert floor[f * Sd + n:(f + 1) * Sd].tobytes() == b"\xa5" * ((Sd - n) * 48)
                yield f, n, bbox

        # the staged call: colour and floor rows of every merged record, in the row of its position (the first staged call of the handle: no earlier one left rows there)
        color = np.full((2 * Sd, 256), -3.0, np.float32)
        floor = np.frombuffer(bytearray(b"\xa5" * (2 * Sd * 48)), HipFloorMapper.REC_DTYPE).copy()
        st = _capi.OpdTileStages(struct_size=C.sizeof(_capi.OpdTileStages), feature_kind=_capi.OPD_TRACK_FEAT_COLOR, features=color.ctypes.data, floor=fmap._require().value,
                                 floor_out=floor.ctypes.data)
        out, counts = _tiled(lib, det, frames, grid, "opd_detr_detect_tiled_stages", st, -1)
        assert counts.tobytes() == pcounts.tobytes() and all(out[f, :pcounts[f]].tobytes() == plain[f, :pcounts[f]].tobytes() for f in range(2))
        for f, n, bbox in twins(out, floor):
            assert color[f * Sd:f * Sd + n].tobytes() == CC.device_color_features(lib, [frames[f]], bbox).tobytes(), f"colour rows of frame {f}"

        # the Re-ID call: no record is labelled -1, so no slot, no row, nothing featured; floor rows as above; the trackers as a motion-only call leaves theirs
        slots = 8
        rows, slot_map, n_person = np.full((slots, E), -3.0, np.float32), np.full(slots, -5, np.int32), np.full(1, -5, np.int32)
        floor = np.frombuffer(bytearray(b"\xa5" * (2 * Sd * 48)), HipFloorMapper.REC_DTYPE).copy()
        ids, n_featured = np.full(2 * Sd, -1, np.int32), np.full(2, -9, np.int32)
        keep = (C.c_void_p * 2)(trackers[0]._h.value, trackers[1]._h.value)
        rs = _capi.OpdTileReidStages(struct_size=C.sizeof(_capi.OpdTileReidStages), slots=slots, reid=ext._handle.value, features=rows.ctypes.data, slot_map=slot_map.ctypes.data,
                                     n_person=n_person.ctypes.data, floor=fmap._require().value, floor_out=floor.ctypes.data, trackers=C.addressof(keep),
                                     track_ids=ids.ctypes.data, n_featured=n_featured.ctypes.data)
        out, counts = _tiled(lib, det, frames, grid, "opd_detr_detect_tiled_reid", rs, -1)
        assert counts.tobytes() == pcounts.tobytes() and all(out[f, :pcounts[f]].tobytes() == plain[f, :pcounts[f]].tobytes() for f in range(2))
        assert int(n_person[0]) == 0 and (slot_map == -5).all() and (rows == -3.0).all() and n_featured.tolist() == [0, 0]
        list(twins(out, floor))
        ids2, nf2 = np.full(2 * Sd, -1, np.int32), np.full(2, -9, np.int32)
        keep2 = (C.c_void_p * 2)(trackers[2]._h.value, trackers[3]._h.value)
        st = _capi.OpdTileStages(struct_size=C.sizeof(_capi.OpdTileStages), feature_kind=_capi.OPD_TRACK_FEAT_NONE, trackers=C.addressof(keep2), track_ids=ids2.ctypes.data,
                                 n_featured=nf2.ctypes.data)
        _tiled(lib, det, frames, grid, "opd_detr_detect_tiled_stages", st, -1)
        assert nf2.tolist() == [0, 0] and ids.tobytes() == ids2.tobytes()
        for f in range(2):
            assert (ids[f * Sd:f * Sd + pcounts[f]] >= 0).any() and (ids[f * Sd + pcounts[f]:(f + 1) * Sd] == -1).all()
            assert [bytes(r) for r in trackers[f]._records()] == [bytes(r) for r in trackers[2 + f]._records()], f"track rows of frame {f}: a record entered with a feature"
    finally:
        for t in trackers:
            t.close()
        fmap.close()
        ext.cleanup()
        det.close()
