"""CPU tests of the fused detect-and-track call (-m "not gpu"): the entry point in the header, the binding and the two libraries; the
struct sizes it must leave alone; the refusals that need no handle (the ones that read a handle are in test_detect_track_gpu.py: no
handle of any kind can be made without a device); and the numpy restatement of the ingest arithmetic (tests/track_ingest_common.py)
against what ``detector.py::_postprocess_batch`` and the packing of ``HipTracker.update`` make of the same records."""

import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import track_ingest_common as TI
from office_person_detection_vit_amd import HipDetrDetector, _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "opd_detr_detect_frames_track"
HOOK = "opd_track_test_ingest"


@pytest.fixture(scope="module")
def lib():
    return _capi.load_library(test_hooks=True)


def test_header_binding_and_libraries_agree_on_the_new_name(lib):
    header = open(os.path.join(ROOT, "include", "opd_detr.h")).read()
    assert re.search(r"OPD_API int " + NAME + r"\(", header) and NAME in _capi.API and NAME not in _capi.TEST_API
    assert HOOK not in header and HOOK in _capi.TEST_API and HOOK not in _capi.API
    proto = re.search(r"OPD_API int " + NAME + r"\((.*?)\);", header, re.S).group(1)
    assert len(proto.split(",")) == len(_capi.API[NAME][1]) == 17
    for k, name in enumerate(("NONE", "ENCODER", "COLOR", "REID")):
        assert re.search(r"#define OPD_TRACK_FEAT_%s %d\b" % (name, k), header) and getattr(_capi, "OPD_TRACK_FEAT_" + name) == k

    def exported(path):
        out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
        return {l.split()[2] for l in out.splitlines() if len(l.split()) == 3 and l.split()[1] == "T"}

    prod, test = exported(_capi.LIB_PATH), exported(_capi.TEST_LIB_PATH)
    assert NAME in prod and NAME in test
    assert HOOK not in prod and HOOK in test


def test_tracker_structs_keep_their_sizes():
    assert C.sizeof(_capi.OpdTrackStatus) == 40
    assert C.sizeof(_capi.OpdTrackConfig) == 64 and C.sizeof(_capi.OpdTrackRec) == 48


def test_arguments_are_refused_before_any_device_call(lib):
    """Without a handle: every check that reads no handle comes first, so a null detector handle is the LAST thing the call reports."""
    frame = np.zeros((40, 52, 3), np.uint8)
    ptrs = (C.c_void_p * 1)(frame.ctypes.data)
    trackers = (C.c_void_p * 1)(None)
    out, counts = (_capi.OpdDet * 100)(), (C.c_int32 * 1)()
    ids, nf = np.zeros(100, np.int32), np.zeros(1, np.int32)

    def call(text, tr=trackers, frames=ptrs, h=40, w=52, kind=_capi.OPD_TRACK_FEAT_NONE, slots=0, o=out, c=counts, i=ids.ctypes.data, f=nf.ctypes.data):
        rc = lib.opd_detr_detect_frames_track(None, None, tr, frames, 1, h, w, 32, 40, 0.05, 1, kind, slots, o, c, i, f)
        assert rc == _capi.OPD_EINVAL and text in _capi.last_error(), (text, _capi.last_error())
        assert NAME in _capi.last_error() or text == "null model handle"

    call("null model handle")
    call("null argument", tr=None)
    call("null argument", frames=None)
    call("null argument", o=None)
    call("null argument", c=None)
    call("null argument", i=None)
    call("null argument", f=None)
    call("unknown feature_kind 4", kind=4)
    call("unknown feature_kind -1", kind=-1)
    call("null Re-ID handle", kind=_capi.OPD_TRACK_FEAT_REID, slots=8)
    call("source frame size 0 x 52 out of range", h=0)
    call("source frame size", w=-1)
    call("4096 x 4096", kind=_capi.OPD_TRACK_FEAT_COLOR, h=4097)
    call("null model handle", kind=_capi.OPD_TRACK_FEAT_ENCODER, h=4097)   # (the edge limit is the colour histogram's alone)
    call("null model handle", kind=_capi.OPD_TRACK_FEAT_COLOR, h=4096, w=4096)


def _python_path(records):
    """boxes and foot points as the two-call path stages them: ``_postprocess_batch`` on ctypes records, then ``HipTracker.update``'s packing."""
    n = len(records)
    recs, counts = (_capi.OpdDet * n)(), (C.c_int32 * 1)(n)
    C.memmove(recs, records.ctypes.data, records.nbytes)
    det = HipDetrDetector(model_path="unused")
    det._nms_set = 0.4   # (the records count as suppressed on the device: the host suppression, a library call, is skipped)
    dets = det._postprocess_batch(recs, counts, n)[0]
    assert len(dets) == n
    boxes, foot, conf = np.zeros((n, 4), np.float32), np.zeros((n, 2), np.float32), np.zeros(n, np.float32)
    for j, d in enumerate(dets):   # tracker.py: HipTracker.update
        boxes[j], foot[j], conf[j] = d.bbox, d.camera_coords, d.confidence
    return boxes, foot, conf, [d.query_index for d in dets]


def test_restatement_equals_the_python_path_on_hard_records():
    records = TI.hard_records()
    assert C.sizeof(_capi.OpdDet) == TI.DET.itemsize == 32
    x1, x2 = records["x1"].astype(np.float64), records["x2"].astype(np.float64)
    assert np.any((x2 - x1).astype(np.float32).astype(np.float64) != x2 - x1), "no width needs a rounding"
    assert np.any(records["x1"] < 0) and np.any(np.frexp(records["x1"][:1])[0] * 2 ** 24 % 2 == 1), "no negative corner / no 24-bit corner"
    # (the foot point in float32 arithmetic is NOT the same number for some of them: the restatement has to go through float64)
    assert np.any(records["x1"] + (records["x2"] - records["x1"]) / np.float32(2) != (x1 + (x2 - x1) / 2).astype(np.float32))
    boxes, foot = TI.pack(records)
    pb, pf, conf, qi = _python_path(records)
    assert boxes.dtype == foot.dtype == np.float32
    assert boxes.tobytes() == pb.tobytes() and foot.tobytes() == pf.tobytes()
    assert conf.tobytes() == records["score"].tobytes() and qi == records["query_index"].tolist()


@pytest.mark.parametrize("kind", [TI.ROWS_NONE, TI.ROWS_BY_QUERY, TI.ROWS_BY_SLOT])
def test_restatement_leaves_everything_beyond_n_alone(kind):
    records, Q, D = TI.hard_records(), 64, 8
    rng = np.random.default_rng(3)
    rows = rng.standard_normal((2 * Q, D)).astype(np.float32)
    slot_map = (Q + records["query_index"][:20][::2]).astype(np.int32)   # frame 1: every second of the first twenty records
    for n in (0, 1, 33):
        boxes, foot, has, feat = np.full((Q, 4), 7.5, np.float32), np.full((Q, 2), 7.5, np.float32), np.full(Q, 9, np.uint8), np.full((Q, D), 7.5, np.float32)
        got = TI.ingest(records, n, Q, D, 1, kind, rows, slot_map, 99, len(slot_map), boxes, foot, has, feat)
        assert got == n
        assert np.all(boxes[n:] == 7.5) and np.all(foot[n:] == 7.5) and np.all(has[n:] == 9) and np.all(feat[n:] == 7.5)
        want = {TI.ROWS_NONE: [0] * n, TI.ROWS_BY_QUERY: [1] * n, TI.ROWS_BY_SLOT: [1 if (i < 20 and i % 2 == 0) else 0 for i in range(n)]}[kind]
        assert has[:n].tolist() == want
        for i in range(n):
            if want[i]:
                q = int(records["query_index"][i])
                src = rows[Q + q] if kind == TI.ROWS_BY_QUERY else rows[i // 2]
                assert feat[i].tobytes() == src.tobytes()
            else:
                assert np.all(feat[i] == 7.5)


def test_python_surface():
    import inspect
    sig = inspect.signature(HipDetrDetector.detect_and_track)
    assert [(k, v.default) for k, v in sig.parameters.items() if k != "self"] == [("frame", inspect.Parameter.empty), ("tracker", inspect.Parameter.empty),
                                                                                  ("features", "color"), ("reid", None), ("reid_slots", 32)]
    det = HipDetrDetector(model_path="unused")
    with pytest.raises(RuntimeError, match="Model not loaded"):
        det.detect_and_track(np.zeros((40, 52, 3), np.uint8), None)
    det.model = 1   # (never dereferenced: the checks below come before any library call)
    with pytest.raises(ValueError, match="features must be"):
        det.detect_and_track(np.zeros((40, 52, 3), np.uint8), None, features="hog")
    with pytest.raises(ValueError, match="needs reid="):
        det.detect_and_track(np.zeros((40, 52, 3), np.uint8), None, features="reid")
    det.model = None
