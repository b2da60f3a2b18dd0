"""Hybrid tracking inside the detect call, without a device (``opd_lwt_interpolate_sequence``, ``opd_detr_detect_frames_hybrid`` and their
Python methods): the symbols are declared, bound and exported; every refusal that needs no handle comes back as OPD_EINVAL with a message
before anything touches a device; and the numpy restatement of the ingest launch (lwt_ingest_common.py) equals what
``detector.py::_postprocess_batch`` and ``HipLightweightTracker.update_with_detections`` make of the same records."""

import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import lwt_ingest_common as LI
from office_person_detection_vit_amd import HipDetrDetector, HipLightweightTracker, _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["opd_lwt_interpolate_sequence", "opd_detr_detect_frames_hybrid", "opd_detr_detect_sequence_hybrid"]
HOOK = "opd_lwt_test_ingest"


@pytest.fixture(scope="module")
def lib():
    return _capi.load_library(test_hooks=True)


def test_the_entry_point_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "opd_detr.h")).read()
    assert HOOK in _capi.TEST_API and HOOK not in header
    for path in (_capi.LIB_PATH, _capi.TEST_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
        exported = {l.split()[2] for l in out.splitlines() if len(l.split()) == 3}
        assert set(NEW) <= exported, path
        assert (HOOK in exported) == (path == _capi.TEST_LIB_PATH), path
        assert not [n for n in exported if "lwt_fused" in n or "lwt_enqueue" in n or "lwt_adopt" in n or "lwt_sequence" in n or "opd_launch_lwt" in n], path
        assert not [n for n in exported if "lwt_enqueue_interp" in n or "flow_check_track" in n or "flow_enqueue_track_from" in n], path
    for name in NEW:
        m = re.search(r"OPD_API\s+int\s+" + name + r"\s*\(([^)]*)\)", header)
        assert m and name in _capi.API, name
        assert len(m.group(1).split(",")) == len(_capi.API[name][1]), name   # the binding has the declaration's argument count


def test_refusals_that_need_no_handle(lib):
    counts = (C.c_int32 * 64)()
    recs = (_capi.OpdLwtRec * 4)()

    def refused(text, t, F, capacity, cnt=counts):
        assert lib.opd_lwt_interpolate_sequence(t, None, 0, F, 0, 0, recs, capacity, cnt) == _capi.OPD_EINVAL, text
        assert text in _capi.last_error(), (text, _capi.last_error())

    refused("0 frames", None, 0, 4)
    refused("-1 frames", None, -1, 4)
    refused("65 frames", None, 65, 4)
    refused("capacity 0", None, 1, 0)
    refused("capacity -3", None, 64, -3)
    refused("null handle", None, 1, 4)
    refused("null handle", None, 64, 4, None)


def test_fused_detection_frame_refusals_that_need_no_handle(lib):
    Q = 100
    recs, counts, ids = (_capi.OpdDet * Q)(), (C.c_int32 * 1)(), np.full(Q, -7, np.int32)
    frame = np.zeros((40, 52, 3), np.uint8)
    ptrs, hs = (C.c_void_p * 1)(frame.ctypes.data), (C.c_void_p * 1)(None)

    def call(text, m=None, trackers=hs, frames=ptrs, h=40, w=52, out=recs, cnt=counts, tid=ids.ctypes.data):
        rc = lib.opd_detr_detect_frames_hybrid(m, trackers, frames, 1, h, w, 40, 52, 0.05, 1, out, cnt, tid)
        assert rc == _capi.OPD_EINVAL and text in _capi.last_error(), (text, _capi.last_error())

    call("null argument", trackers=None)
    call("null argument", frames=None)
    call("null argument", out=None)
    call("null argument", cnt=None)
    call("null argument", tid=None)
    call("source frame size 0 x 52 out of range", h=0)
    call("source frame size", w=-1)
    call("null model handle")
    assert np.all(ids == -7)


def test_fused_sequence_refusals_that_need_no_handle(lib):
    Q = 100
    recs, counts, ids = (_capi.OpdDet * Q)(), (C.c_int32 * 1)(), np.full(Q, -7, np.int32)
    lrecs, lcounts, done = (_capi.OpdLwtRec * 8)(), (C.c_int32 * 64)(), C.c_int32(-7)
    frame = np.zeros((40, 52, 3), np.uint8)
    ptrs, flags = (C.c_void_p * 64)(*([frame.ctypes.data] * 64)), (C.c_uint8 * 64)(1, 0)

    def call(text, frames=ptrs, is_key=flags, F=2, h=40, w=52, out=recs, cnt=counts, tid=ids.ctypes.data, lr=lrecs, cap=4, lc=lcounts, fd=C.byref(done)):
        rc = lib.opd_detr_detect_sequence_hybrid(None, None, frames, is_key, F, h, w, 40, 52, 0.05, 1, out, cnt, tid, lr, cap, lc, fd)
        assert rc == _capi.OPD_EINVAL and text in _capi.last_error(), (text, _capi.last_error())

    call("0 frames", F=0)
    call("65 frames", F=65)
    call("capacity 0", cap=0)
    call("null argument", frames=None)
    call("null argument", is_key=None)
    call("null argument", fd=None)
    call("null output of the key frames", out=None)
    call("null output of the key frames", tid=None)
    call("null output of the in-between frames", lr=None)
    call("null output of the in-between frames", lc=None)
    call("source frame size 0 x 52 out of range", h=0)
    call("null model handle")
    call("null model handle", out=None, cnt=None, tid=None, is_key=(C.c_uint8 * 64)())   # no key frame: their outputs are not needed
    assert np.all(ids == -7) and done.value == -7


def _python_path(records):
    """The boxes as the two-call path hands them to ``opd_lwt_update``: ``_postprocess_batch`` on ctypes records, then the array of
    ``update_with_detections``."""
    n = len(records)
    recs, counts = (_capi.OpdDet * max(n, 1))(), (C.c_int32 * 1)(n)
    C.memmove(recs, records.ctypes.data, records.nbytes)
    det = HipDetrDetector(model_path="unused")
    det._nms_set = 0.4   # (the records count as suppressed on the device: the host suppression, a library call, is skipped)
    dets = det._postprocess_batch(recs, counts, max(n, 1))[0]
    assert len(dets) == n
    return np.array([d.bbox for d in dets], np.float32).reshape(n, 4)


@pytest.mark.parametrize("n", [0, 1, 100])
def test_ingest_restatement_equals_the_python_path(n):
    records = LI.edge_records()
    assert records["x1"][:7].min() == 0.0 and records["x2"][:7].max() == 1280.0 and records["y2"][:7].max() == 720.0   # boxes touching 0 and the frame edge
    want = _python_path(records[:n])
    assert LI.pack(records[:n]).tobytes() == want.tobytes()
    boxes = np.full((100, 4), 7.5, np.float32)
    assert LI.ingest(records, n, 100, boxes) == n
    assert boxes[:n].tobytes() == want.tobytes() and np.all(boxes[n:] == 7.5)
    assert LI.ingest(records, 250, 100, boxes.copy()) == 100 and LI.ingest(records, -3, 100, boxes.copy()) == 0   # the count is clamped


def test_the_class_method_without_a_handle():
    t = HipLightweightTracker()
    assert t.interpolate_sequence([]) == [] and t.interpolate_sequence([None, None, None]) == [[], [], []]
    assert t.info() is None   # no handle was made for it
    assert HipLightweightTracker.SEQUENCE_MAX == 64
