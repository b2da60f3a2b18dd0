"""CPU tests of the sequence calls (-m "not gpu"): ``opd_track_update_sequence`` and ``opd_detr_detect_sequence_track`` in the header, the
binding and the two libraries; the association hook in the test library only; the struct sizes the calls must leave alone; the refusals
that need no handle (the ones that read a handle are in test_track_sequence_gpu.py: no handle of any kind can be made without a device);
and the Python surface of ``HipTracker.update_sequence`` and ``HipDetrDetector.detect_and_track_batch``."""

import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from office_person_detection_vit_amd import HipDetrDetector, HipTracker, _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UPDATE, DETECT = "opd_track_update_sequence", "opd_detr_detect_sequence_track"
HOOK = "opd_track_test_assoc"


@pytest.fixture(scope="module")
def lib():
    return _capi.load_library(test_hooks=True)


def test_header_binding_and_libraries_agree_on_the_new_names(lib):
    header = open(os.path.join(ROOT, "include", "opd_detr.h")).read()
    for name, n_args in ((UPDATE, 11), (DETECT, 18)):
        assert re.search(r"OPD_API int " + name + r"\(", header) and name in _capi.API and name not in _capi.TEST_API
        proto = re.search(r"OPD_API int " + name + r"\((.*?)\);", header, re.S).group(1)
        assert len(proto.split(",")) == len(_capi.API[name][1]) == n_args, name
    assert HOOK not in header and HOOK in _capi.TEST_API and HOOK not in _capi.API
    # the 17-argument per-frame call is as it was
    proto = re.search(r"OPD_API int opd_detr_detect_frames_track\((.*?)\);", header, re.S).group(1)
    assert len(proto.split(",")) == len(_capi.API["opd_detr_detect_frames_track"][1]) == 17
    assert len(_capi.API["opd_track_update"][1]) == 9 and len(_capi.API["opd_assign"][1]) == 4

    def exported(path):
        out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
        return {l.split()[2] for l in out.splitlines() if len(l.split()) == 3 and l.split()[1] == "T"}

    prod, test = exported(_capi.LIB_PATH), exported(_capi.TEST_LIB_PATH)
    for name in (UPDATE, DETECT):
        assert name in prod and name in test
    assert HOOK not in prod and HOOK in test


def test_tracker_structs_keep_their_sizes():
    assert C.sizeof(_capi.OpdTrackConfig) == 64 and C.sizeof(_capi.OpdTrackRec) == 48 and C.sizeof(_capi.OpdTrackStatus) == 40


def test_update_sequence_refuses_before_any_device_call(lib):
    """Without a handle: every check that reads no handle comes first, so the null handle is the LAST thing the call reports."""
    boxes, foot, conf = np.zeros((3, 4), np.float32), np.zeros((3, 2), np.float32), np.zeros(3, np.float32)
    counts, ids, done = np.array([1, 2], np.int32), np.full(3, -7, np.int32), np.full(1, -7, np.int32)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)   # noqa: E731

    def call(text, b=boxes, f=foot, c=conf, kind=_capi.OPD_MEM_HOST, n=counts, F=2, i=ids, d=done):
        rc = lib.opd_track_update_sequence(None, p(b), p(f), p(c), None, None, kind, p(n), F, p(i), p(d))
        assert rc == _capi.OPD_EINVAL and text in _capi.last_error() and UPDATE in _capi.last_error(), (text, _capi.last_error())
        assert np.all(ids == -7) and np.all(done == -7)

    call("null handle")
    call("null argument", n=None)
    call("null argument", i=None)
    call("null argument", d=None)
    call("at least one frame, got F = 0", F=0)
    call("at least one frame, got F = -2", F=-2)
    call("feat_mem_kind", kind=7)
    call("negative detection count of frame 1", n=np.array([1, -1], np.int32))
    call("null boxes, foot points or confidences", b=None)
    call("null boxes, foot points or confidences", c=None)
    call("null handle", b=None, f=None, c=None, n=np.zeros(2, np.int32))   # (frames without detections need no arrays)


def test_detect_sequence_refuses_before_any_device_call(lib):
    """The refusals of opd_detr_detect_frames_track, in its order, under this call's name."""
    frame = np.zeros((40, 52, 3), np.uint8)
    ptrs = (C.c_void_p * 1)(frame.ctypes.data)
    out, counts = (_capi.OpdDet * 100)(), (C.c_int32 * 1)()
    ids, nf, done = np.zeros(100, np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32)

    def call(text, frames=ptrs, h=40, w=52, kind=_capi.OPD_TRACK_FEAT_NONE, slots=0, o=out, c=counts, i=ids.ctypes.data, f=nf.ctypes.data, d=done.ctypes.data):
        rc = lib.opd_detr_detect_sequence_track(None, None, None, frames, 1, h, w, 32, 40, 0.05, 1, kind, slots, o, c, i, f, d)
        assert rc == _capi.OPD_EINVAL and text in _capi.last_error(), (text, _capi.last_error())
        assert DETECT in _capi.last_error() or text == "null model handle"

    call("null model handle")
    call("null argument", frames=None)
    call("null argument", o=None)
    call("null argument", c=None)
    call("null argument", i=None)
    call("null argument", f=None)
    call("null argument", d=None)
    call("unknown feature_kind 4", kind=4)
    call("unknown feature_kind -1", kind=-1)
    call("null Re-ID handle", kind=_capi.OPD_TRACK_FEAT_REID, slots=8)
    call("source frame size 0 x 52 out of range", h=0)
    call("source frame size", w=-1)
    call("4096 x 4096", kind=_capi.OPD_TRACK_FEAT_COLOR, h=4097)
    call("null model handle", kind=_capi.OPD_TRACK_FEAT_ENCODER, h=4097)   # (the edge limit is the colour histogram's alone)
    call("null model handle", kind=_capi.OPD_TRACK_FEAT_COLOR, h=4096, w=4096)


def test_python_surface():
    sig = inspect.signature(HipTracker.update_sequence)
    assert [(k, v.default) for k, v in sig.parameters.items() if k != "self"] == [("detections_per_frame", inspect.Parameter.empty)]
    sig = inspect.signature(HipDetrDetector.detect_and_track_batch)
    assert [(k, v.default) for k, v in sig.parameters.items() if k != "self"] == [("frames", inspect.Parameter.empty), ("tracker", inspect.Parameter.empty),
                                                                                  ("features", "color"), ("reid", None), ("reid_slots", 32)]
    sig = inspect.signature(HipDetrDetector.detect_and_track)   # keeps its signature
    assert [k for k in sig.parameters if k != "self"] == ["frame", "tracker", "features", "reid", "reid_slots"]
    det = HipDetrDetector(model_path="unused")
    frames = [np.zeros((40, 52, 3), np.uint8)] * 2
    with pytest.raises(RuntimeError, match="Model not loaded"):
        det.detect_and_track_batch(frames, None)
    det.model = 1   # (never dereferenced: the checks below come before any library call)
    with pytest.raises(ValueError, match="features must be"):
        det.detect_and_track_batch(frames, None, features="hog")
    with pytest.raises(ValueError, match="needs reid="):
        det.detect_and_track_batch(frames, None, features="reid")
    det.model = None
