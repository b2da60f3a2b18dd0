"""CPU tests of the streams calls (-m "not gpu"): ``opd_track_update_streams`` and ``opd_detr_detect_streams_track`` in the header, the binding and
the two libraries, their hooks in the test library only; the refusals that need no handle (the ones that read a handle are in
test_track_streams_gpu.py); the schedule of a call as the host plans it; the Python planner that cuts the cameras' runs into calls; and the
Python surface of ``HipTracker.update_streams`` and ``HipDetrDetector.detect_and_track_streams``."""

import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from office_person_detection_vit_amd import HipDetrDetector, HipTracker, _capi
from office_person_detection_vit_amd.tracker import MAX_STREAM_TRACKERS, plan_stream_calls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UPDATE, DETECT = "opd_track_update_streams", "opd_detr_detect_streams_track"
HOOKS = ("opd_track_test_streams_schedule", "opd_track_test_assoc_multi")


@pytest.fixture(scope="module")
def lib():
    return _capi.load_library(test_hooks=True)


def test_header_binding_and_libraries_agree_on_the_new_names(lib):
    header = open(os.path.join(ROOT, "include", "opd_detr.h")).read()
    for name, n_args in ((UPDATE, 13), (DETECT, 20)):
        assert re.search(r"OPD_API int " + name + r"\(", header) and name in _capi.API and name not in _capi.TEST_API
        proto = re.search(r"OPD_API int " + name + r"\((.*?)\);", header, re.S).group(1)
        assert len(proto.split(",")) == len(_capi.API[name][1]) == n_args, name
    for hook in HOOKS:
        assert hook not in header and hook in _capi.TEST_API and hook not in _capi.API
    # the one-camera calls are as they were
    assert len(_capi.API["opd_track_update_sequence"][1]) == 11 and len(_capi.API["opd_detr_detect_sequence_track"][1]) == 18
    assert len(_capi.API["opd_detr_detect_frames_track"][1]) == 17

    def exported(path):
        out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
        return {l.split()[2] for l in out.splitlines() if len(l.split()) == 3 and l.split()[1] == "T"}

    prod, test = exported(_capi.LIB_PATH), exported(_capi.TEST_LIB_PATH)
    for name in (UPDATE, DETECT):
        assert name in prod and name in test
    for hook in HOOKS:
        assert hook not in prod and hook in test
    assert not [n for n in prod if "test" in n and "streams" in n]


def test_update_streams_refuses_before_any_device_call(lib):
    """Without a handle: every check that reads no handle comes first, so the null handle is the LAST thing the call reports."""
    boxes, foot, conf = np.zeros((3, 4), np.float32), np.zeros((3, 2), np.float32), np.zeros(3, np.float32)
    counts, cams = np.array([1, 2], np.int32), np.array([0, 1], np.int32)
    ids, done = np.full(3, -7, np.int32), np.full(2, -7, np.int32)
    two = (C.c_void_p * 2)(None, None)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)   # noqa: E731

    def call(text, t=two, n_cams=2, cam=cams, b=boxes, f=foot, c=conf, kind=_capi.OPD_MEM_HOST, n=counts, F=2, i=ids, d=done):
        rc = lib.opd_track_update_streams(t, n_cams, p(cam), F, p(b), p(f), p(c), None, None, kind, p(n), p(i), p(d))
        assert rc == _capi.OPD_EINVAL and text in _capi.last_error() and UPDATE in _capi.last_error(), (text, _capi.last_error())
        assert np.all(ids == -7) and np.all(done == -7)

    call("null handle (camera 0)")
    call("null argument", t=None)
    call("null argument", cam=None)
    call("null argument", n=None)
    call("null argument", i=None)
    call("null argument", d=None)
    call("C = 0 outside 1 .. 64", n_cams=0)
    call("C = -1 outside 1 .. 64", n_cams=-1)
    call("C = 65 outside 1 .. 64", n_cams=65)
    call("at least one frame, got F = 0", F=0)
    call("feat_mem_kind", kind=7)
    call("negative detection count of frame 1", n=np.array([1, -1], np.int32))
    call("null boxes, foot points or confidences", b=None)
    call("camera_of[1] = 2 outside 0 .. C - 1 = 1", cam=np.array([0, 2], np.int32))
    call("camera_of[0] = -1 outside", cam=np.array([-1, 0], np.int32))
    # with handles that are never read: the list checks come before anything of a tracker is looked at
    fake = np.zeros(64, np.uint8)
    same = (C.c_void_p * 2)(fake.ctypes.data, fake.ctypes.data)
    call("cameras 0 and 1 name the same tracker", t=same)
    apart = (C.c_void_p * 2)(fake.ctypes.data, fake.ctypes.data + 32)
    call("camera 1 gets no frame", t=apart, cam=np.array([0, 0], np.int32))


def test_detect_streams_refuses_before_any_device_call(lib):
    """The refusals of opd_detr_detect_frames_track, in its order, under this call's name, behind the ones of the list that need no handle."""
    frame = np.zeros((40, 52, 3), np.uint8)
    ptrs = (C.c_void_p * 1)(frame.ctypes.data)
    out, counts = (_capi.OpdDet * 100)(), (C.c_int32 * 1)()
    ids, nf, done, cams = np.zeros(100, np.int32), np.zeros(1, np.int32), np.full(1, -7, np.int32), np.zeros(1, np.int32)
    one = (C.c_void_p * 1)(None)

    def call(text, t=one, n_cams=1, cam=cams.ctypes.data, frames=ptrs, h=40, w=52, kind=_capi.OPD_TRACK_FEAT_NONE, slots=0, o=out, c=counts, i=ids.ctypes.data,
             f=nf.ctypes.data, d=done.ctypes.data):
        rc = lib.opd_detr_detect_streams_track(None, None, t, n_cams, cam, frames, 1, h, w, 32, 40, 0.05, 1, kind, slots, o, c, i, f, d)
        assert rc == _capi.OPD_EINVAL and text in _capi.last_error(), (text, _capi.last_error())
        assert DETECT in _capi.last_error() or text == "null model handle"
        assert done[0] == -7

    call("null model handle")
    call("null argument", t=None)
    call("null argument", cam=None)
    call("null argument", frames=None)
    call("null argument", o=None)
    call("null argument", c=None)
    call("null argument", i=None)
    call("null argument", f=None)
    call("null argument", d=None)
    call("C = 0 outside 1 .. 64", n_cams=0)
    call("C = 65 outside 1 .. 64", n_cams=65)
    call("unknown feature_kind 4", kind=4)
    call("null Re-ID handle", kind=_capi.OPD_TRACK_FEAT_REID, slots=8)
    call("source frame size 0 x 52 out of range", h=0)
    call("4096 x 4096", kind=_capi.OPD_TRACK_FEAT_COLOR, h=4097)
    call("null model handle", kind=_capi.OPD_TRACK_FEAT_COLOR, h=4096, w=4096)


def _schedule(lib, camera_of, n_cams):
    cam = np.asarray(camera_of, np.int32)
    out, steps = np.full(max(len(cam), 1) * n_cams, -9, np.int32), np.full(1, -9, np.int32)
    rc = lib.opd_track_test_streams_schedule(cam.ctypes.data_as(C.c_void_p), len(cam), n_cams, out.ctypes.data_as(C.c_void_p), len(out), steps.ctypes.data_as(C.c_void_p))
    assert rc == 0, _capi.last_error()
    return out[:steps[0] * n_cams].reshape(steps[0], n_cams).tolist()


def test_schedule_of_a_call(lib):
    assert _schedule(lib, [0, 1, 0, 2, 2, 0], 3) == [[0, 1, 3], [2, -1, 4], [5, -1, -1]]
    assert _schedule(lib, [0] * 7, 1) == [[f] for f in range(7)]                       # all frames in one camera: a step a frame
    assert _schedule(lib, [1] * 4, 2) == [[-1, f] for f in range(4)]                   # (the other camera is the caller's to refuse)
    assert _schedule(lib, list(range(9)), 9) == [list(range(9))]                       # all cameras distinct: one step
    assert _schedule(lib, [3, 2, 1, 0], 4) == [[3, 2, 1, 0]]
    rng = np.random.default_rng(11)
    cam = np.concatenate([np.arange(64), rng.integers(0, 64, 200)]).astype(np.int32)   # C = 64, every camera with a frame
    steps = _schedule(lib, cam, 64)
    want = [[f for f in range(len(cam)) if cam[f] == c] for c in range(64)]
    assert len(steps) == max(len(w) for w in want)
    for c in range(64):
        assert [s[c] for s in steps if s[c] >= 0] == want[c] and [s[c] for s in steps[len(want[c]):]] == [-1] * (len(steps) - len(want[c]))
    bad = np.array([0, 64], np.int32)
    out, n = np.zeros(128, np.int32), np.zeros(1, np.int32)
    assert lib.opd_track_test_streams_schedule(bad.ctypes.data_as(C.c_void_p), 2, 64, out.ctypes.data_as(C.c_void_p), 128, n.ctypes.data_as(C.c_void_p)) == _capi.OPD_EINVAL
    assert lib.opd_track_test_streams_schedule(bad.ctypes.data_as(C.c_void_p), 2, 65, out.ctypes.data_as(C.c_void_p), 128, n.ctypes.data_as(C.c_void_p)) == _capi.OPD_EINVAL


@pytest.mark.parametrize("max_batch", [1, 5, 8, None])
@pytest.mark.parametrize("lengths", [[30, 8, 1, 0, 14], [3, 1, 2], [0, 0], [], [1] * 70, [2] * 130, [40]])
def test_planner(lengths, max_batch):
    calls = plan_stream_calls(lengths, max_batch)
    seen = [[] for _ in lengths]
    for call in calls:
        assert call and len(call) == len({c for c, _, _ in call}) <= MAX_STREAM_TRACKERS, "a camera once a call, at most 64 of them"
        assert all(0 <= a < b <= lengths[c] for c, a, b in call), "no empty run, no camera of 0 frames"
        assert max_batch is None or sum(b - a for _, a, b in call) <= max_batch
        for c, a, b in call:
            seen[c].extend(range(a, b))
    assert seen == [list(range(n)) for n in lengths], "every frame exactly once, every camera's order kept"
    if max_batch is not None and sum(lengths):   # no call is emptier than it has to be: only the last may fall short by more than the cut allows
        assert len(calls) <= sum(lengths) and sum(sum(b - a for _, a, b in call) for call in calls) == sum(lengths)
    if max_batch is None and 0 < len([n for n in lengths if n]) <= 64:
        assert len(calls) == 1


def test_planner_argument_errors():
    with pytest.raises(ValueError, match="max_batch"):
        plan_stream_calls([3], 0)
    with pytest.raises(ValueError, match="max_trackers"):
        plan_stream_calls([3], 4, 65)
    assert plan_stream_calls([5, 5, 5], 8, 2) and all(len(call) <= 2 for call in plan_stream_calls([5, 5, 5], 8, 2))


def test_python_surface():
    sig = inspect.signature(HipTracker.update_streams)
    assert [(k, v.default) for k, v in sig.parameters.items()] == [("trackers", inspect.Parameter.empty), ("detections_per_camera", inspect.Parameter.empty)]
    sig = inspect.signature(HipDetrDetector.detect_and_track_streams)
    assert [(k, v.default) for k, v in sig.parameters.items() if k != "self"] == [("frames_per_camera", inspect.Parameter.empty), ("trackers", inspect.Parameter.empty),
                                                                                  ("features", "color"), ("reid", None), ("reid_slots", 32)]
    sig = inspect.signature(HipDetrDetector.detect_and_track_batch)   # keeps its signature
    assert [k for k in sig.parameters if k != "self"] == ["frames", "tracker", "features", "reid", "reid_slots"]
    a = HipTracker(feature_dim=16, max_dets=2)
    assert HipTracker.update_streams([], []) == [] and HipTracker.update_streams([a], [[]]) == [[]]   # (nothing to do: no handle is made)
    with pytest.raises(ValueError, match="1 trackers for 2 cameras"):
        HipTracker.update_streams([a], [[], []])
    with pytest.raises(ValueError, match="named twice"):
        HipTracker.update_streams([a, a], [[], []])
    with pytest.raises(ValueError, match="camera 0 has 3 detections"):
        HipTracker.update_streams([a], [[[None] * 3]])
    det = HipDetrDetector(model_path="unused")
    frames = [[np.zeros((40, 52, 3), np.uint8)] * 2]
    with pytest.raises(RuntimeError, match="Model not loaded"):
        det.detect_and_track_streams(frames, [a])
    det.model = 1   # (never dereferenced: the checks below come before any library call)
    with pytest.raises(ValueError, match="features must be"):
        det.detect_and_track_streams(frames, [a], features="hog")
    with pytest.raises(ValueError, match="needs reid="):
        det.detect_and_track_streams(frames, [a], features="reid")
    with pytest.raises(ValueError, match="2 trackers for 1 cameras"):
        det.detect_and_track_streams(frames, [a, a])
    with pytest.raises(ValueError, match="named twice"):
        det.detect_and_track_streams(frames * 2, [a, a])
    det.model = None
