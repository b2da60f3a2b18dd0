"""The detect / forward entry points of the C-ABI against each other (GPU): every way of handing the same frames to the library gives the
same bytes back, and every refusal keeps its return code and its exact ``opd_last_error()`` text (csrc/opd_api.cpp).

Small on purpose: r50 "mild" weights, max_batch 2, model size 64 x 96, two frames per call."""

import ctypes as C

import numpy as np
import pytest
import torch

import floor_common as F
import track_common as TC
from office_person_detection_vit_amd import _capi
from office_person_detection_vit_amd.frames import structured_frames
from office_person_detection_vit_amd.weights import DetrArch, ensure_weight_file

pytestmark = pytest.mark.gpu

B, H, W = 2, 64, 96
U8, HOST, DEVICE, DEVOUT = _capi.OPD_PIXELS_U8_BGR_HWC, _capi.OPD_MEM_HOST, _capi.OPD_MEM_DEVICE, _capi.OPD_MEM_HOST_PIXELS_DEVICE_OUT
PERSON = 1
NMS_IOU = 0.4
TRACKER = dict(max_tracks=128, max_dets=128, min_hits=1, high_conf_threshold=0.5)   # (room for every query of both frames)
DetP, I32P, F32P = C.POINTER(_capi.OpdDet), C.POINTER(C.c_int32), C.POINTER(C.c_float)


@pytest.fixture(scope="module")
def handle(weight_cache):
    lib = _capi.load_library()
    path = ensure_weight_file(weight_cache, DetrArch(), 0, 1.0, "r50")
    cfg = _capi.OpdConfig(struct_size=C.sizeof(_capi.OpdConfig), max_batch=B, max_height=H, max_width=W, flags=0)
    h = C.c_void_p()
    _capi.check(lib.opd_detr_create(C.byref(cfg), path.encode(), 0, C.byref(h)), "opd_detr_create")
    info = _capi.OpdModelInfo()
    _capi.check(lib.opd_detr_info(h, C.byref(info)), "opd_detr_info")
    yield lib, h, info
    lib.opd_detr_destroy(h)


class _Out:
    """Fresh output buffers of one call, host or device, pre-filled so that nothing left over from another call can pass for a result."""

    def __init__(self, Q, device):
        self.Q, self.device = Q, device
        if device:
            self.t = torch.full((B * Q * 8 + B,), 0x55555555, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            self.recs = C.cast(C.c_void_p(self.t.data_ptr()), DetP)
            self.cnts = C.cast(C.c_void_p(self.t[B * Q * 8:].data_ptr()), I32P)
        else:
            self.r = np.full((B, Q, 8), 0x55555555, np.int32)
            self.c = np.full(B, 0x55555555, np.int32)
            self.recs, self.cnts = self.r.ctypes.data_as(DetP), self.c.ctypes.data_as(I32P)

    def result(self):
        """(counts, the records of every frame up to its count) as bytes"""
        if self.device:
            torch.cuda.synchronize()
            a = self.t.cpu().numpy()
            r, c = a[:B * self.Q * 8].reshape(B, self.Q, 8), a[B * self.Q * 8:]
        else:
            r, c = self.r, self.c
        assert all(0 <= int(n) <= self.Q for n in c), f"counts {c.tolist()}"
        return c.tobytes(), b"".join(r[b, :int(c[b])].tobytes() for b in range(B))


@pytest.fixture(scope="module")
def floor(handle):
    lib = handle[0]
    f = F.create(lib, F.case_model(np.load(F.GOLDEN), "homography_config"))
    yield f
    lib.opd_floor_destroy(f)


def _entries(lib, h, info, frames, pix, host_only, floor, nms):
    """name -> call(out) for every detect entry point on `frames` ([B][h][w][3] camera frames; `pix`: the same at model resolution).
    `nms`: the handle's suppression is on, which the tracking entries need: they join."""
    fh, fw = frames.shape[1:3]
    hw = np.asarray([[fh, fw]] * B, np.int32)
    hw_p = hw.ctypes.data_as(C.c_void_p)
    ptrs = (C.c_void_p * B)(*[frames[b].ctypes.data for b in range(B)])
    d_frames = torch.from_numpy(frames).cuda()
    torch.cuda.synchronize()
    feats = np.empty((B, info.num_queries, info.d_model), np.float32)
    rows = np.empty(B * info.num_queries, F.REC_DTYPE)
    ids, nf, done = np.empty((B, info.num_queries), np.int32), np.empty(B, np.int32), np.empty(1, np.int32)
    keep = [hw, ptrs, d_frames, feats, frames, pix, rows, ids, nf, done]

    def async_(kind):
        def call(o):
            t = C.c_int(-1)
            _capi.check(lib.opd_detr_detect_async(h, pix.ctypes.data, U8, kind, B, H, W, 0.05, hw_p, o.recs, o.cnts, C.byref(t)), "opd_detr_detect_async")
            _capi.check(lib.opd_detr_wait(h, t.value), "opd_detr_wait")
            return 0
        return call

    def track(kind, sequence):
        def call(o):   # a fresh tracker per call (one per frame, or one for the run): what an earlier call left in one is not this call's input
            ts = [TC.create(lib, _capi, info.d_model, **TRACKER) for _ in range(1 if sequence else B)]
            try:
                if sequence:
                    return lib.opd_detr_detect_sequence_track(h, None, ts[0], ptrs, B, fh, fw, H, W, 0.05, PERSON, kind, 0, o.recs, o.cnts, ids.ctypes.data,
                                                              nf.ctypes.data, done.ctypes.data)
                return lib.opd_detr_detect_frames_track(h, None, (C.c_void_p * B)(*[t.value for t in ts]), ptrs, B, fh, fw, H, W, 0.05, PERSON, kind, 0, o.recs,
                                                        o.cnts, ids.ctypes.data, nf.ctypes.data)
            finally:
                for t in ts:
                    lib.opd_track_destroy(t)
        return call

    e = {
        ("detect", False): lambda o: lib.opd_detr_detect(h, pix.ctypes.data, U8, HOST, B, H, W, 0.05, hw_p, o.recs, o.cnts),
        ("detect_resized host", False): lambda o: lib.opd_detr_detect_resized(h, frames.ctypes.data, HOST, B, fh, fw, H, W, 0.05, o.recs, o.cnts),
        ("detect_resized device", True): lambda o: lib.opd_detr_detect_resized(h, d_frames.data_ptr(), DEVICE, B, fh, fw, H, W, 0.05, o.recs, o.cnts),
        ("detect_frames host", False): lambda o: lib.opd_detr_detect_frames(h, ptrs, HOST, B, fh, fw, H, W, 0.05, o.recs, o.cnts),
        ("detect_frames device out", True): lambda o: lib.opd_detr_detect_frames(h, ptrs, DEVOUT, B, fh, fw, H, W, 0.05, o.recs, o.cnts),
        ("detect_frames_features", False): lambda o: lib.opd_detr_detect_frames_features(h, ptrs, B, fh, fw, H, W, 0.05, PERSON, o.recs, o.cnts,
                                                                                          feats.ctypes.data_as(F32P)),
        ("detect_frames_color", False): lambda o: lib.opd_detr_detect_frames_color(h, ptrs, B, fh, fw, H, W, 0.05, PERSON, o.recs, o.cnts,
                                                                                    feats.ctypes.data_as(F32P)),
        ("detect_frames_floor", False): lambda o: lib.opd_detr_detect_frames_floor(h, floor, ptrs, B, fh, fw, H, W, 0.05, PERSON, o.recs, o.cnts, rows.ctypes.data),
        ("detect_async host", False): async_(HOST),
        ("detect_async device out", True): async_(DEVOUT),
    }
    if nms:
        e.update({("detect_frames_track none", False): track(_capi.OPD_TRACK_FEAT_NONE, False),
                  ("detect_frames_track colour", False): track(_capi.OPD_TRACK_FEAT_COLOR, False),
                  ("detect_sequence_track none", False): track(_capi.OPD_TRACK_FEAT_NONE, True),
                  ("detect_sequence_track colour", False): track(_capi.OPD_TRACK_FEAT_COLOR, True)})
    return {k: v for k, v in e.items() if not (host_only and k[1])}, keep


@pytest.mark.parametrize("cam,nms", [((48, 64), False), ((64, 96), False), ((48, 64), True), ((64, 96), True)],
                         ids=["resize", "direct", "resize-nms", "direct-nms"])
def test_all_entry_points_return_the_same_bytes(handle, floor, cam, nms):
    """Camera frames 48 x 64 (device resize) and 64 x 96 (straight upload) through every detect entry point, each called twice (eager, then
    the captured graph): counts and records are byte-identical to opd_detr_detect on the resized pixels with orig_hw = the camera size; the
    two forward entries agree bit for bit; a clone of the handle returns the same through the host-output entries.  Once with the handle's
    suppression off, once with opd_detr_set_nms(PERSON, 0.4): opd_detr_detect's bytes are then the suppressed ones, every frame keeps a
    record, and the tracking entries (a fresh tracker per call, feature kinds none and colour) return them too."""
    lib, h, info = handle
    Q, ncls = info.num_queries, info.num_classes_plus1
    fh, fw = cam
    frames = np.ascontiguousarray(np.stack(structured_frames(B, fh, fw, seed=77)))
    if cam == (H, W):
        pix = frames.copy()
    else:
        pix = np.empty((B, H, W, 3), np.uint8)
        _capi.check(lib.opd_detr_resize_u8(h, frames.ctypes.data, B, fh, fw, H, W, pix.ctypes.data), "opd_detr_resize_u8")
    clone = C.c_void_p()
    _capi.check(lib.opd_detr_clone(h, C.byref(clone)), "opd_detr_clone")
    try:
        want = None
        for hd, host_only in ((h, False), (clone, True)):
            if nms:
                _capi.check(lib.opd_detr_set_nms(hd, PERSON, NMS_IOU), "opd_detr_set_nms")
            entries, keep = _entries(lib, hd, info, frames, pix, host_only, floor, nms)
            for (name, device), call in entries.items():
                for rep in range(2):
                    out = _Out(Q, device)
                    assert call(out) == 0, f"{name}: {_capi.last_error()}"
                    got = out.result()
                    if want is None:
                        want = got
                        assert len(want[1]) > 0, "no record at threshold 0.05: nothing to compare"
                        if nms:
                            kept = np.frombuffer(want[0], np.int32)
                            assert (kept > 0).all(), f"suppression left a frame without a record (counts {kept.tolist()}): nothing for a tracker to take"
                    assert got == want, f"{name} (call {rep + 1}{', clone' if host_only else ''}) differs from opd_detr_detect"
            fw_out = []
            for rep in range(2):
                for resized in (True, False):
                    lg, bx = np.full((B, Q, ncls), np.nan, np.float32), np.full((B, Q, 4), np.nan, np.float32)
                    if resized:
                        rc = lib.opd_detr_forward_resized(hd, frames.ctypes.data, HOST, B, fh, fw, H, W, lg.ctypes.data, bx.ctypes.data, None)
                    else:
                        rc = lib.opd_detr_forward(hd, pix.ctypes.data, U8, HOST, B, H, W, lg.ctypes.data, bx.ctypes.data, None)
                    assert rc == 0, _capi.last_error()
                    fw_out.append((lg.tobytes(), bx.tobytes()))
            assert all(o == fw_out[0] for o in fw_out) and np.isfinite(np.frombuffer(fw_out[0][0], np.float32)).all()
            del keep
    finally:
        lib.opd_detr_destroy(clone)
        _capi.check(lib.opd_detr_set_nms(h, PERSON, -1.0), "opd_detr_set_nms")


def test_refusals_keep_their_code_and_wording(handle):
    """Every detect / forward entry point with bad arguments: the return code and the exact opd_last_error() text, including which fault wins
    when two are present.  Every case is refused by host-side checks before anything is enqueued; the handle works afterwards."""
    lib, h, info = handle
    Q = info.num_queries
    EINVAL, ESTATE = _capi.OPD_EINVAL, _capi.OPD_ESTATE
    frames = np.ascontiguousarray(np.stack(structured_frames(3, H, W, seed=78)))
    pix = frames.ctypes.data
    hw = np.asarray([[H, W]] * 3, np.int32).ctypes.data_as(C.c_void_p)
    ptrs = (C.c_void_p * 3)(*[frames[b].ctypes.data for b in range(3)])
    holed = (C.c_void_p * 3)(frames[0].ctypes.data, None, frames[2].ctypes.data)
    o = _Out(Q, False)
    R, N = o.recs, o.cnts
    feats = np.empty((3, Q, info.d_model), np.float32)
    F = feats.ctypes.data_as(F32P)
    t = C.c_int(-1)
    T = C.byref(t)

    # every entry as f(handle, pixels-or-list, pixel_format, mem_kind, B, H, records, counts); entries without a format / mem_kind ignore it
    E = {
        "forward": lambda m, p, fmt, kind, b, hh, r, n: lib.opd_detr_forward(m, p, fmt, kind, b, hh, W, None, None, None),
        "forward_ragged": lambda m, p, fmt, kind, b, hh, r, n: lib.opd_detr_forward_ragged(m, p, fmt, kind, b, hh, W, None, None, None, None),
        "forward_resized": lambda m, p, fmt, kind, b, hh, r, n: lib.opd_detr_forward_resized(m, p, kind, b, 48, 64, hh, W, None, None, None),
        "detect": lambda m, p, fmt, kind, b, hh, r, n: lib.opd_detr_detect(m, p, fmt, kind, b, hh, W, 0.5, hw, r, n),
        "detect_ragged": lambda m, p, fmt, kind, b, hh, r, n: lib.opd_detr_detect_ragged(m, p, fmt, kind, b, hh, W, None, 0.5, hw, r, n),
        "detect_async": lambda m, p, fmt, kind, b, hh, r, n: lib.opd_detr_detect_async(m, p, fmt, kind, b, hh, W, 0.5, hw, r, n, T),
        "detect_resized": lambda m, p, fmt, kind, b, hh, r, n: lib.opd_detr_detect_resized(m, p, kind, b, 48, 64, hh, W, 0.5, r, n),
        "detect_frames": lambda m, p, fmt, kind, b, hh, r, n: lib.opd_detr_detect_frames(m, p, kind, b, 48, 64, hh, W, 0.5, r, n),
        "detect_frames_features": lambda m, p, fmt, kind, b, hh, r, n: lib.opd_detr_detect_frames_features(m, p, b, 48, 64, hh, W, 0.5, PERSON, r, n, F),
        "detect_frames_color": lambda m, p, fmt, kind, b, hh, r, n: lib.opd_detr_detect_frames_color(m, p, b, 48, 64, hh, W, 0.5, PERSON, r, n, F),
    }
    LISTS = ("detect_frames", "detect_frames_features", "detect_frames_color")
    FORMATTED = ("forward", "forward_ragged", "detect", "detect_ragged", "detect_async")
    KINDED = FORMATTED + ("forward_resized", "detect_resized")
    DETECTS = tuple(k for k in E if k.startswith("detect"))
    NULL_OUT = {"detect": "opd_detr_detect: null output buffer", "detect_ragged": "opd_detr_detect: null output buffer",
                "detect_async": "opd_detr_detect_async: null argument", "detect_resized": "opd_detr_detect_resized: null output buffer",
                "detect_frames": "opd_detr_detect_frames: null output buffer",
                "detect_frames_features": "opd_detr_detect_frames_features: null output buffer",
                "detect_frames_color": "opd_detr_detect_frames_color: null output buffer"}
    PUBLIC = {"detect": "opd_detr_detect", "detect_ragged": "opd_detr_detect", "detect_async": "opd_detr_detect_async",
              "detect_resized": "opd_detr_detect_resized", "detect_frames": "opd_detr_detect_frames"}
    not_dev = ": this mem_kind takes DEVICE output pointers; the ones given are not device-accessible memory"
    outside = lambda b, hh: f"frame batch [{b},{hh},{W}] outside the configured maximum [{B},{H},{W}] (either orientation)"
    src = lambda k: ptrs if k in LISTS else pix

    rows = []   # (what, entry, call, code, message)
    for k, f in E.items():
        rows.append(("null handle", k, lambda f=f, k=k: f(None, src(k), U8, HOST, B, H, R, N), EINVAL, "null model handle"))
        rows.append(("null handle and null outputs", k, lambda f=f, k=k: f(None, src(k), U8, HOST, B, H, None, None), EINVAL, "null model handle"))
        rows.append(("B = max_batch + 1", k, lambda f=f, k=k: f(h, src(k), U8, HOST, B + 1, H, R, N), EINVAL, outside(B + 1, H)))
        rows.append(("H = 31", k, lambda f=f, k=k: f(h, src(k), U8, HOST, B, 31, R, N), EINVAL, outside(B, 31)))
        rows.append(("null outputs and H = 31", k, lambda f=f, k=k: f(h, src(k), U8, HOST, B, 31, None, None), EINVAL, outside(B, 31)))
        rows.append(("null pixels", k, lambda f=f: f(h, None, U8, HOST, B, H, R, N), EINVAL, "null pixel buffer"))
    for k in DETECTS:
        rows.append(("null records", k, lambda f=E[k], k=k: f(h, src(k), U8, HOST, B, H, None, N), EINVAL, NULL_OUT[k]))
        rows.append(("null counts", k, lambda f=E[k], k=k: f(h, src(k), U8, HOST, B, H, R, None), EINVAL, NULL_OUT[k]))
    for k in LISTS:
        rows.append(("null pointer in the frame list", k, lambda f=E[k]: f(h, holed, U8, HOST, B, H, R, N), EINVAL,
                     f"opd_detr_{k}: null frame pointer"))
        rows.append(("null pointer in the frame list and null outputs", k, lambda f=E[k]: f(h, holed, U8, HOST, B, H, None, None), EINVAL,
                     f"opd_detr_{k}: null frame pointer"))
    rows.append(("OPD_MEM_DEVICE", "detect_frames", lambda: E["detect_frames"](h, ptrs, U8, DEVICE, B, H, R, N), EINVAL, "opd_detr_detect_frames takes host frames"))
    rows.append(("OPD_MEM_DEVICE and H = 31", "detect_frames", lambda: E["detect_frames"](h, ptrs, U8, DEVICE, B, 31, R, N), EINVAL,
                 "opd_detr_detect_frames takes host frames"))
    rows.append(("unknown mem_kind", "detect_frames", lambda: E["detect_frames"](h, ptrs, U8, 9, B, H, R, N), EINVAL, "opd_detr_detect_frames takes host frames"))
    for k, name in PUBLIC.items():
        rows.append(("pageable pointers as device outputs", k, lambda f=E[k], k=k: f(h, src(k), U8, DEVOUT, B, H, R, N), EINVAL, name + not_dev))
    for k in KINDED:
        rows.append(("pageable pixels as device pixels", k, lambda f=E[k]: f(h, pix, U8, DEVICE, B, H, R, N), EINVAL,
                     "OPD_MEM_DEVICE: the pixel pointer is not device-accessible memory"))
        rows.append(("unknown mem_kind", k, lambda f=E[k]: f(h, pix, U8, 9, B, H, R, N), EINVAL, "unknown mem_kind"))
    for k in FORMATTED:
        rows.append(("unknown pixel_format", k, lambda f=E[k]: f(h, pix, 7, HOST, B, H, R, N), EINVAL, "unknown pixel_format"))
        rows.append(("unknown pixel_format and mem_kind", k, lambda f=E[k]: f(h, pix, 7, 9, B, H, R, N), EINVAL, "unknown pixel_format"))
    rows.append(("null ticket", "detect_async", lambda: lib.opd_detr_detect_async(h, pix, U8, HOST, B, H, W, 0.5, hw, R, N, None), EINVAL,
                 "opd_detr_detect_async: null argument"))
    rows.append(("4097 columns", "detect_frames_color", lambda: lib.opd_detr_detect_frames_color(h, ptrs, B, 48, 4097, H, W, 0.5, PERSON, R, N, F), EINVAL,
                 "opd_detr_detect_frames_color: frames of 48 x 4097 are outside the 4096 x 4096 the exact integer sums are sized for"))
    rows.append(("0 rows", "detect_frames_color", lambda: lib.opd_detr_detect_frames_color(h, ptrs, B, 0, 64, H, W, 0.5, PERSON, R, N, F), EINVAL,
                 "opd_detr_detect_frames_color: frames of 0 x 64 are outside the 4096 x 4096 the exact integer sums are sized for"))
    rows.append(("null communicator", "comm_detect", lambda: lib.opd_comm_detect(None, 0, pix, U8, HOST, B, H, W, 0.5, hw), EINVAL,
                 "opd_comm_detect: null communicator"))

    bad = []
    for what, entry, call, code, msg in rows:
        rc = call()
        err = _capi.last_error()
        if rc != code or err != msg:
            bad.append(f"{entry}, {what}: got ({rc}, {err!r}), expected ({code}, {msg!r})")
    assert not bad, "\n".join(bad)

    _capi.check(lib.opd_detr_set_profiling(h, 1), "opd_detr_set_profiling")
    try:
        assert E["detect_async"](h, pix, U8, HOST, B, H, R, N) == ESTATE
        assert _capi.last_error() == "opd_detr_detect_async is not available in profiling mode"
        assert E["detect_async"](h, pix, U8, HOST, B, 31, R, N) == EINVAL and _capi.last_error() == outside(B, 31)   # (the shape check comes first)
    finally:
        _capi.check(lib.opd_detr_set_profiling(h, 0), "opd_detr_set_profiling")
    assert t.value == -1 and (o.c == 0x55555555).all() and (o.r == 0x55555555).all(), "a refused call wrote to its outputs"
    assert E["detect"](h, pix, U8, HOST, B, H, R, N) == 0, _capi.last_error()
    assert all(0 <= int(n) <= Q for n in o.c)
