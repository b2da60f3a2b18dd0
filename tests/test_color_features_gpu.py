"""Colour-histogram appearance features on the device: ``opd_color_features`` and ``opd_detr_detect_frames_color`` against the host
restatement (``FeatureExtractor.extract_batch`` on ``crop_boxes``, itself pinned to the reference's rows by test_color_features_cpu.py).

The bound.  Before normalisation 195 of a row's 198 entries are integer counts or correctly rounded fp64 quotients of exact integers:
bit-identical to numpy's.  The three std entries are within one float32 ulp.  One fp64 norm and one rounding then put every output
within 2^-24 of the exactly evaluated formula; the host rows lie d_ref from it (recorded in the fixture).  Asserted:
max |device - host| <= 2^-23 + d_ref, for every case, none left out."""

import ctypes as C
import faulthandler

import numpy as np
import pytest
import torch

import color_common as CC
from office_person_detection_vit_amd import HipDetrDetector, _capi
from office_person_detection_vit_amd.feature_extractor import FeatureExtractor, crop_boxes
from office_person_detection_vit_amd.frames import structured_frames
from office_person_detection_vit_amd.weights import DetrArch, ensure_weight_file

pytestmark = pytest.mark.gpu

PERSON = 1


@pytest.fixture(autouse=True)
def _time_limit():
    """Every test runs under its own limit: a hang ends the process (with a traceback) instead of holding the GPU."""
    faulthandler.dump_traceback_later(300, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def lib():
    return _capi.load_library()


@pytest.fixture(scope="module")
def bound():
    d_ref = float(np.load(CC.GOLDEN)["d_ref"])
    return 2.0 ** -23 + d_ref


def _frames(n, h, w, seed):
    frames = [np.ascontiguousarray(f).copy() for f in structured_frames(n, h, w, seed=seed)]
    for f in frames:
        f[60:80, 100:130] = CC.UNIFORM_BGR   # the fixture's uniform box stays uniform on every test frame
    return frames


def _boxes(rng, n, h, w):
    """Person-sized boxes, a share of them overhanging the frame."""
    bh = rng.uniform(40, 0.6 * h, n)
    return np.stack([rng.uniform(-60, w - 20, n), rng.uniform(-60, h - 20, n), bh * rng.uniform(0.3, 0.6, n), bh], 1).astype(np.float32)


def _host(frame, boxes):
    return FeatureExtractor().extract_batch(crop_boxes(frame, boxes))


def test_staging_pair_regrown_between_calls(lib, bound):
    """The per-device staging pair starts at 64 KiB and lives as long as the process: one 8 x 8 box on a 32 x 32 frame, then a whole
    160 x 160 frame (76 800 bytes of window: as the first test of the module this frees the pair and allocates it anew), then the first
    input again.  The first and third rows are the same bits; the second meets the parity test's bound.  Then the same once more around a
    whole 1100 x 1930 frame, larger than any frame another test of this module stages, so that a regrow happens wherever the test runs."""
    small = np.ascontiguousarray(structured_frames(1, 32, 32, seed=5)[0]).copy()
    large = np.ascontiguousarray(structured_frames(1, 160, 160, seed=6)[0]).copy()
    box, whole = np.array([(8, 8, 8, 8)], np.float32), np.array([(0, 0, 160, 160)], np.float32)
    first = CC.device_color_features(lib, [small], box)
    second = CC.device_color_features(lib, [large], whole)
    third = CC.device_color_features(lib, [small], box)
    assert np.isfinite(first).all() and first.tobytes() == third.tobytes()
    d = float(np.abs(second.astype(np.float64) - _host(large, whole).astype(np.float64)).max())
    d_exact = float(np.abs(second.astype(np.float64) - CC.exact_rows([large])).max())
    print(f"160x160 whole-frame crop across a regrow: max |device - host| = {d:.3e}, |device - exact| = {d_exact:.3e}, bound {bound:.3e}")
    assert d <= bound and d_exact <= bound
    huge = np.ascontiguousarray(np.tile(large, (7, 13, 1))[:1100, :1930])   # (tiled: cheap to make)
    everything = np.array([(0, 0, 1930, 1100)], np.float32)
    fourth = CC.device_color_features(lib, [huge], everything)
    fifth = CC.device_color_features(lib, [small], box)
    d = float(np.abs(fourth.astype(np.float64) - _host(huge, everything).astype(np.float64)).max())
    print(f"1100x1930 whole-frame crop across a regrow: max |device - host| = {d:.3e}, bound {bound:.3e}")
    assert first.tobytes() == fifth.tobytes() and d <= bound


@pytest.mark.parametrize("hw", [(720, 1280), (1080, 1920)])
def test_parity_with_the_host_restatement(lib, bound, hw):
    h, w = hw
    frame = _frames(1, h, w, seed=7)[0]
    rng = np.random.default_rng(h)
    edge = np.array([(w - 30.5, h - 20.25, 90.0, 90.0), (-5.0, h - 1.0, 50.0, 10.0), (w, 10.0, 5.0, 5.0), (w - 1.0, h - 1.0, 1.0, 1.0),
                     (0.0, 0.0, w, h), (-3.0, -3.0, w + 6.0, h + 6.0)], np.float32)   # (the last two: whole-frame crops over many workgroups)
    boxes = np.concatenate([CC.GOLDEN_BOXES, edge, _boxes(rng, 160, h, w)])
    want = _host(frame, boxes)
    got = CC.device_color_features(lib, [frame], boxes)
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape == (len(boxes), 256)
    d = np.abs(got.astype(np.float64) - want.astype(np.float64)).max(axis=1)
    print(f"{h}x{w}: {len(boxes)} boxes, max |device - host| = {d.max():.3e} (box {int(d.argmax())}), bound {bound:.3e}")
    assert np.isfinite(got).all()
    assert d.max() <= bound
    assert not got[:, 198:].any()


def test_fixture_rows_on_the_device(lib, bound):
    g = np.load(CC.GOLDEN)
    got = CC.device_color_features(lib, [g["frame"]], g["boxes"])
    d = np.abs(got.astype(np.float64) - g["rows"].astype(np.float64)).max()
    print(f"fixture: max |device - reference rows| = {d:.3e}, bound {bound:.3e}")
    assert d <= bound
    want = np.zeros(256, np.float32)
    want[[0, 64, 128]] = np.float32(1.0 / np.sqrt(3.0))
    for k in np.flatnonzero(g["rects"][:, 4] == 0):   # degenerate boxes: the dummy-crop row
        assert np.abs(got[k] - want).max() <= 2.0 ** -24
    uniform = int(np.flatnonzero((g["boxes"] == (100.0, 60.0, 30.0, 20.0)).all(axis=1))[0])
    assert (got[uniform, [193, 195, 197]] == 0.0).all()   # std of a uniform crop is exactly 0


def test_rows_do_not_depend_on_batch_run_or_memory_kind(lib):
    h, w = 720, 1280
    frames = _frames(3, h, w, seed=11)
    rng = np.random.default_rng(3)
    boxes = np.concatenate([_boxes(rng, 157, h, w), np.array([(0, 0, w, h), (5, 5, 1, 1), (w + 1, 0, 4, 4)], np.float32)])
    owner = (np.arange(len(boxes)) % 3).astype(np.int32)
    batch = CC.device_color_features(lib, frames, boxes, owner)
    assert np.array_equal(batch, CC.device_color_features(lib, frames, boxes, owner))                       # a second run
    for k in (0, 1, 77, 157, 158, 159):                                                                      # alone
        alone = CC.device_color_features(lib, frames, boxes[k:k + 1], owner[k:k + 1])
        assert np.array_equal(alone[0], batch[k]), k
    keep = [torch.from_numpy(f).cuda() for f in frames]
    torch.cuda.synchronize()
    dev = CC.device_color_features(lib, [(t.data_ptr(), h, w) for t in keep], boxes, owner, mem_kind=_capi.OPD_MEM_DEVICE)
    assert np.array_equal(dev, batch)                                                                        # frames read in place
    odd = torch.zeros(h * w * 3 + 1, dtype=torch.uint8, device="cuda")                                       # a frame at an odd address
    odd[1:] = keep[0].reshape(-1)
    torch.cuda.synchronize()
    shifted = CC.device_color_features(lib, [(odd.data_ptr() + 1, h, w)], boxes[owner == 0], mem_kind=_capi.OPD_MEM_DEVICE)
    assert np.array_equal(shifted, batch[owner == 0])
    for f in range(3):                                                                                       # per-frame calls
        assert np.array_equal(CC.device_color_features(lib, [frames[f]], boxes[owner == f]), batch[owner == f])
    # a few large crops make the whole frames the smaller upload: same rows
    big = np.array([(0, 0, w, h), (10, 10, w - 20, h - 20), (3, 3, 200, 300)], np.float32)
    a = CC.device_color_features(lib, frames[:1], big)
    for k in range(3):
        assert np.array_equal(a[k:k + 1], CC.device_color_features(lib, frames[:1], big[k:k + 1])), k


def _records(lib_fn, det, frame, target, features):
    Q = det.num_queries
    recs, counts = (_capi.OpdDet * Q)(), (C.c_int32 * 1)()
    ptrs = (C.c_void_p * 1)(frame.ctypes.data)
    args = [C.c_void_p(det.model), ptrs]
    if features is None:
        rc = lib_fn(*args, _capi.OPD_MEM_HOST, 1, frame.shape[0], frame.shape[1], target[0], target[1], float(det.confidence_threshold), recs, counts)
    else:
        rc = lib_fn(*args, 1, frame.shape[0], frame.shape[1], target[0], target[1], float(det.confidence_threshold), PERSON, recs, counts,
                    features.ctypes.data_as(C.POINTER(C.c_float)))
    _capi.check(rc, "detect")
    n = int(counts[0])
    return n, [(r.x1, r.y1, r.x2, r.y2, r.score, r.label, r.query_index, r.frame) for r in recs[:n]]


@pytest.mark.parametrize("hw", [(288, 512), (180, 320)])   # model resolution (frames read from the model's own input), and resized
def test_fused_call_rows_equal_the_standalone_call(lib, weight_cache, hw):
    path = ensure_weight_file(weight_cache, DetrArch(), 0, 1.0, "r50")
    det = HipDetrDetector(model_path=path, max_batch=2, max_size=(288, 512), resize=True, confidence_threshold=0.05)
    det.load_model()
    try:
        Q = det.num_queries
        total = 0
        for frame in _frames(3, hw[0], hw[1], seed=41):
            target = det._frame_list_target([frame])
            assert target == (288, 512)
            n0, plain = _records(lib.opd_detr_detect_frames, det, frame, target, None)
            feats = np.zeros((1, Q, 256), np.float32)
            n1, fused = _records(lib.opd_detr_detect_frames_color, det, frame, target, feats)
            assert n0 == n1 and plain == fused                      # records and counts: what opd_detr_detect_frames gives
            person = [r for r in fused if r[5] == PERSON]
            total += len(person)
            for r in person:
                bbox = (float(r[0]), float(r[1]), float(r[2] - r[0]), float(r[3] - r[1]))   # Detection.bbox as the shim derives it
                want = CC.device_color_features(lib, [frame], [bbox])[0]
                assert np.array_equal(feats[0, r[6]], want), r
            # the Python surface: same detections as the default mode, rows assigned, default mode unchanged
            dets_c, fc = det.detect_with_features(frame, features="color")
            dets_e, fe = det.detect_with_features(frame)
            dets_x, fx = det.detect_with_features(frame, features="encoder")
            sig = lambda ds: [(d.query_index, d.bbox, d.confidence) for d in ds]
            assert sig(dets_c) == sig(dets_e) == sig(dets_x) and np.array_equal(np.asarray(fe), np.asarray(fx))
            enc = np.zeros((1, Q, 256), np.float32)
            _records(lib.opd_detr_detect_frames_features, det, frame, target, enc)
            for i, d in enumerate(dets_c):
                assert np.array_equal(d.features, feats[0, d.query_index]) and np.array_equal(fc[i], d.features)
                assert np.array_equal(dets_e[i].features, enc[0, d.query_index])
            if dets_c:
                assert fc.shape == (len(dets_c), 256) and fc.dtype == np.float32
                assert np.array_equal(det.extract_color_features(frame, dets_c), fc)
        # a batch of two frames in one call: every frame's rows come from its own pixels
        pair = _frames(2, hw[0], hw[1], seed=43)
        ptrs = (C.c_void_p * 2)(*[f.ctypes.data for f in pair])
        recs, counts, feats = (_capi.OpdDet * (2 * Q))(), (C.c_int32 * 2)(), np.zeros((2, Q, 256), np.float32)
        _capi.check(lib.opd_detr_detect_frames_color(C.c_void_p(det.model), ptrs, 2, hw[0], hw[1], 288, 512, 0.05, PERSON, recs, counts,
                                                     feats.ctypes.data_as(C.POINTER(C.c_float))), "opd_detr_detect_frames_color")
        for b in range(2):
            _, single = _records(lib.opd_detr_detect_frames, det, pair[b], (288, 512), None)
            got = [(r.x1, r.y1, r.x2, r.y2, r.score, r.label, r.query_index) for r in recs[b * Q:b * Q + int(counts[b])]]
            assert got == [r[:7] for r in single] and all(r.frame == b for r in recs[b * Q:b * Q + int(counts[b])])
            for r in got:
                if r[5] == PERSON:
                    bbox = (float(r[0]), float(r[1]), float(r[2] - r[0]), float(r[3] - r[1]))
                    assert np.array_equal(feats[b, r[6]], CC.device_color_features(lib, [pair[b]], [bbox])[0]), (b, r)
                    total += 1
        assert total >= 2, f"the test frames give {total} person records at threshold 0.05: nothing to compare"
        assert det.extract_color_features(frame, []).shape == (0,)
    finally:
        det.close()


def test_refusals(lib, weight_cache):
    frame = _frames(1, 96, 160, seed=5)[0]
    box = np.array([(1, 1, 10, 10)], np.float32)
    out = np.zeros((1, 256), np.float32)
    ptrs = (C.c_void_p * 1)(frame.ctypes.data)
    hw = np.array([96, 160], np.int32)

    def call(frames=ptrs, frame_hw=hw, n_frames=1, mem_kind=_capi.OPD_MEM_HOST, boxes=box, owner=None, n=1, dst=out):
        return lib.opd_color_features(0, frames, frame_hw.ctypes.data_as(C.c_void_p) if frame_hw is not None else None, n_frames, mem_kind,
                                      boxes.ctypes.data_as(C.c_void_p) if boxes is not None else None,
                                      owner.ctypes.data_as(C.c_void_p) if owner is not None else None, n,
                                      dst.ctypes.data_as(C.c_void_p) if dst is not None else None)

    assert call() == _capi.OPD_OK
    assert call(n=0, boxes=None, dst=None) == _capi.OPD_OK                                   # nothing to do is not an error
    for kwargs, text in (
            (dict(owner=np.array([1], np.int32)), "box 0 names frame 1"),
            (dict(owner=np.array([-1], np.int32)), "box 0 names frame -1"),
            (dict(boxes=None), "null argument"),
            (dict(dst=None), "null argument"),
            (dict(frame_hw=None), "null argument"),
            (dict(frames=(C.c_void_p * 1)(None)), "frame 0 has no pixels"),
            (dict(frame_hw=np.array([4097, 160], np.int32)), "above the 4096 x 4096"),
            (dict(frame_hw=np.array([96, 5000], np.int32)), "above the 4096 x 4096"),
            (dict(mem_kind=_capi.OPD_MEM_HOST_PIXELS_DEVICE_OUT), "mem_kind must be"),
            (dict(mem_kind=_capi.OPD_MEM_DEVICE), "not device-accessible"),                  # a host pointer is refused, not read
            (dict(n=-1), "negative box count")):
        assert call(**kwargs) == _capi.OPD_EINVAL, kwargs
        assert text in _capi.last_error(), (kwargs, _capi.last_error())
    path = ensure_weight_file(weight_cache, DetrArch(), 0, 1.0, "r50")
    det = HipDetrDetector(model_path=path, max_batch=1, max_size=(288, 512), resize=True)
    det.load_model()
    try:
        Q = det.num_queries
        recs, counts, feats = (_capi.OpdDet * Q)(), (C.c_int32 * 1)(), np.zeros((1, Q, 256), np.float32)
        fp = feats.ctypes.data_as(C.POINTER(C.c_float))
        fn = lib.opd_detr_detect_frames_color
        assert fn(C.c_void_p(det.model), ptrs, 1, 4097, 160, 288, 512, 0.5, PERSON, recs, counts, fp) == _capi.OPD_EINVAL
        assert "outside the 4096 x 4096" in _capi.last_error()
        assert fn(C.c_void_p(det.model), ptrs, 1, 96, 160, 288, 512, 0.5, PERSON, recs, counts, None) == _capi.OPD_EINVAL
        assert "null output buffer" in _capi.last_error()
        assert fn(C.c_void_p(det.model), (C.c_void_p * 1)(None), 1, 96, 160, 288, 512, 0.5, PERSON, recs, counts, fp) == _capi.OPD_EINVAL
        assert "null frame pointer" in _capi.last_error()
        with pytest.raises(ValueError, match="features must be"):
            det.detect_with_features(frame, features="hog")
    finally:
        det.close()
