"""GPU tests of the OSNet Re-ID model (-m gpu): device pixels bit-exact with Pillow + torchvision in fp16, each kernel family against
fp32 torch on fp16-rounded operands through the test hooks, features against the fp32 goldens within the bounds the fp16 emulation
supports (osnet_common.py), and determinism: bit-identical across batches, chunks, eager / graph, host / device frames, threads, and
handles of both models and a detector alive in one process."""

import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import osnet_common as O
from office_person_detection_vit_amd import HipOSNetReIDExtractor, _capi, create_reid_extractor
from office_person_detection_vit_amd.weights import ensure_clip_weight_file, ensure_osnet_weight_file

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return _capi.load_library(test_hooks=True)


@pytest.fixture(scope="module")
def frames():
    return [np.ascontiguousarray(f) for f in O.golden_frames()]


class Handle:
    def __init__(self, lib, path, max_crops, flags=0, model=_capi.OPD_REID_MODEL_OSNET):
        cfg = _capi.OpdReidConfig()
        cfg.struct_size = C.sizeof(_capi.OpdReidConfig)
        cfg.max_crops = max_crops
        cfg.flags = flags
        cfg.model = model
        self.lib, self.h = lib, C.c_void_p()
        _capi.check(lib.opd_reid_create(C.byref(cfg), path.encode(), 0, C.byref(self.h)), "opd_reid_create")

    def extract(self, frames, boxes, owner, mem_kind=_capi.OPD_MEM_HOST, ptrs=None):
        boxes = np.ascontiguousarray(boxes, np.float32)
        owner = np.ascontiguousarray(owner, np.int32)
        hw = np.array([f.shape[:2] for f in frames], np.int32)
        p = (C.c_void_p * len(frames))(*(ptrs or [f.ctypes.data for f in frames]))
        out = np.zeros((len(boxes), 512), np.float32)
        _capi.check(self.lib.opd_reid_extract(self.h, p, hw.ctypes.data, len(frames), mem_kind, boxes.ctypes.data, owner.ctypes.data,
                                              len(boxes), out.ctypes.data), "opd_reid_extract")
        return out

    def close(self):
        self.lib.opd_reid_destroy(self.h)


@pytest.fixture(scope="module")
def mild(lib, weight_cache):
    h = Handle(lib, ensure_osnet_weight_file(weight_cache, "mild"), 64)
    yield h
    h.close()


def _f16(a):
    return np.ascontiguousarray(np.asarray(a, np.float32).astype(np.float16))


def _t(a):
    return torch.from_numpy(np.asarray(a, np.float32))


def _nchw(a, nb, H, W):
    return _t(a).reshape(nb, H, W, -1).permute(0, 3, 1, 2)


# ---- 1. pixels ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mem_kind", [_capi.OPD_MEM_HOST, _capi.OPD_MEM_DEVICE])
def test_device_pixels_equal_pil(lib, frames, mild, mem_kind):
    boxes = np.asarray(O.PIXEL_BOXES, np.float32)
    n = len(boxes)
    owner = (np.arange(n) % 2).astype(np.int32)
    hw = np.array([f.shape[:2] for f in frames], np.int32)
    keep = [torch.from_numpy(f).cuda() for f in frames] if mem_kind == _capi.OPD_MEM_DEVICE else None
    ptrs = [t.data_ptr() for t in keep] if keep else [f.ctypes.data for f in frames]
    torch.cuda.synchronize()
    p = (C.c_void_p * 2)(*ptrs)
    out = np.zeros((n, 256, 128, 4), np.uint16)
    _capi.check(lib.opd_test_reid_pixels(mild.h, p, hw.ctypes.data, 2, mem_kind, boxes.ctypes.data, owner.ctypes.data, n, out.ctypes.data),
                "opd_test_reid_pixels")
    ref = O.to_device_layout(O.reference_pixels(frames, boxes, owner))
    for i in range(n):
        np.testing.assert_array_equal(out[i], ref[i], err_msg=f"box {i}: {O.PIXEL_BOXES[i]}")


# ---- 2. kernel families ----------------------------------------------------------------------------------------------------------------
def _gemm(lib, epi, a1, k1, w, bias=None, a2=None, k2=0, res=None, out=None, N=None, groups=1, a_gcol=0, o_gcol=0):
    M, lda1 = a1.shape
    lda2 = a2.shape[1] if a2 is not None else 0
    out = np.zeros((M, N * groups if out is None else 0), np.float16) if out is None else out
    _capi.check(lib.opd_test_osnet_gemm(epi, a1.ctypes.data, lda1, k1, a2.ctypes.data if a2 is not None else None, lda2, k2, w.ctypes.data,
                                        bias.ctypes.data if bias is not None else None, res.ctypes.data if res is not None else None,
                                        res.shape[1] if res is not None else 0, out.ctypes.data, out.shape[1], M, N, groups, a_gcol, o_gcol),
                "opd_test_osnet_gemm")
    return out


def _dw(lib, u, t, w9, bias, nb, H, W, c0, nc):
    ld = u.shape[1]
    _capi.check(lib.opd_test_osnet_dwconv(u.ctypes.data, t.ctypes.data, w9.ctypes.data, bias.ctypes.data, nb, H, W, ld, c0, nc, w9.shape[1]),
                "opd_test_osnet_dwconv")


@pytest.mark.parametrize("level", [1, 4])
def test_lightconv_level(lib, level):
    """One LightConv level of an OSBlock: the 1x1 of the running streams (level 1: one GEMM with N = 4 mid on x1; level 4: the grouped
    GEMM on stream d alone) and the depthwise 3x3 + folded BN + ReLU, against torch fp32 on the same fp16 operands."""
    rng = np.random.default_rng(level)
    nb, H, W, mid = 3, 32, 16, 96
    M, ld = nb * H * W, 4 * mid
    S = 5 - level
    c0 = (level - 1) * mid
    if level == 1:
        a = _f16(rng.standard_normal((M, mid)))
        wl = _f16(rng.standard_normal((4 * mid, mid)) * mid ** -0.5)
        u = _gemm(lib, 0, a, mid, wl, N=4 * mid)
        ref_u = _t(a) @ _t(wl).T
    else:
        t_in = _f16(rng.standard_normal((M, ld)))
        wl = _f16(rng.standard_normal((S, mid, mid)) * mid ** -0.5)
        u = np.zeros((M, ld), np.float16)
        a_view = np.ascontiguousarray(t_in[:, c0:])   # the hook takes a1 from column 0: pass the slice with the same pitch
        a_pad = np.zeros((M, ld), np.float16)
        a_pad[:, :S * mid] = a_view
        u_part = np.zeros((M, ld), np.float16)
        _gemm(lib, 0, a_pad, mid, wl, out=u_part, N=mid, groups=S, a_gcol=mid, o_gcol=mid)
        u[:, c0:] = u_part[:, :S * mid]
        ref_u = torch.cat([_t(t_in[:, c0 + z * mid:c0 + (z + 1) * mid]) @ _t(wl[z]).T for z in range(S)], 1)
    np.testing.assert_allclose(u[:, c0:].astype(np.float32), ref_u.numpy(), atol=2e-2, rtol=2e-3)
    w9 = (rng.standard_normal((9, ld)) * 0.4).astype(np.float32)
    bias = (rng.standard_normal(ld) * 0.2).astype(np.float32)
    t = np.zeros((M, ld), np.float16)
    _dw(lib, u, t, w9, bias, nb, H, W, c0, S * mid)
    x = _nchw(u[:, c0:].astype(np.float32), nb, H, W)
    k = _t(w9[:, c0:]).T.reshape(S * mid, 1, 3, 3)
    ref = F.relu(F.conv2d(x, k, padding=1, groups=S * mid) + _t(bias[c0:])[None, :, None, None]).permute(0, 2, 3, 1).reshape(M, -1)
    assert np.abs(t[:, c0:].astype(np.float32) - ref.numpy()).max() < 1e-2
    assert not t[:, :c0].any()   # columns of finished streams untouched


@pytest.mark.parametrize("mid", [64, 96, 128])
@pytest.mark.parametrize("down", [False, True])
def test_gated_block_output(lib, mid, down):
    """Gate (pooled means -> fc1 -> ReLU -> fc2 -> sigmoid), x2 = sum of gated streams, then [conv3 | downsample] with biases summed and
    ReLU, or conv3 + identity + ReLU."""
    rng = np.random.default_rng(mid + down)
    nb, H, W = 2, 16, 8
    HW, M, hid = H * W, nb * H * W, mid // 16
    cout = 4 * mid
    cin = 2 * mid if down else cout
    t = _f16(np.abs(rng.standard_normal((M, 4 * mid))))
    w1 = (rng.standard_normal((hid, mid)) * mid ** -0.5 * 2).astype(np.float32)
    b1 = (rng.standard_normal(hid) * 0.1).astype(np.float32)
    w2 = (rng.standard_normal((mid, hid)) * hid ** -0.5 * 2).astype(np.float32)
    b2 = (rng.standard_normal(mid) * 0.1).astype(np.float32)
    gates = np.zeros((nb, 4, mid), np.float32)
    x2 = np.zeros((M, mid), np.float16)
    _capi.check(lib.opd_test_osnet_gate(t.ctypes.data, w1.ctypes.data, b1.ctypes.data, w2.ctypes.data, b2.ctypes.data, gates.ctypes.data,
                                        x2.ctypes.data, nb, HW, mid, hid), "opd_test_osnet_gate")
    tt = _t(t).reshape(nb, HW, 4, mid)
    pooled = tt.mean(1)
    g = torch.sigmoid(F.relu(pooled @ _t(w1).T + _t(b1)) @ _t(w2).T + _t(b2))
    np.testing.assert_allclose(gates, g.numpy(), atol=2e-6, rtol=1e-5)
    ref_x2 = (tt * g[:, None]).sum(2).reshape(M, mid)
    assert np.abs(x2.astype(np.float32) - ref_x2.numpy()).max() < 1e-2
    x = _f16(rng.standard_normal((M, cin)))
    w3 = _f16(rng.standard_normal((cout, mid + (cin if down else 0))) * (mid + cin) ** -0.5)
    b3 = (rng.standard_normal(cout) * 0.1).astype(np.float32)
    if down:
        out = _gemm(lib, 1, x2, mid, w3, b3, a2=x, k2=cin, N=cout)
        ref = F.relu(torch.cat([_t(x2), _t(x)], 1) @ _t(w3).T + _t(b3))
    else:
        out = _gemm(lib, 2, x2, mid, w3, b3, res=x, N=cout)
        ref = F.relu(_t(x2) @ _t(w3).T + _t(b3) + _t(x))
    assert np.abs(out.astype(np.float32) - ref.numpy()).max() < 1e-2


def test_transition_with_pool(lib):
    rng = np.random.default_rng(5)
    nb, H, W, C = 2, 64, 32, 256
    M = nb * H * W
    x = _f16(rng.standard_normal((M, C)))
    w = _f16(rng.standard_normal((C, C)) * C ** -0.5)
    b = (rng.standard_normal(C) * 0.1).astype(np.float32)
    y = _gemm(lib, 1, x, C, w, b, N=C)
    ref = F.relu(_t(x) @ _t(w).T + _t(b))
    assert np.abs(y.astype(np.float32) - ref.numpy()).max() < 1e-2
    pooled = np.zeros((nb * H * W // 4, C), np.float16)
    _capi.check(lib.opd_test_osnet_avgpool2(y.ctypes.data, pooled.ctypes.data, nb, H, W, C), "opd_test_osnet_avgpool2")
    refp = F.avg_pool2d(_nchw(y, nb, H, W), 2, 2).permute(0, 2, 3, 1).reshape(-1, C)
    assert np.abs(pooled.astype(np.float32) - refp.numpy()).max() < 4e-3


def test_stem_and_maxpool(lib):
    rng = np.random.default_rng(6)
    nb, C0 = 2, 64
    img = np.zeros((nb, 256, 128, 4), np.float16)
    img[..., :3] = rng.standard_normal((nb, 256, 128, 3))
    w = _f16(rng.standard_normal((147, 64)) * 147 ** -0.5)
    b = (rng.standard_normal(64) * 0.1).astype(np.float32)
    out = np.zeros((nb, 64, 32, C0), np.float16)
    _capi.check(lib.opd_test_osnet_stem(img.ctypes.data, w.ctypes.data, b.ctypes.data, out.ctypes.data, nb, C0), "opd_test_osnet_stem")
    x = _t(img[..., :3]).permute(0, 3, 1, 2)
    k = _t(w).reshape(7, 7, 3, 64).permute(3, 2, 0, 1)
    s = F.relu(F.conv2d(x, k, stride=2, padding=3) + _t(b)[None, :, None, None]).half().float()
    ref = F.max_pool2d(s, 3, 2, 1).permute(0, 2, 3, 1)
    assert np.abs(out.astype(np.float32) - ref.numpy()).max() < 1e-2


def test_head(lib):
    rng = np.random.default_rng(7)
    nb, HW, C = 5, 128, 512
    x = _f16(np.abs(rng.standard_normal((nb, HW, C))))
    wt = (rng.standard_normal((C, 512)) * C ** -0.5).astype(np.float32)
    b = (rng.standard_normal(512) * 0.1).astype(np.float32)
    feat = np.zeros((nb, 512), np.float32)
    _capi.check(lib.opd_test_osnet_head(x.ctypes.data, wt.ctypes.data, b.ctypes.data, feat.ctypes.data, nb, HW, C), "opd_test_osnet_head")
    y = F.relu(_t(x).mean(1) @ _t(wt) + _t(b))
    ref = (y / y.norm(dim=-1, keepdim=True)).numpy()
    assert np.abs(feat - ref).max() < 1e-5


# ---- 3. features against the goldens ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["mild", "sharp", "half", "odd"])
def test_features_match_golden(lib, weight_cache, golden_dir, frames, parity_log, tag):
    """x1.0 (mild, sharp), x0.5 (half) and the odd widths 16 / 64 / 192 / 320 with one block per stage (odd), each within its own
    bound (osnet_common.feat_bounds; the x1.0 ones are FEAT_MAX_ABS / FEAT_MIN_COS)."""
    g = np.load(os.path.join(golden_dir, f"osnet_{tag}.npz"))
    max_abs, min_cos = O.feat_bounds(tag)
    name = {"half": "osnet-x0.5", "odd": "osnet-odd"}.get(tag, "osnet-x1.0")
    h = Handle(lib, ensure_osnet_weight_file(weight_cache, tag), 64)
    try:
        for n in (1, 7, 37):
            got = h.extract(frames, g["boxes"][:n], g["owner"][:n])
            d, cos = O.drift(got, g["features"][:n])
            parity_log(f"reid {name} {tag} n={n} (unit features; dprob = 1 - min cos)", dprob=1.0 - cos, denc=d,
                       note=f"bound {max_abs:g} / {min_cos}")
            assert np.all(np.isfinite(got))
            np.testing.assert_allclose(np.linalg.norm(got, axis=1), 1.0, atol=1e-5)
            assert d <= max_abs and cos >= min_cos, (tag, n, d, cos)
    finally:
        h.close()


# ---- 4. determinism ----------------------------------------------------------------------------------------------------------------------
def test_bit_identical_across_batches_chunks_graph_and_memory(lib, weight_cache, frames, mild):
    boxes, owner = O.golden_boxes()
    full = mild.extract(frames, boxes, owner)
    np.testing.assert_array_equal(mild.extract(frames, boxes, owner), full)   # graph replay
    for i in (0, 9, 36):
        np.testing.assert_array_equal(mild.extract(frames, boxes[i:i + 1], owner[i:i + 1])[0], full[i])
    perm = np.random.default_rng(3).permutation(len(boxes))
    np.testing.assert_array_equal(mild.extract(frames, boxes[perm], owner[perm]), full[perm])
    path = ensure_osnet_weight_file(weight_cache, "mild")
    eager = Handle(lib, path, 64, _capi.OPD_FLAG_NO_GRAPH)
    chunked = Handle(lib, path, 16)   # 37 boxes > max_crops: three chunks
    try:
        np.testing.assert_array_equal(eager.extract(frames, boxes, owner), full)
        np.testing.assert_array_equal(chunked.extract(frames, boxes, owner), full)
    finally:
        eager.close()
        chunked.close()
    keep = [torch.from_numpy(f).cuda() for f in frames]
    torch.cuda.synchronize()
    dev = mild.extract(frames, boxes, owner, _capi.OPD_MEM_DEVICE, [t.data_ptr() for t in keep])
    np.testing.assert_array_equal(dev, full)
    assert mild.extract(frames, boxes[:0], owner[:0]).shape == (0, 512)


@pytest.mark.parametrize("tag", ["half", "odd"])
def test_bit_identical_across_batches_chunks_and_graph_other_widths(lib, weight_cache, frames, tag):
    """The determinism above at the x0.5 widths and the odd widths (one block per stage)."""
    boxes, owner = O.golden_boxes()
    path = ensure_osnet_weight_file(weight_cache, tag)
    h = Handle(lib, path, 64)
    eager = Handle(lib, path, 64, _capi.OPD_FLAG_NO_GRAPH)
    chunked = Handle(lib, path, 16)
    try:
        full = h.extract(frames, boxes, owner)
        np.testing.assert_array_equal(h.extract(frames, boxes, owner), full)
        for i in (0, 9, 36):
            np.testing.assert_array_equal(h.extract(frames, boxes[i:i + 1], owner[i:i + 1])[0], full[i])
        perm = np.random.default_rng(3).permutation(len(boxes))
        np.testing.assert_array_equal(h.extract(frames, boxes[perm], owner[perm]), full[perm])
        np.testing.assert_array_equal(eager.extract(frames, boxes, owner), full)
        np.testing.assert_array_equal(chunked.extract(frames, boxes, owner), full)
    finally:
        h.close()
        eager.close()
        chunked.close()


def test_two_threads_bit_identical(lib, weight_cache, frames, mild):
    import threading
    boxes, owner = O.golden_boxes()
    want = mild.extract(frames, boxes, owner)
    path = ensure_osnet_weight_file(weight_cache, "mild")
    results, errors = {}, []

    def work(k, max_crops):
        try:
            h = Handle(lib, path, max_crops)
            try:
                results[k] = [h.extract(frames, boxes, owner) for _ in range(3)]
            finally:
                h.close()
        except Exception as e:   # (reported below, on the main thread)
            errors.append(repr(e))

    ts = [threading.Thread(target=work, args=(k, mc)) for k, mc in enumerate((8, 32))]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=300)
    assert not errors, errors
    for k in range(2):
        for got in results[k]:
            np.testing.assert_array_equal(got, want)


def test_clip_osnet_and_detector_interleaved(lib, weight_cache, frames, mild, golden_dir):
    """A CLIP handle, an OSNet handle and a detector handle alive in one process, calls interleaved: each model's features equal what it
    gives alone (OSNet) and stay within its golden bounds (CLIP)."""
    import reid_common as R
    from office_person_detection_vit_amd import HipDetrDetector
    from office_person_detection_vit_amd.frames import structured_frames
    from office_person_detection_vit_amd.weights import DetrArch, ensure_weight_file
    boxes, owner = O.golden_boxes()
    want = mild.extract(frames, boxes, owner)
    clip = Handle(lib, ensure_clip_weight_file(weight_cache, "mild"), 64, model=_capi.OPD_REID_MODEL_CLIP)
    det = HipDetrDetector(model_path=ensure_weight_file(weight_cache, DetrArch.resnet50(), 0, 1.0, "r50"), device="hip:0", max_batch=1,
                          max_size=(256, 320), resize=False)
    det.load_model()
    try:
        g = np.load(os.path.join(golden_dir, "reid_mild.npz"))
        frame = structured_frames(1, 256, 320, seed=5)[0]
        for _ in range(2):
            det.forward_raw([frame])
            c = clip.extract(frames, g["boxes"], g["owner"])
            np.testing.assert_array_equal(mild.extract(frames, boxes, owner), want)
            d, cos = R.drift(c, g["features"])
            assert d <= R.FEAT_MAX_ABS and cos >= R.FEAT_MIN_COS
    finally:
        det.close()
        clip.close()


# ---- 5. facade ------------------------------------------------------------------------------------------------------------------------------
def test_osnet_facade_contract(weight_cache, frames, golden_dir):
    path = ensure_osnet_weight_file(weight_cache, "mild")
    ex = create_reid_extractor(model_type="osnet", model_path=path, max_crops=8)
    assert isinstance(ex, HipOSNetReIDExtractor) and not ex.is_loaded
    ex.load_model()
    assert ex.is_loaded and ex.feature_dim == 512
    assert ex.extract_features(frames[0], []).shape == (0, 512)
    g = np.load(os.path.join(golden_dir, "osnet_mild.npz"))
    sel = np.where(g["owner"] == 0)[0][:5]
    f = ex.extract_features(frames[0], [tuple(b) for b in g["boxes"][sel]])
    d, cos = O.drift(f, g["features"][sel])
    assert f.dtype == np.float32 and d <= O.FEAT_MAX_ABS and cos >= O.FEAT_MIN_COS
    batch = ex.extract_features_batch(frames, [[tuple(g["boxes"][0])], [tuple(g["boxes"][1])]])
    assert batch.shape == (2, 512)
    x1, y1, w, h = 100, 50, 60, 150
    np.testing.assert_array_equal(ex.extract_single(frames[0][y1:y1 + h, x1:x1 + w]), ex.extract_features(frames[0], [(x1, y1, w, h)])[0])
    ex.cleanup()
    assert not ex.is_loaded
