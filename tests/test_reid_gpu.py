"""GPU tests of the Re-ID path (-m gpu): device pre-processing bit-exact with HF pixel_values in fp16, features against the HF fp32
goldens within the bounds the fp16 emulation supports (tests/test_reid_cpu.py::test_fp16_emulation_within_feature_bounds), batch
independence (bit-identical), the kernels against torch fp32 through the hooks, and the facade's contract."""

import ctypes as C
import os

import numpy as np
import pytest
import torch

import reid_common as R
from office_person_detection_vit_amd import HipReIDExtractor, _capi
from office_person_detection_vit_amd.weights import ensure_clip_weight_file

pytestmark = pytest.mark.gpu

FEAT_MAX_ABS, FEAT_MIN_COS = R.FEAT_MAX_ABS, R.FEAT_MIN_COS   # from the fp16 emulation (reid_common.py)


@pytest.fixture(scope="module")
def lib():
    return _capi.load_library(test_hooks=True)


@pytest.fixture(scope="module")
def frames():
    return [np.ascontiguousarray(f) for f in R.golden_frames()]


class Handle:
    def __init__(self, lib, path, max_crops, flags=0):
        cfg = _capi.OpdReidConfig()
        cfg.struct_size = C.sizeof(_capi.OpdReidConfig)
        cfg.max_crops = max_crops
        cfg.flags = flags
        self.lib, self.h = lib, C.c_void_p()
        _capi.check(lib.opd_reid_create(C.byref(cfg), path.encode(), 0, C.byref(self.h)), "opd_reid_create")

    def extract(self, frames, boxes, owner, mem_kind=_capi.OPD_MEM_HOST, ptrs=None, dim=512):
        boxes = np.ascontiguousarray(boxes, np.float32)
        owner = np.ascontiguousarray(owner, np.int32)
        hw = np.array([f.shape[:2] for f in frames], np.int32)
        p = (C.c_void_p * len(frames))(*(ptrs or [f.ctypes.data for f in frames]))
        out = np.zeros((len(boxes), dim), np.float32)
        _capi.check(self.lib.opd_reid_extract(self.h, p, hw.ctypes.data, len(frames), mem_kind, boxes.ctypes.data, owner.ctypes.data,
                                              len(boxes), out.ctypes.data), "opd_reid_extract")
        return out

    def close(self):
        self.lib.opd_reid_destroy(self.h)


@pytest.fixture(scope="module")
def mild(lib, weight_cache):
    h = Handle(lib, ensure_clip_weight_file(weight_cache, "mild"), 64)
    yield h
    h.close()


# ---- 1. pixels ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mem_kind", [_capi.OPD_MEM_HOST, _capi.OPD_MEM_DEVICE])
def test_device_pixels_equal_hf_fp16(lib, weight_cache, frames, mem_kind):
    h = Handle(lib, ensure_clip_weight_file(weight_cache, "tiny"), 16)
    try:
        boxes = np.asarray(R.PIXEL_BOXES, np.float32)
        n = len(boxes)
        owner = (np.arange(n) % 2).astype(np.int32)
        hw = np.array([f.shape[:2] for f in frames], np.int32)
        keep = [torch.from_numpy(f).cuda() for f in frames] if mem_kind == _capi.OPD_MEM_DEVICE else None
        ptrs = [t.data_ptr() for t in keep] if keep else [f.ctypes.data for f in frames]
        torch.cuda.synchronize()
        p = (C.c_void_p * 2)(*ptrs)
        out = np.zeros((n, 50, 3072), np.uint16)
        _capi.check(lib.opd_test_reid_pixels(h.h, p, hw.ctypes.data, 2, mem_kind, boxes.ctypes.data, owner.ctypes.data, n, out.ctypes.data),
                    "opd_test_reid_pixels")
        ref = R.to_patch_rows(R.hf_pixel_values(frames, boxes, owner)).numpy().astype(np.float16).view(np.uint16)
        for i in range(n):
            np.testing.assert_array_equal(out[i], ref[i], err_msg=f"box {i}: {R.PIXEL_BOXES[i]}")
    finally:
        h.close()


# ---- 2. features against HF ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["mild", "sharp", "tiny", "p56"])
def test_features_match_hf(lib, weight_cache, golden_dir, frames, parity_log, tag):
    """B/32 (mild, sharp), hidden 128 (tiny) and patch 56 / 17 tokens / hidden 256 (p56), each within its own bound
    (reid_common.feat_bounds; the B/32 ones are FEAT_MAX_ABS / FEAT_MIN_COS)."""
    g = np.load(os.path.join(golden_dir, f"reid_{tag}.npz"))
    max_abs, min_cos = R.feat_bounds(tag)
    name = "clip-b32" if tag in ("mild", "sharp") else "clip"
    h = Handle(lib, ensure_clip_weight_file(weight_cache, tag), 64)
    try:
        for n in (1, 7, 37):
            got = h.extract(frames, g["boxes"][:n], g["owner"][:n], dim=g["features"].shape[1])
            d, cos = R.drift(got, g["features"][:n])
            parity_log(f"reid {name} {tag} n={n} (unit features; dprob = 1 - min cos)", dprob=1.0 - cos, denc=d, note=f"bound {max_abs:g} / {min_cos}")
            assert np.all(np.isfinite(got))
            assert d <= max_abs and cos >= min_cos, (tag, n, d, cos)
    finally:
        h.close()


# ---- 3. batch independence ------------------------------------------------------------------------------------------------------------
def test_batch_independence_bit_identical(lib, weight_cache, frames, mild):
    boxes, owner = R.golden_boxes()
    full = mild.extract(frames, boxes, owner)
    again = mild.extract(frames, boxes, owner)
    np.testing.assert_array_equal(full, again)   # first call against a repeated (graph replay) call
    for i in (0, 9, 36):
        alone = mild.extract(frames, boxes[i:i + 1], owner[i:i + 1])
        np.testing.assert_array_equal(alone[0], full[i])
    perm = np.random.default_rng(3).permutation(len(boxes))
    shuffled = mild.extract(frames, boxes[perm], owner[perm])
    np.testing.assert_array_equal(shuffled, full[perm])
    path = ensure_clip_weight_file(weight_cache, "mild")
    eager = Handle(lib, path, 64, _capi.OPD_FLAG_NO_GRAPH)
    chunked = Handle(lib, path, 16)   # 37 boxes > max_crops: three chunks
    try:
        np.testing.assert_array_equal(eager.extract(frames, boxes, owner), full)
        np.testing.assert_array_equal(chunked.extract(frames, boxes, owner), full)
    finally:
        eager.close()
        chunked.close()


@pytest.mark.parametrize("tag", ["tiny", "p56"])
def test_batch_independence_bit_identical_small_sets(lib, weight_cache, frames, tag):
    """The batch independence above at hidden 128 / 2 heads (tiny) and patch 56 / 17 tokens / 4 heads (p56)."""
    boxes, owner = R.golden_boxes()
    dim = 128 if tag == "tiny" else 512
    path = ensure_clip_weight_file(weight_cache, tag)
    h = Handle(lib, path, 64)
    eager = Handle(lib, path, 64, _capi.OPD_FLAG_NO_GRAPH)
    chunked = Handle(lib, path, 16)
    try:
        full = h.extract(frames, boxes, owner, dim=dim)
        np.testing.assert_array_equal(h.extract(frames, boxes, owner, dim=dim), full)
        for i in (0, 9, 36):
            np.testing.assert_array_equal(h.extract(frames, boxes[i:i + 1], owner[i:i + 1], dim=dim)[0], full[i])
        perm = np.random.default_rng(3).permutation(len(boxes))
        np.testing.assert_array_equal(h.extract(frames, boxes[perm], owner[perm], dim=dim), full[perm])
        np.testing.assert_array_equal(eager.extract(frames, boxes, owner, dim=dim), full)
        np.testing.assert_array_equal(chunked.extract(frames, boxes, owner, dim=dim), full)
    finally:
        h.close()
        eager.close()
        chunked.close()


def test_kernel_table_hook_sums_per_name_and_leaves_the_handle_as_it_was(lib, weight_cache, frames):
    """opd_test_reid_kernel_table (tiny tower, 2 crops): the rows of one and of two timed forwards name the same kernels in the same
    (first-seen) order, launches and FLOPs of every row double exactly, every row took time; and the hook leaves profiling off and the
    captured graphs valid: an extract after it returns the bytes of the extract before it."""
    boxes, owner = R.golden_boxes()
    boxes, owner = np.ascontiguousarray(boxes[:2], np.float32), np.ascontiguousarray(owner[:2], np.int32)
    h = Handle(lib, ensure_clip_weight_file(weight_cache, "tiny"), 16)
    try:
        before = h.extract(frames, boxes, owner, dim=128)
        hw = np.array([f.shape[:2] for f in frames], np.int32)
        ptrs = (C.c_void_p * len(frames))(*[f.ctypes.data for f in frames])

        def table(iters):
            cap = 64
            rows, count = (_capi.OpdKernelStat * cap)(), C.c_int()
            _capi.check(lib.opd_test_reid_kernel_table(h.h, ptrs, hw.ctypes.data, len(frames), boxes.ctypes.data, owner.ctypes.data, 2, iters, rows, cap,
                                                       C.byref(count)), "opd_test_reid_kernel_table")
            assert 0 < count.value <= cap
            return [(rows[i].name.decode(), rows[i].launches, rows[i].ms, rows[i].flops) for i in range(count.value)]

        one, two = table(1), table(2)
        for r in one:
            print(f"reid kernel table: {r[0]:60s} launches {r[1]:3d}  {r[2]:.4f} ms  {r[3]:.3e} flop")
        assert [r[0] for r in one] == [r[0] for r in two] and len({r[0] for r in one}) == len(one)
        assert all(r[0] and r[0] != "(unnamed)" for r in one)
        assert [r[1] * 2 for r in one] == [r[1] for r in two] and all(r[1] > 0 for r in one)
        assert [r[3] * 2 for r in one] == [r[3] for r in two] and any(r[3] > 0 for r in one)
        assert all(r[2] > 0 for r in one + two)
        after = h.extract(frames, boxes, owner, dim=128)
        assert before.tobytes() == after.tobytes() and np.all(np.isfinite(after))
    finally:
        h.close()


def test_handles_on_two_threads_bit_identical(lib, weight_cache, frames, mild):
    """Two Re-ID handles driven from two threads at once (graph captures, staging growth and copies interleaved) give the features a
    single thread gets: the entry points hold the library's API lock and a capture takes it exclusively."""
    import threading
    boxes, owner = R.golden_boxes()
    want = mild.extract(frames, boxes, owner)
    path = ensure_clip_weight_file(weight_cache, "mild")
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


# ---- 4. kernels -------------------------------------------------------------------------------------------------------------------------
def _f16(a):
    return np.ascontiguousarray(np.asarray(a, np.float32).astype(np.float16))


def test_attention_kernel(lib):
    rng = np.random.default_rng(0)
    crops, T, H = 3, 50, 256
    qkv = _f16(rng.standard_normal((crops * T, 3 * H)) * 1.5)
    out = np.zeros((crops * T, H), np.float16)
    _capi.check(lib.opd_test_reid_attention(qkv.ctypes.data, out.ctypes.data, crops, T, H), "opd_test_reid_attention")
    t = torch.from_numpy(qkv.astype(np.float32)).reshape(crops, T, 3, H // 64, 64)
    q, k, v = (t[:, :, j].transpose(1, 2) for j in range(3))
    ref = (torch.softmax(q @ k.transpose(-1, -2), -1) @ v).transpose(1, 2).reshape(crops * T, H).numpy()
    assert np.abs(out.astype(np.float32) - ref).max() < 1e-2


def test_layernorm_kernel(lib):
    rng = np.random.default_rng(1)
    rows, stride, H = 5, 50, 768
    x = (rng.standard_normal((rows * stride, H)) * 3 + 1).astype(np.float32)
    g = (1 + 0.1 * rng.standard_normal(H)).astype(np.float32)
    b = (0.1 * rng.standard_normal(H)).astype(np.float32)
    y16 = np.zeros((rows, H), np.float16)
    _capi.check(lib.opd_test_reid_layernorm(x.ctypes.data, g.ctypes.data, b.ctypes.data, None, y16.ctypes.data, rows, stride, H), "ln")
    ref = torch.nn.functional.layer_norm(torch.from_numpy(x[::stride]), (H,), torch.from_numpy(g), torch.from_numpy(b), 1e-5).numpy()
    assert np.abs(y16.astype(np.float32) - ref).max() < 4e-3
    y32 = np.zeros_like(x)
    y16 = np.zeros((rows * stride, H), np.float16)
    _capi.check(lib.opd_test_reid_layernorm(x.ctypes.data, g.ctypes.data, b.ctypes.data, y32.ctypes.data, y16.ctypes.data, rows * stride, 1, H),
                "ln")
    ref = torch.nn.functional.layer_norm(torch.from_numpy(x), (H,), torch.from_numpy(g), torch.from_numpy(b), 1e-5).numpy()
    assert np.abs(y32 - ref).max() < 1e-4


@pytest.mark.parametrize("M", [50, 130])
def test_quick_gelu_linear_kernel(lib, M):
    rng = np.random.default_rng(2)
    N, K = 3072, 768
    X = _f16(rng.standard_normal((M, K)))
    W = _f16(rng.standard_normal((N, K)) * K ** -0.5)
    bias = (0.1 * rng.standard_normal(N)).astype(np.float32)
    out = np.zeros((M, N), np.float16)
    _capi.check(lib.opd_test_reid_gemm(2, X.ctypes.data, W.ctypes.data, bias.ctypes.data, 0, out.ctypes.data, M, N, K), "gemm")
    z = torch.from_numpy(X.astype(np.float32)) @ torch.from_numpy(W.astype(np.float32)).T + torch.from_numpy(bias)
    ref = (z * torch.sigmoid(1.702 * z)).numpy()
    assert np.abs(out.astype(np.float32) - ref).max() < 2e-2
    # the residual epilogue on the same operands
    res = rng.standard_normal((M, N)).astype(np.float32)
    o32 = res.copy()
    _capi.check(lib.opd_test_reid_gemm(1, X.ctypes.data, W.ctypes.data, bias.ctypes.data, 0, o32.ctypes.data, M, N, K), "gemm")
    assert np.abs(o32 - (res + z.numpy())).max() < 1e-3


# ---- 5. facade ------------------------------------------------------------------------------------------------------------------------------
def test_facade_contract(weight_cache, frames, golden_dir):
    path = ensure_clip_weight_file(weight_cache, "mild")
    ex = HipReIDExtractor(model_type="clip", model_path=path, device="hip:0", max_crops=8)
    assert not ex.is_loaded
    ex.load_model()
    assert ex.is_loaded and ex.feature_dim == 512
    e = ex.extract_features(frames[0], [])
    assert e.shape == (0, 512) and e.dtype == np.float32
    g = np.load(os.path.join(golden_dir, "reid_mild.npz"))
    sel = np.where(g["owner"] == 0)[0][:5]
    f = ex.extract_features(frames[0], [tuple(b) for b in g["boxes"][sel]])
    assert f.shape == (5, 512) and f.dtype == np.float32
    np.testing.assert_allclose(np.linalg.norm(f, axis=1), 1.0, atol=1e-5)
    d, cos = R.drift(f, g["features"][sel])
    assert d <= FEAT_MAX_ABS and cos >= FEAT_MIN_COS
    batch = ex.extract_features_batch(frames, [[tuple(g["boxes"][0])], [tuple(g["boxes"][1])]])
    assert batch.shape == (2, 512)
    x1, y1, w, h = 100, 50, 60, 150
    single = ex.extract_single(frames[0][y1:y1 + h, x1:x1 + w])
    np.testing.assert_array_equal(single, ex.extract_features(frames[0], [(x1, y1, w, h)])[0])
    ex.cleanup()
    assert not ex.is_loaded
    with pytest.raises(RuntimeError):
        ex.extract_features(frames[0], [(0, 0, 10, 10)])
    ex.load_model()
    np.testing.assert_array_equal(ex.extract_features(frames[0], [tuple(b) for b in g["boxes"][sel]]), f)
    ex.cleanup()
    with pytest.raises(ValueError, match="osnet"):
        HipReIDExtractor(model_type="osnet")
