"""Stage 1's first 1x1 reduce inside the fused stem launch (kernels_gemm.hip, StemReduce) and the stage-2 tails' LDS-DMA residual, as
switches of the whole forward.

Kernel level: the stem launch that also writes z0 = relu(w0 . pooled + b0) against the same launch without it followed by the implicit-GEMM
launch on the pooled map -- the pooled map and z0 must agree BIT FOR BIT (the in-kernel GEMM runs conv_gemm_dma_kernel's arithmetic for
this K = 64 layer: accumulators from the bias, k-block 0 before k-block 1, ReLU, one rounding), for uint8 frames and for the fp16 image,
for both element types.

End to end: OPD_STEM_REDUCE and OPD_RES_DMA128 are speed choices only -- raw logits, boxes and the encoder map are bit-identical over the
four settings, eager, captured and replayed, on the created handle and on its clone (the second handle of a streams = 2 detector)."""

import ctypes as C
import os

import numpy as np
import pytest

from office_person_detection_vit_amd import HipDetrDetector, _capi
from office_person_detection_vit_amd.frames import structured_frames
from office_person_detection_vit_amd.weights import DetrArch, ensure_weight_file

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mild_path(weight_cache):
    return ensure_weight_file(weight_cache, DetrArch(), 0, 1.0, "r50")


@pytest.fixture(scope="module")
def lib():
    return _capi.load_library(test_hooks=True)


@pytest.fixture(params=["fp16", "bf16"])
def elem(request, lib):
    lib.opd_test_set_elem_bf16(int(request.param == "bf16"))
    yield request.param
    lib.opd_test_set_elem_bf16(0)


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _bits(a, elem):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16 if elem == "bf16" else torch.float16)
    return np.ascontiguousarray(t.view(torch.int16).numpy().view(np.uint16))


STEM_CASES = [
    # B, H, W, valid_hw
    (2, 37, 53, None),                     # pooled 10 x 14: a single partial tile in x, five tile rows
    (1, 64, 200, None),                    # pooled 16 x 50: four x-tiles per workgroup -> the pipelined GEMM and its flush, last tile partial
    (2, 61, 83, [[61, 83], [40, 57]]),     # ragged batch: the second frame fills part of the canvas
]


@pytest.mark.parametrize("u8", [1, 0], ids=["uint8_frames", "fp16_image"])
@pytest.mark.parametrize("B,H,W,valid", STEM_CASES)
def test_stem_with_first_reduce_inside_is_bit_identical(lib, elem, B, H, W, valid, u8):
    rng = np.random.default_rng(B * 1000 + H + W)
    frames = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    w = np.zeros((64, 8, 8, 4), np.float32)                                     # [n][kh][kw][c], eighth row / column and fourth channel zero
    w[:, :7, :7, :3] = rng.standard_normal((64, 7, 7, 3)) / np.sqrt(147.0)
    bias = (rng.standard_normal(64) * 0.2).astype(np.float32)
    w0 = rng.standard_normal((64, 64)) * np.sqrt(2.0 / 64)                      # asymmetric: a transposed or permuted operand shows
    b0 = (rng.standard_normal(64) * 0.3).astype(np.float32)
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    PH, PW = (OH - 1) // 2 + 1, (OW - 1) // 2 + 1
    outs = [np.empty((B, PH, PW, 64), np.uint16) for _ in range(4)]
    vhw = np.ascontiguousarray(valid, np.int32) if valid is not None else None
    rc = lib.opd_test_stem_reduce(_p(frames), _p(vhw), _p(_bits(w.reshape(64, 256), elem)), _p(bias), _p(_bits(w0, elem)), _p(b0),
                                  *[_p(o) for o in outs], B, H, W, u8)
    _capi.check(rc, "opd_test_stem_reduce")
    pool_f, z_f, pool_r, z_r = outs
    np.testing.assert_array_equal(pool_f, pool_r)
    np.testing.assert_array_equal(z_f, z_r)
    # the reference is a real layer: some channels pass the ReLU, some do not, and it depends on the pixel
    nz = (z_r & 0x7FFF) != 0
    assert 0.2 < nz.mean() < 0.8 and nz.reshape(-1, 64).any(0).sum() > 32


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_stem_reduce_and_lds_dma_residual_are_invisible_end_to_end(mild_path, dtype):
    H, W, B = 256, 320, 2
    frames = structured_frames(B, H, W, seed=128)
    names = ("OPD_RES_DMA128", "OPD_STEM_REDUCE")
    outs = {}
    for setting in (("1", "1"), ("0", "1"), ("1", "0"), ("0", "0")):
        for k, v in zip(names, setting):
            os.environ[k] = v
        try:
            det = HipDetrDetector(model_path=mild_path, max_batch=B, max_size=(H, W), resize=False, streams=2, dtype=dtype)
            det.load_model()
        finally:
            for k in names:
                del os.environ[k]
        try:
            calls = [det.forward_raw(frames) for _ in range(3)]   # eager, capture, replay
            det.model = det._handles[1]                           # the same through the clone (opd_detr_clone copies the switches)
            calls += [det.forward_raw(frames) for _ in range(3)]
            outs[setting] = calls
        finally:
            det.close()
    ref = outs[("0", "0")][0]
    assert any(np.abs(np.asarray(x, np.float32)).max() > 0 for x in ref)
    for setting, calls in outs.items():
        for call in calls:
            for x, y in zip(call, ref):
                np.testing.assert_array_equal(x, y)
