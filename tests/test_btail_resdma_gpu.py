"""The 128-channel bottleneck tails (stage 2) with the residual through LDS-DMA (kernels_btail.hip, one wave-private residual buffer) against
the register-load form of the same kernel (``BtailParams::dbg`` bit 16, ``opd_test_set_btail_res_regs``): the residual path moves bytes and
computes nothing, so y and z must agree BIT FOR BIT -- for both fused-reduce widths (C3 = 128 / 0), with and without a residual, for both
element types, on shapes whose last tile and last wave are ragged.  One shape is also checked exactly against torch on integer-valued
operands, and a repeat screen looks for a wait that is one count short (a rare wrong tile that comes and goes with timing)."""

import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from office_person_detection_vit_amd import _capi

pytestmark = pytest.mark.gpu

C1 = 128
C2 = 4 * C1
SHAPES = [(2, 9, 13),   # M = 234: two 128-pixel tiles, the last wave of the second one partly valid
          (1, 5, 7)]    # M = 35: less than one tile, one wave full, one partly valid, two empty


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
    """fp32 array -> uint16 bit patterns of the element type (round to nearest even)."""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16 if elem == "bf16" else torch.float16)
    return np.ascontiguousarray(t.view(torch.int16).numpy().view(np.uint16))


def _operands(rng, B, H, W, C3, use_res, elem):
    M = B * H * W
    ops = dict(
        x1=_bits(np.abs(rng.standard_normal((B, H, W, C1))), elem),
        w1=_bits((rng.standard_normal((C1, C1, 3, 3)) * np.sqrt(2.0 / (9 * C1))).transpose(0, 2, 3, 1).reshape(C1, 9 * C1), elem),
        b1=(rng.standard_normal(C1) * 0.1).astype(np.float32),
        w2=_bits(rng.standard_normal((C2, C1)) * np.sqrt(2.0 / C1), elem),
        b2=(rng.standard_normal(C2) * 0.1).astype(np.float32),
        res=_bits(rng.standard_normal((M, C2)), elem) if use_res else None,
        w3=_bits(rng.standard_normal((C3, C2)) * np.sqrt(2.0 / C2), elem) if C3 else None,
        b3=(rng.standard_normal(C3) * 0.1).astype(np.float32) if C3 else None)
    return ops


def _run(lib, ops, B, H, W, C3, res_regs):
    M = B * H * W
    y = np.full((M, C2), 0xFFFF, np.uint16)
    z = np.full((M, max(C3, 1)), 0xFFFF, np.uint16)
    lib.opd_test_set_btail_res_regs(int(res_regs))
    try:
        rc = lib.opd_test_btail(_p(ops["x1"]), _p(ops["w1"]), _p(ops["b1"]), _p(ops["w2"]), _p(ops["b2"]), _p(ops["res"]), _p(ops["w3"]), _p(ops["b3"]),
                                _p(y), _p(z), B, H, W, C1, C3, 1)
    finally:
        lib.opd_test_set_btail_res_regs(0)
    _capi.check(rc, "opd_test_btail")
    return y, (z if C3 else None)


@pytest.mark.parametrize("use_res", [True, False], ids=["residual", "no_residual"])
@pytest.mark.parametrize("C3", [128, 0])
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_lds_dma_residual_equals_register_residual_bit_for_bit(lib, elem, B, H, W, C3, use_res):
    rng = np.random.default_rng(1000 * B + 10 * H + W + C3 + int(use_res))
    ops = _operands(rng, B, H, W, C3, use_res, elem)
    y_dma, z_dma = _run(lib, ops, B, H, W, C3, res_regs=False)
    y_reg, z_reg = _run(lib, ops, B, H, W, C3, res_regs=True)
    assert not (y_reg == 0xFFFF).all()   # (the hook's outputs were written)
    np.testing.assert_array_equal(y_dma, y_reg)
    if C3:
        np.testing.assert_array_equal(z_dma, z_reg)
    if use_res:   # the residual is really part of the result: without it y differs
        y_none, _ = _run(lib, dict(ops, res=None), B, H, W, C3, res_regs=False)
        assert (y_none != y_dma).any()


@pytest.mark.parametrize("C3", [128, 0])
def test_lds_dma_residual_integer_exact_against_torch(lib, C3):
    """Small-integer operands: the three GEMMs and the residual add are exact in fp16 and fp32, so y and z must equal the torch reference
    bit for bit; the residual differs in every pixel and channel, so a row, chunk or 16-byte slot read from the wrong place shows."""
    B, H, W = SHAPES[0]
    M = B * H * W
    rng = np.random.default_rng(C3 + 5)
    x1 = rng.integers(0, 3, (B, H, W, C1)).astype(np.float32)
    w1 = np.zeros((C1, C1, 3, 3), np.float32)
    for n in range(C1):
        w1[n, (n * 7 + 3) % C1, n % 3, (n // 3) % 3] = 1 + (n % 3)
        w1[n, (n * 5 + 1) % C1, (n + 1) % 3, (n // 2) % 3] = -1
    w2 = np.zeros((C2, C1), np.float32)
    for n in range(C2):
        w2[n, (n * 11 + 5) % C1] = 1 + (n % 2)
        w2[n, (n * 3 + 2) % C1] -= 1
    w3 = np.zeros((max(C3, 1), C2), np.float32)
    for n in range(C3):
        w3[n, (n * 13 + 7) % C2] = 1
        w3[n, (n * 29 + 1) % C2] += 1 + (n % 2)
        w3[n, (n * 17 + 4) % C2] -= 1
    b1 = rng.integers(-1, 2, C1).astype(np.float32)
    b2 = rng.integers(-1, 2, C2).astype(np.float32)
    b3 = rng.integers(-2, 3, max(C3, 1)).astype(np.float32)
    res = ((np.arange(M)[:, None] * 7 + np.arange(C2)[None, :] * 3) % 23 - 11).astype(np.float32)   # every (pixel, channel) its own value

    t = lambda a: torch.from_numpy(a)
    a1 = F.relu(F.conv2d(t(x1).permute(0, 3, 1, 2), t(w1), t(b1), padding=1))
    yr = F.relu(F.conv2d(a1, t(w2)[:, :, None, None], t(b2)) + t(res).reshape(B, H, W, C2).permute(0, 3, 1, 2))
    zr = F.relu(F.conv2d(yr, t(w3)[:, :, None, None], t(b3)))
    yr = yr.permute(0, 2, 3, 1).reshape(M, C2).numpy()
    zr = zr.permute(0, 2, 3, 1).reshape(M, -1).numpy()
    assert np.abs(yr).max() < 2048 and np.abs(zr).max() < 2048   # integers that fp16 holds exactly

    ops = dict(x1=_bits(x1, "fp16"), w1=_bits(w1.transpose(0, 2, 3, 1).reshape(C1, 9 * C1), "fp16"), b1=b1, w2=_bits(w2, "fp16"), b2=b2,
               res=_bits(res, "fp16"), w3=_bits(w3, "fp16") if C3 else None, b3=b3 if C3 else None)
    y, z = _run(lib, ops, B, H, W, C3, res_regs=False)
    np.testing.assert_array_equal(y.view(np.float16).astype(np.float32), yr)
    if C3:
        np.testing.assert_array_equal(z.view(np.float16).astype(np.float32), zr)


def test_lds_dma_residual_repeated_launches_are_bit_identical(lib):
    """Race screen: the residual pieces of chunk j+1 land in the buffer chunk j has just been read out of, and are read behind a counted
    wait with the next operands in flight.  12 launches on the same operands (alternating tile walk direction, a 256-MiB copy on a second
    stream per launch to vary the latencies): no launch may differ from the first."""
    B, H, W, C3 = 2, 17, 23, 128
    ops = _operands(np.random.default_rng(1723), B, H, W, C3, True, "fp16")
    n_diff = C.c_int(-1)
    rc = lib.opd_test_btail_repeat(_p(ops["x1"]), _p(ops["w1"]), _p(ops["b1"]), _p(ops["w2"]), _p(ops["b2"]), _p(ops["res"]), _p(ops["w3"]), _p(ops["b3"]),
                                   B, H, W, C1, C3, 12, C.byref(n_diff))
    _capi.check(rc, "opd_test_btail_repeat")
    assert n_diff.value == 0
