"""Launch options of the GEMM kernels that the model's forward turns on and the basic kernel tests leave off (GPU): the L2 warm-up of the
weights (wprefetch), split-K on a convolution with taps + reduce_act16, the second activation source of the fused q | k | v projection
(x_alt), per-frame periodic bias tables (bias_ptrs) and per-frame position tables (pos_ptrs).  Each option runs through its own hook of
csrc/opd_test_api.cpp against a plain reference of the same operation on the same fp16-rounded operands.

Every bound here is bit equality or one that tests/test_kernels_gpu.py already uses for the same kernel:
  fp16 output of the implicit GEMM     atol 1.5e-3 * max|want|, rtol 1e-3   (test_conv_gemm_matches_torch)
  fp32 output with a row-periodic bias atol 2e-4, rtol 1e-5                 (test_gemm_rowbias_f32_residual)
  reduce + LayerNorm / gemm_ln, fp32 y atol 3e-5, rtol 1e-5                 (test_gemm_splitk_reduce_ln, test_gemm_ln_deep_matches_torch)
  enc_ffn, fp32 y                      atol 2e-4, rtol 1e-5                 (test_enc_ffn_matches_torch)
"""

import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from office_person_detection_vit_amd import _capi

pytestmark = pytest.mark.gpu

WPREFETCH = 0x2000   # bit 13 of opd_test_set_conv_flags: ConvGemmParams::wprefetch


@pytest.fixture(scope="module")
def lib():
    return _capi.load_library()


@pytest.fixture(autouse=True)
def _options_off_afterwards(lib):
    yield
    lib.opd_test_set_conv_flags(0)
    lib.opd_test_set_encffn_wprefetch(0)
    lib.opd_test_set_pos_frames(0)


# the tile-height params of test_kernels_gpu.py's gemm_variant, each also with the weight warm-up on as in the model
TILE_FLAGS = [0, 0x400, 0x500, 0x600, WPREFETCH | 0x500]
TILE_IDS = ["auto_tiles", "128rows", "160rows", "192rows", "160rows_wprefetch"]


@pytest.fixture(params=TILE_FLAGS, ids=TILE_IDS)
def tile_variant(request, lib):
    lib.opd_test_set_conv_flags(request.param)
    return request.param


def _h(a):
    """fp32 array -> (fp16-rounded fp32 array, uint16 bit pattern)."""
    h = np.ascontiguousarray(a, dtype=np.float32).astype(np.float16)
    return h.astype(np.float32), np.ascontiguousarray(h.view(np.uint16))


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _f16(bits):
    return bits.view(np.float16).astype(np.float32)


def ref_conv(x_nhwc, w_oihw, bias, stride, pad, relu):
    y = F.conv2d(torch.from_numpy(x_nhwc).permute(0, 3, 1, 2), torch.from_numpy(w_oihw), torch.from_numpy(bias), stride=stride,
                 padding=pad).permute(0, 2, 3, 1)
    return (F.relu(y) if relu else y).numpy()


def _conv_operands(x_nhwc, w_oihw):
    N, Cin, KH, KW = w_oihw.shape
    xb = np.ascontiguousarray(x_nhwc.astype(np.float16).view(np.uint16))
    wb = np.ascontiguousarray(w_oihw.transpose(0, 2, 3, 1).reshape(N, KH * KW * Cin).astype(np.float16).view(np.uint16))
    return xb, wb


def _geom(x_nhwc, w_oihw, stride):
    B, H, W, Cin = x_nhwc.shape
    N, _, KH, KW = w_oihw.shape
    pad = KH // 2
    return B, H, W, Cin, (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1, N, KH, KW, stride, pad


def run_conv_bits(lib, x_nhwc, w_oihw, bias, stride, relu):
    """The unsplit implicit GEMM (opd_test_conv_gemm): fp16 bit patterns [M][N]."""
    g = _geom(x_nhwc, w_oihw, stride)
    xb, wb = _conv_operands(x_nhwc, w_oihw)
    out = np.full((g[0] * g[4] * g[5], g[6]), 0xFFFF, np.uint16)
    _capi.check(lib.opd_test_conv_gemm(_p(xb), _p(wb), _p(bias), None, None, _p(out), *g, int(relu), 0, 0, 0), "opd_test_conv_gemm")
    return out


def run_conv_splitk_bits(lib, x_nhwc, w_oihw, bias, stride, relu, splits, out=None):
    g = _geom(x_nhwc, w_oihw, stride)
    xb, wb = _conv_operands(x_nhwc, w_oihw)
    if out is None:
        out = np.full((g[0] * g[4] * g[5], g[6]), 0xFFFF, np.uint16)
    rc = lib.opd_test_conv_splitk(_p(xb), _p(wb), _p(bias), _p(out), *g, int(relu), splits)
    return rc, out


# ---- 1. wprefetch: the warm-up requests land in the second stage buffer (conv_gemm_dma_kernel) / the hidden-chunk buffer (enc_ffn_kernel)
# before those are first used; results must not change by a bit, and must not change from launch to launch -------------------------------
@pytest.mark.parametrize("B,H,W,Cin,N,k", [(1, 25, 42, 2048, 512, 1), (2, 13, 17, 256, 256, 3)], ids=["1x1", "3x3"])
def test_wprefetch_conv_is_bit_identical_and_reproducible(lib, B, H, W, Cin, N, k):
    rng = np.random.default_rng(B * 1000 + Cin + k)
    x, _ = _h(rng.standard_normal((B, H, W, Cin)))
    w, _ = _h(rng.standard_normal((N, Cin, k, k)) * np.sqrt(2.0 / (Cin * k * k)))
    bias = (rng.standard_normal(N) * 0.1).astype(np.float32)
    lib.opd_test_set_conv_flags(0)
    off = run_conv_bits(lib, x, w, bias, 1, True)
    assert np.isfinite(_f16(off)).all() and np.count_nonzero(off) > off.size // 4
    lib.opd_test_set_conv_flags(WPREFETCH)
    for rep in range(10):
        on = run_conv_bits(lib, x, w, bias, 1, True)
        assert np.array_equal(on, off), f"launch {rep} with wprefetch: {np.count_nonzero(on != off)} elements differ from the launch without"


def test_wprefetch_dual_source_is_bit_identical_and_reproducible(lib):
    B, H, W, Cin, N, Cin2, stride2 = 2, 13, 11, 256, 1024, 512, 2
    rng = np.random.default_rng(21)
    H2, W2 = (H - 1) * stride2 + 1 + (stride2 - 1), (W - 1) * stride2 + 1
    _, xb = _h(np.abs(rng.standard_normal((B, H, W, Cin))))
    _, x2b = _h(np.abs(rng.standard_normal((B, H2, W2, Cin2))))
    _, w1b = _h(rng.standard_normal((N, Cin)) / np.sqrt(Cin))
    _, w2b = _h(rng.standard_normal((N, Cin2)) / np.sqrt(Cin2))
    bias = (0.1 * rng.standard_normal(N)).astype(np.float32)

    def run():
        out = np.full((B * H * W, N), 0xFFFF, np.uint16)
        _capi.check(lib.opd_test_conv_dual(_p(xb), _p(w1b), _p(x2b), _p(w2b), _p(bias), _p(out), B, H, W, Cin, 1, 1, 0, N, H2, W2, Cin2, stride2, 1),
                    "opd_test_conv_dual")
        return out

    lib.opd_test_set_conv_flags(0)
    off = run()
    assert np.isfinite(_f16(off)).all() and np.count_nonzero(off) > off.size // 4
    lib.opd_test_set_conv_flags(WPREFETCH)
    for rep in range(10):
        on = run()
        assert np.array_equal(on, off), f"launch {rep} with wprefetch: {np.count_nonzero(on != off)} elements differ from the launch without"


def _enc_ffn_operands(M, FF, period, frames, seed):
    rng = np.random.default_rng(seed)
    f32 = lambda n, s=0.1: (rng.standard_normal(n) * s).astype(np.float32)
    d = {}
    d["x"], d["xb"] = _h(rng.standard_normal((M, 256)))
    d["wo"], d["wob"] = _h(rng.standard_normal((256, 256)) / 16.0)
    d["w1"], d["w1b"] = _h(rng.standard_normal((FF, 256)) / 16.0)
    d["w2"], d["w2b"] = _h(rng.standard_normal((256, FF)) / np.sqrt(FF))
    d["wt"], d["wtb"] = _h(rng.standard_normal((3 * 256, 256)) / 16.0)
    d["b1"], d["b2"], d["bo"], d["tb"] = f32(FF, 0.3), f32(256), f32(256), f32(3 * 256, 0.2)
    d["g1"], d["be1"], d["gamma"], d["beta"] = 1.0 + f32(256), f32(256), 1.0 + f32(256), f32(256)
    d["res"] = rng.standard_normal((M, 256)).astype(np.float32)
    d["pos"] = rng.standard_normal((max(frames, 1), period, 256)).astype(np.float32)   # one table per frame, all different
    return d


def _run_enc_ffn(lib, d, M, FF, period, front, tail):
    y = np.empty((M, 256), np.float32)
    y16 = np.empty((M, 256), np.uint16)
    yp16 = np.empty((M, 256), np.uint16)
    tout = np.zeros((M, 3 * 256), np.uint16)
    fr = (_p(d["wob"]), _p(d["bo"]), _p(d["g1"]), _p(d["be1"])) if front else (None, None, None, None)
    tl = (_p(d["wtb"]), _p(d["tb"]), 3, 2, _p(tout)) if tail else (None, None, 0, 0, None)
    _capi.check(lib.opd_test_enc_ffn(_p(d["xb"]), _p(d["w1b"]), _p(d["b1"]), _p(d["w2b"]), _p(d["b2"]), _p(d["res"]), _p(d["gamma"]), _p(d["beta"]),
                                     _p(d["pos"]), period, _p(y), _p(y16), _p(yp16), M, FF, 1, *tl, *fr, 1), "opd_test_enc_ffn")
    return y, y16, yp16, tout


@pytest.mark.parametrize("front", [False, True], ids=["ffn_only", "front_phase"])
@pytest.mark.parametrize("M,FF,period", [(333, 256, 111), (130, 1024, 13)])
def test_wprefetch_enc_ffn_is_bit_identical(lib, M, FF, period, front):
    """enc_ffn_kernel with its tail projection (and its front phase): the warm-up's 512 bytes per wave land in the hidden-chunk buffer."""
    d = _enc_ffn_operands(M, FF, period, 0, M + FF + front)
    lib.opd_test_set_encffn_wprefetch(0)
    off = _run_enc_ffn(lib, d, M, FF, period, front, True)
    assert np.isfinite(off[0]).all() and np.abs(off[0]).max() > 0.5
    lib.opd_test_set_encffn_wprefetch(1)
    for rep in range(3):
        on = _run_enc_ffn(lib, d, M, FF, period, front, True)
        for name, a, b in zip(("y", "y16", "yp16", "tail_out"), on, off):
            assert a.tobytes() == b.tobytes(), f"launch {rep} with wprefetch: {name} differs from the launch without"


# ---- 2. split-K convolution + reduce_act16 (run_conv on max_batch = 1 handles) --------------------------------------------------------------
SPLITK_CASES = [
    # B, H, W, Cin, N, k, stride, splits
    (1, 7, 9, 512, 512, 3, 1, 8),      # 9 k-steps per slice against 8 per tap: every slice but the first starts in the middle of a tap; one ragged tile
    (2, 13, 17, 256, 256, 3, 1, 6),    # the model's stage-3 split; image borders inside a tile
    (1, 14, 15, 256, 256, 3, 2, 4),    # stride 2
    (1, 25, 42, 2048, 512, 1, 1, 4),   # pointwise
    (2, 25, 42, 512, 512, 3, 1, 8),    # tiles * splits >= 384: the 128-column instantiation
]


@functools.lru_cache(maxsize=None)
def _splitk_random(case):
    B, H, W, Cin, N, k, stride, _ = case
    rng = np.random.default_rng(sum(case) + 17 * Cin)
    x, _ = _h(rng.standard_normal((B, H, W, Cin)))
    w, _ = _h(rng.standard_normal((N, Cin, k, k)) * np.sqrt(2.0 / (Cin * k * k)))
    bias = (rng.standard_normal(N) * 0.1).astype(np.float32)
    return x, w, bias, ref_conv(x, w, bias, stride, k // 2, False)


@functools.lru_cache(maxsize=None)
def _splitk_integer(case):
    """x in [-3, 3]; per output channel two integer weights at different taps and channels (asymmetric, as test_conv_gemm_integer_exact); integer
    bias: every partial sum of every slice is a small integer, exact in fp32 whatever the order."""
    B, H, W, Cin, N, k, stride, _ = case
    rng = np.random.default_rng(5 + sum(case))
    x = rng.integers(-3, 4, (B, H, W, Cin)).astype(np.float32)
    w = np.zeros((N, Cin, k, k), np.float32)
    for n in range(N):
        w[n, (n * 7) % Cin, n % k, (n // 3) % k] = 1 + (n % 5)
        w[n, (n * 3 + 1) % Cin, (n + 1) % k, n % k] += -2
    bias = (np.arange(N, dtype=np.float32) % 121) - 60
    worst = 3.0 * np.abs(w).reshape(N, -1).sum(1).max() + np.abs(bias).max()   # the largest possible |partial sum|
    assert worst < 2 ** 24, worst
    return x, w, bias, ref_conv(x, w, bias, stride, k // 2, False)


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "linear"])
@pytest.mark.parametrize("case", SPLITK_CASES)
def test_conv_splitk_matches_torch(lib, case, relu):
    stride, splits = case[6], case[7]
    x, w, bias, pre = _splitk_random(case)
    want = np.maximum(pre, 0) if relu else pre
    lib.opd_test_set_conv_flags(WPREFETCH)   # as the model launches it
    rc, out = run_conv_splitk_bits(lib, x, w, bias, stride, relu, splits)
    _capi.check(rc, "opd_test_conv_splitk")
    got = _f16(out).reshape(want.shape)
    scale = float(np.abs(want).max())
    print(f"splitk {case} relu={relu}: max |got - want| = {np.abs(got - want).max():.3e}, scale {scale:.3f}")
    np.testing.assert_allclose(got, want, atol=1.5e-3 * scale, rtol=1e-3)


@pytest.mark.parametrize("flags", [0, WPREFETCH, 0x500, 0x600, 0x20], ids=["auto_tiles", "wprefetch", "160rows", "192rows", "flat_staging"])
@pytest.mark.parametrize("relu", [True, False], ids=["relu", "linear"])
@pytest.mark.parametrize("case", SPLITK_CASES)
def test_conv_splitk_integer_exact_and_equals_unsplit(lib, case, relu, flags):
    stride, splits = case[6], case[7]
    x, w, bias, pre = _splitk_integer(case)
    want = (np.maximum(pre, 0) if relu else pre).astype(np.float16)   # float16(exact sum)
    lib.opd_test_set_conv_flags(flags)
    rc, out = run_conv_splitk_bits(lib, x, w, bias, stride, relu, splits)
    _capi.check(rc, "opd_test_conv_splitk")
    got = out.view(np.float16).reshape(want.shape)
    assert np.array_equal(got, want), f"{np.count_nonzero(got != want)} of {want.size} elements differ from the exact sum"
    unsplit = run_conv_bits(lib, x, w, bias, stride, relu)
    assert np.array_equal(out, unsplit), "split-K + reduce_act16 differs from the unsplit launch"


def test_conv_splitk_refuses_a_split_that_does_not_divide_the_k_steps(lib):
    case = (1, 7, 9, 512, 512, 3, 1, 5)   # 72 k-steps, 5 slices
    x, w, bias, _ = _splitk_integer(case)
    out = np.full((7 * 9, 512), 0xABCD, np.uint16)
    rc, out = run_conv_splitk_bits(lib, x, w, bias, 1, True, 5, out)
    assert rc != 0 and "opd_launch_conv_gemm" in _capi.last_error()
    assert (out == 0xABCD).all()   # refused by the launcher's host check: nothing ran, nothing was copied back


@pytest.mark.parametrize("relu", [1, 0], ids=["relu", "linear"])
@pytest.mark.parametrize("pad", [0, 64], ids=["dense", "padded_slabs"])
@pytest.mark.parametrize("nsplit", [1, 3, 8])
def test_reduce_act16_is_the_slice_order_sum(lib, nsplit, pad, relu):
    n = 8 * (3 * 256 + 5)   # four blocks of 256 threads x 8 elements, the last one partial
    stride = n + pad
    rng = np.random.default_rng(nsplit * 10 + pad + relu)
    part = (rng.standard_normal((nsplit, stride)) * 4).astype(np.float32)
    part[0, 0:64] = -0.0                     # sums that are -0.0, exact zeros, and exact cancellations
    part[1:, 0:64] = -0.0
    part[0, 64:128] = 0.0
    if nsplit > 1:
        part[1, 128:192] = -part[0, 128:192]
        part[2:, 128:192] = 0.0
    assert (part < 0).any()
    flat = np.ascontiguousarray(part.reshape(-1)[:(nsplit - 1) * stride + n])
    out = np.full(n, 0xFFFF, np.uint16)
    _capi.check(lib.opd_test_reduce_act16(_p(flat), nsplit, stride, n, relu, _p(out)), "opd_test_reduce_act16")
    acc = part[0, :n].copy()
    for z in range(1, nsplit):
        acc = acc + part[z, :n]              # float32, slice order
    want = (np.maximum(acc, np.float32(0)) if relu else acc).astype(np.float16)
    got = out.view(np.float16)
    assert np.array_equal(got, want), f"{np.count_nonzero(got != want)} of {n} elements differ"


# ---- 3. x_alt: column groups of one pointwise launch read different activations (q / k columns: x + pos, v columns: x) ----------------------
ALT_CASES = [(300, 768, 256, 768, 512),      # 64-column tiles: the encoder's q | k | v
             (2100, 3072, 256, 512, 256)]    # 17 x 24 128-column tiles: the decoder's memory [k | v] x 6 layers


def _alt_want(x, xa, w, bias, alt_mod, alt_cols):
    N = w.shape[0]
    first = (np.arange(N) % alt_mod) < alt_cols
    a = x.astype(np.float64) @ w.astype(np.float64).T
    b = xa.astype(np.float64) @ w.astype(np.float64).T
    return np.where(first[None, :], a, b) + bias.astype(np.float64)


@functools.lru_cache(maxsize=None)
def _alt_data(case, integer):
    M, N, K, alt_mod, alt_cols = case
    rng = np.random.default_rng(M + N + (7 if integer else 0))
    if integer:
        x = rng.integers(-3, 4, (M, K)).astype(np.float32)
        xa = x + rng.integers(1, 3, (M, K)).astype(np.float32)          # differs from x in EVERY element
        w = np.zeros((N, K), np.float32)
        for n in range(N):
            w[n, (n * 37 + 5) % K] = 1 + (n % 3)
            w[n, (n * 11 + 2) % K] -= 2
        bias = ((np.arange(N) % 13) - 6).astype(np.float32)
    else:
        x, _ = _h(rng.standard_normal((M, K)))
        xa, _ = _h(x + np.where(rng.random((M, K)) < 0.5, -1.0, 1.0) * rng.uniform(0.25, 1.0, (M, K)))
        w, _ = _h(rng.standard_normal((N, K)) / np.sqrt(K))
        bias = (rng.standard_normal(N) * 0.1).astype(np.float32)
    assert (x != xa).all()
    return x, xa, w, bias, _alt_want(x, xa, w, bias, alt_mod, alt_cols)


def _run_alt(lib, x, xa, w, bias, N, alt_mod, alt_cols):
    M, K = x.shape
    out = np.full((M, N), 0xFFFF, np.uint16)
    rc = lib.opd_test_gemm_alt(_p(_h(x)[1]), _p(_h(xa)[1]), _p(_h(w)[1]), _p(bias), _p(out), M, N, K, alt_mod, alt_cols)
    return rc, out


@pytest.mark.parametrize("case", ALT_CASES)
def test_gemm_alt_source_matches_reference(lib, tile_variant, case):
    M, N, K, alt_mod, alt_cols = case
    x, xa, w, bias, want = _alt_data(case, False)
    rc, out = _run_alt(lib, x, xa, w, bias, N, alt_mod, alt_cols)
    _capi.check(rc, "opd_test_gemm_alt")
    got = _f16(out)
    scale = float(np.abs(want).max())
    print(f"gemm_alt {case}: max |got - want| = {np.abs(got - want).max():.3e}, scale {scale:.3f}")
    np.testing.assert_allclose(got, want, atol=1.5e-3 * scale, rtol=1e-3)


@pytest.mark.parametrize("case", ALT_CASES)
def test_gemm_alt_source_integer_exact(lib, tile_variant, case):
    M, N, K, alt_mod, alt_cols = case
    x, xa, w, bias, want = _alt_data(case, True)
    assert np.abs(want).max() < 2048
    rc, out = _run_alt(lib, x, xa, w, bias, N, alt_mod, alt_cols)
    _capi.check(rc, "opd_test_gemm_alt")
    got = out.view(np.float16)
    assert np.array_equal(got, want.astype(np.float16)), f"{np.count_nonzero(got != want.astype(np.float16))} elements differ"


@pytest.mark.parametrize("flags,alt_mod,alt_cols", [(0x20, 768, 512), (0, 96, 64)], ids=["flat_staging", "alt_mod_96"])
def test_gemm_alt_source_refused_where_unsupported(lib, flags, alt_mod, alt_cols):
    """The flat-address staging path does not implement x_alt, and a column group must be whole tiles: the launcher refuses both."""
    x, xa, w, bias, _ = _alt_data(ALT_CASES[0], True)
    lib.opd_test_set_conv_flags(flags)
    rc, out = _run_alt(lib, x, xa, w, bias, 768, alt_mod, alt_cols)
    assert rc != 0 and "opd_launch_conv_gemm" in _capi.last_error()
    assert (out == 0xFFFF).all()


# ---- 4. bias_ptrs: one row-periodic bias table per frame (ragged batches), chosen per ROW, so a tile may straddle two frames ------------------
FRAME_BIAS_CASES = [(3, 100, 768, 768, 512), (2, 1050, 3072, 512, 256), (3, 100, 256, 0, 0)]   # frames, period, N, pmod, pcols


@functools.lru_cache(maxsize=None)
def _frame_bias_data(case, integer):
    B, period, N, pmod, pcols = case
    M, K = B * period, 256
    rng = np.random.default_rng(B * period + N + (3 if integer else 0))
    varying = ((np.arange(N) % pmod) < pcols) if pcols else np.ones(N, bool)
    nvar = B * period * int(varying.sum())
    if integer:
        x = rng.integers(-3, 4, (M, K)).astype(np.float32)
        w = np.zeros((N, K), np.float32)
        for n in range(N):
            w[n, (n * 37 + 5) % K] = 1 + (n % 3)
            w[n, (n * 11 + 2) % K] -= 2
        # distinct multiples of 2^-s in (-1024, 1024): with |x . w| <= 15 every sum is exact in fp32
        s = max(0, int(np.ceil(np.log2(nvar / 2048.0))))
        vals = ((rng.permutation(nvar) - nvar // 2) * 2.0 ** -s).astype(np.float32)
        const = ((np.arange(N) % 17) - 8).astype(np.float32)
        assert s <= 12 and np.abs(vals).max() <= 1024
    else:
        x, _ = _h(rng.standard_normal((M, K)))
        w, _ = _h(rng.standard_normal((N, K)) / np.sqrt(K))
        vals = rng.permutation(np.linspace(-2.0, 2.0, nvar)).astype(np.float32)   # distinct: the spacing is above one fp32 ulp at 2
        const = rng.standard_normal(N).astype(np.float32)
    tables = np.empty((B, period, N), np.float32)
    tables[:] = const
    tables[:, :, varying] = vals.reshape(B, period, -1)
    # the kernel's contract: outside the varying columns every row of every table is the same; inside, every entry is its own
    assert (tables[:, :, ~varying] == tables[0, 0, ~varying]).all()
    assert np.unique(tables[:, :, varying]).size == nvar
    want = x.astype(np.float64) @ w.astype(np.float64).T + tables.reshape(M, N).astype(np.float64)
    return x, w, tables, want


def _run_frame_bias(lib, x, w, tables, case, out_f32):
    B, period, N, pmod, pcols = case
    M, K = x.shape
    out = np.full((M, N), np.nan, np.float32) if out_f32 else np.full((M, N), 0xFFFF, np.uint16)
    _capi.check(lib.opd_test_gemm_frame_bias(_p(_h(x)[1]), _p(_h(w)[1]), _p(tables), _p(out), M, N, K, period, pmod, pcols, int(out_f32)),
                "opd_test_gemm_frame_bias")
    return out


@pytest.mark.parametrize("out_f32", [False, True], ids=["f16_out", "f32_out"])
@pytest.mark.parametrize("case", FRAME_BIAS_CASES)
def test_gemm_frame_bias_matches_reference(lib, tile_variant, case, out_f32):
    x, w, tables, want = _frame_bias_data(case, False)
    out = _run_frame_bias(lib, x, w, tables, case, out_f32)
    got = out if out_f32 else _f16(out)
    scale = float(np.abs(want).max())
    print(f"frame_bias {case} f32={out_f32}: max |got - want| = {np.abs(got - want).max():.3e}, scale {scale:.3f}")
    if out_f32:
        np.testing.assert_allclose(got, want, atol=2e-4, rtol=1e-5)
    else:
        np.testing.assert_allclose(got, want, atol=1.5e-3 * scale, rtol=1e-3)


@pytest.mark.parametrize("out_f32", [False, True], ids=["f16_out", "f32_out"])
@pytest.mark.parametrize("case", FRAME_BIAS_CASES)
def test_gemm_frame_bias_integer_exact(lib, tile_variant, case, out_f32):
    x, w, tables, want = _frame_bias_data(case, True)
    out = _run_frame_bias(lib, x, w, tables, case, out_f32)
    if out_f32:
        assert np.array_equal(out, want.astype(np.float32)), f"{np.count_nonzero(out != want.astype(np.float32))} elements differ"
    else:
        w16 = want.astype(np.float32).astype(np.float16)   # (exact in fp32, then the kernel's one rounding)
        assert np.array_equal(out.view(np.float16), w16), f"{np.count_nonzero(out.view(np.float16) != w16)} elements differ"


# ---- 5. pos_ptrs: per-frame position tables for the shadow output yp16 = fp16(y + pos[frame][row % period]) -----------------------------------
POS_B, POS_PERIOD = 3, 111      # 333 rows: neither the 4 rows of a reduce block nor the row slabs of the GEMM kernels divide the period
POS_M = POS_B * POS_PERIOD


def _pos_rows(tables, frames):
    """Row m's position-table row: table[m // period] (per frame) or the single table 0 (frames == 0)."""
    m = np.arange(POS_M)
    return tables[m // POS_PERIOD if frames else 0, m % POS_PERIOD]


@pytest.mark.parametrize("frames", [POS_B, 0], ids=["per_frame", "one_table"])
@pytest.mark.parametrize("ln", [True, False], ids=["layernorm", "plain_sum"])
def test_reduce_ln_pos_tables(lib, ln, frames):
    nsplit = 4
    rng = np.random.default_rng(40 + ln)
    part = rng.standard_normal((nsplit, POS_M, 256)).astype(np.float32)
    res = rng.standard_normal((POS_M, 256)).astype(np.float32)
    gamma = (1.0 + 0.1 * rng.standard_normal(256)).astype(np.float32)
    beta = (0.1 * rng.standard_normal(256)).astype(np.float32)
    tables = rng.standard_normal((POS_B, POS_PERIOD, 256)).astype(np.float32)
    y = np.empty((POS_M, 256), np.float32)
    y16 = np.empty((POS_M, 256), np.uint16)
    yp16 = np.empty((POS_M, 256), np.uint16)
    _capi.check(lib.opd_test_reduce_ln_pos(_p(part), nsplit, _p(res), _p(gamma) if ln else None, _p(beta) if ln else None,
                                           None if frames else _p(tables), _p(tables) if frames else None, frames, POS_PERIOD,
                                           _p(y), _p(y16), _p(yp16), POS_M), "opd_test_reduce_ln_pos")
    acc = part[0].copy()
    for z in range(1, nsplit):
        acc = acc + part[z]          # float32, slice order
    acc = acc + res
    if ln:
        T = lambda a: torch.from_numpy(a).double()
        want = F.layer_norm(T(part).sum(0) + T(res), (256,), T(gamma), T(beta), 1e-5).float().numpy()
        np.testing.assert_allclose(y, want, atol=3e-5, rtol=1e-5)
    else:
        assert np.array_equal(y, acc)
    assert np.array_equal(y16.view(np.float16), y.astype(np.float16))
    assert np.array_equal(yp16.view(np.float16), (y + _pos_rows(tables, frames)).astype(np.float16))


@pytest.mark.parametrize("frames", [POS_B, 0], ids=["per_frame", "one_table"])
def test_gemm_ln_deep_pos_tables(lib, frames):
    M, K = POS_M, 128
    rng = np.random.default_rng(M * 3 + K)
    x, xb = _h(rng.standard_normal((M, K)))
    w, wb = _h(rng.standard_normal((256, K)) / np.sqrt(K))
    bias = rng.standard_normal(256).astype(np.float32) * 0.1
    res = rng.standard_normal((M, 256)).astype(np.float32)
    gamma = (1.0 + 0.1 * rng.standard_normal(256)).astype(np.float32)
    beta = (0.1 * rng.standard_normal(256)).astype(np.float32)
    tables = rng.standard_normal((POS_B, POS_PERIOD, 256)).astype(np.float32)
    y = np.empty((M, 256), np.float32)
    y16 = np.empty((M, 256), np.uint16)
    yp16 = np.empty((M, 256), np.uint16)
    lib.opd_test_set_pos_frames(frames)
    _capi.check(lib.opd_test_gemm_ln_deep(_p(xb), _p(wb), _p(bias), _p(res), _p(gamma), _p(beta), _p(tables), POS_PERIOD, _p(y), _p(y16), _p(yp16),
                                          M, K, 1), "opd_test_gemm_ln_deep")
    T = lambda a: torch.from_numpy(a).double()
    want = F.layer_norm(T(x) @ T(w).T + T(bias) + T(res), (256,), T(gamma), T(beta), 1e-5).float().numpy()
    np.testing.assert_allclose(y, want, atol=3e-5, rtol=1e-5)
    assert np.array_equal(yp16.view(np.float16), (y + _pos_rows(tables, frames)).astype(np.float16))


@pytest.mark.parametrize("frames", [POS_B, 0], ids=["per_frame", "one_table"])
def test_enc_ffn_pos_tables(lib, frames):
    """yp16 from the per-frame tables, and the tail passes that multiply y + pos (they read the same shadow)."""
    M, FF = POS_M, 256
    d = _enc_ffn_operands(M, FF, POS_PERIOD, POS_B, 99)
    tables = d["pos"]
    lib.opd_test_set_pos_frames(frames)
    lib.opd_test_set_encffn_wprefetch(1)   # as the model launches it
    y, y16, yp16, tout = _run_enc_ffn(lib, d, M, FF, POS_PERIOD, False, True)
    T = lambda a: torch.from_numpy(a).double()
    hid = torch.relu(T(d["x"]) @ T(d["w1"]).T + T(d["b1"])).float().half().double()
    want = F.layer_norm(hid @ T(d["w2"]).T + T(d["b2"]) + T(d["res"]), (256,), T(d["gamma"]), T(d["beta"]), 1e-5).float().numpy()
    np.testing.assert_allclose(y, want, atol=2e-4, rtol=1e-5)
    assert np.array_equal(yp16.view(np.float16), (y + _pos_rows(tables, frames)).astype(np.float16))
    # tail passes 0 and 1 on fp16(y + pos), pass 2 on fp16(y): the bound test_enc_ffn_matches_torch uses for them
    got = _f16(tout)
    for t in range(3):
        src = (yp16 if t < 2 else y16).view(np.float16).astype(np.float64)
        want_t = src @ d["wt"][256 * t:256 * t + 256].astype(np.float64).T + d["tb"][256 * t:256 * t + 256]
        np.testing.assert_allclose(got[:, 256 * t:256 * t + 256], want_t, atol=2e-3, rtol=1.2e-3)
