"""Kernel tests of the two Re-ID towers (-m gpu) at every shape their loaders accept: csrc/kernels_reid.hip (CLIP) and
csrc/kernels_osnet.hip (OSNet), called through the test hooks, against float64 references on the same fp16 operands.

Two kinds of assertion:
- integer-exact: small-integer fp16 operands and integer biases make every product and sum exact in fp32 and every output exact in
  fp16, so the kernel must equal the float64 reference bit for bit.  A wrong fragment map, a lost K step, a wrong bias row or a
  stray store shows as a visibly wrong value.
- derived bounds (reid_bounds.py): each bound is the sum of the fp16 output rounding, the fp32 accumulation error of the kernel's
  summation order and, for attention, the fp16 rounding of P, evaluated per element.  test_reid_bounds_cpu.py shows on the CPU that
  an fp32 restatement of each kernel meets its bound and that a one-line mistake in it breaks the bound.

Every launch also checks that the columns, channels and rows outside the range it writes keep their values.
"""

import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import reid_bounds as B
from office_person_detection_vit_amd import _capi

pytestmark = pytest.mark.gpu

SENTINEL = np.float16(-1234.0)   # fills what a launch must not write; no tested output takes this value


@pytest.fixture(scope="module")
def lib():
    return _capi.load_library(test_hooks=True)


def _ints(rng, lo, hi, shape, dtype=np.float16):
    return np.ascontiguousarray(rng.integers(lo, hi + 1, shape).astype(dtype))


def _p(a):
    return a.ctypes.data if a is not None else None


def _t64(a):
    return torch.from_numpy(np.asarray(a, np.float64))


# ==== CLIP: kernels_reid.hip ================================================================================================================
EPI_F16_BIAS, EPI_F32_RESID, EPI_F16_QGELU, EPI_F32_PBIAS = 0, 1, 2, 3


def _reid_gemm(lib, epi, X, W, bias, period, out):
    M, K = X.shape
    N = W.shape[0]
    assert W.shape[1] == K and out.shape == (M, N) and out.flags.c_contiguous
    if bias is not None:
        assert bias.shape == ((period, N) if epi == EPI_F32_PBIAS else (N,))
    _capi.check(lib.opd_test_reid_gemm(epi, _p(X), _p(W), _p(bias), period, _p(out), M, N, K), "opd_test_reid_gemm")
    return out


# (M, N, K): every M, N and K of the issue's lists, the forward's own shapes among them (qkv 3H x H, out-proj / fc2 H x H / H x F)
GEMM_SHAPES = [(1, 2304, 768), (17, 64, 3072), (63, 128, 64), (64, 768, 128), (65, 2304, 3072), (130, 768, 768), (50 * 160, 2304, 768)]
RESID_SHAPES = [(1, 768, 3072), (17, 768, 768), (63, 64, 128), (64, 128, 3072), (65, 2304, 64), (130, 768, 768), (50 * 160, 768, 3072)]


@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
def test_reid_gemm_f16_bias_integer_exact(lib, M, N, K):
    """The qkv epilogue (REID_EPI_F16_BIAS): fp32 accumulators + bias, one fp16 rounding; exact on integers."""
    rng = np.random.default_rng(M * 7 + N + K)
    X, W = _ints(rng, -2, 2, (M, K)), _ints(rng, -2, 2, (N, K))
    bias = _ints(rng, -8, 8, N, np.float32)
    out = _reid_gemm(lib, EPI_F16_BIAS, X, W, bias, 0, np.zeros((M, N), np.float16))
    want = (_t64(X) @ _t64(W).T + _t64(bias)).numpy()
    assert np.abs(want).max() < 2048   # every value an fp16 integer
    np.testing.assert_array_equal(out.astype(np.float64), want)


@pytest.mark.parametrize("M,N,K", RESID_SHAPES)
def test_reid_gemm_f32_resid_integer_exact(lib, M, N, K):
    """The residual epilogue (REID_EPI_F32_RESID): out += acc + bias in fp32; exact on integers."""
    rng = np.random.default_rng(M * 5 + N + K)
    X, W = _ints(rng, -2, 2, (M, K)), _ints(rng, -2, 2, (N, K))
    bias = _ints(rng, -8, 8, N, np.float32)
    res = _ints(rng, -1000, 1000, (M, N), np.float32)
    out = _reid_gemm(lib, EPI_F32_RESID, X, W, bias, 0, res.copy())
    np.testing.assert_array_equal(out.astype(np.float64), (_t64(X) @ _t64(W).T + _t64(bias) + _t64(res)).numpy())


# (M, N, K, period): the patch embedding at patch 32 / 56 / 224 (T = 50 / 17 / 2, K = 3 P P) with its per-token bias table, and the
# projection with no bias (period 0)
PBIAS_CASES = [(50, 768, 3072, 50), (50 * 160, 768, 3072, 50), (63, 128, 64, 50), (17, 256, 9408, 17), (17 * 7, 1024, 9408, 17),
               (65, 64, 128, 17), (2, 128, 150528, 2), (130, 64, 150528, 2), (64, 128, 768, 2),
               (1, 512, 768, 0), (17, 512, 1024, 0), (65, 64, 128, 0), (160, 512, 768, 0)]


@pytest.mark.parametrize("M,N,K,period", PBIAS_CASES)
def test_reid_gemm_f32_pbias_integer_exact(lib, M, N, K, period):
    """REID_EPI_F32_PBIAS: fp32 out = acc + bias[m % period] (null bias: acc alone); exact on integers.  Every bias row differs, so
    the wrong row (m / period, (m + 1) % period, row 0) shows."""
    rng = np.random.default_rng(M + N + K + period)
    X, W = _ints(rng, -2, 2, (M, K)), _ints(rng, -2, 2, (N, K))
    bias = _ints(rng, -500, 500, (period, N), np.float32) if period else None
    out = _reid_gemm(lib, EPI_F32_PBIAS, X, W, bias, period, np.full((M, N), np.nan, np.float32))
    want = _t64(X) @ _t64(W).T
    if period:
        want = want + _t64(bias)[np.arange(M) % period]
    np.testing.assert_array_equal(out.astype(np.float64), want.numpy())


@pytest.mark.parametrize("M,N,K", [(1, 64, 64), (65, 128, 64), (50, 3072, 768), (130, 3072, 768), (63, 3072, 1024)])
def test_reid_gemm_quick_gelu_within_derived_bound(lib, M, N, K):
    """REID_EPI_F16_QGELU: z = acc + bias is exact (integer acc, bias on a 1/16 grid), so the only errors are quick_gelu's fp32
    arithmetic (expf and three roundings) and the one fp16 rounding: |out - y64| <= B.qgelu_bound, at most 1 fp16 ulp of y64 plus the
    fp32 term."""
    rng = np.random.default_rng(M + N + K)
    X, W = _ints(rng, -1, 1, (M, K)), _ints(rng, -1, 1, (N, K))
    bias = (rng.integers(-64, 65, N) / 16).astype(np.float32)
    out = _reid_gemm(lib, EPI_F16_QGELU, X, W, bias, 0, np.zeros((M, N), np.float16))
    z = (_t64(X) @ _t64(W).T + _t64(bias)).numpy()
    assert (np.abs(z) < 8).mean() > 0.05   # a good share of the arguments on the curved part of quick_gelu
    y, bound = B.qgelu(z), B.qgelu_bound(z)
    err = np.abs(out.astype(np.float64) - y)
    assert (err <= bound).all(), (err.max(), np.unravel_index((err - bound).argmax(), err.shape))


# ---- attention ----------------------------------------------------------------------------------------------------------------------------
ATTN_CASES = [(1, 64, 1), (2, 768, 3), (5, 1024, 3), (17, 256, 160), (50, 768, 3), (63, 64, 160), (64, 1024, 1), (64, 64, 160),
              (50, 64, 160), (17, 1024, 3)]


def _attention(lib, qkv, crops, T, H):
    assert qkv.shape == (crops * T, 3 * H)
    out = np.full((crops * T, H), SENTINEL, np.float16)
    _capi.check(lib.opd_test_reid_attention(_p(qkv), _p(out), crops, T, H), "opd_test_reid_attention")
    return out


@pytest.mark.parametrize("T,H,crops", ATTN_CASES)
@pytest.mark.parametrize("peaked", [False, True], ids=["spread", "peaked"])
def test_reid_attention_within_derived_bound(lib, T, H, crops, peaked):
    """softmax(q k^T) v per (crop, head) at every token count the loader accepts (1 .. 64; patch 224 / 112 / 56 / 32 give 2 / 5 / 17 /
    50) against float64 on the same fp16 q, k, v.  Peaked rows (q k up to ~60) put nearly all of P on one key."""
    rng = np.random.default_rng(T * 1000 + H + crops + peaked)
    qkv = rng.standard_normal((crops * T, 3 * H))
    if peaked:
        qkv[:, :H] *= 8.0
    qkv = np.ascontiguousarray(qkv.astype(np.float16))
    out = _attention(lib, qkv, crops, T, H)
    q, k, v = B.split_qkv(qkv, crops, T, H)
    want, bound = B.attention(q, k, v), B.attention_bound(q, k, v)
    err = np.abs(B.heads_to_rows(out.astype(np.float64), crops, T, H) - want)
    assert (err <= bound).all(), (err.max(), bound.max())
    if peaked:
        assert B.softmax(q @ np.swapaxes(k, -1, -2)).max(-1).mean() > 0.9


# ---- LayerNorm ----------------------------------------------------------------------------------------------------------------------------
LN_CASES = [(128, 1, 1), (128, 7, 17), (256, 5, 2), (256, 130, 1), (768, 3, 50), (768, 161, 1), (1024, 10, 17), (1024, 6, 50)]


@pytest.mark.parametrize("H,rows,stride", LN_CASES)
@pytest.mark.parametrize("kind", ["offset", "narrow"])
def test_reid_layernorm_within_derived_bound(lib, H, rows, stride, kind):
    """LayerNorm of rows r * stride, row counts not multiples of 4.  'offset': a common offset of ~1e3 on unit-scale rows, where a
    one-pass variance (E[x^2] - mean^2 in fp32) fails; 'narrow': standard deviation ~3e-3, where the 1e-5 epsilon matters.  fp16 out
    against float64 within B.layernorm_bound; the fp32 rewrite of the selected rows (stride 1) too, and every other row untouched."""
    rng = np.random.default_rng(H + rows * 3 + stride)
    n = rows * stride
    if kind == "offset":
        x = 1000.0 + rng.uniform(-3, 3, (n, 1)) + rng.standard_normal((n, H)) * rng.uniform(0.5, 3, (n, 1))
    else:
        x = rng.standard_normal((n, 1)) + rng.standard_normal((n, H)) * 3e-3
    x = x.astype(np.float32)
    g = (1 + 0.2 * rng.standard_normal(H)).astype(np.float32)
    b = (0.1 * rng.standard_normal(H)).astype(np.float32)
    y16 = np.full((rows, H), SENTINEL, np.float16)
    y32 = np.full_like(x, np.nan)
    _capi.check(lib.opd_test_reid_layernorm(_p(x), _p(g), _p(b), _p(y32), _p(y16), rows, stride, H), "opd_test_reid_layernorm")
    sel = x[::stride]
    want, bound = B.layernorm(sel, g, b), B.layernorm_bound(sel, g, b)
    err16 = np.abs(y16.astype(np.float64) - want)
    assert (err16 <= bound + 0.5 * B.ulp16(np.abs(want) + bound)).all(), err16.max()
    err32 = np.abs(y32[::stride].astype(np.float64) - want)
    assert (err32 <= bound).all(), err32.max()
    keep = np.ones(n, bool)
    keep[::stride] = False
    np.testing.assert_array_equal(y32[keep], x[keep])


# ---- L2 norm --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [128, 256, 512, 100])
def test_reid_l2norm_within_derived_bound(lib, E):
    rng = np.random.default_rng(E)
    rows = 37
    y = (rng.standard_normal((rows, E)) * rng.uniform(1e-2, 1e2, (rows, 1))).astype(np.float32)
    y[3, : E // 2] = 0.0
    got = y.copy()
    _capi.check(lib.opd_test_reid_l2norm(_p(got), rows, E), "opd_test_reid_l2norm")
    want, bound = B.l2norm(y), B.l2norm_bound(y)
    err = np.abs(got.astype(np.float64) - want)
    assert (err <= bound).all(), (err.max(), bound.max())


# ==== OSNet: kernels_osnet.hip ==============================================================================================================
OS_NONE, OS_RELU, OS_RESID = 0, 1, 2


def _osnet_gemm(lib, epi, M, N, k1, lda1, k2=0, lda2=0, groups=1, a_gcol=0, o_gcol=0, ldo=None, ldr=0, seed=0):
    """One osnet_gemm launch on integer operands, checked bit for bit against float64, with every column of `out` outside the
    written ranges still holding SENTINEL."""
    ldo = ldo or (groups - 1) * o_gcol + N
    # the hook's buffers are exactly [M][lda]: every column the launch reads or writes must lie inside them
    assert (groups - 1) * a_gcol + k1 <= lda1 and k2 <= lda2 and (groups - 1) * o_gcol + N <= ldo and (epi != OS_RESID or N <= ldr)
    assert groups == 1 or o_gcol >= N
    rng = np.random.default_rng(seed)
    a1 = _ints(rng, -2, 2, (M, lda1))
    a2 = _ints(rng, -2, 2, (M, lda2)) if k2 else None
    w = _ints(rng, -2, 2, (groups, N, k1 + k2))
    bias = _ints(rng, -16, 16, (groups, N), np.float32) if epi != OS_NONE else None
    res = _ints(rng, -50, 50, (M, ldr)) if epi == OS_RESID else None
    out = np.full((M, ldo), SENTINEL, np.float16)
    _capi.check(lib.opd_test_osnet_gemm(epi, _p(a1), lda1, k1, _p(a2), lda2, k2, _p(w), _p(bias), _p(res), ldr, _p(out), ldo, M, N, groups,
                                        a_gcol, o_gcol), "opd_test_osnet_gemm")
    want = np.full((M, ldo), np.float64(SENTINEL))
    for z in range(groups):
        x = _t64(a1[:, z * a_gcol:z * a_gcol + k1])
        if k2:
            x = torch.cat([x, _t64(a2[:, :k2])], 1)
        y = x @ _t64(w[z]).T
        if epi != OS_NONE:
            y = y + _t64(bias[z])
        if epi == OS_RESID:
            y = y + _t64(res[:, :N])
        if epi != OS_NONE:
            y = torch.relu(y)
        want[:, z * o_gcol:z * o_gcol + N] = y.numpy()
    assert np.abs(want).max() <= 2048
    np.testing.assert_array_equal(out.astype(np.float64), want)


# (epi, M, N, k1, lda1, k2, lda2, groups, a_gcol, o_gcol, ldo, ldr).  N = 16 / 48 / 80 leave the second 16-column tile of the last
# workgroup missing; k1 / k2 = 16 / 48 / 96 leave a zero-filled K tail; lda2 != k2; groups 1 .. 4 with gaps between the groups' columns
OSNET_GEMM_CASES = [
    (OS_RELU, 1, 16, 16, 16, 0, 0, 1, 0, 0, 20, 0),
    (OS_NONE, 127, 48, 48, 216, 0, 0, 4, 56, 52, 212, 0),
    (OS_RELU, 128, 80, 64, 72, 16, 24, 1, 0, 0, 84, 0),
    (OS_RELU, 129, 96, 96, 192, 32, 40, 2, 96, 100, 196, 0),
    (OS_NONE, 129, 16, 16, 48, 0, 0, 3, 16, 16, 48, 0),
    (OS_NONE, 160 * 128, 80, 48, 104, 0, 0, 2, 56, 84, 168, 0),
    (OS_RELU, 128, 16, 16, 16, 128, 136, 1, 0, 0, 16, 0),
    (OS_RELU, 160 * 128, 512, 96, 96, 128, 136, 1, 0, 0, 512, 0),
    (OS_RELU, 127, 48, 16, 16, 48, 56, 1, 0, 0, 52, 0),
    (OS_RESID, 1, 48, 16, 16, 0, 0, 1, 0, 0, 48, 52),
    (OS_RESID, 127, 80, 48, 48, 0, 0, 1, 0, 0, 88, 88),
    (OS_RESID, 129, 96, 96, 104, 0, 0, 1, 0, 0, 96, 128),
    (OS_RESID, 160 * 128, 512, 64, 64, 0, 0, 1, 0, 0, 520, 576),
    (OS_RESID, 128, 16, 16, 24, 0, 0, 1, 0, 0, 16, 24),
    (OS_NONE, 1, 512, 64, 64, 16, 16, 1, 0, 0, 512, 0),
]


@pytest.mark.parametrize("case", OSNET_GEMM_CASES, ids=lambda c: "epi{}_M{}_N{}_k{}+{}_g{}".format(c[0], c[1], c[2], c[3], c[5], c[7]))
def test_osnet_gemm_integer_exact(lib, case):
    epi, M, N, k1, lda1, k2, lda2, groups, a_gcol, o_gcol, ldo, ldr = case
    _osnet_gemm(lib, epi, M, N, k1, lda1, k2, lda2, groups, a_gcol, o_gcol, ldo, ldr, seed=sum(case))


@pytest.mark.parametrize("C0", [16, 32, 48, 64])
def test_osnet_stem_and_maxpool_integer_exact(lib, C0):
    """7x7 stride-2 stem (+ bias, ReLU) and 3x3 stride-2 max-pool at every stem width: exact on integers.  The padded weight columns
    and bias entries >= C0, and image channel 3, hold large values that must not reach the output."""
    rng = np.random.default_rng(C0)
    nb = 2
    img = _ints(rng, -2, 2, (nb, 256, 128, 4))
    img[..., 3] = 99
    w = _ints(rng, -1, 1, (147, 64))
    w[:, C0:] = 50
    b = _ints(rng, -20, 20, 64, np.float32)
    b[C0:] = 1000
    out = np.full((nb, 64, 32, C0), SENTINEL, np.float16)
    _capi.check(lib.opd_test_osnet_stem(_p(img), _p(w), _p(b), _p(out), nb, C0), "opd_test_osnet_stem")
    x = _t64(img[..., :3]).permute(0, 3, 1, 2)
    k = _t64(w[:, :C0]).reshape(7, 7, 3, C0).permute(3, 2, 0, 1)
    s = F.relu(F.conv2d(x, k, stride=2, padding=3) + _t64(b[:C0])[None, :, None, None])
    want = F.max_pool2d(s, 3, 2, 1).permute(0, 2, 3, 1).numpy()
    np.testing.assert_array_equal(out.astype(np.float64), want)


# (H, W, ld, c0, nc, ldw): the three stage resolutions, channel ranges starting inside the row (levels 2 .. 4), ldw != ld
DW_CASES = [(64, 32, 64, 16, 48, 68), (64, 32, 128, 0, 128, 128), (32, 16, 192, 96, 96, 200), (32, 16, 320, 160, 160, 324),
            (16, 8, 320, 240, 80, 320), (16, 8, 1024, 512, 512, 1028), (16, 8, 64, 48, 16, 72)]


@pytest.mark.parametrize("H,W,ld,c0,nc,ldw", DW_CASES)
def test_osnet_dwconv_integer_exact(lib, H, W, ld, c0, nc, ldw):
    rng = np.random.default_rng(H + ld + c0 + nc)
    nb = 3
    x = _ints(rng, -3, 3, (nb, H, W, ld))
    w9 = _ints(rng, -2, 2, (9, ldw), np.float32)
    bias = _ints(rng, -10, 10, ldw, np.float32)
    out = np.full((nb, H, W, ld), SENTINEL, np.float16)
    _capi.check(lib.opd_test_osnet_dwconv(_p(x), _p(out), _p(w9), _p(bias), nb, H, W, ld, c0, nc, ldw), "opd_test_osnet_dwconv")
    xs = _t64(x[..., c0:c0 + nc]).permute(0, 3, 1, 2)
    k = _t64(w9[:, c0:c0 + nc]).T.reshape(nc, 1, 3, 3)
    want = np.full(out.shape, np.float64(SENTINEL))
    want[..., c0:c0 + nc] = F.relu(F.conv2d(xs, k, padding=1, groups=nc) + _t64(bias[c0:c0 + nc])[None, :, None, None]).permute(0, 2, 3, 1).numpy()
    np.testing.assert_array_equal(out.astype(np.float64), want)


# (mid, HW): every stream width of osnet_x1_0 / x0_5 and the odd set (16 .. 256: 16, 5, 3 and 1 parts; hid = mid / 16 = 1 .. 16) at
# the stage resolutions
GATE_CASES = [(16, 2048), (32, 2048), (48, 512), (64, 2048), (80, 128), (96, 512), (128, 128), (256, 128), (80, 512), (48, 128)]


@pytest.mark.parametrize("mid,HW", GATE_CASES)
def test_osnet_gate_and_combine_within_derived_bound(lib, mid, HW):
    rng = np.random.default_rng(mid * 10 + HW)
    nb, hid = 3, max(1, mid // 16)
    t = np.ascontiguousarray(np.abs(rng.standard_normal((nb * HW, 4 * mid)) * rng.uniform(0.2, 2, 4 * mid)).astype(np.float16))
    w1 = (rng.standard_normal((hid, mid)) * mid ** -0.5 * 2).astype(np.float32)
    b1 = (rng.standard_normal(hid) * 0.1).astype(np.float32)
    w2 = (rng.standard_normal((mid, hid)) * hid ** -0.5 * 2).astype(np.float32)
    b2 = (rng.standard_normal(mid) * 0.1).astype(np.float32)
    gates = np.full((nb, 4, mid), np.nan, np.float32)
    x2 = np.full((nb * HW, mid), SENTINEL, np.float16)
    _capi.check(lib.opd_test_osnet_gate(_p(t), _p(w1), _p(b1), _p(w2), _p(b2), _p(gates), _p(x2), nb, HW, mid, hid), "opd_test_osnet_gate")
    g, gb = B.gate(t, w1, b1, w2, b2, nb, HW, mid), B.gate_bound(t, w1, b1, w2, b2, nb, HW, mid)
    err = np.abs(gates.astype(np.float64) - g)
    assert (err <= gb).all(), (err.max(), gb.max())
    x, xb = B.combine(t, g, nb, HW, mid), B.combine_bound(t, g, gb, nb, HW, mid)
    err = np.abs(x2.astype(np.float64) - x)
    assert (err <= xb).all(), (err.max(), xb.max())


# (H, W, C): the transitions of osnet_x1_0 (256, 384), x0_5 (128, 192) and the odd set (64, 192)
@pytest.mark.parametrize("H,W,C", [(64, 32, 256), (32, 16, 384), (64, 32, 128), (32, 16, 192), (64, 32, 64)])
def test_osnet_avgpool_exact(lib, H, W, C):
    """2x2 average pool: integer inputs make every quarter-sum exact in fp16."""
    rng = np.random.default_rng(H + C)
    nb = 3
    x = _ints(rng, -100, 100, (nb, H, W, C))
    out = np.full((nb, H // 2, W // 2, C), SENTINEL, np.float16)
    _capi.check(lib.opd_test_osnet_avgpool2(_p(x), _p(out), nb, H, W, C), "opd_test_osnet_avgpool2")
    want = F.avg_pool2d(_t64(x).permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1).numpy()
    np.testing.assert_array_equal(out.astype(np.float64), want)


@pytest.mark.parametrize("C", [128, 256, 320, 512])
def test_osnet_head_within_derived_bound(lib, C):
    rng = np.random.default_rng(C)
    nb, HW = 5, 128
    x = np.ascontiguousarray(np.abs(rng.standard_normal((nb, HW, C))).astype(np.float16))
    wt = (rng.standard_normal((C, 512)) * C ** -0.5).astype(np.float32)
    b = (rng.standard_normal(512) * 0.1).astype(np.float32)
    feat = np.full((nb, 512), np.nan, np.float32)
    _capi.check(lib.opd_test_osnet_head(_p(x), _p(wt), _p(b), _p(feat), nb, HW, C), "opd_test_osnet_head")
    want, bound = B.head(x, wt, b), B.head_bound(x, wt, b)
    err = np.abs(feat.astype(np.float64) - want)
    assert (err <= bound).all(), (err.max(), bound.max())
