"""Both instantiations of the 16-bit kernels (csrc/opd_elem.h: one source, compiled for fp16 and for bf16) at kernel level, through the
hooks of csrc/opd_test_api.cpp under ``opd_test_set_elem_bf16``.  Every test body runs for both element types: the fp16 leg proves the
test, a failure on the bf16 leg alone points at the instantiation.

Three kinds of assertion (tests/elem_common.py; the CPU side of each is tests/test_elem_common_cpu.py):
 (a) exact arithmetic: small-integer operands, every stored value an integer <= EXACT_INT[elem]; the precondition and non-triviality are
     asserted on the float64 reference, then bits are compared;
 (b) bit identity of two routes of one instantiation on random operands, one launch per route;
 (c) a derived bound per output element against float64 on the same rounded operands, where a result is inherently rounded.  Each such
     test prints its worst error / bound ratio ("RATIO ...").
"""

import ctypes as C

import numpy as np
import pytest

import elem_common as E
from elem_common import U, from_bits, round_bound, round_elem, to_bits
from office_person_detection_vit_amd import _capi

pytestmark = pytest.mark.gpu

f32 = np.float32
SCALE = 32 ** -0.5


@pytest.fixture(scope="module")
def lib():
    return _capi.load_library(test_hooks=True)


@pytest.fixture(params=E.ELEMS)
def elem(request, lib):
    lib.opd_test_set_elem_bf16(int(request.param == "bf16"))
    yield request.param
    lib.opd_test_set_elem_bf16(0)


@pytest.fixture(autouse=True)
def _options_off_afterwards(lib):
    yield
    lib.opd_test_set_conv_flags(0)
    lib.opd_test_set_gemm_ln_kloop(0)
    lib.opd_test_set_pos_frames(0)


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _c32(a):
    return np.ascontiguousarray(a, dtype=f32) if a is not None else None


def _ratio(name, elem, err, bound):
    r = E.excess(err, bound)
    print(f"RATIO {name} {elem}: {r:.3f}")
    return r


def _exact(ref, elem):
    """The precondition of an exact-arithmetic comparison, and the reference's bit patterns."""
    assert np.array_equal(ref, np.round(ref)) and np.abs(ref).max() <= E.EXACT_INT[elem], float(np.abs(ref).max())
    assert E.nontrivial(ref)
    return to_bits(ref + 0.0, elem)


def _same(got, want, what):
    assert np.array_equal(got, want), f"{what}: {np.count_nonzero(got != want)} of {want.size} elements differ"


# ---- launch helpers (operands as float arrays, rounded to the element type here; outputs as bit patterns) -----------------------------------------
def conv_bits(lib, elem, x, w, bias, k, stride, relu, res=None):
    """x [B][H][W][Cin], w [N][k * k * Cin] (hook layout) -> [M][N] bits."""
    B, H, W, Cin = x.shape
    N, pad = w.shape[0], k // 2
    OH, OW = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    out = np.full((B * OH * OW, N), 0xFFFF, np.uint16)
    rc = lib.opd_test_conv_gemm(_p(to_bits(x, elem)), _p(to_bits(w, elem)), _p(_c32(bias)), _p(to_bits(res, elem)) if res is not None else None, None,
                                _p(out), B, H, W, Cin, OH, OW, N, k, k, stride, pad, int(relu), 0, 0, 0)
    _capi.check(rc, "opd_test_conv_gemm")
    return out


def btail_bits(lib, elem, d, B, H, W, C1, C3, stride):
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    M = B * OH * OW
    y = np.full((M, 4 * C1), 0xFFFF, np.uint16)
    z = np.full((M, max(C3, 1)), 0xFFFF, np.uint16)
    bits = lambda a: to_bits(a, elem) if a is not None else None
    rc = lib.opd_test_btail(_p(bits(d["x1"])), _p(bits(d["w1"])), _p(_c32(d["b1"])), _p(bits(d["w2"])), _p(_c32(d["b2"])), _p(bits(d["res"])),
                            _p(bits(d["w3"])), _p(_c32(d["b3"])), _p(y), _p(z), B, H, W, C1, C3, stride)
    _capi.check(rc, "opd_test_btail")
    return y, (z if C3 else None)


# ================================================================ (a) exact arithmetic ================================================================
@pytest.mark.parametrize("case", E.TAIL_CASES, ids=lambda c: "x".join(map(str, c[:6])))
def test_btail_exact_and_equals_unfused(lib, elem, case):
    """The fused bottleneck tails (kernels_btail.hip, kernels_btail3.hip) on integer operands with random weight positions: y and z equal the
    exact sums bit for bit, and the three unfused implicit-GEMM launches."""
    B, H, W, C1, C3, stride, use_res = case
    d = E.tail_recipe(case)
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    M, C2 = B * OH * OW, 4 * C1
    want_y = _exact(d["y"].reshape(M, C2), elem)
    want_z = _exact(d["z"].reshape(M, C3), elem) if C3 else None
    assert np.abs(d["a1"]).max() <= E.EXACT_INT[elem]
    y, z = btail_bits(lib, elem, d, B, H, W, C1, C3, stride)
    _same(y, want_y, "y against the exact sums")
    if C3:
        _same(z, want_z, "z against the exact sums")
    a1 = from_bits(conv_bits(lib, elem, d["x1"], d["w1"], d["b1"], 3, stride, True), elem).reshape(B, OH, OW, C1)
    yu = conv_bits(lib, elem, a1, d["w2"], d["b2"], 1, 1, True, d["res"].reshape(M, C2) if use_res else None)
    _same(y, yu, "y against the unfused launches")
    if C3:
        zu = conv_bits(lib, elem, from_bits(yu, elem).reshape(B, OH, OW, C2), d["w3"], d["b3"], 1, 1, True)
        _same(z, zu, "z against the unfused launches")


def test_btail_fused_shortcut_exact(lib, elem):
    """The first tail of stage 1 (shortcut convolution as a second GEMM into the expand's accumulators): exact sums, and the two-launch route."""
    B, H, W = E.TAIL_SC_SHAPE
    M = B * H * W
    d = E.tail_sc_recipe()
    want_y, want_z = _exact(d["y"].reshape(M, 256), elem), _exact(d["z"].reshape(M, 64), elem)
    assert max(np.abs(d["a1"]).max(), np.abs(d["sc"]).max()) <= E.EXACT_INT[elem]
    y = np.full((M, 256), 0xFFFF, np.uint16)
    z = np.full((M, 64), 0xFFFF, np.uint16)
    bits = lambda a: to_bits(a, elem)
    args = [bits(d["x1"]), bits(d["w1"]), _c32(d["b1"]), bits(d["w2"]), _c32(d["b2"] + d["bsc"]), bits(d["xs"]), bits(d["wsc"]), bits(d["w3"]), _c32(d["b3"]), y, z]
    _capi.check(lib.opd_test_btail_sc(*[_p(a) for a in args], B, H, W), "opd_test_btail_sc")
    _same(y, want_y, "y against the exact sums")
    _same(z, want_z, "z against the exact sums")
    sc = conv_bits(lib, elem, d["xs"], d["wsc"], d["bsc"], 1, 1, False)             # the two-launch route: shortcut, then a residual tail
    _same(sc, to_bits(d["sc"].reshape(M, 256) + 0.0, elem), "the shortcut launch")
    yu, zu = btail_bits(lib, elem, dict(d, res=from_bits(sc, elem)), B, H, W, 64, 64, 1)
    _same(y, yu, "y against the two-launch route")
    _same(z, zu, "z against the two-launch route")


@pytest.mark.parametrize("flags", E.TILE_FLAGS, ids=E.TILE_IDS)
@pytest.mark.parametrize("name", list(E.CONV_INT_CASES))
def test_conv_gemm_exact(lib, elem, name, flags):
    """The implicit GEMM under every tile height and the flat staging path: a 3x3 with signed outputs, and the residual + ReLU epilogue on
    M = 135 (rows >= M of the last tile)."""
    B, H, W, Cin, N, k, relu, use_res = E.CONV_INT_CASES[name]
    d = E.conv_int_recipe(name)
    want = _exact(d["y"].reshape(-1, N), elem)
    lib.opd_test_set_conv_flags(flags)
    got = conv_bits(lib, elem, d["x"], d["w"], d["bias"], k, 1, relu, d["res"].reshape(-1, N) if use_res else None)
    _same(got, want, name)


def test_conv_dual_source_exact(lib, elem):
    """The shortcut convolution as extra K of the 1x1 expand (stride 2 on the second source, odd sizes)."""
    B, H, W, Cin, N, Cin2, s2 = E.DUAL_CASE
    d = E.dual_recipe()
    want = _exact(d["y"].reshape(-1, N), elem)
    out = np.full((B * H * W, N), 0xFFFF, np.uint16)
    rc = lib.opd_test_conv_dual(_p(to_bits(d["x"], elem)), _p(to_bits(d["w1"], elem)), _p(to_bits(d["x2"], elem)), _p(to_bits(d["w2"], elem)), _p(_c32(d["bias"])),
                                _p(out), B, H, W, Cin, 1, 1, 0, N, d["H2"], d["W2"], Cin2, s2, 1)
    _capi.check(rc, "opd_test_conv_dual")
    _same(out, want, "dual-source GEMM")


def test_conv_splitk_exact_and_equals_unsplit(lib, elem):
    """Split-K slabs + reduce_act16 on a convolution with taps (every slice but the first starts in the middle of a tap)."""
    B, H, W, Cin, N, k, stride, splits = E.SPLITK_CASE
    d = E.splitk_recipe()
    want = _exact(d["y"].reshape(-1, N), elem)
    pad = k // 2
    out = np.full((B * H * W, N), 0xFFFF, np.uint16)
    rc = lib.opd_test_conv_splitk(_p(to_bits(d["x"], elem)), _p(to_bits(d["w"], elem)), _p(_c32(d["bias"])), _p(out), B, H, W, Cin, H, W, N, k, k, stride, pad, 1, splits)
    _capi.check(rc, "opd_test_conv_splitk")
    _same(out, want, "split-K against the exact sums")
    _same(out, conv_bits(lib, elem, d["x"], d["w"], d["bias"], k, stride, True), "split-K against the unsplit launch")


def test_gemm_k256_exact(lib, elem):
    M, N = E.K256_CASE
    d = E.k256_recipe()
    want = _exact(d["y"], elem)
    out = np.full((M, N), 0xFFFF, np.uint16)
    rc = lib.opd_test_gemm_k256(_p(to_bits(d["x"], elem)), _p(to_bits(d["w"], elem)), _p(_c32(d["bias"].reshape(1, N))), _p(out), None, M, N, 256, 0, 0)
    _capi.check(rc, "opd_test_gemm_k256")
    _same(out, want, "gemm_k256")


def test_gemm_alt_source_exact(lib, elem):
    """Column groups of one pointwise launch read different activations (x_alt)."""
    M, N, K, alt_mod, alt_cols = E.ALT_CASE
    d = E.alt_recipe()
    want = _exact(d["y"], elem)
    out = np.full((M, N), 0xFFFF, np.uint16)
    rc = lib.opd_test_gemm_alt(_p(to_bits(d["x"], elem)), _p(to_bits(d["xa"], elem)), _p(to_bits(d["w"], elem)), _p(_c32(d["bias"])), _p(out), M, N, K, alt_mod, alt_cols)
    _capi.check(rc, "opd_test_gemm_alt")
    _same(out, want, "gemm_alt")


@pytest.mark.parametrize("out_f32", [False, True], ids=["elem_out", "f32_out"])
def test_gemm_frame_bias_exact(lib, elem, out_f32):
    """Per-frame periodic bias tables, every entry its own value: sums exact in fp32; a 16-bit output is the exact sum rounded once."""
    Bf, period, N, pmod, pcols = E.FRAME_BIAS_CASE
    d = E.frame_bias_recipe()
    M = Bf * period
    out = np.full((M, N), np.nan, f32) if out_f32 else np.full((M, N), 0xFFFF, np.uint16)
    rc = lib.opd_test_gemm_frame_bias(_p(to_bits(d["x"], elem)), _p(to_bits(d["w"], elem)), _p(d["tables"]), _p(out), M, N, 256, period, pmod, pcols, int(out_f32))
    _capi.check(rc, "opd_test_gemm_frame_bias")
    if out_f32:
        _same(out, d["y"].astype(f32), "fp32 output")
    else:
        _same(out, to_bits(d["y"], elem), "16-bit output")


def test_maxpool_exact(lib, elem):
    """MaxPool2d(3, 2, 1) on values both types hold exactly, windows far below zero included (the starting value of the maximum).  A maximum
    of 16-bit floats is the same selection of bit patterns in either type, so the bf16 leg also holds one value that only bf16 has: 2^125,
    whose pattern is a NaN to an fp16 comparison."""
    B, H, W, Cc = E.MAXPOOL_SHAPE
    d = E.maxpool_recipe()
    if elem == "bf16":
        d["x"][0, 5, 7, 3] = 2.0 ** 125
        d["y"] = E.maxpool64(d["x"])
        assert (d["y"] == 2.0 ** 125).sum() == 4
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    assert np.array_equal(round_elem(d["x"], elem), d["x"])
    out = np.full((B, OH, OW, Cc), 0xFFFF, np.uint16)
    _capi.check(lib.opd_test_maxpool(_p(to_bits(d["x"], elem)), _p(out), B, H, W, Cc, OH, OW), "opd_test_maxpool")
    _same(out, to_bits(d["y"], elem), "maxpool")


@pytest.mark.parametrize("relu", [1, 0], ids=["relu", "linear"])
def test_reduce_act16_exact(lib, elem, relu):
    nsplit, n, pad = E.REDUCE_ACT16
    d = E.reduce_act16_recipe()
    want = np.maximum(d["y"], 0) if relu else d["y"]
    bits = _exact(want, elem)
    flat = np.ascontiguousarray(d["part"].reshape(-1)[:(nsplit - 1) * (n + pad) + n])
    out = np.full(n, 0xFFFF, np.uint16)
    _capi.check(lib.opd_test_reduce_act16(_p(flat), nsplit, n + pad, n, relu, _p(out)), "opd_test_reduce_act16")
    _same(out, bits, "reduce_act16")


# ================================================================ (b) two routes, one instantiation ===================================================
def _random_conv(rng, B, H, W, Cin, N, k, elem):
    x = round_elem(rng.standard_normal((B, H, W, Cin)), elem)
    w = round_elem(rng.standard_normal((N, k * k * Cin)) * np.sqrt(2.0 / (Cin * k * k)), elem)
    return x, w, (rng.standard_normal(N) * 0.1).astype(f32)


@pytest.mark.parametrize("case", [(1, 9, 11, 64, 256, 3, True), (1, 16, 24, 192, 256, 1, False)], ids=["3x3", "1x1_3ksteps"])
def test_conv_w8_equals_four_wave_kernel(lib, elem, case):
    """kernels_w8.hip against kernels_gemm.hip: the same k order and MFMA order per accumulator element, hence the same bits."""
    B, H, W, Cin, N, k, relu = case
    x, w, bias = _random_conv(np.random.default_rng(Cin + k), B, H, W, Cin, N, k, elem)
    base = conv_bits(lib, elem, x, w, bias, k, 1, relu)
    lib.opd_test_set_conv_flags(1 << 12)
    got = conv_bits(lib, elem, x, w, bias, k, 1, relu)
    v = from_bits(base, elem)
    assert np.isfinite(v).all() and np.abs(v).max() > 0.5 and np.count_nonzero(base & 0x7FFF) > base.size // 4
    _same(got, base, "eight-wave against four-wave kernel")


def test_wprefetch_conv_is_bit_identical(lib, elem):
    """The L2 warm-up of the weights at launch start changes no bit (the 3x3 case of test_gemm_options_gpu.py)."""
    B, H, W, Cin, N, k = 2, 13, 17, 256, 256, 3
    x, w, bias = _random_conv(np.random.default_rng(B * 1000 + Cin + k), B, H, W, Cin, N, k, elem)
    off = conv_bits(lib, elem, x, w, bias, k, 1, True)
    lib.opd_test_set_conv_flags(0x2000)
    on = conv_bits(lib, elem, x, w, bias, k, 1, True)
    assert np.isfinite(from_bits(off, elem)).all() and np.count_nonzero(off & 0x7FFF) > off.size // 4
    _same(on, off, "with against without wprefetch")


def _stem_weights(rng, elem):
    w = np.zeros((64, 8, 8, 4), f32)                                      # [n][kh][kw][c]: eighth row / column and fourth channel zero
    w[:, :7, :7, :3] = rng.standard_normal((64, 7, 7, 3)) * 0.1
    return round_elem(w, elem), (rng.standard_normal(64) * 0.1).astype(f32)


@pytest.mark.parametrize("B,H,W,valid", [(2, 61, 83, [[61, 83], [40, 57]]), (2, 37, 53, None)], ids=["ragged", "full"])
def test_stem_pool_with_preprocessing_inside_equals_split(lib, elem, B, H, W, valid):
    """stem_pool2_kernel<U8> (normalisation by fma while the patch is staged) against preprocess_u8_kernel -> stem_pool2_kernel: the same
    bits.  Two routes of the wrong instantiation would agree as well, so the split route is also held to the stem's derived bound
    (elem_common.stem_pool_reference) on the image preprocess_u8_kernel makes of these frames."""
    rng = np.random.default_rng(B * 7919 + H * 31 + W)
    frames = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    frames[0, :5, :7] = 255
    frames[-1, -3:, -5:] = 0
    w, bias = _stem_weights(rng, elem)
    vhw = np.ascontiguousarray(valid, np.int32) if valid is not None else None
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    PH, PW = (OH - 1) // 2 + 1, (OW - 1) // 2 + 1
    fused = np.full((B, PH, PW, 64), 0xFFFF, np.uint16)
    split = np.full((B, PH, PW, 64), 0xFFFF, np.uint16)
    rc = lib.opd_test_stem_pool_u8(_p(frames), _p(vhw), _p(to_bits(w.reshape(64, 256), elem)), _p(bias), _p(fused), _p(split), B, H, W)
    _capi.check(rc, "opd_test_stem_pool_u8")
    v = from_bits(split, elem)
    assert np.isfinite(v).all() and v.max() > 0.5 and (v >= 0).all() and 0.2 < (v > 0).mean()
    _same(fused, split, "fused against split")
    Hp, Wp = 2 * OH + 6, 2 * OW + 6
    x4p = np.full((B, Hp, Wp, 4), 0xFFFF, np.uint16)
    _capi.check(lib.opd_test_preprocess_u8(_p(frames), _p(x4p), B, H, W, Hp, Wp, _p(vhw)), "opd_test_preprocess_u8")
    want, bound = E.stem_pool_reference(from_bits(x4p, elem)[:, 3:3 + H, 3:3 + W, :3], w[:, :7, :7, :3], bias, elem)
    assert _ratio(f"stem_pool_u8 ({H},{W})", elem, np.abs(v - want), bound) <= 1


@pytest.mark.parametrize("B,H,W", [(1, 10, 14), (2, 13, 17)])
def test_btail_chain_routes_are_bit_identical(lib, elem, B, H, W):
    """Stage 1's three tails both ways (residual read back / rebuilt; y stored everywhere / at even positions only): everything the old route
    stores comes out with the same bits, and nothing else of the strided buffer is touched (pre-filled with 0xA5 bytes)."""
    rng = np.random.default_rng(1000 * B + 10 * H + W)
    M = B * H * W
    bits = lambda a: to_bits(a, elem)
    x1 = bits(np.abs(rng.standard_normal((B, H, W, 64))))
    xs = bits(np.abs(rng.standard_normal((M, 64))))
    wsc = bits(rng.standard_normal((256, 64)) / 8)
    w1 = [bits(rng.standard_normal((64, 576)) / 24) for _ in range(3)]
    w2 = [bits(rng.standard_normal((256, 64)) / 8) for _ in range(3)]
    w3 = [bits(rng.standard_normal((c3, 256)) / 16) for c3 in (64, 64, 128)]
    b1 = [_c32(0.1 * rng.standard_normal(64)) for _ in range(3)]
    b2 = [_c32(0.1 * rng.standard_normal(256)) for _ in range(3)]
    b3 = [_c32(0.1 * rng.standard_normal(c3)) for c3 in (64, 64, 128)]
    arr = lambda xs_: (C.c_void_p * len(xs_))(*[x.ctypes.data for x in xs_])
    yb = [np.empty((M, 256), np.uint16) for _ in range(2)]
    zb = [np.empty((M, 64), np.uint16) for _ in range(2)]
    yc = [np.empty((B, H, W, 256), np.uint16) for _ in range(2)]
    zc = [np.empty((M, 128), np.uint16) for _ in range(2)]
    rc = lib.opd_test_btail_chain(_p(x1), _p(xs), arr(w1), arr(b1), arr(w2), arr(b2), _p(wsc), arr(w3), arr(b3), arr(yb), arr(zb), arr(yc), arr(zc), B, H, W, 0xA5)
    _capi.check(rc, "opd_test_btail_chain")
    v = from_bits(yb[0], elem)
    assert np.isfinite(v).all() and v.max() > 0.5
    _same(yb[1], yb[0], "second tail's y, residual rebuilt against read back")
    _same(zb[1], zb[0], "second tail's z")
    _same(zc[1], zc[0], "third tail's z")
    _same(yc[1][:, ::2, ::2], yc[0][:, ::2, ::2], "third tail's y where a stride-2 1x1 reads it")
    untouched = np.ones((B, H, W), bool)
    untouched[:, ::2, ::2] = False
    assert (yc[1][untouched] == 0xA5A5).all(), "third tail stored y at positions nobody reads"
    assert not (yc[0] == 0xA5A5).all()


# ================================================================ (c) derived bounds ===================================================================
def _ln_operands(rng, M, K, elem, use_res=True):
    x = round_elem(rng.standard_normal((M, K)), elem)
    w = round_elem(rng.standard_normal((256, K)) / np.sqrt(K), elem)
    bias = (rng.standard_normal(256) * 0.1).astype(f32)
    res = rng.standard_normal((M, 256)).astype(f32) if use_res else None
    g = (1.0 + 0.1 * rng.standard_normal(256)).astype(f32)
    b = (0.1 * rng.standard_normal(256)).astype(f32)
    pre = x.astype(np.float64) @ w.astype(np.float64).T + bias
    if use_res:
        pre = pre + res
    return x, w, bias, res, g, b, pre


@pytest.mark.parametrize("variant", [1, 0], ids=["oneshot_k256", "kloop"])
@pytest.mark.parametrize("M,K", [(37, 256), (33, 64), (97, 256)])
def test_gemm_ln_bound(lib, elem, M, K, variant):
    """Linear(K -> 256) + bias + residual + LayerNorm in one kernel.  DERIVED bound: gemm_e (K + 2 roundings on the absolute sum) as the row's
    input error, carried through a two-pass LayerNorm whose sums may be added in any order (layernorm_bound); the 16-bit copy one rounding more."""
    x, w, bias, res, g, b, pre = _ln_operands(np.random.default_rng(M * 7 + K), M, K, elem)
    y = np.full((M, 256), np.nan, f32)
    y16 = np.full((M, 256), 0xFFFF, np.uint16)
    lib.opd_test_set_gemm_ln_kloop(1 - variant)
    rc = lib.opd_test_gemm_ln(_p(to_bits(x, elem)), _p(to_bits(w, elem)), _p(bias), _p(res), _p(g), _p(b), _p(y), _p(y16), M, K)
    _capi.check(rc, "opd_test_gemm_ln")
    want = E.layernorm64(pre, g, b)
    bound = E.layernorm_bound(pre, g, b, E.gemm_e(x, w, bias, res))
    r32 = _ratio(f"gemm_ln y32 ({M},{K},{variant})", elem, np.abs(y - want), bound)
    # and the EXISTING fp32 tolerance of test_gemm_ln_matches_torch, unchanged: products of bf16 operands are exact in fp32 as fp16 products are
    np.testing.assert_allclose(y, want, atol=3e-5, rtol=1e-5)
    r16 = _ratio(f"gemm_ln y16 ({M},{K},{variant})", elem, np.abs(from_bits(y16, elem) - want), round_bound(bound, want, elem))
    assert r32 <= 1 and r16 <= 1


@pytest.mark.parametrize("M,K,period,in_place,ln", [(333, 128, 111, True, True), (1, 192, 0, True, True), (77, 320, 11, True, False)])
def test_gemm_ln_deep_bound(lib, elem, M, K, period, in_place, ln):
    """The row-owner ring kernel, in place on the residual stream, with the position shadow, with and without the LayerNorm.  DERIVED bound as
    test_gemm_ln_bound (no LayerNorm: gemm_e alone); the shadow is one rounding of the kernel's own fp32 y + pos."""
    rng = np.random.default_rng(M * 3 + K)
    x, w, bias, res, g, b, pre = _ln_operands(rng, M, K, elem)
    pos = rng.standard_normal((period, 256)).astype(f32) if period else None
    y = np.full((M, 256), np.nan, f32)
    y16 = np.full((M, 256), 0xFFFF, np.uint16)
    yp16 = np.full((M, 256), 0xFFFF, np.uint16)
    rc = lib.opd_test_gemm_ln_deep(_p(to_bits(x, elem)), _p(to_bits(w, elem)), _p(bias), _p(res), _p(g if ln else None), _p(b if ln else None), _p(pos), period,
                                   _p(y), _p(y16), _p(yp16), M, K, int(in_place))
    _capi.check(rc, "opd_test_gemm_ln_deep")
    e = E.gemm_e(x, w, bias, res)
    want, bound = (E.layernorm64(pre, g, b), E.layernorm_bound(pre, g, b, e)) if ln else (pre, e)
    r32 = _ratio(f"gemm_ln_deep y32 ({M},{K})", elem, np.abs(y - want), bound)
    np.testing.assert_allclose(y, want, atol=3e-5, rtol=1e-5)   # the EXISTING fp32 tolerance of test_gemm_ln_deep_matches_torch as well
    r16 = _ratio(f"gemm_ln_deep y16 ({M},{K})", elem, np.abs(from_bits(y16, elem) - want), round_bound(bound, want, elem))
    assert r32 <= 1 and r16 <= 1
    if period:
        _same(yp16, to_bits(y + pos[np.arange(M) % period], elem), "position shadow")


def test_gemm_splitk_ln_bound(lib, elem):
    """Split-K slabs + reduce_ln256_kernel without the LayerNorm at (530, 2048, 4).  DERIVED bound: gemm_e; the 16-bit copy is the kernel's own
    fp32 result rounded once, bit for bit (under bf16 this needs the reduce kernel's bf16 instantiation: an fp16 pattern is another number)."""
    M, K, splits = 530, 2048, 4
    x, w, bias, res, _, _, pre = _ln_operands(np.random.default_rng(M + K + splits), M, K, elem)
    y = np.full((M, 256), np.nan, f32)
    y16 = np.full((M, 256), 0xFFFF, np.uint16)
    rc = lib.opd_test_gemm_splitk_ln(_p(to_bits(x, elem)), _p(to_bits(w, elem)), _p(bias), _p(res), None, None, _p(y), _p(y16), M, K, splits)
    _capi.check(rc, "opd_test_gemm_splitk_ln")
    assert _ratio("gemm_splitk_ln y32", elem, np.abs(y - pre), E.gemm_e(x, w, bias, res)) <= 1
    np.testing.assert_allclose(y, pre, atol=3e-5, rtol=1e-5)   # the EXISTING fp32 tolerance of test_gemm_splitk_reduce_ln as well
    _same(y16, to_bits(y, elem), "y16 against the kernel's own y, rounded once")


@pytest.mark.parametrize("ln", [True, False], ids=["layernorm", "plain_sum"])
def test_reduce_ln_pos_bound(lib, elem, ln):
    """reduce_ln256_kernel with per-frame position tables (333 rows, 4 slabs).  The plain sum is the slice-order fp32 sum exactly; with the
    LayerNorm, DERIVED bound: (nsplit + 1) roundings on the absolute sum as the input error, through layernorm_bound with the kernel's own
    chain (3 additions per lane + 6 shuffle levels, one more for the squares).  Both 16-bit outputs are single roundings of the kernel's fp32."""
    Bf, period, nsplit = 3, 111, 4
    M = Bf * period
    rng = np.random.default_rng(40 + ln)
    part = rng.standard_normal((nsplit, M, 256)).astype(f32)
    res = rng.standard_normal((M, 256)).astype(f32)
    g = (1.0 + 0.1 * rng.standard_normal(256)).astype(f32)
    b = (0.1 * rng.standard_normal(256)).astype(f32)
    tables = rng.standard_normal((Bf, period, 256)).astype(f32)
    y = np.full((M, 256), np.nan, f32)
    y16 = np.full((M, 256), 0xFFFF, np.uint16)
    yp16 = np.full((M, 256), 0xFFFF, np.uint16)
    rc = lib.opd_test_reduce_ln_pos(_p(part), nsplit, _p(res), _p(g) if ln else None, _p(b) if ln else None, None, _p(tables), Bf, period, _p(y), _p(y16), _p(yp16), M)
    _capi.check(rc, "opd_test_reduce_ln_pos")
    if ln:
        pre = part.astype(np.float64).sum(0) + res
        e_in = (nsplit + 1) * U * (np.abs(part).astype(np.float64).sum(0) + np.abs(res))
        assert _ratio("reduce_ln_pos y32", elem, np.abs(y - E.layernorm64(pre, g, b)), E.layernorm_bound(pre, g, b, e_in, depth=10)) <= 1
    else:
        acc = part[0].copy()
        for z in range(1, nsplit):
            acc = acc + part[z]
        _same(y, acc + res, "slice-order fp32 sum")
    _same(y16, to_bits(y, elem), "y16")
    _same(yp16, to_bits(y + tables.reshape(M, 256), elem), "position shadow")


def test_layernorm_bound(lib, elem):
    """layernorm256_kernel on 37 rows (the last block one row).  DERIVED bound: layernorm_bound with the kernel's chain; the 16-bit copy is the
    kernel's own fp32 output rounded once, bit for bit."""
    rows = 37
    rng = np.random.default_rng(2)
    x = (rng.standard_normal((rows, 256)) * 3 + 0.7).astype(f32)
    g = rng.uniform(0.8, 1.2, 256).astype(f32)
    b = (rng.standard_normal(256) * 0.05).astype(f32)
    y = np.full((rows, 256), np.nan, f32)
    y16 = np.full((rows, 256), 0xFFFF, np.uint16)
    _capi.check(lib.opd_test_layernorm(_p(x), _p(g), _p(b), _p(y), _p(y16), rows), "opd_test_layernorm")
    assert _ratio("layernorm y32", elem, np.abs(y - E.layernorm64(x, g, b)), E.layernorm_bound(x, g, b, depth=10)) <= 1
    _same(y16, to_bits(y, elem), "y16 against the kernel's own y, rounded once")


def test_preprocess_bound(lib, elem):
    """preprocess_u8_kernel on a ragged batch (2, 37, 53).  DERIVED bound: the fp32 normalisation's error (preprocess_e) and one rounding;
    outside a frame's valid rectangle, in the border and in the fourth channel: zero bits."""
    B, H, W = 2, 37, 53
    rng = np.random.default_rng(77)
    frames = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    frames[0, :3, :3] = 255
    frames[0, 3:6, :3] = 0
    valid = np.asarray([[37, 53], [29, 41]], np.int32)
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    Hp, Wp = 2 * OH + 6, 2 * OW + 6
    out = np.full((B, Hp, Wp, 4), 0xFFFF, np.uint16)
    _capi.check(lib.opd_test_preprocess_u8(_p(frames), _p(out), B, H, W, Hp, Wp, _p(valid)), "opd_test_preprocess_u8")
    inside = np.zeros((B, Hp, Wp, 4), bool)
    for i in range(B):
        inside[i, 3:3 + valid[i, 0], 3:3 + valid[i, 1], :3] = True
    assert not out[~inside].any()
    want = np.zeros((B, Hp, Wp, 4))
    bound = np.zeros((B, Hp, Wp, 4))
    want[:, 3:3 + H, 3:3 + W, :3] = E.preprocess64(frames)
    bound[:, 3:3 + H, 3:3 + W, :3] = round_bound(E.preprocess_e(frames), E.preprocess64(frames), elem)
    assert _ratio("preprocess_u8", elem, np.abs(from_bits(out, elem) - want)[inside], bound[inside]) <= 1


@pytest.mark.parametrize("H,W", [(37, 34), (45, 51)])
def test_stem_pool_bound(lib, elem, H, W):
    """Stem conv + ReLU + 3x3 s2 max-pool in one kernel on the zero-bordered NHWC4 image.  DERIVED bound (elem_common.stem_pool_reference):
    conv_e with the GEMM's K = 256 and one rounding per convolution output, the largest over the pooling window."""
    rng = np.random.default_rng(H * 1000 + W)
    B = 2
    x = round_elem(rng.standard_normal((B, H, W, 3)), elem)
    w, bias = _stem_weights(rng, elem)
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    PH, PW = (OH - 1) // 2 + 1, (OW - 1) // 2 + 1
    Hp, Wp = 2 * OH + 6, 2 * OW + 6
    x4p = np.zeros((B, Hp, Wp, 4), f32)
    x4p[:, 3:3 + H, 3:3 + W, :3] = x
    out = np.full((B, PH, PW, 64), 0xFFFF, np.uint16)
    rc = lib.opd_test_stem_pool(_p(to_bits(x4p, elem)), _p(to_bits(w.reshape(64, 256), elem)), _p(bias), _p(out), B, Hp, Wp, OH, OW, PH, PW)
    _capi.check(rc, "opd_test_stem_pool")
    want, bound = E.stem_pool_reference(x, w[:, :7, :7, :3], bias, elem)
    assert want.shape == out.shape and (want > 0).mean() > 0.3
    assert _ratio(f"stem_pool ({H},{W})", elem, np.abs(from_bits(out, elem) - want), bound) <= 1


def _qkv(rng, B, Lq, Lk, elem):
    q = round_elem(rng.standard_normal((B, Lq, 256)) * 1.5, elem)
    k = round_elem(rng.standard_normal((B, Lk, 256)) * 1.5, elem)
    v = round_elem(rng.standard_normal((B, Lk, 256)), elem)
    return q, k, v


def _heads(a, B, L):
    return np.asarray(a, np.float64).reshape(B, L, 8, 32).transpose(0, 2, 1, 3)


def _key_mask(valid, key_row, Lk):
    """valid [B][2] -> [B][1][1][Lk] bool."""
    idx = np.arange(Lk)
    return np.stack([(idx // key_row < r) & (idx % key_row < c) for r, c in valid])[:, None, None, :]


def test_attention_masked_bound(lib, elem):
    """attention_kernel<MASKED> at (2, 70, 300), key rows of 42, frame 1 a quarter valid.  DERIVED bound: elem_common.attention_bound."""
    B, Lq, Lk, key_row = 2, 70, 300, 42
    q, k, v = _qkv(np.random.default_rng(21), B, Lq, Lk, elem)
    valid = np.asarray([[8, 42], [2, 30]], np.int32)
    out = np.full((B, Lq, 256), 0xFFFF, np.uint16)
    rc = lib.opd_test_attention_masked(_p(to_bits(q, elem)), _p(to_bits(k, elem)), _p(to_bits(v, elem)), _p(out), B, 8, Lq, Lk, SCALE, _p(valid), key_row)
    _capi.check(rc, "opd_test_attention_masked")
    mask = _key_mask(valid, key_row, Lk)
    qh, kh, vh = _heads(q, B, Lq), _heads(k, B, Lk), _heads(v, B, Lk)
    _, want = E.attention64(qh, kh, vh, SCALE, mask)
    bound = E.attention_bound(qh, kh, vh, SCALE, elem, mask, key_tile=128)
    got = _heads(from_bits(out, elem), B, Lq)
    assert _ratio("attention_masked", elem, np.abs(got - want), bound) <= 1


@pytest.mark.parametrize("B,Lq,Lk,splits", [(2, 70, 300, 2), (1, 100, 100, 3)])
def test_attention_split_bound(lib, elem, B, Lq, Lk, splits):
    """attention_kernel<SPLIT>: fp32 partials per key range, combined as dec_cross_out_kernel combines them (in float64 here); the second case
    has empty ranges.  DERIVED bound: attention_bound without the output rounding."""
    q, k, v = _qkv(np.random.default_rng(Lk + splits), B, Lq, Lk, elem)
    M = B * Lq
    part_o = np.full((splits, M, 256), np.nan, f32)
    part_ml = np.full((splits, M, 8, 2), np.nan, f32)
    rc = lib.opd_test_attention_split(_p(to_bits(q, elem)), _p(to_bits(k, elem)), _p(to_bits(v, elem)), B, 8, Lq, Lk, SCALE, splits, None, 0, _p(part_o), _p(part_ml))
    _capi.check(rc, "opd_test_attention_split")
    assert np.isfinite(part_o).all()
    m, l = part_ml[..., 0].astype(np.float64), part_ml[..., 1].astype(np.float64)
    if Lk <= 128 * (splits - 1):
        assert np.isinf(m[-1]).all() and not l[-1].any() and not part_o[-1].any()      # an empty range carries no weight
    wgt = np.where(np.isinf(m), 0.0, np.exp2(m - m.max(axis=0, keepdims=True)))
    O = (np.repeat(wgt, 32, axis=2) * part_o.astype(np.float64)).sum(axis=0) / np.repeat((wgt * l).sum(axis=0), 32, axis=1)
    qh, kh, vh = _heads(q, B, Lq), _heads(k, B, Lk), _heads(v, B, Lk)
    _, want = E.attention64(qh, kh, vh, SCALE)
    bound = E.attention_bound(qh, kh, vh, SCALE, elem, key_tile=128, out16=False)
    assert _ratio(f"attention_split ({Lq},{Lk},{splits})", elem, np.abs(_heads(O, B, Lq) - want), bound) <= 1


@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "masked"])
@pytest.mark.parametrize("sel", [[7], [3, 0, 17, 9, 33]], ids=["nsel1", "nsel5"])
def test_attention_map_bound(lib, elem, sel, masked):
    """attn_map_*_kernel: the mean over heads and selected queries of softmax(q k^T scale), fp32 arithmetic on 16-bit q / k; k with the row
    stride of the decoder's [k | v] memory.  DERIVED bound: elem_common.attention_map64."""
    heads, Lk, key_row, ldk = 8, 300, 20, 512
    rng = np.random.default_rng(5 + len(sel))
    q = round_elem(rng.standard_normal((40, 256)) * 1.5, elem)
    kv = round_elem(rng.standard_normal((Lk, ldk)) * 1.5, elem)
    valid = np.asarray([9, 13], np.int32) if masked else None
    scale = float(f32(SCALE))
    out = np.full(Lk, np.nan, f32)
    s = np.asarray(sel, np.int32)
    rc = lib.opd_test_attention_map(_p(to_bits(q, elem)), 256, _p(to_bits(kv, elem)), ldk, _p(s), len(sel), heads, Lk, scale, _p(valid), key_row, _p(out))
    _capi.check(rc, "opd_test_attention_map")
    want, bound = E.attention_map64(q, kv[:, :256], sel, heads, scale, valid, key_row)
    assert abs(float(out.sum()) - 1) < 1e-4
    if masked:
        assert not out[want == 0].any()
    assert _ratio(f"attention_map nsel={len(sel)} masked={masked}", elem, np.abs(out - want), bound) <= 1


def test_dec_self_query_store(lib, elem):
    """dec_self_kernel at (2, 36): its cross-attention query is stored in the handle's element type (DecSelfParams::qc_bf16).  The kernel's
    operands are fp16 whatever the element type; h against float64 at the EXISTING tolerance of test_decoder_gpu.py (2.5e-3: P in fp16), the
    query against round_bound(2e-6, want, elem) from the kernel's own h, that test's construction."""
    def k_frag(k, pad):   # [B][Q][256] -> [B][8 heads][8 key tiles][64 lanes][8], the order dec_qkv_kernel writes (tests/test_decoder_gpu.py)
        kp = np.full((k.shape[0], 128, 256), pad, np.float64)
        kp[:, :k.shape[1]] = k
        return kp.reshape(-1, 8, 16, 8, 4, 8).transpose(0, 3, 1, 4, 2, 5).reshape(-1, 8, 8, 64, 8)

    def v_frag(v, pad):   # [B][Q][256] -> [B][8 heads][4 kb][2 dt][64 lanes][8]
        vp = np.full((v.shape[0], 128, 256), pad, np.float64)
        vp[:, :v.shape[1]] = v
        return vp.reshape(-1, 4, 2, 4, 4, 8, 2, 16).transpose(0, 5, 1, 6, 3, 7, 2, 4).reshape(-1, 8, 4, 2, 64, 8)

    B, Q, D = 2, 36, 256
    M = B * Q
    rng = np.random.default_rng(B * 77 + Q)
    h16 = lambda a: np.ascontiguousarray(np.asarray(a, f32).astype(np.float16).view(np.uint16))
    q = (rng.standard_normal((B, Q, D)) * 1.5).astype(f32)
    k_r = (rng.standard_normal((B, Q, D)) * 1.5).astype(np.float16).astype(np.float64)
    v_r = rng.standard_normal((B, Q, D)).astype(np.float16).astype(np.float64)
    q16 = h16(q.reshape(M, D))
    k16 = h16(k_frag(k_r, np.nan))
    vT = h16(v_frag(v_r, np.nan))
    h = rng.standard_normal((M, D)).astype(f32)
    wo = (rng.standard_normal((D, D)) / 16).astype(f32)
    bo = (rng.standard_normal(D) * 0.1).astype(f32)
    g = (1.0 + 0.1 * rng.standard_normal(D)).astype(f32)
    be = (0.1 * rng.standard_normal(D)).astype(f32)
    wq = (rng.standard_normal((D, D)) / 16).astype(f32)
    rbq = (rng.standard_normal((Q, D)) * 0.5).astype(f32)
    h_io = h.copy()
    qc16 = np.full((M, D), 0xFFFF, np.uint16)
    rc = lib.opd_test_dec_self(_p(q16), _p(k16), _p(vT), _p(h_io), _p(wo), _p(bo), _p(g), _p(be), _p(wq), _p(rbq), B, Q, SCALE, _p(qc16))
    _capi.check(rc, "opd_test_dec_self")
    qh = _heads(q16.view(np.float16), B, Q)
    _, o = E.attention64(qh, _heads(k_r, B, Q), _heads(v_r, B, Q), SCALE)
    o = o.transpose(0, 2, 1, 3).reshape(M, D)
    h1 = E.layernorm64(h.astype(np.float64) + o @ wo.astype(np.float64).T + bo, g, be)
    np.testing.assert_allclose(h_io, h1, atol=2.5e-3)
    want = (h_io.astype(np.float64) @ wq.astype(np.float64).T).reshape(B, Q, D) + rbq[None]
    want = want.reshape(M, D)
    assert _ratio("dec_self qc16", elem, np.abs(from_bits(qc16, elem) - want), round_bound(2e-6, want, elem)) <= 1
