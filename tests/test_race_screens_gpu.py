"""Race screens (GPU): every kernel that orders LDS-DMA traffic by hand-counted ``s_waitcnt vmcnt(N)`` and raw ``s_barrier`` is launched
40 times on the same device-resident operands while a second stream copies 256 MiB per repetition, and every output of its hook must come
out with the same bits each time (csrc/opd_test_util.h: launch_repeated; the outputs are refilled and the in-place buffers restored before
every repetition).  A count that is one too permissive passes every reference check as long as the data happens to land in time; it shows
here as a repetition that differs.  tools/scan_dma_waits.py and tests/test_isa_cpu.py catch a wait that counts the wrong KIND of request
statically; a count that is simply too small only shows dynamically.

Section 1 tests the screen itself: a screen that cannot see a difference is worse than none.

Section 2 holds the screens.  Each case sets the repeat count, runs ONE hook call through the body of the kernel's existing test (or the
case builder that test uses), asserts ``launches == 40`` and ``n_diff == 0``, and thereby also that existing test's reference bound on the
last repetition's outputs: no tolerance is introduced here.  Shapes: the kernel's model shape at batch 8 where that is small (a race needs
the machine filled and memory busy, not large data), and one ragged shape.  Kernel files that are built for both element types run both;
the bf16 leg takes the bound of the kernel's both-type test in tests/test_bf16_kernels_gpu.py or tests/test_bf16_gpu.py, and where there is
none for the form under test it asserts bit identity (and finite outputs) only -- the docstring says so.  The decoder kernels and the heads
are built once.

Kernels with a screen elsewhere: the fused tails (test_kernels_gpu.py::test_btail_repeated_launches_are_bit_identical), the eight-wave conv
(test_kernels_gpu.py::test_conv_w8_repeated_launches_are_bit_identical) and enc_ffn_kernel (test_kernels_gpu.py::
test_enc_ffn_is_reproducible_under_load), all through the same helper.  None of the listed kernels is non-deterministic by design: no
floating-point atomic occurs in kernels_dec / rowln / attn / gemm / w8 / btail*.hip."""

import ctypes as C
import faulthandler

import numpy as np
import pytest

import elem_common as E
import test_bf16_gpu as T16
import test_bf16_kernels_gpu as TB
import test_decoder_gpu as TD
import test_gemm_options_gpu as TG
import test_kernels_gpu as TK
import test_stem_reduce_gpu as TS
from arch_common import RACE_REPS, _p, race_screened, repeat_result
from elem_common import from_bits, to_bits
from office_person_detection_vit_amd import _capi

pytestmark = pytest.mark.gpu

f32 = np.float32
SCALE = 32 ** -0.5


@pytest.fixture(autouse=True)
def _time_limit():
    """Every test runs under its own limit: a hang ends the process (with a traceback) instead of holding the GPU."""
    faulthandler.dump_traceback_later(120, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


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
    lib.opd_test_set_repeat(0)
    lib.opd_test_set_elem_bf16(0)
    lib.opd_test_set_conv_flags(0)
    lib.opd_test_set_gemm_ln_kloop(0)
    lib.opd_test_set_encffn_wprefetch(0)
    lib.opd_test_set_pos_frames(0)


# ================================================================ 1. the screen itself ================================================================
ALL_BLOCKS = 3 * 64 * 256 * 4 + 4096 + 8   # more than 64 blocks x 256 threads x 4 bytes: every checksum block has work, the last pass is partial


def _selftest(lib, mode, nbytes):
    n_diff = C.c_int(-1)
    rc = lib.opd_test_repeat_selftest(mode, nbytes, C.byref(n_diff))
    return rc, n_diff.value


@pytest.mark.parametrize("nbytes", [4096, ALL_BLOCKS])
@pytest.mark.parametrize("mode,want", [(0, 0), (1, 1), (2, 1), (3, 2), (4, 0), (5, RACE_REPS - 1)],
                         ids=["same", "last_16_bits_of_rep7", "rep3_writes_nothing", "reps5_6_swap_two_words", "in_place_restored", "in_place_not_restored"])
def test_screen_counts_exactly_the_repetitions_that_differ(lib, mode, want, nbytes):
    """launch_repeated on a pattern written by plain copies (opd_test_repeat_selftest): identical repetitions count 0; one repetition that
    differs in the buffer's last 16-bit value counts 1; one that writes nothing counts 1 (the 0xff refill survives); two that swap two words
    of one checksum slot count 2 (the sum is position-weighted); an in-place buffer that every launch advances counts 0 only because it is
    restored -- without the restore every later repetition differs (mode 4 checks that inside the hook as well, mode 5 reports it)."""
    lib.opd_test_set_repeat(RACE_REPS)
    rc, n_diff = _selftest(lib, mode, nbytes)
    _capi.check(rc, "opd_test_repeat_selftest")
    assert n_diff == want
    launches, again = repeat_result(lib)
    assert launches == RACE_REPS and again == n_diff
    assert repeat_result(lib) == (0, 0)   # the read clears the record


def test_screen_refuses_a_buffer_it_would_cover_only_partly(lib):
    """The checksum sums whole 32-bit words: 4098 bytes would leave two bytes unseen."""
    lib.opd_test_set_repeat(RACE_REPS)
    rc, _ = _selftest(lib, 0, 4098)
    assert rc != 0 and "multiple of 4" in _capi.last_error()
    assert repeat_result(lib) == (0, 0)


def test_repeat_off_is_one_launch_and_other_hooks_report_none(lib):
    """With the repeat count off a converted hook is exactly one launch; a hook that does not launch through the helper (opd_test_maxpool)
    reports no launch at all, also with the count set, so that a screen cannot pass on a hook that was never converted."""
    TK.test_gemm_k256_integer_exact(lib)
    assert repeat_result(lib) == (1, 0)
    lib.opd_test_set_repeat(RACE_REPS)
    TK.test_gemm_k256_integer_exact(lib)
    assert repeat_result(lib) == (RACE_REPS, 0)
    TK.test_maxpool_exact(lib)
    assert repeat_result(lib) == (0, 0)
    with pytest.raises(AssertionError, match="0 launches"):
        race_screened(lib, TK.test_maxpool_exact, lib)


# ================================================================ 2. the screens ======================================================================
# ---- kernels_dec.hip (built once): weight ring with wait counts computed at run time, raw barriers throughout ----------------------------------------
@pytest.mark.parametrize("B,Q,with_partials", [(8, 100, True), (3, 116, False)], ids=["model_16slab_prologue", "ragged_plain"])
def test_dec_qkv_screen(lib, B, Q, with_partials):
    """dec_qkv_kernel; bounds of test_decoder_gpu.py::test_dec_qkv_kernel (incl. the zero fill of the padding keys, which the helper refills
    with zeros; without the prologue h_out is read by the launch and restored)."""
    race_screened(lib, TD.test_dec_qkv_kernel, lib, B, Q, with_partials)


@pytest.mark.parametrize("B,Q", [(8, 100), (2, 116)], ids=["model", "ragged"])
def test_dec_self_screen(lib, B, Q):
    """dec_self_kernel, in place on h (restored before every repetition); bounds of test_decoder_gpu.py::test_dec_self_kernel."""
    race_screened(lib, TD.test_dec_self_kernel, lib, B, Q)


def test_dec_self_bf16_query_store_screen(lib):
    """dec_self_kernel with DecSelfParams::qc_bf16 at the shape and bounds of test_bf16_kernels_gpu.py::test_dec_self_query_store."""
    lib.opd_test_set_elem_bf16(1)
    race_screened(lib, TB.test_dec_self_query_store, lib, "bf16")


@pytest.mark.parametrize("M,splits,period", [(800, 3, 0), (800, 3, 1), (36, 4, 0)], ids=["model", "model_constant_residual", "ragged"])
def test_dec_cross_out_screen(lib, M, splits, period):
    """dec_cross_out_kernel; bounds of test_decoder_gpu.py::test_dec_cross_out_kernel."""
    race_screened(lib, TD.test_dec_cross_out_kernel, lib, M, splits, period)


@pytest.mark.parametrize("M,Fh", [(800, 2048), (37, 256)], ids=["model", "ragged"])
def test_dec_ffn_screen(lib, M, Fh):
    """dec_ffn_kernel; bounds of test_decoder_gpu.py::test_dec_ffn_kernel."""
    race_screened(lib, TD.test_dec_ffn_kernel, lib, M, Fh)


@pytest.mark.parametrize("split", [1, 0], ids=["heads2_kernel", "heads_kernel"])
def test_heads_screen(lib, split):
    """heads2_kernel / heads_kernel at rows = 800 with the FFN prologue (bounds of test_decoder_gpu.py::test_heads_kernel_with_ffn_prologue)
    and at rows = 37, 92 classes (bounds of test_kernels_gpu.py::test_heads_kernel_matches_torch)."""
    race_screened(lib, TD.test_heads_kernel_with_ffn_prologue, lib, split)
    race_screened(lib, TK.test_heads_kernel_matches_torch, lib, 37, True, split)


# ---- kernels_rowln.hip (both element types) ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,K,period,in_place,ln", [(8400, 2048, 1050, True, True), (8400, 2048, 0, False, False), (333, 128, 111, True, True)],
                         ids=["model_in_place_ln", "model_plain", "ragged_in_place_ln"])
def test_gemm_ln_deep_screen(lib, elem, M, K, period, in_place, ln):
    """gemm_ln256_ring_kernel (three-stage ring, vmcnt(PIECES), one raw barrier per k-step), both LN forms, in place on the residual stream
    (restored before every repetition) and not.  fp16: bounds of test_kernels_gpu.py::test_gemm_ln_deep_matches_torch; bf16: the derived
    bound of test_bf16_kernels_gpu.py::test_gemm_ln_deep_bound."""
    if elem == "fp16":
        race_screened(lib, TK.test_gemm_ln_deep_matches_torch, lib, M, K, period, in_place, ln)
    else:
        race_screened(lib, TB.test_gemm_ln_deep_bound, lib, elem, M, K, period, in_place, ln)


@pytest.mark.parametrize("variant", [1, 0], ids=["oneshot_k256", "kloop"])
@pytest.mark.parametrize("M,K", [(8400, 256), (97, 256)], ids=["model", "ragged"])
def test_gemm_ln_screen(lib, elem, M, K, variant):
    """gemm_ln256_os_kernel (one batch of LDS-DMA) and gemm_ln256_kernel (double buffer), both behind OPD_DMA_BARRIER.  fp16: bounds of
    test_kernels_gpu.py::test_gemm_ln_matches_torch; bf16: the derived bound of test_bf16_kernels_gpu.py::test_gemm_ln_bound."""
    if elem == "fp16":
        race_screened(lib, TK.test_gemm_ln_matches_torch, lib, M, K, True, variant)
    else:
        race_screened(lib, TB.test_gemm_ln_bound, lib, elem, M, K, variant)


def _gemm_k256_bits(lib, elem, M, N, K, period):
    rng = np.random.default_rng(M + N + K)
    x = E.round_elem(rng.standard_normal((M, K)), elem)
    w = E.round_elem(rng.standard_normal((N, K)) / np.sqrt(K), elem)
    bias = np.ascontiguousarray((rng.standard_normal((max(period, 1), N)) * 0.1).astype(f32))
    out16 = np.full((M, N), 0xFFFF, np.uint16)
    out32 = np.full((M, N), np.nan, f32)
    _capi.check(lib.opd_test_gemm_k256(_p(to_bits(x, elem)), _p(to_bits(w, elem)), _p(bias), _p(out16), _p(out32), M, N, K, period, 0), "opd_test_gemm_k256")
    return out32 if K > 256 else from_bits(out16, elem)


@pytest.mark.parametrize("M,N,K,period", [(800, 768, 256, 100), (800, 256, 2048, 0), (37, 64, 256, 0)], ids=["model_qkv", "eight_slices_reduce", "ragged"])
def test_gemm_k256_screen(lib, elem, M, N, K, period):
    """gemm_k256_kernel, one slice and eight slices + reduce (the slabs and the sum are all compared).  fp16: bounds of
    test_kernels_gpu.py::test_gemm_k256_matches_torch.  bf16: the kernel's both-type test (test_gemm_k256_exact) is an exact-arithmetic
    case of one fixed shape, so this leg asserts bit identity of the repetitions and finite, non-trivial outputs only."""
    if elem == "fp16":
        race_screened(lib, TK.test_gemm_k256_matches_torch, lib, M, N, K, period, False)
    else:
        got = race_screened(lib, _gemm_k256_bits, lib, elem, M, N, K, period)
        assert np.isfinite(got).all() and np.abs(got).max() > 0.5


# ---- kernels_attn.hip (both element types): double-buffered K / V tiles by LDS-DMA ---------------------------------------------------------------------
@pytest.mark.parametrize("B,Lq,Lk", [(8, 1050, 1050), (3, 197, 333)], ids=["encoder_self", "ragged"])
def test_attention_screen(lib, elem, B, Lq, Lk):
    """attention_kernel, unmasked.  fp16: bounds of test_kernels_gpu.py::test_attention_matches_torch; bf16: the bound of
    test_bf16_gpu.py::test_attention_bf16."""
    if elem == "fp16":
        race_screened(lib, TK.test_attention_matches_torch, lib, (B, Lq, Lk))
    else:
        race_screened(lib, T16.test_attention_bf16, lib, B, Lq, Lk)


def _attention_masked(lib, elem, B, Lq, Lk, key_row, valid):
    """The body of test_bf16_kernels_gpu.py::test_attention_masked_bound at another shape; returns (err, bound)."""
    q, k, v = TB._qkv(np.random.default_rng(21), B, Lq, Lk, elem)
    out = np.full((B, Lq, 256), 0xFFFF, np.uint16)
    rc = lib.opd_test_attention_masked(_p(to_bits(q, elem)), _p(to_bits(k, elem)), _p(to_bits(v, elem)), _p(out), B, 8, Lq, Lk, SCALE, _p(valid), key_row)
    _capi.check(rc, "opd_test_attention_masked")
    mask = TB._key_mask(valid, key_row, Lk)
    qh, kh, vh = TB._heads(q, B, Lq), TB._heads(k, B, Lk), TB._heads(v, B, Lk)
    _, want = E.attention64(qh, kh, vh, SCALE, mask)
    return np.abs(TB._heads(from_bits(out, elem), B, Lq) - want), E.attention_bound(qh, kh, vh, SCALE, elem, mask, key_tile=128)


@pytest.mark.parametrize("B,Lq,Lk,key_row,valid", [(2, 1050, 1050, 42, [[25, 42], [17, 30]]), (3, 70, 300, 42, [[8, 42], [2, 30], [1, 1]])],
                         ids=["encoder_ragged_mask", "ragged"])
def test_attention_masked_screen(lib, elem, B, Lq, Lk, key_row, valid):
    """attention_kernel<MASKED> with a ragged key mask (a frame that fills part of the map; a frame with one valid key), both element types:
    the derived bound of test_bf16_kernels_gpu.py::test_attention_masked_bound (elem_common.attention_bound) on these shapes."""
    err, bound = race_screened(lib, _attention_masked, lib, elem, B, Lq, Lk, key_row, np.asarray(valid, np.int32))
    assert TB._ratio(f"attention_masked ({B},{Lq},{Lk})", elem, err, bound) <= 1


def _attention_split_finite(lib, elem, B, Lq, Lk, splits, masked):
    q, k, v = TB._qkv(np.random.default_rng(Lk + splits), B, Lq, Lk, elem)
    key_row = 42
    rows = (Lk + key_row - 1) // key_row
    valid = np.asarray([[rows, key_row]] + [[max(1, rows // 4), 30]] * (B - 1), np.int32) if masked else None   # as arch_common.attention_split_case
    part_o = np.full((splits, B * Lq, 256), np.nan, f32)
    part_ml = np.full((splits, B * Lq, 8, 2), np.nan, f32)
    rc = lib.opd_test_attention_split(_p(to_bits(q, elem)), _p(to_bits(k, elem)), _p(to_bits(v, elem)), B, 8, Lq, Lk, SCALE, splits, _p(valid),
                                      key_row if masked else 0, _p(part_o), _p(part_ml))
    _capi.check(rc, "opd_test_attention_split")
    return part_o, part_ml


@pytest.mark.parametrize("B,Lq,Lk,splits,masked", [(8, 100, 1050, 3, False), (8, 100, 1050, 3, True), (3, 4, 20, 3, False)],
                         ids=["decoder_cross", "decoder_cross_masked", "more_splits_than_key_tiles"])
def test_attention_split_screen(lib, elem, B, Lq, Lk, splits, masked):
    """attention_kernel<SPLIT> (KT = 128, fp32 partials).  fp16: bounds of test_decoder_gpu.py::test_attention_key_split_partials.  bf16,
    unmasked: the derived bound of test_bf16_kernels_gpu.py::test_attention_split_bound; bf16 with a key mask has no both-type test: bit
    identity of the repetitions and finite partial sums only."""
    if elem == "fp16":
        race_screened(lib, TD.test_attention_key_split_partials, lib, B, Lq, Lk, splits, masked)
    elif not masked:
        race_screened(lib, TB.test_attention_split_bound, lib, elem, B, Lq, Lk, splits)
    else:
        part_o, part_ml = race_screened(lib, _attention_split_finite, lib, elem, B, Lq, Lk, splits, masked)
        assert np.isfinite(part_o).all() and np.isfinite(part_ml[..., 1]).all() and np.abs(part_o).max() > 0.5


# ---- kernels_gemm.hip (both element types): conv_gemm_dma_kernel and the fused stem ----------------------------------------------------------------------
POINTWISE = (8, 25, 42, 256, 768, 1, 1, False, False)   # the encoder's q | k | v projection: M = 8400, N = 768, K = 256 (the PW form)
CONV3X3 = (2, 25, 42, 512, 512, 3, 1, True, False)       # stage 4's 3x3 at batch 2
RAGGED_PW = (1, 17, 21, 256, 512, 1, 2, False, False)    # 99 rows, strided (CONV_CASES of test_kernels_gpu.py)


@pytest.mark.parametrize("flags", [0, 0x400, 0x500, 0x600, 0x20], ids=["auto_tiles", "128rows", "160rows", "192rows", "flat_staging"])
@pytest.mark.parametrize("case", [POINTWISE, CONV3X3, RAGGED_PW], ids=["pointwise_qkv", "3x3", "ragged_pointwise"])
def test_conv_gemm_screen(lib, elem, case, flags):
    """conv_gemm_dma_kernel: the pointwise and the 3x3 form, each at the dispatcher's own tile height, at every forced height and with flat
    staging.  fp16: bounds of test_kernels_gpu.py::test_conv_gemm_matches_torch; bf16: bounds of test_bf16_gpu.py::test_conv_gemm_bf16."""
    B, H, W, Cin, N, k, stride, relu, res = case
    lib.opd_test_set_conv_flags(flags)
    if elem == "fp16":
        race_screened(lib, TK.test_conv_gemm_matches_torch, lib, flags, case)
    else:
        race_screened(lib, T16.test_conv_gemm_bf16, lib, B, H, W, Cin, N, k, stride, relu, res)


@pytest.mark.parametrize("B,H,W,Cin,N,Cin2,stride2", [(1, 25, 42, 512, 2048, 1024, 2), (2, 13, 11, 256, 1024, 512, 2)], ids=["stage4", "ragged"])
def test_conv_dual_source_screen(lib, B, H, W, Cin, N, Cin2, stride2):
    """conv_gemm_dma_kernel, dual-source form, fp16: bounds of test_kernels_gpu.py::test_conv_dual_source_matches_torch."""
    race_screened(lib, TK.test_conv_dual_source_matches_torch, lib, B, H, W, Cin, N, Cin2, stride2)


def test_conv_dual_source_screen_both_types(lib, elem):
    """... and for both element types the exact-arithmetic case of test_bf16_kernels_gpu.py::test_conv_dual_source_exact."""
    race_screened(lib, TB.test_conv_dual_source_exact, lib, elem)


@pytest.mark.parametrize("case", [TG.SPLITK_CASES[4], TG.SPLITK_CASES[0]], ids=["stage4_128col", "ragged"])
def test_conv_splitk_screen(lib, case):
    """conv_gemm_dma_kernel with split-K + reduce_act16 (slabs and output both compared), fp16, launched with the weight warm-up as in the
    model: bounds of test_gemm_options_gpu.py::test_conv_splitk_matches_torch."""
    race_screened(lib, TG.test_conv_splitk_matches_torch, lib, case, True)


def _splitk_exact(lib, elem):
    """The first half of test_bf16_kernels_gpu.py::test_conv_splitk_exact_and_equals_unsplit (that test calls a second hook afterwards)."""
    B, H, W, Cin, N, k, stride, splits = E.SPLITK_CASE
    d = E.splitk_recipe()
    want = TB._exact(d["y"].reshape(-1, N), elem)
    out = np.full((B * H * W, N), 0xFFFF, np.uint16)
    rc = lib.opd_test_conv_splitk(_p(to_bits(d["x"], elem)), _p(to_bits(d["w"], elem)), _p(TB._c32(d["bias"])), _p(out), B, H, W, Cin, H, W, N, k, k, stride, k // 2, 1,
                                  splits)
    _capi.check(rc, "opd_test_conv_splitk")
    TB._same(out, want, "split-K against the exact sums")


def test_conv_splitk_screen_both_types(lib, elem):
    """... and for both element types the exact sums of test_bf16_kernels_gpu.py::test_conv_splitk_exact_and_equals_unsplit."""
    race_screened(lib, _splitk_exact, lib, elem)


def test_stem_pool_u8_screen(lib, elem):
    """stem_pool2_kernel<U8> against preprocess_u8_kernel -> stem_pool2_kernel on a ragged batch at (3, 97, 131); both pooled maps are compared
    across the repetitions.  fp16: test_kernels_gpu.py::test_stem_pool_with_preprocessing_inside_is_bit_identical; bf16: the bit identity and
    the derived bound of test_bf16_kernels_gpu.py::test_stem_pool_with_preprocessing_inside_equals_split (its second hook, preprocess_u8,
    does not launch through the helper and leaves the record alone)."""
    if elem == "fp16":
        race_screened(lib, TK.test_stem_pool_with_preprocessing_inside_is_bit_identical, lib, 3, 97, 131, True)
    else:
        race_screened(lib, TB.test_stem_pool_with_preprocessing_inside_equals_split, lib, elem, 3, 97, 131, [[97, 131], [84, 102], [49, 45]])


@pytest.mark.parametrize("u8", [1, 0], ids=["uint8_frames", "fp16_image"])
@pytest.mark.parametrize("B,H,W,valid", [TS.STEM_CASES[1], TS.STEM_CASES[2]], ids=["pipelined_gemm", "ragged"])
def test_stem_reduce_screen(lib, elem, B, H, W, valid, u8):
    """stem_pool2_kernel with StemReduce (stage 1's first reduce inside), all four maps compared across the repetitions: the bit identities of
    test_stem_reduce_gpu.py::test_stem_with_first_reduce_inside_is_bit_identical at its shapes."""
    race_screened(lib, TS.test_stem_with_first_reduce_inside_is_bit_identical, lib, elem, B, H, W, valid, u8)
