"""Kernel-level parity of the FUSED DECODER (csrc/kernels_dec.hip, the key-split form of csrc/kernels_attn.hip, the heads kernel's
FFN prologue) against float64 torch on identical inputs, through the test hooks of libopd_hip_test.so.

The decoder's linear layers run on SPLIT fp16 operands (x = hi + lo / 2048, three MFMAs per product, fp32 accumulate): the weights
and the GEMM inputs here are ordinary fp32 values — NOT fp16-representable — and the tolerances are fp32-grade (1e-5 on O(1) outputs),
which a single-fp16-operand GEMM misses by two orders of magnitude.  Attention scores / P.V use single fp16 operands (q, k, v are stored as
fp16): those tests compare on the fp16-rounded q / k / v.  Follows HF:models/detr/modeling_detr.py:650-739 (decoder layer)."""

import numpy as np
import pytest

from office_person_detection_vit_amd import _capi

from arch_common import (_from16, _ulp16, attention_split_case, dec_cross_out_case, dec_ffn_case, dec_qkv_case, dec_self_case, heads_fused_case,
                         k_frag, v_frag)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return _capi.load_library()


@pytest.mark.parametrize("B,Q,with_partials", [(8, 100, True), (2, 100, False), (1, 100, True), (3, 40, True)])
def test_dec_qkv_kernel(lib, B, Q, with_partials):
    """[h = LN3(h_in + b2 + sum of 16 partial slabs)] ; q | k | v = h . Wqkv^T + bias[row mod Q]; v written transposed per (frame, head)."""
    c = dec_qkv_case(lib, B, Q, with_partials)
    M, qkv, q16, k16, vT = B * Q, c["want_qkv"], c["q16"], c["k16"], c["vT"]
    if with_partials:
        np.testing.assert_allclose(c["h_out"], c["want_h"], atol=3e-6, rtol=2e-6)
    ulp = _ulp16   # one fp16 output rounding
    want_q = qkv[..., :256].reshape(M, 256)
    assert np.all(np.abs(_from16(q16) - want_q) <= 0.51 * ulp(want_q) + 2e-6)
    # k and v arrive in MFMA-fragment order; padding keys are never written (the hook zero-fills the buffers)
    for got, want in ((_from16(k16), k_frag(qkv[..., 256:512])), (_from16(vT), v_frag(qkv[..., 512:]))):
        assert np.all(np.abs(got - want) <= 0.51 * ulp(want) + 2e-6)
    valid = k_frag(np.ones((B, Q, 256)))
    assert not _from16(k16)[valid == 0].any() and not _from16(vT)[v_frag(np.ones((B, Q, 256))) == 0].any()


@pytest.mark.parametrize("B,Q", [(8, 100), (1, 100), (2, 36)])
def test_dec_self_kernel(lib, B, Q):
    """Self-attention of every (frame, 16-query slab) with wave = head, o-proj + residual + LayerNorm, then the cross-attention query
    projection; q / k / v are the fp16 operands dec_qkv_kernel writes (garbage in v^T's padding keys must not matter)."""
    c = dec_self_case(lib, B, Q)
    _capi.check(c["rc"], "opd_test_dec_self")
    # P is rounded to fp16 before P.V (relative 2^-11 per weight, averaged over the keys): 2e-3 on O(1) rows after the LayerNorm's gain
    np.testing.assert_allclose(c["h"], c["want_h"], atol=2.5e-3)
    want = c["want_qc"]
    assert np.all(np.abs(_from16(c["qc16"]) - want) <= 0.51 * _ulp16(want) + 2e-6)


@pytest.mark.parametrize("B,Lq,Lk,splits,masked", [(8, 100, 1050, 3, False), (2, 100, 1050, 3, True), (1, 100, 100, 3, False), (2, 70, 300, 2, False),
                                                  (1, 100, 2040, 3, False), (2, 100, 1050, 4, True)])
def test_attention_key_split_partials(lib, B, Lq, Lk, splits, masked):
    """attention_kernel<SPLIT>: each key range's unnormalised sum_k p v, exponent reference and sum_k p; combined like
    dec_cross_out_kernel does they give softmax(Q K^T) V.  Incl. more splits than key tiles (an empty range carries zero weight)
    and, with a key mask, a range whose keys are all masked."""
    O, want, part_o = attention_split_case(lib, B, Lq, Lk, splits, masked)
    np.testing.assert_allclose(O, want, atol=2e-3)               # P in fp16
    assert np.isfinite(part_o).all()


@pytest.mark.parametrize("M,splits,period", [(800, 3, 0), (800, 3, 1), (100, 2, 0), (36, 4, 0)])
def test_dec_cross_out_kernel(lib, M, splits, period):
    """Combine the key splits (incl. a split that carries no weight), o-proj + residual + LayerNorm; residual rows either per row or
    one constant row (layer 0's state)."""
    h, want, o = dec_cross_out_case(lib, M, splits, period)
    err = np.abs(h - want)
    bad = np.argwhere(err > 1e-5 + 1e-5 * np.abs(want))
    if len(bad):   # diagnostics: which rows / columns, how large the combined attention output is there
        rows = sorted(set(int(b[0]) for b in bad))
        print("violating rows", rows[:20], "cols", sorted(set(int(b[1]) for b in bad))[:20], "max err", err.max(),
              "max|o| in those rows", [float(np.abs(o[r_]).max()) for r_ in rows[:8]], "max|o| overall", float(np.abs(o).max()))
    np.testing.assert_allclose(h, want, atol=1e-5, rtol=1e-5)


@pytest.mark.parametrize("M,Fh", [(800, 2048), (100, 2048), (37, 256)])
def test_dec_ffn_kernel(lib, M, Fh):
    """relu(h . W1^T + b1) . W2^T as F / 128 partial slabs over 64-row slabs: the slabs' sum against float64, fp32-grade."""
    parts, want, c, want_c = dec_ffn_case(lib, M, Fh)
    np.testing.assert_allclose(parts.astype(np.float64).sum(axis=0), want, atol=2e-5, rtol=1e-5)
    np.testing.assert_allclose(parts[c], want_c, atol=1e-5, rtol=1e-5)   # one slab on its own


@pytest.mark.parametrize("split", [1, 0])
def test_heads_kernel_with_ffn_prologue(lib, split):
    """The heads fed by the fused decoder: rows = LN3(hs + b2 + sum of the FFN's partial slabs), final LayerNorm, heads; through
    heads2_kernel (split fp16 operands, the model's default) and heads_kernel (fp32 matrix pipe)."""
    logits, boxes, want_logits, want_boxes = heads_fused_case(lib, split)
    np.testing.assert_allclose(logits, want_logits, atol=3e-5, rtol=1e-5)
    np.testing.assert_allclose(boxes, want_boxes, atol=2e-6)
