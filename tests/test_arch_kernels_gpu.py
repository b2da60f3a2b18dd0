"""Kernel-level parity at the LIMITS of what the loader accepts (csrc/opd_loader.cpp::infer_arch: 1 to 128 queries, 2 to 128 classifier
rows): the fused decoder's kernels, key-split attention, the heads and the post-process kernel at the query and class counts where their
padding, their ragged last tile or their per-lane class registers change shape.  tests/test_decoder_gpu.py and tests/test_kernels_gpu.py
run the same hooks at the default architecture (100 queries, 92 rows); the inputs, the float64 references and every bound are theirs
(tests/arch_common.py): no reduction length depends on the query or class count, so no bound does either."""

import numpy as np
import pytest

from office_person_detection_vit_amd import _capi
from oracle import detr_oracle as O

from arch_common import (DET, HEADS_SENTINEL, _from16, _p, _ulp16, attention_split_case, compare_records, dec_cross_out_case, dec_ffn_case,
                         dec_qkv_case, dec_self_case, heads_case, heads_fused_case, k_frag, v_frag)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return _capi.load_library()


# ---- fused decoder: one 16-query slab a quarter full (Q = 4), exactly one slab, a ragged last slab (116), no padding key at all (128) ----
@pytest.mark.parametrize("with_partials", [True, False], ids=["prologue", "plain"])
@pytest.mark.parametrize("B,Q", [(5, 4), (3, 16), (3, 116), (2, 128)])
def test_dec_qkv_kernel_at_query_limits(lib, B, Q, with_partials):
    """q | k | v within one fp16 rounding of float64 on the fp32 weights; the padding keys of k16 / vT (keys Q .. 127 of every frame and
    head) keep the hook's zero fill; at Q = 128 there is no padding position."""
    c = dec_qkv_case(lib, B, Q, with_partials)
    M, qkv = B * Q, c["want_qkv"]
    if with_partials:
        np.testing.assert_allclose(c["h_out"], c["want_h"], atol=3e-6, rtol=2e-6)
    want_q = qkv[..., :256].reshape(M, 256)
    assert np.all(np.abs(_from16(c["q16"]) - want_q) <= 0.51 * _ulp16(want_q) + 2e-6)
    for got, want in ((_from16(c["k16"]), k_frag(qkv[..., 256:512])), (_from16(c["vT"]), v_frag(qkv[..., 512:]))):
        assert np.all(np.abs(got - want) <= 0.51 * _ulp16(want) + 2e-6)
    k_valid, v_valid = k_frag(np.ones((B, Q, 256))), v_frag(np.ones((B, Q, 256)))
    assert int((k_valid == 0).sum()) == int((v_valid == 0).sum()) == B * (128 - Q) * 256
    if Q == 128:
        assert k_valid.all() and v_valid.all()
    # bit patterns, not values: a stored -0.0 would be a write too
    assert not c["k16"][k_valid == 0].any() and not c["vT"][v_valid == 0].any()


@pytest.mark.parametrize("B,Q", [(3, 4), (1, 16), (2, 116), (2, 128)])
def test_dec_self_kernel_at_query_limits(lib, B, Q):
    """124 of 128 keys padding (NaN in k and v^T there) down to none: the state after self-attention + o-proj + LayerNorm within the
    P-in-fp16 bound, the cross-attention query projection within one fp16 rounding."""
    c = dec_self_case(lib, B, Q)
    _capi.check(c["rc"], "opd_test_dec_self")
    assert c["pad_keys"] == B * (128 - Q) * 256   # (every padding key of every head holds NaN in k16; v^T likewise)
    assert np.isfinite(c["h"]).all()
    np.testing.assert_allclose(c["h"], c["want_h"], atol=2.5e-3)
    want = c["want_qc"]
    assert np.all(np.abs(_from16(c["qc16"]) - want) <= 0.51 * _ulp16(want) + 2e-6)


def test_dec_self_kernel_refuses_a_query_count_off_the_key_groups(lib):
    """Q = 102: v^T's groups of four keys would straddle the padding; the launch is refused with an error code and writes nothing."""
    fill = 0x5a5a
    c = dec_self_case(lib, 1, 102, fill=fill)
    assert c["rc"] == _capi.OPD_EHIP, (c["rc"], _capi.last_error())
    np.testing.assert_array_equal(c["h"], c["h0"])
    assert (c["qc16"] == fill).all()


@pytest.mark.parametrize("B,Lq,Lk,splits,masked", [(2, 4, 300, 2, False), (1, 128, 1050, 3, False), (2, 128, 1050, 3, True), (3, 4, 20, 3, False)])
def test_attention_key_split_partials_at_query_limits(lib, B, Lq, Lk, splits, masked):
    """Key-split attention at 4 and 128 queries; the last case has more splits than key tiles with a quarter-full query tile."""
    got, want, part_o = attention_split_case(lib, B, Lq, Lk, splits, masked)
    np.testing.assert_allclose(got, want, atol=2e-3)               # P in fp16
    assert np.isfinite(part_o).all()


@pytest.mark.parametrize("M", [4, 256])
def test_dec_cross_out_kernel_at_row_limits(lib, M):
    h, want, _ = dec_cross_out_case(lib, M, 3, 0)
    np.testing.assert_allclose(h, want, atol=1e-5, rtol=1e-5)


@pytest.mark.parametrize("M,Fh", [(4, 2048), (256, 2048)])
def test_dec_ffn_kernel_at_row_limits(lib, M, Fh):
    parts, want, c, want_c = dec_ffn_case(lib, M, Fh)
    np.testing.assert_allclose(parts.astype(np.float64).sum(axis=0), want, atol=2e-5, rtol=1e-5)
    np.testing.assert_allclose(parts[c], want_c, atol=1e-5, rtol=1e-5)


# ---- heads: the class matrix padded to 128 rows (heads2_kernel) / tiled by 16 with a ragged last tile (heads_kernel) -----------------------
SPARE = 16


def _check_heads(rows, ncls, logits, boxes, want_logits, want_boxes):
    assert logits.shape == (rows + SPARE, ncls) and boxes.shape == (rows + SPARE, 4)
    np.testing.assert_allclose(logits[:rows], want_logits, atol=2e-5, rtol=1e-5)
    np.testing.assert_allclose(boxes[:rows], want_boxes, atol=2e-6)
    # nothing past rows * ncls floats (rows * 4 for the boxes) changed
    assert (logits[rows:] == HEADS_SENTINEL).all() and (boxes[rows:] == HEADS_SENTINEL).all()


@pytest.mark.parametrize("split", [1, 0], ids=["heads2", "heads"])
@pytest.mark.parametrize("rows", [1, 37])
@pytest.mark.parametrize("ncls", [2, 3, 16, 17, 64, 65, 128])
def test_heads_kernels_at_class_limits(lib, ncls, rows, split):
    _check_heads(rows, ncls, *heads_case(lib, rows, True, split, ncls=ncls, spare=SPARE))


@pytest.mark.parametrize("rows", [1, 37])
@pytest.mark.parametrize("ncls", [129, 256])
def test_heads_kernel_above_128_classes(lib, ncls, rows):
    """heads_kernel serves up to 256 rows (the loader stops at 128, which is what the post-process kernel holds)."""
    _check_heads(rows, ncls, *heads_case(lib, rows, True, 0, ncls=ncls, spare=SPARE))


def test_heads_dispatch_leaves_heads2_above_128_classes(lib):
    """With heads2_kernel selected and 129 classes the heads hook must take heads_kernel (heads2_kernel pads the class matrix to 128
    rows): both settings of the hook then run the same kernel on the same inputs and agree bit for bit; at 128 classes they are two
    kernels with different summation orders, which is what makes the equality at 129 say something."""
    a = heads_case(lib, 37, True, 1, ncls=129, spare=SPARE)
    b = heads_case(lib, 37, True, 0, ncls=129, spare=SPARE)
    _check_heads(37, 129, *a)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    c = heads_case(lib, 37, True, 1, ncls=128)
    d = heads_case(lib, 37, True, 0, ncls=128)
    assert c[0].tobytes() != d[0].tobytes() or c[1].tobytes() != d[1].tobytes()


@pytest.mark.parametrize("split", [1, 0], ids=["heads2", "heads"])
@pytest.mark.parametrize("ncls", [2, 128])
def test_heads_ffn_prologue_at_class_limits(lib, ncls, split):
    logits, boxes, want_logits, want_boxes = heads_fused_case(lib, split, rows=37, ncls=ncls, spare=SPARE)
    print(f"heads_fused ncls {ncls} split {split}: max |dlogit| {np.abs(logits[:37] - want_logits).max():.3e}, max |dbox| {np.abs(boxes[:37] - want_boxes).max():.3e}")
    _check_heads(37, ncls, logits, boxes, want_logits, want_boxes)


# ---- post-process: classes in two registers per lane (lane, lane + 64), the last class outside the maximum ------------------------------
POST_THR = 0.3
PEAK = 12.0   # a designed logit: exp(12) against at most 127 background classes of exp(N(0, 0.5))


def _post_inputs(B, Q, ncls):
    """Logits whose designed queries put the class boundary of postprocess_kernel through both registers.  Returns logits, boxes and
    `designed`: {(frame, query): expected label, or None for a query that must not be kept}."""
    rng = np.random.default_rng(1000 * Q + ncls)
    logits = (rng.standard_normal((B, Q, ncls)) * 0.5).astype(np.float32)
    boxes = rng.uniform(0.05, 0.95, (B, Q, 4)).astype(np.float32)
    noobj, last = ncls - 1, ncls - 2
    designed = {}
    for q in range(Q):                               # frame 0 keeps every query; the winner walks over every real class
        logits[0, q, q % noobj] = PEAK
        designed[(0, q)] = q % noobj
    logits[1, :, noobj] = PEAK                       # frame 1 keeps none: the no-object class takes the probability mass
    for q in range(Q):
        designed[(1, q)] = None
    slots = iter(range(Q))

    def put(label, **at):
        q = next(slots, None)
        if q is None:                                # (fewer queries than designs: the cases with 100 and 128 queries hold them all)
            return
        for idx, v in at.items():
            logits[2, q, int(idx[1:])] = v
        designed[(2, q)] = label

    put(0, c0=PEAK)
    put(last, **{f"c{last}": PEAK})
    # the largest logit on the no-object class: it enters the softmax sum and never the label ...
    put(None, **{f"c{noobj}": PEAK, f"c{last}": PEAK - 2.0})          # ... score 0.12: dropped
    put(last, **{f"c{noobj}": PEAK, f"c{last}": PEAK - 0.2})          # ... score 0.45: kept, labelled with the best real class
    if 63 < noobj:
        put(63, c63=PEAK)
    if 64 < noobj:
        put(64, c64=PEAK)
        put(63, c63=PEAK, c64=PEAK)                                   # a tie across the two registers: the lower index
        put(64, c63=PEAK - 1.0, c64=PEAK)
        put(63, c63=PEAK, c64=PEAK - 1.0)
    return logits, boxes, designed


@pytest.mark.parametrize("Q,ncls", [(1, 2), (4, 3), (100, 64), (100, 65), (100, 66), (128, 128), (128, 2)])
def test_postprocess_kernel_at_query_and_class_limits(lib, Q, ncls):
    B = 3
    logits, boxes, designed = _post_inputs(B, Q, ncls)
    hw = np.asarray([[720, 1280], [333, 203], [1080, 1920]], np.int32)
    # on the float64 reference alone: no score within 1e-4 of the threshold, so every record is compared and none set aside
    e = np.exp(logits.astype(np.float64) - logits.astype(np.float64).max(-1, keepdims=True))
    scores = (e / e.sum(-1, keepdims=True))[..., :-1].max(-1)
    assert np.abs(scores - POST_THR).min() > 1e-4
    want = O.post_process_object_detection(logits, boxes, POST_THR, [tuple(int(v) for v in r) for r in hw])
    # the reference itself shows what the inputs were built for
    for (b, q), label in designed.items():
        hit = np.flatnonzero(want[b]["query_index"] == q)
        assert (len(hit) == 0) if label is None else (len(hit) == 1 and want[b]["labels"][hit[0]] == label), (b, q, label)
    assert len(want[0]["scores"]) == Q and len(want[1]["scores"]) == 0
    if Q >= 100:
        labels2 = set(int(v) for v in want[2]["labels"])
        assert {0, ncls - 2} <= labels2 and (ncls < 66 or {63, 64} <= labels2) and (ncls != 65 or 63 in labels2)
    recs = np.zeros((B, Q), DET)
    counts = np.full(B, -7, np.int32)
    _capi.check(lib.opd_test_postprocess(_p(logits), _p(boxes), _p(hw), B, Q, ncls, POST_THR, _p(recs), _p(counts)), "opd_test_postprocess")
    compare_records(recs, counts, want)
    assert (recs["label"] < ncls - 1).all() and (recs["label"] >= 0).all()
    for b in range(B):   # records past counts[b] keep the hook's fill (zero bytes)
        assert not recs[b, counts[b]:].view(np.uint8).any()


@pytest.mark.parametrize("Q,ncls", [(129, 92), (100, 129)])
def test_postprocess_refuses_what_its_block_cannot_hold(lib, Q, ncls):
    """More than 128 queries or 128 classifier rows (two class registers per lane): an error code, nothing written.  The loader refuses such
    a checkpoint before a handle exists (tests/test_host_cpu.py)."""
    B = 2
    logits = np.zeros((B, Q, ncls), np.float32); logits[..., 1] = 9.0
    boxes = np.full((B, Q, 4), 0.5, np.float32)
    hw = np.asarray([[100, 100]] * B, np.int32)
    recs = np.zeros((B, Q), DET); recs["frame"] = -3
    counts = np.full(B, -7, np.int32)
    assert lib.opd_test_postprocess(_p(logits), _p(boxes), _p(hw), B, Q, ncls, 0.5, _p(recs), _p(counts)) == _capi.OPD_EHIP
    assert (recs["frame"] == -3).all() and (counts == -7).all()
