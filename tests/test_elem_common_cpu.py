"""tests/elem_common.py without a GPU: the helpers against torch's CPU casts, the integer recipes of the exact-arithmetic tests against
the range in which bf16 holds every integer (the precondition of tests/test_bf16_kernels_gpu.py, at its shapes), and every derived bound
against an fp32 restatement of the kernel with element-typed storage -- honest, it stays within the bound; with one plausible one-line
mistake, it breaks it.  The pattern of tests/test_reid_bounds_cpu.py."""

import numpy as np
import pytest
import torch

import elem_common as E

f32 = np.float32


@pytest.fixture(params=E.ELEMS)
def elem(request):
    return request.param


# ---- the helpers ----------------------------------------------------------------------------------------------------------------------------
def _edge_values(elem):
    """Binade edges, their neighbours, subnormals and the smallest normal numbers of the element type."""
    emin = E.MIN_NORMAL_EXP[elem]
    f = E.FRACTION_BITS[elem]
    exps = [emin - f, emin - f + 1, emin - 1, emin, emin + 1, -1, 0, 1, 7, 8, 10, 11, 14]
    vals = []
    for e in exps:
        b = 2.0 ** e
        vals += [b, b * (1 + 2.0 ** -f), b * (2 - 2.0 ** -f), b * 1.5] if e >= emin else [b]
    vals += [3 * 2.0 ** (emin - f), 2.0 ** emin - 2.0 ** (emin - f)]   # subnormals that are no powers of two; the largest one
    return np.asarray(vals, np.float64)


def test_ulp_elem_is_the_spacing_of_the_type(elem):
    x = _edge_values(elem)
    bits = E.to_bits(x, elem)
    assert np.array_equal(E.from_bits(bits, elem).astype(np.float64), x)               # all representable
    up = E.from_bits(bits + 1, elem).astype(np.float64)                                 # the next value up
    assert np.array_equal(up - x, E.ulp_elem(x, elem))
    assert np.array_equal(E.ulp_elem(-x, elem), E.ulp_elem(x, elem))
    assert E.ulp_elem(0.0, elem) == 2.0 ** (E.MIN_NORMAL_EXP[elem] - E.FRACTION_BITS[elem])
    assert E.ulp_elem(1.0, "fp16") == 2.0 ** -10 and E.ulp_elem(1.0, "bf16") == 2.0 ** -7 and E.ulp_elem(2.0 ** -20, "fp16") == 2.0 ** -24


def test_round_elem_is_torchs_cast_and_within_half_an_ulp(elem):
    rng = np.random.default_rng(1)
    x = np.concatenate([_edge_values(elem) * (1 + 0.37 * 2.0 ** -E.FRACTION_BITS[elem]), rng.standard_normal(4096) * 10.0 ** rng.uniform(-7, 4, 4096)])
    x = np.concatenate([x, -x]).astype(f32)
    x = x[np.abs(x) < 60000]
    r = E.round_elem(x, elem)
    t = torch.from_numpy(x).to(torch.bfloat16 if elem == "bf16" else torch.float16)
    assert np.array_equal(r, t.to(torch.float32).numpy())
    assert np.array_equal(E.to_bits(r, elem), E.to_bits(x, elem))                        # idempotent
    assert (np.abs(r.astype(np.float64) - x) <= E.round_bound(0.0, x, elem)).all()
    # ties go to the even neighbour: 1 + half an ulp -> 1, 1 + three halves -> 1 + 2 ulp
    u = 2.0 ** -E.FRACTION_BITS[elem]
    assert np.array_equal(E.round_elem(np.asarray([1 + u / 2, 1 + 3 * u / 2]), elem), np.asarray([1.0, 1 + 2 * u], f32))


def test_exact_int_is_the_last_gapless_integer(elem):
    n = E.EXACT_INT[elem]
    ints = np.arange(-n, n + 1, dtype=np.float64)
    assert np.array_equal(E.round_elem(ints, elem).astype(np.float64), ints)
    assert E.round_elem(np.asarray([n + 1.0]), elem)[0] != n + 1


def test_sparse_int_rows():
    w = E.sparse_int_rows(np.random.default_rng(0), 50, 64, 8, (-2, -1, 1, 2))
    assert w.shape == (50, 64) and ((w != 0).sum(1) == 8).all() and set(np.unique(w)) == {-2, -1, 0, 1, 2}
    assert len({tuple(np.flatnonzero(r)) for r in w}) > 40                               # random positions, not a progression


# ---- (a) the integer recipes stay in bf16's range at the shapes the GPU test uses --------------------------------------------------------------
def test_integer_recipes_are_exact_in_both_element_types():
    refs = E.exact_references()
    assert len(refs) >= 2 * len(E.TAIL_CASES) + 9
    for name, tensors in refs.items():
        for t in tensors:
            assert np.array_equal(t, np.round(t)), name
            assert np.abs(t).max() <= E.EXACT_INT["bf16"], (name, float(np.abs(t).max()))
            if not name.endswith("/between"):
                assert E.nontrivial(t), (name, float((np.maximum(t, 0) != 0).mean()), float(np.abs(t).max()))


def test_frame_bias_and_maxpool_recipes():
    d = E.frame_bias_recipe()
    assert np.abs(d["y"]).max() < 256 and np.array_equal(d["y"].astype(f32).astype(np.float64), d["y"])
    m = E.maxpool_recipe()
    for elem in E.ELEMS:
        assert np.array_equal(E.round_elem(m["x"], elem), m["x"])                        # every value exact in both types
    assert (m["y"] == -61440).any() and (m["y"][1] < 0).all() and (m["y"][0] > 0).any()


def test_stem_normalisation_by_fma_gives_the_same_element_as_the_three_step_form(elem):
    """stem_pool2_kernel<U8> normalises a byte as fma(v, A_c, -B_c), preprocess_u8_kernel as (v k - mean_c) / std_c: the fused and the split
    launch agree bit for bit only if the two round to the same element for all 256 x 3 inputs (tests/test_host_cpu.py enumerates fp16)."""
    import os
    import re
    src = open(os.path.join(os.path.dirname(__file__), "..", "office_person_detection_vit_amd", "csrc", "kernels_gemm.hip")).read()
    na = [f32(x) for x in re.search(r"STEM_NA\[3\] = \{([^}]*)\}", src).group(1).replace("f", "").split(",")]
    nb = [f32(x) for x in re.search(r"STEM_NB\[3\] = \{([^}]*)\}", src).group(1).replace("f", "").split(",")]
    mean, std = np.array([0.485, 0.456, 0.406], f32), np.array([0.229, 0.224, 0.225], f32)
    v = np.arange(256, dtype=f32)
    for c in range(3):
        three = ((v * (f32(1) / f32(255)) - mean[c]) / std[c]).astype(f32)
        fma = (v.astype(np.float64) * np.float64(na[c]) - np.float64(nb[c])).astype(f32)
        assert np.array_equal(E.to_bits(three, elem), E.to_bits(fma, elem))


# ---- (c) the bounds against fp32 restatements -----------------------------------------------------------------------------------------------------
def _gemm32(x, w, bias=None, res=None, order="seq"):
    """fp32 x . w^T (+ bias + res) on exact products: numpy's blocked order, or 32-wide blocks added in k order as the MFMA does."""
    x, w = x.astype(f32), w.astype(f32)
    if order == "blocks":
        acc = np.zeros((x.shape[0], w.shape[0]), f32) if bias is None else np.broadcast_to(bias.astype(f32), (x.shape[0], w.shape[0])).copy()
        for k0 in range(0, x.shape[1], 32):
            acc = acc + x[:, k0:k0 + 32] @ w[:, k0:k0 + 32].T
    else:
        acc = x @ w.T
        if bias is not None:
            acc = acc + bias.astype(f32)
    return acc + res.astype(f32) if res is not None else acc


@pytest.mark.parametrize("M,N,K", [(37, 64, 64), (33, 256, 256), (20, 256, 2048)])
def test_gemm_bound(elem, M, N, K):
    rng = np.random.default_rng(M + K)
    x = E.round_elem(rng.standard_normal((M, K)), elem)
    w = E.round_elem(rng.standard_normal((N, K)) / np.sqrt(K), elem)
    bias = (rng.standard_normal(N) * 0.1).astype(f32)
    res = E.round_elem(rng.standard_normal((M, N)), elem)
    want = x.astype(np.float64) @ w.astype(np.float64).T + bias + res
    e = E.gemm_e(x, w, bias, res)
    bound = E.round_bound(e, want, elem)
    for order in ("seq", "blocks"):
        y32 = _gemm32(x, w, bias, res, order)
        assert E.excess(np.abs(y32 - want), e) <= 1                                                  # an fp32 output
        assert E.excess(np.abs(E.round_elem(y32, elem) - want), bound) <= 1                          # a 16-bit output
    assert E.excess(np.abs(E.round_elem(_gemm32(x, w, None, res), elem) - want), bound) > 1          # the bias dropped
    if N == K:
        assert E.excess(np.abs(E.round_elem(_gemm32(x, w.T.copy(), bias, res), elem) - want), bound) > 1   # the weight transposed
    if K <= 256:   # (a deep sum's own fp32 term outgrows half an fp16 ulp)
        twice = E.round_elem(E.round_elem(_gemm32(x, w, bias), elem) + res, elem)                    # rounded before the residual is added
        assert E.excess(np.abs(twice - want), bound) > 1


def _ln32(x, g, b, unbiased=False):
    x = x.astype(f32)
    m = x.sum(-1, keepdims=True, dtype=f32) * f32(1 / 256)
    d = x - m
    var = (d * d).sum(-1, keepdims=True, dtype=f32) / f32(255 if unbiased else 256)
    return d * (f32(1) / np.sqrt(var + f32(1e-5))) * g + b


@pytest.mark.parametrize("K", [64, 256, 2048])
def test_gemm_layernorm_bound(elem, K):
    """Linear + bias + residual + LayerNorm with fp32 output (gemm_ln, gemm_ln_deep, gemm_splitk_ln, reduce_ln_pos, layernorm): the row's
    largest GEMM error carried through the LayerNorm."""
    rng = np.random.default_rng(K)
    M = 40
    x = E.round_elem(rng.standard_normal((M, K)), elem)
    w = E.round_elem(rng.standard_normal((256, K)) / np.sqrt(K), elem)
    bias = (rng.standard_normal(256) * 0.1).astype(f32)
    res = rng.standard_normal((M, 256)).astype(f32)
    res[:4] = res[:4] * 0.01 + 30.0                                  # rows with a large common offset: the mean's error matters
    g = (1 + 0.1 * rng.standard_normal(256)).astype(f32)
    b = (0.1 * rng.standard_normal(256)).astype(f32)
    pre = x.astype(np.float64) @ w.astype(np.float64).T + bias + res
    want = E.layernorm64(pre, g, b)
    bound = E.layernorm_bound(pre, g, b, E.gemm_e(x, w, bias, res))
    for order in ("seq", "blocks"):
        y = _ln32(_gemm32(x, w, bias, res, order), g, b)
        assert E.excess(np.abs(y - want), bound) <= 1
        assert E.excess(np.abs(E.round_elem(y, elem) - want), E.round_bound(bound, want, elem)) <= 1
    assert E.excess(np.abs(_ln32(_gemm32(x, w, bias, None), g, b) - want), bound) > 1                 # the residual dropped
    if K <= 256:   # (1 / 510 relative: below the fp32 term of a 2048-deep sum)
        assert E.excess(np.abs(_ln32(_gemm32(x, w, bias, res), g, b, unbiased=True) - want), bound) > 1   # variance over 255
    assert E.excess(np.abs(_ln32(_gemm32(x, w, bias, res), g, np.zeros(256, f32)) - want), bound) > 1  # beta dropped
    # the plain LayerNorm kernel: no input error
    plain = E.layernorm_bound(res, g, b)
    assert E.excess(np.abs(_ln32(res, g, b) - E.layernorm64(res, g, b)), plain) <= 1
    assert E.excess(np.abs(_ln32(res, g, b, unbiased=True) - E.layernorm64(res, g, b)), plain) > 1


def _pre32(frames, swap=True):
    v = frames.astype(f32)[..., ::-1] if swap else frames.astype(f32)
    mean, std = np.array([0.485, 0.456, 0.406], f32), np.array([0.229, 0.224, 0.225], f32)
    return (v * (f32(1) / f32(255)) - mean) / std


def test_preprocess_bound(elem):
    frames = np.stack(np.meshgrid(np.arange(256), np.arange(256), indexing="ij"), -1).reshape(256, 256, 2)
    frames = np.concatenate([frames, (frames[..., :1] * 7 + 3) % 256], -1).astype(np.uint8)          # every byte value in every channel
    want, bound = E.preprocess64(frames), E.round_bound(E.preprocess_e(frames), E.preprocess64(frames), elem)
    assert E.excess(np.abs(_pre32(frames) - want), E.preprocess_e(frames)) <= 1
    assert E.excess(np.abs(E.round_elem(_pre32(frames), elem) - want), bound) <= 1
    assert E.excess(np.abs(E.round_elem(_pre32(frames, swap=False), elem) - want), bound) > 1         # BGR taken for RGB
    assert E.excess(np.abs(E.round_elem(E.round_elem(_pre32(frames), "bf16"), elem) - want), bound) > (1 if elem == "fp16" else 0)  # rounded to the coarser type first


def _stem_pool32(x, w, bias, elem, pad_value=-np.inf, relu=True):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=f32))
    c = torch.nn.functional.conv2d(t(x).permute(0, 3, 1, 2), t(w).permute(0, 3, 1, 2), t(bias), stride=2, padding=3)
    c = torch.from_numpy(E.round_elem(c.numpy(), elem))
    c = torch.nn.functional.pad(c, (1, 1, 1, 1), value=pad_value)
    y = torch.nn.functional.max_pool2d(c, 3, 2, 0).permute(0, 2, 3, 1).numpy()
    return np.maximum(y, 0) if relu else y


def test_stem_pool_bound(elem):
    rng = np.random.default_rng(7)
    x = E.round_elem(rng.standard_normal((2, 21, 18, 3)), elem)
    w = E.round_elem(rng.standard_normal((64, 7, 7, 3)) * 0.1, elem)
    bias = (rng.standard_normal(64) * 0.1).astype(f32)
    want, bound = E.stem_pool_reference(x, w, bias, elem)
    assert E.excess(np.abs(_stem_pool32(x, w, bias, elem) - want), bound) <= 1
    assert E.excess(np.abs(_stem_pool32(x, w, bias, elem, pad_value=0.0, relu=False) - want), bound) > 1   # zero padding and no ReLU
    assert E.excess(np.abs(_stem_pool32(x, w, np.zeros(64, f32), elem) - want), bound) > 1                # the bias dropped
    # rounding before or after the pooling is the same thing: rounding is monotone
    c = E.conv64(x, w, bias, 2, 3)
    assert np.array_equal(E.round_elem(E.maxpool64(c), elem), E.maxpool64(E.round_elem(c, elem)).astype(f32))


def _attn32(q, k, v, scale, elem, mask=None, lag=0.0, leak=None, normalise_first=False):
    """attention_kernel's arithmetic in fp32: base-2 exponent against a reference `lag` below the row maximum, weights rounded to the
    element type unnormalised, the row sum of the ROUNDED weights, one division, one output rounding."""
    s = (q.astype(f32) @ np.swapaxes(k, -1, -2).astype(f32))
    if mask is not None:
        m = mask.copy()
        if leak is not None:
            m[..., leak] = True
        s = np.where(m, s, -np.inf).astype(f32)
    sc2 = f32(f32(scale) * f32(1.44269504088896340736))
    ref = (s.max(-1, keepdims=True) * sc2 - f32(lag)).astype(f32)
    t = np.exp2((s * sc2 - ref).astype(f32)).astype(f32)
    if normalise_first:
        t = t / t.sum(-1, keepdims=True, dtype=f32)
    tr = E.round_elem(t, elem)
    o = (tr @ v.astype(f32)) / tr.sum(-1, keepdims=True, dtype=f32)
    return E.round_elem(o, elem)


@pytest.mark.parametrize("lag", [0.0, 7.5])
def test_attention_bound(elem, lag):
    rng = np.random.default_rng(11)
    B, H, Lq, Lk = 2, 3, 20, 150
    q = E.round_elem(rng.standard_normal((B, H, Lq, 32)) * 1.5, elem)
    k = E.round_elem(rng.standard_normal((B, H, Lk, 32)) * 1.5, elem)
    v = E.round_elem(rng.standard_normal((B, H, Lk, 32)), elem)
    idx = np.arange(Lk)
    mask = np.stack([np.ones(Lk, bool), (idx // 30 < 2) & (idx % 30 < 17)])[:, None, None, :]        # frame 1: a sub-rectangle of a 5 x 30 map
    mask = np.broadcast_to(mask, (B, H, 1, Lk))
    scale = 32 ** -0.5
    for m in (None, mask):
        _, want = E.attention64(q, k, v, scale, m)
        bound = E.attention_bound(q, k, v, scale, elem, m, key_tile=128)
        assert E.excess(np.abs(_attn32(q, k, v, scale, elem, m, lag) - want), bound) <= 1
    assert E.excess(np.abs(_attn32(q, k, v, scale, elem, mask, lag, leak=149) - want), bound) > 1     # one masked key takes part
    _, want = E.attention64(q, k, v, scale)
    bound = E.attention_bound(q, k, v, scale, elem, key_tile=128)
    assert E.excess(np.abs(_attn32(q, k[..., :-1, :], v[..., :-1, :], scale, elem) - want), bound) > 1  # the last key dropped
    assert E.excess(np.abs(_attn32(q, k, v, scale * 1.01, elem) - want), bound) > 1                     # a scale that is 1 % off
    # fp32 partials (the key-split form): no output rounding
    e32 = E.attention_bound(q, k, v, scale, elem, key_tile=128, out16=False)
    assert (e32 < bound).all() and (e32 > 0).all()


def _attn_map32(q, k, sel, heads, scale, valid, key_row, leak=None, rows=None):
    Lk = k.shape[0]
    qh = q[np.asarray(sel)].reshape(len(sel), heads, 32).astype(f32)
    kh = k.reshape(Lk, heads, 32).astype(f32)
    x = (np.einsum("qhd,khd->qhk", qh, kh).astype(f32) * f32(scale)).astype(f32)
    ok = np.ones(Lk, bool)
    if valid is not None:
        idx = np.arange(Lk)
        ok = (idx // key_row < valid[0]) & (idx % key_row < valid[1])
        if leak is not None:
            ok[leak] = True
    x = np.where(ok, x, -np.inf).astype(f32)
    e = np.exp((x - x.max(-1, keepdims=True)).astype(f32)).astype(f32)
    p = (e / e.sum(-1, keepdims=True, dtype=f32)).astype(f32)
    n = len(sel) * heads
    return p.reshape(n, Lk).sum(0, dtype=f32) / f32(rows or n)


def test_attention_map_bound(elem):
    rng = np.random.default_rng(5)
    heads, Lk = 8, 300
    q = E.round_elem(rng.standard_normal((40, 256)) * 1.5, elem)
    k = E.round_elem(rng.standard_normal((Lk, 256)) * 1.5, elem)
    scale = float(f32(32 ** -0.5))
    for sel in ([7], [3, 0, 17, 9, 33]):
        for valid in (None, (9, 13)):
            want, bound = E.attention_map64(q, k, sel, heads, scale, valid, 20)
            assert abs(want.sum() - 1) < 1e-12
            assert E.excess(np.abs(_attn_map32(q, k, sel, heads, scale, valid, 20) - want), bound) <= 1
            assert E.excess(np.abs(_attn_map32(q, k, sel, heads, scale, valid, 20, rows=len(sel) * heads + 1) - want), bound) > 1   # one row too many in the mean
            if valid is not None:
                assert E.excess(np.abs(_attn_map32(q, k, sel, heads, scale, valid, 20, leak=299) - want), bound) > 1               # a masked key takes part
            other = [s + 1 for s in sel]
            assert E.excess(np.abs(_attn_map32(q, k, other, heads, scale, valid, 20) - want), bound) > 1                            # the wrong queries
