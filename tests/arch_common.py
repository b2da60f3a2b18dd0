"""What the kernel tests of the decoder and the output kernels share (tests/test_decoder_gpu.py, tests/test_kernels_gpu.py at the default
architecture; tests/test_arch_kernels_gpu.py at the limits of what the loader accepts): the fragment orders of dec_qkv_kernel, the seeded
inputs of each kernel hook, the hook call, and the float64 reference on the same inputs.  A `*_case` function asserts nothing: it returns
what the kernel wrote next to what float64 torch gives, and the tests state the bounds.  Follows HF:models/detr/modeling_detr.py:650-739
(decoder layer), :1284-1300 and :1410-1411 (heads)."""

import ctypes as C

import numpy as np
import torch
import torch.nn.functional as F

from office_person_detection_vit_amd import _capi

D = 256
SCALE = 32 ** -0.5

DET = np.dtype([("x1", "<f4"), ("y1", "<f4"), ("x2", "<f4"), ("y2", "<f4"), ("score", "<f4"), ("label", "<i4"), ("query_index", "<i4"),
                ("frame", "<i4")])   # opd_det (include/opd_detr.h)


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _f16(a):
    return np.ascontiguousarray(np.asarray(a, np.float32).astype(np.float16).view(np.uint16))


def _from16(a):
    return a.view(np.float16).astype(np.float64)


def t(a):
    return torch.from_numpy(np.asarray(a)).double()


def _ulp16(x):
    """Spacing of fp16 at |x| (subnormal spacing below 2^-14)."""
    with np.errstate(over="ignore"):
        return np.spacing(np.abs(x).astype(np.float16)).astype(np.float64)


def k_frag(k, pad=0.0):
    """k [B][Q][256] -> kf [B][8 heads][8 key tiles][64 lanes][8]: lane 16 g + li of tile kt holds k[16 kt + li][32 h + 8 g ..]
    (the order dec_qkv_kernel writes and dec_self_kernel streams: one KiB per MFMA A operand).  Keys >= Q: `pad`."""
    B, Q, _ = k.shape
    kp = np.full((B, 128, 256), pad, np.float64)
    kp[:, :Q] = k
    return kp.reshape(B, 8, 16, 8, 4, 8).transpose(0, 3, 1, 4, 2, 5).reshape(B, 8, 8, 64, 8)   # [b][kt][li][h][g][e] -> [b][h][kt][g][li][e]


def v_frag(v, pad=0.0):
    """v [B][Q][256] -> vf [B][8 heads][4 kb][2 dt][64 lanes][8]: lane 16 g + li holds v[key][32 h + 16 dt + li] for the keys
    kb*32 + 4g + (0..3) and kb*32 + 16 + 4g + (0..3)."""
    B, Q, _ = v.shape
    vp = np.full((B, 128, 256), pad, np.float64)
    vp[:, :Q] = v
    x = vp.reshape(B, 4, 2, 4, 4, 8, 2, 16)            # [b][kb][half][g][j4][h][dt][li]
    return x.transpose(0, 5, 1, 6, 3, 7, 2, 4).reshape(B, 8, 4, 2, 64, 8)   # -> [b][h][kb][dt][g][li][half][j4]


# ---- race screen (csrc/opd_test_util.h: launch_repeated) ---------------------------------------------------------------------------------
RACE_REPS = 40   # the project's figure (test_btail_repeated_launches_are_bit_identical), like the 256-MiB noise copy per repetition


def repeat_result(lib):
    """(launches, n_diff) of the last hook call; the read clears the record."""
    launches, n_diff = C.c_int(-1), C.c_int(-1)
    _capi.check(lib.opd_test_repeat_result(C.byref(launches), C.byref(n_diff)), "opd_test_repeat_result")
    return launches.value, n_diff.value


def race_screened(lib, call, *args, **kwargs):
    """`call(*args, **kwargs)` -- a case builder or a test body that calls exactly ONE kernel hook -- with that hook's launch repeated RACE_REPS
    times under memory noise: every repetition must leave the same bits in every output of the hook.  Returns what `call` returns (made from
    the last repetition's outputs), so the caller goes on to compare with its reference."""
    lib.opd_test_set_repeat(RACE_REPS)
    try:
        out = call(*args, **kwargs)
        launches, n_diff = repeat_result(lib)
    finally:
        lib.opd_test_set_repeat(0)
    assert launches == RACE_REPS, f"{launches} launches: the hook does not launch through launch_repeated, or more than one hook was called"
    assert n_diff == 0, f"{n_diff} of {RACE_REPS - 1} repetitions differ from the first"
    return out


def _ln_params(rng):
    return (1.0 + 0.1 * rng.standard_normal(D)).astype(np.float32), (0.1 * rng.standard_normal(D)).astype(np.float32)


# ---- fused decoder (csrc/kernels_dec.hip) ----------------------------------------------------------------------------------------------
def dec_qkv_case(lib, B, Q, with_partials):
    """[h = LN3(h_in + b2 + sum of 16 partial slabs)] ; q | k | v = h . Wqkv^T + bias[row mod Q]; k / v in fragment order.
    Returns rc and, when the launch was taken: h_out / q16 / k16 / vT as written (the hook zero-fills k16 and vT first: padding keys are
    never written), want_h (None without the prologue) and want_qkv [B][Q][768] in float64 on the fp32 weights."""
    rng = np.random.default_rng(B * 1000 + Q)
    M, ns = B * Q, 16
    h_in = rng.standard_normal((M, D)).astype(np.float32)
    parts = (rng.standard_normal((ns, M, D)) * 0.3).astype(np.float32)
    b2 = (rng.standard_normal(D) * 0.1).astype(np.float32)
    g, be = _ln_params(rng)
    w = (rng.standard_normal((768, D)) / 16).astype(np.float32)
    bias = (rng.standard_normal((Q, 768)) * 0.5).astype(np.float32)
    h_out = np.zeros((M, D), np.float32)
    q16 = np.zeros((M, D), np.uint16); k16 = np.zeros((B, 8, 8, 64, 8), np.uint16); vT = np.zeros((B, 8, 4, 2, 64, 8), np.uint16)
    rc = lib.opd_test_dec_qkv(_p(h_in), _p(parts) if with_partials else None, ns, _p(b2), _p(g), _p(be), _p(w), _p(bias), M, Q, _p(h_out), _p(q16), _p(k16), _p(vT))
    _capi.check(rc, "opd_test_dec_qkv")
    want_h = None
    if with_partials:
        pre = t(h_in) + t(b2)
        for s in range(ns):
            pre = pre + t(parts[s])
        h = F.layer_norm(pre, (D,), t(g), t(be), 1e-5)
        want_h = h.numpy()
    else:
        h = t(h_in)
    qkv = (h @ t(w).T).reshape(B, Q, 768) + t(bias)[None]
    return {"h_out": h_out, "q16": q16, "k16": k16, "vT": vT, "want_h": want_h, "want_qkv": qkv.numpy()}


def dec_self_case(lib, B, Q, fill=None):
    """Self-attention of every (frame, 16-query slab) with wave = head, o-proj + residual + LayerNorm, then the cross-attention query
    projection; q / k / v are the fp16 operands dec_qkv_kernel writes, with NaN in the padding keys of k and v^T.  `fill`: the 16-bit
    pattern qc16 starts with (a launch that is refused must leave it and h alone).  Returns rc, h0 (the state before), h (after), qc16,
    want_h (float64) and want_qc (float64 projection of the state the kernel produced)."""
    rng = np.random.default_rng(B * 77 + Q)
    M = B * Q
    q = (rng.standard_normal((B, Q, D)) * 1.5).astype(np.float32)
    k = (rng.standard_normal((B, Q, D)) * 1.5).astype(np.float32)
    v = rng.standard_normal((B, Q, D)).astype(np.float32)
    q16 = _f16(q.reshape(M, D))
    k_r, v_r = k.astype(np.float16).astype(np.float64), v.astype(np.float16).astype(np.float64)   # the fp16 operands, row-major
    k16 = np.ascontiguousarray(k_frag(k_r, np.nan).astype(np.float16).view(np.uint16))            # NaN in the padding keys
    vT = np.ascontiguousarray(v_frag(v_r, np.nan).astype(np.float16).view(np.uint16))
    h = rng.standard_normal((M, D)).astype(np.float32)
    wo = (rng.standard_normal((D, D)) / 16).astype(np.float32); bo = (rng.standard_normal(D) * 0.1).astype(np.float32)
    g, be = _ln_params(rng)
    wq = (rng.standard_normal((D, D)) / 16).astype(np.float32); rbq = (rng.standard_normal((Q, D)) * 0.5).astype(np.float32)
    h_io = h.copy()
    qc16 = np.zeros((M, D), np.uint16) if fill is None else np.full((M, D), fill, np.uint16)
    rc = lib.opd_test_dec_self(_p(q16), _p(k16), _p(vT), _p(h_io), _p(wo), _p(bo), _p(g), _p(be), _p(wq), _p(rbq), B, Q, SCALE, _p(qc16))
    out = {"rc": rc, "h0": h, "h": h_io, "qc16": qc16, "pad_keys": int(np.isnan(_from16(k16)).sum())}
    if rc != 0:
        return out
    qh = t(_from16(q16)).reshape(B, Q, 8, 32).transpose(1, 2)
    kh = t(k_r).reshape(B, Q, 8, 32).transpose(1, 2)
    vh = t(v_r).reshape(B, Q, 8, 32).transpose(1, 2)
    p = torch.softmax(qh @ kh.transpose(2, 3) * SCALE, -1)
    o = (p @ vh).transpose(1, 2).reshape(M, D)
    out["want_h"] = F.layer_norm(t(h) + o @ t(wo).T + t(bo), (D,), t(g), t(be), 1e-5).numpy()
    # the projection itself is fp32-grade: check it on the state the kernel actually produced
    out["want_qc"] = ((t(h_io) @ t(wq).T).reshape(B, Q, D) + t(rbq)[None]).reshape(M, D).numpy()
    return out


def attention_split_case(lib, B, Lq, Lk, splits, masked):
    """attention_kernel<SPLIT>: each key range's unnormalised sum_k p v, exponent reference and sum_k p; combined like
    dec_cross_out_kernel does they give softmax(Q K^T) V.  Returns O (the combination, float64), want, part_o."""
    rng = np.random.default_rng(Lk + splits)
    heads, Dm = 8, 256
    q = (rng.standard_normal((B, Lq, Dm)) * 1.5).astype(np.float32)
    k = (rng.standard_normal((B, Lk, Dm)) * 1.5).astype(np.float32)
    v = rng.standard_normal((B, Lk, Dm)).astype(np.float32)
    q16, k16, v16 = _f16(q), _f16(k), _f16(v)
    key_valid, key_row = None, 0
    mask = torch.zeros(B, 1, 1, Lk, dtype=torch.float64)
    if masked:
        key_row = 42
        rows = (Lk + key_row - 1) // key_row
        kv = np.asarray([[rows, key_row]] + [[max(1, rows // 4), 30]] * (B - 1), np.int32)[:B]   # frame 1: only the first quarter of the rows valid
        key_valid = kv
        for b in range(B):
            idx = np.arange(Lk)
            ok = (idx // key_row < kv[b, 0]) & (idx % key_row < kv[b, 1])
            mask[b, 0, 0, ~torch.from_numpy(ok)] = -np.inf
    M = B * Lq
    part_o = np.zeros((splits, M, Dm), np.float32)
    part_ml = np.zeros((splits, M, heads, 2), np.float32)
    _capi.check(lib.opd_test_attention_split(_p(q16), _p(k16), _p(v16), B, heads, Lq, Lk, SCALE, splits, _p(key_valid), key_row, _p(part_o), _p(part_ml)),
                "opd_test_attention_split")
    m = part_ml[..., 0].astype(np.float64)                      # [S][M][heads]
    l = part_ml[..., 1].astype(np.float64)
    mmax = m.max(axis=0, keepdims=True)
    wgt = np.where(np.isinf(m), 0.0, np.exp2(m - mmax))
    L = (wgt * l).sum(axis=0)                                    # [M][heads]
    O = (np.repeat(wgt, 32, axis=2) * part_o.astype(np.float64)).sum(axis=0) / np.repeat(L, 32, axis=1)
    qh = t(_from16(q16)).reshape(B, Lq, heads, 32).transpose(1, 2)
    kh = t(_from16(k16)).reshape(B, Lk, heads, 32).transpose(1, 2)
    vh = t(_from16(v16)).reshape(B, Lk, heads, 32).transpose(1, 2)
    p = torch.softmax(qh @ kh.transpose(2, 3) * SCALE + mask, -1)
    want = (p @ vh).transpose(1, 2).reshape(M, Dm).numpy()
    return O, want, part_o


def dec_cross_out_case(lib, M, splits, period):
    """Combine the key splits (incl. a split that carries no weight), o-proj + residual + LayerNorm; residual rows either per row or
    one constant row (layer 0's state).  Returns h, want and o (the combined attention output, for diagnostics)."""
    rng = np.random.default_rng(M + splits)
    part_o = rng.standard_normal((splits, M, D)).astype(np.float32) * 3.0
    m = (rng.standard_normal((splits, M, 8)) * 4.0).astype(np.float32)
    l = rng.uniform(0.5, 40.0, (splits, M, 8)).astype(np.float32)
    m[splits - 1, ::5, :] = -np.inf                                # every fifth row: the last split is empty / fully masked
    l[splits - 1, ::5, :] = 0.0
    part_o[splits - 1, ::5, :] = 0.0
    part_ml = np.ascontiguousarray(np.stack([m, l], axis=-1))
    res = rng.standard_normal((period if period else M, D)).astype(np.float32)
    wo = (rng.standard_normal((D, D)) / 16).astype(np.float32); bo = (rng.standard_normal(D) * 0.1).astype(np.float32)
    g, be = _ln_params(rng)
    h = np.zeros((M, D), np.float32)
    _capi.check(lib.opd_test_dec_cross_out(_p(part_o), _p(part_ml), splits, _p(res), period, _p(wo), _p(bo), _p(g), _p(be), M, _p(h)), "opd_test_dec_cross_out")
    m64, l64 = m.astype(np.float64), l.astype(np.float64)
    wgt = np.where(np.isinf(m64), 0.0, np.exp2(m64 - m64.max(axis=0, keepdims=True)))
    o = (np.repeat(wgt, 32, axis=2) * part_o).sum(axis=0) / np.repeat((wgt * l64).sum(axis=0), 32, axis=1)
    r = t(res) if not period else t(res)[torch.arange(M) % period]
    want = F.layer_norm(r + t(o) @ t(wo).T + t(bo), (D,), t(g), t(be), 1e-5)
    return h, want.numpy(), o


def dec_ffn_case(lib, M, Fh):
    """relu(h . W1^T + b1) . W2^T as F / 128 partial slabs over 64-row slabs.  Returns parts [F / 128][M][256], want (the whole product,
    float64) and (c, want_c): one slab on its own."""
    rng = np.random.default_rng(M + Fh)
    h = rng.standard_normal((M, D)).astype(np.float32)
    w1 = (rng.standard_normal((Fh, D)) / 16).astype(np.float32); b1 = (rng.standard_normal(Fh) * 0.1).astype(np.float32)
    w2 = (rng.standard_normal((D, Fh)) / 32).astype(np.float32)
    parts = np.zeros((Fh // 128, M, D), np.float32)
    _capi.check(lib.opd_test_dec_ffn(_p(h), _p(w1), _p(b1), _p(w2), M, Fh, _p(parts)), "opd_test_dec_ffn")
    hid = F.relu(t(h) @ t(w1).T + t(b1))
    want = hid @ t(w2).T
    c = 3 % (Fh // 128)
    want_c = hid[:, c * 128:(c + 1) * 128] @ t(w2)[:, c * 128:(c + 1) * 128].T
    return parts, want.numpy(), c, want_c.numpy()


# ---- heads (kernels_dec.hip::heads2_kernel for split = 1, kernels_untyped.hip::heads_kernel for split = 0) ----------------------------------
HEADS_SENTINEL = np.float32(-12345.5)


def _heads_weights(rng, ncls, wc_scale):
    wc = (rng.standard_normal((ncls, D)) * wc_scale).astype(np.float32); bc = rng.standard_normal(ncls).astype(np.float32)
    w1 = (rng.standard_normal((D, D)) / 11).astype(np.float32); b1 = rng.standard_normal(D).astype(np.float32) * 0.1
    w2 = (rng.standard_normal((D, D)) / 11).astype(np.float32); b2 = rng.standard_normal(D).astype(np.float32) * 0.1
    w3 = (rng.standard_normal((4, D)) / 8).astype(np.float32); b3 = rng.standard_normal(4).astype(np.float32) * 0.1
    return wc, bc, w1, b1, w2, b2, w3, b3


def _heads_outputs(lib, rows, ncls, spare):
    """logits / boxes as the hooks take them: exactly `rows` rows, or with `spare` rows of HEADS_SENTINEL behind them that travel to the
    device and back (opd_test_set_heads_spare_rows)."""
    lib.opd_test_set_heads_spare_rows(spare)
    if not spare:
        return np.empty((rows, ncls), np.float32), np.empty((rows, 4), np.float32)
    return np.full((rows + spare, ncls), HEADS_SENTINEL, np.float32), np.full((rows + spare, 4), HEADS_SENTINEL, np.float32)


def _heads_reference(x, wc, bc, w1, b1, w2, b2, w3, b3):
    y = F.relu(F.relu(x @ t(w1).T + t(b1)) @ t(w2).T + t(b2))
    return (x @ t(wc).T + t(bc)).numpy(), torch.sigmoid(y @ t(w3).T + t(b3)).numpy()


def heads_case(lib, rows, ln, split, ncls=92, spare=0):
    """class_labels_classifier + DetrMLPPredictionHead + sigmoid, with and without the decoder's final LayerNorm inside.  Returns logits
    [rows + spare][ncls], boxes [rows + spare][4] and the float64 references of the first `rows` rows."""
    lib.opd_test_set_heads2(split)
    rng = np.random.default_rng(rows)
    hs = rng.standard_normal((rows, 256)).astype(np.float32) * 1.5
    g = (1.0 + 0.1 * rng.standard_normal(256)).astype(np.float32)
    b = (0.1 * rng.standard_normal(256)).astype(np.float32)
    wc, bc, w1, b1, w2, b2, w3, b3 = _heads_weights(rng, ncls, 1 / 16 * 2)
    logits, boxes = _heads_outputs(lib, rows, ncls, spare)
    try:
        _capi.check(lib.opd_test_heads(_p(hs), _p(g if ln else None), _p(b if ln else None), _p(wc), _p(bc), _p(w1), _p(b1), _p(w2), _p(b2), _p(w3),
                                       _p(b3), _p(logits), _p(boxes), rows, ncls), "opd_test_heads")
    finally:
        lib.opd_test_set_heads2(1)
        lib.opd_test_set_heads_spare_rows(0)
    x = t(hs)
    if ln:
        x = F.layer_norm(x, (256,), t(g), t(b), 1e-5)
    want_logits, want_boxes = _heads_reference(x, wc, bc, w1, b1, w2, b2, w3, b3)
    return logits, boxes, want_logits, want_boxes


def heads_fused_case(lib, split, rows=800, ncls=92, spare=0):
    """The heads fed by the fused decoder: rows = LN3(hs + b2 + sum of the FFN's partial slabs), final LayerNorm, heads."""
    lib.opd_test_set_heads2(split)
    rng = np.random.default_rng(9)
    ns = 16
    hs = rng.standard_normal((rows, D)).astype(np.float32)
    parts = (rng.standard_normal((ns, rows, D)) * 0.3).astype(np.float32)
    b2f = (rng.standard_normal(D) * 0.1).astype(np.float32)
    g3, b3_ = _ln_params(rng)
    g, b = _ln_params(rng)
    wc, bc, w1, b1, w2, b2, w3, b3 = _heads_weights(rng, ncls, 1 / 8)
    logits, boxes = _heads_outputs(lib, rows, ncls, spare)
    try:
        _capi.check(lib.opd_test_heads_fused(_p(hs), _p(parts), ns, _p(b2f), _p(g3), _p(b3_), _p(g), _p(b), _p(wc), _p(bc), _p(w1), _p(b1), _p(w2), _p(b2),
                                             _p(w3), _p(b3), rows, ncls, _p(logits), _p(boxes)), "opd_test_heads_fused")
    finally:
        lib.opd_test_set_heads2(1)
        lib.opd_test_set_heads_spare_rows(0)
    x = t(hs) + t(b2f)
    for s in range(ns):
        x = x + t(parts[s])
    x = F.layer_norm(F.layer_norm(x, (D,), t(g3), t(b3_), 1e-5), (D,), t(g), t(b), 1e-5)
    want_logits, want_boxes = _heads_reference(x, wc, bc, w1, b1, w2, b2, w3, b3)
    return logits, boxes, want_logits, want_boxes


# ---- post-process (kernels_untyped.hip::postprocess_kernel) -----------------------------------------------------------------------------------
def compare_records(recs, counts, want, atol_box=1e-3):
    """Records [B][Q] (DET) + counts [B] of the post-process kernel against the oracle's post_process_object_detection: the count, the
    compaction order (query_index), label and frame exactly, score and box within the kernel test's bounds."""
    assert counts.tolist() == [len(w["scores"]) for w in want]
    for b in range(len(want)):
        n = counts[b]
        np.testing.assert_array_equal(recs[b, :n]["query_index"], want[b]["query_index"])
        np.testing.assert_array_equal(recs[b, :n]["label"], want[b]["labels"])
        assert (recs[b, :n]["frame"] == b).all()
        np.testing.assert_allclose(recs[b, :n]["score"], want[b]["scores"], rtol=2e-6, atol=1e-7)
        got_xyxy = np.stack([recs[b, :n][k] for k in ("x1", "y1", "x2", "y2")], -1) if n else np.zeros((0, 4), np.float32)
        np.testing.assert_allclose(got_xyxy, want[b]["boxes"], rtol=1e-6, atol=atol_box)
