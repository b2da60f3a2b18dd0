"""Helpers of the tests that run ONE test body over both element types of the 16-bit kernels (csrc/opd_elem.h: fp16 and bf16), shared by
tests/test_bf16_kernels_gpu.py (the kernels) and tests/test_elem_common_cpu.py (the helpers, the integer recipes and the bounds, without a GPU).

Three kinds of check, in this order of preference:
 (a) exact arithmetic: small-integer operands chosen so that every product, every fp32 sum and every stored 16-bit value is an integer of
     magnitude <= EXACT_INT[elem]; the kernel's bits must equal the float64 reference's.  The recipes live here so that the CPU test can
     check that precondition at the very shapes the GPU test uses;
 (b) bit identity of two routes of the same instantiation (nothing to share);
 (c) a bound per output element against float64 on the same rounded operands, the sum of named terms and never a round number:
     - fp32 accumulation: a sum whose longest chain of roundings is d long is within d * U * sum |terms| of the exact sum (U = 2^-24);
     - one rounding of a stored 16-bit value: half an element ulp (round_bound);
     - in attention, the rounding of P to the element type;
     first-order propagation carries them through a LayerNorm or a softmax, as tests/reid_bounds.py does.
"""

from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

ELEMS = ["fp16", "bf16"]
EXACT_INT = {"fp16": 2048, "bf16": 256}   # every integer up to this magnitude is representable (11 / 8 significand bits)
FRACTION_BITS = {"fp16": 10, "bf16": 7}
MIN_NORMAL_EXP = {"fp16": -14, "bf16": -126}
U = 2.0 ** -24                            # fp32 unit roundoff


def _tdtype(elem):
    return torch.bfloat16 if elem == "bf16" else torch.float16


def to_bits(a, elem):
    """array -> uint16 bit patterns of the element type (one rounding to nearest even from fp32)."""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(_tdtype(elem))
    return np.ascontiguousarray(t.view(torch.int16).numpy().view(np.uint16))


def from_bits(bits, elem):
    """uint16 bit patterns of the element type -> float32 values."""
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).view(_tdtype(elem)).to(torch.float32).numpy()


def round_elem(a, elem):
    """The values of `a` (rounded to fp32 first, as a kernel's accumulator is) after one rounding to the element type, as float32."""
    return from_bits(to_bits(a, elem), elem)


def ulp_elem(x, elem):
    """The element type's ulp at |x| (below the smallest normal number: the subnormal spacing, 2^-24 for fp16)."""
    a = np.maximum(np.abs(np.asarray(x, np.float64)), 2.0 ** MIN_NORMAL_EXP[elem])
    return 2.0 ** (np.floor(np.log2(a)) - FRACTION_BITS[elem])


def round_bound(e, x, elem):
    """Bound of one rounding to the element type of a value within e of x (the shape of reid_bounds.round16)."""
    return e + 0.5 * ulp_elem(np.abs(x) + e, elem)


def sparse_int_rows(rng, rows, cols, k, values):
    """[rows][cols] float32: each row has k non-zeros at random distinct columns, drawn from `values`."""
    w = np.zeros((rows, cols), np.float32)
    vals = np.asarray(values, np.float32)
    for r in range(rows):
        w[r, rng.choice(cols, size=k, replace=False)] = vals[rng.integers(0, len(vals), k)]
    return w


def nontrivial(ref):
    """An exact-arithmetic reference worth comparing bits with: more than 30 % non-zero after a ReLU, and a magnitude of 16 or more."""
    ref = np.asarray(ref)
    return float((np.maximum(ref, 0) != 0).mean()) > 0.3 and float(np.abs(ref).max()) >= 16


def excess(err, bound):
    """max err / bound (<= 1: within the bound); a zero bound admits a zero error only."""
    err, bound = np.broadcast_arrays(np.asarray(err, np.float64), np.asarray(bound, np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    return float(r.max())


# ---- float64 references -------------------------------------------------------------------------------------------------------------------
def conv64(x_nhwc, w_nkkc, bias, stride, pad):
    """x [B][H][W][C], w [N][KH][KW][C] (the hooks' layout), bias [N] -> [B][OH][OW][N] in float64."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
    y = F.conv2d(t(x_nhwc).permute(0, 3, 1, 2), t(w_nkkc).permute(0, 3, 1, 2), t(bias) if bias is not None else None, stride=stride, padding=pad)
    return y.permute(0, 2, 3, 1).numpy()


def maxpool64(x_nhwc):
    """MaxPool2d(3, 2, 1) on [B][H][W][C], float64."""
    t = torch.from_numpy(np.ascontiguousarray(x_nhwc, dtype=np.float64)).permute(0, 3, 1, 2)
    return F.max_pool2d(t, 3, 2, 1).permute(0, 2, 3, 1).numpy()


def layernorm64(x, g, b):
    x = np.asarray(x, np.float64)
    d = x - x.mean(-1, keepdims=True)
    return d / np.sqrt((d * d).mean(-1, keepdims=True) + 1e-5) * np.asarray(g, np.float64) + np.asarray(b, np.float64)


# ---- (a) the integer recipes, at the shapes the GPU test runs -----------------------------------------------------------------------------------
TAIL_CASES = [  # B, H, W, C1, C3, stride, residual
    (2, 15, 13, 64, 64, 1, True), (2, 15, 13, 64, 128, 1, True), (2, 15, 13, 128, 128, 1, True), (2, 15, 13, 128, 128, 2, True),
    (2, 15, 13, 256, 256, 1, True), (2, 15, 13, 256, 256, 2, True),   # 390 rows at stride 1: three full tiles and a ragged one; stride 2 on odd sizes
    (1, 9, 11, 256, 0, 1, False),                                     # no fused reduce, no residual, one partial tile
]


def tail_recipe(case):
    """Operands of a fused bottleneck tail and its exact results: x1 in {0, 1, 2}; w1 / w2: 8 non-zeros of +-1, +-2 per row at random
    columns; w3: 4 of +-1; biases in {-1, 0, 1}; residual in [-4, 4].  Weights in the hooks' layout (w1 [C1][3][3][C1])."""
    B, H, W, C1, C3, stride, use_res = case
    rng = np.random.default_rng(sum(case) + 1000 * C3)
    C2 = 4 * C1
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    d = dict(x1=rng.integers(0, 3, (B, H, W, C1)).astype(np.float32),
             w1=sparse_int_rows(rng, C1, 9 * C1, 8, (-2, -1, 1, 2)), b1=rng.integers(-1, 2, C1).astype(np.float32),
             w2=sparse_int_rows(rng, C2, C1, 8, (-2, -1, 1, 2)), b2=rng.integers(-1, 2, C2).astype(np.float32),
             res=rng.integers(-4, 5, (B, OH, OW, C2)).astype(np.float32) if use_res else None,
             w3=sparse_int_rows(rng, C3, C2, 4, (-1, 1)) if C3 else None, b3=rng.integers(-1, 2, C3).astype(np.float32) if C3 else None)
    a1 = np.maximum(conv64(d["x1"], d["w1"].reshape(C1, 3, 3, C1), d["b1"], stride, 1), 0)
    y = conv64(a1, d["w2"].reshape(C2, 1, 1, C1), d["b2"], 1, 0)
    y = np.maximum(y + d["res"] if use_res else y, 0)
    z = np.maximum(conv64(y, d["w3"].reshape(C3, 1, 1, C2), d["b3"], 1, 0), 0) if C3 else None
    d.update(a1=a1, y=y, z=z)
    return d


TAIL_SC_SHAPE = (2, 10, 9)


def tail_sc_recipe():
    """The first tail of stage 1 (shortcut convolution inside, C1 = C3 = 64): the tail recipe plus xs in {0, 1, 2}, wsc: 4 of +-1 per row,
    the shortcut's bias in {-1, 0, 1}."""
    B, H, W = TAIL_SC_SHAPE
    d = tail_recipe((B, H, W, 64, 64, 1, False))
    rng = np.random.default_rng(77)
    d["xs"] = rng.integers(0, 3, (B, H, W, 64)).astype(np.float32)
    d["wsc"] = sparse_int_rows(rng, 256, 64, 4, (-1, 1))
    d["bsc"] = rng.integers(-1, 2, 256).astype(np.float32)
    d["sc"] = conv64(d["xs"], d["wsc"].reshape(256, 1, 1, 64), d["bsc"], 1, 0)       # what the two-launch route stores (no ReLU)
    d["y"] = np.maximum(conv64(d["a1"], d["w2"].reshape(256, 1, 1, 64), d["b2"], 1, 0) + d["sc"], 0)
    d["z"] = np.maximum(conv64(d["y"], d["w3"].reshape(64, 1, 1, 256), d["b3"], 1, 0), 0)
    return d


CONV_INT_CASES = {  # B, H, W, Cin, N, k, relu, residual
    "3x3": (1, 12, 11, 64, 128, 3, False, False),
    "residual_1x1": (1, 9, 15, 64, 256, 1, True, True),      # M = 135: one full tile + 7 rows
}
TILE_FLAGS = [0, 0x400, 0x500, 0x600, 0x20]
TILE_IDS = ["auto_tiles", "128rows", "160rows", "192rows", "flat_staging"]


def conv_int_recipe(name):
    B, H, W, Cin, N, k, relu, use_res = CONV_INT_CASES[name]
    rng = np.random.default_rng(5 + k)
    d = dict(x=rng.integers(-3, 4, (B, H, W, Cin)).astype(np.float32), w=sparse_int_rows(rng, N, k * k * Cin, 8, (-2, -1, 1, 2)),
             bias=rng.integers(-8, 9, N).astype(np.float32), res=rng.integers(-20, 21, (B, H, W, N)).astype(np.float32) if use_res else None)
    y = conv64(d["x"], d["w"].reshape(N, k, k, Cin), d["bias"], 1, k // 2)
    if use_res:
        y = y + d["res"]
    d["y"] = np.maximum(y, 0) if relu else y
    return d


DUAL_CASE = (2, 13, 11, 256, 1024, 512, 2)   # B, H, W, Cin, N, Cin2, stride2


def dual_recipe():
    B, H, W, Cin, N, Cin2, s2 = DUAL_CASE
    rng = np.random.default_rng(3)
    H2, W2 = (H - 1) * s2 + 1 + (s2 - 1), (W - 1) * s2 + 1    # x2 at the resolution before the stride (the last row is not sampled)
    d = dict(x=rng.integers(0, 3, (B, H, W, Cin)).astype(np.float32), x2=rng.integers(0, 3, (B, H2, W2, Cin2)).astype(np.float32),
             w1=sparse_int_rows(rng, N, Cin, 8, (-2, -1, 1, 2)), w2=sparse_int_rows(rng, N, Cin2, 8, (-2, -1, 1, 2)),
             bias=rng.integers(-3, 4, N).astype(np.float32), H2=H2, W2=W2)
    y = conv64(d["x"], d["w1"].reshape(N, 1, 1, Cin), d["bias"], 1, 0) + conv64(d["x2"], d["w2"].reshape(N, 1, 1, Cin2), None, s2, 0)[:, :H, :W]
    d["y"] = np.maximum(y, 0)
    return d


SPLITK_CASE = (1, 7, 9, 512, 512, 3, 1, 8)   # B, H, W, Cin, N, k, stride, splits: the smallest of test_gemm_options_gpu.py's SPLITK_CASES


def splitk_recipe():
    """The non-zeros of a row fall into random k-slices, so every slab holds partial sums of its own; all of them small integers."""
    B, H, W, Cin, N, k, stride, _ = SPLITK_CASE
    rng = np.random.default_rng(5 + sum(SPLITK_CASE))
    d = dict(x=rng.integers(-3, 4, (B, H, W, Cin)).astype(np.float32), w=sparse_int_rows(rng, N, k * k * Cin, 8, (-2, -1, 1, 2)),
             bias=((np.arange(N) % 121) - 60).astype(np.float32))
    d["y"] = np.maximum(conv64(d["x"], d["w"].reshape(N, k, k, Cin), d["bias"], stride, k // 2), 0)
    return d


K256_CASE = (97, 768)   # M, N (K = 256, no bias period)


def k256_recipe():
    M, N = K256_CASE
    rng = np.random.default_rng(3)
    d = dict(x=rng.integers(-2, 3, (M, 256)).astype(np.float32), w=sparse_int_rows(rng, N, 256, 8, (-2, -1, 1, 2)),
             bias=rng.integers(-3, 4, N).astype(np.float32))
    d["y"] = d["x"].astype(np.float64) @ d["w"].astype(np.float64).T + d["bias"]
    return d


ALT_CASE = (300, 768, 256, 768, 512)   # M, N, K, alt_mod, alt_cols: the smaller of test_gemm_options_gpu.py's ALT_CASES


def alt_recipe():
    """test_gemm_options_gpu.py's integer construction (x in [-3, 3], x_alt differs from x in every element, two weights per row, bias in
    [-6, 6]): |result| <= 5 * 5 + 6, in range for both element types as it stands."""
    M, N, K, alt_mod, alt_cols = ALT_CASE
    rng = np.random.default_rng(M + N + 7)
    x = rng.integers(-3, 4, (M, K)).astype(np.float32)
    xa = x + rng.integers(1, 3, (M, K)).astype(np.float32)
    w = np.zeros((N, K), np.float32)
    for n in range(N):
        w[n, (n * 37 + 5) % K] = 1 + (n % 3)
        w[n, (n * 11 + 2) % K] -= 2
    bias = ((np.arange(N) % 13) - 6).astype(np.float32)
    first = (np.arange(N) % alt_mod) < alt_cols
    w64 = w.astype(np.float64)
    y = np.where(first[None, :], x.astype(np.float64) @ w64.T, xa.astype(np.float64) @ w64.T) + bias
    return dict(x=x, xa=xa, w=w, bias=bias, y=y)


FRAME_BIAS_CASE = (3, 100, 256, 0, 0)   # frames, period, N, pmod, pcols: the smallest of test_gemm_options_gpu.py's FRAME_BIAS_CASES


def frame_bias_recipe():
    """test_gemm_options_gpu.py's integer construction with the tables scaled into (-128, 128): every table entry is its own multiple of
    2^-s, |x . w| <= 15, so every sum is exact in fp32; a 16-bit output is that exact sum rounded once."""
    B, period, N, pmod, pcols = FRAME_BIAS_CASE
    M, K = B * period, 256
    rng = np.random.default_rng(B * period + N + 3)
    x = rng.integers(-3, 4, (M, K)).astype(np.float32)
    w = np.zeros((N, K), np.float32)
    for n in range(N):
        w[n, (n * 37 + 5) % K] = 1 + (n % 3)
        w[n, (n * 11 + 2) % K] -= 2
    nvar = B * period * N
    s = int(np.ceil(np.log2(nvar / 256.0)))
    tables = ((rng.permutation(nvar) - nvar // 2) * 2.0 ** -s).astype(np.float32).reshape(B, period, N)
    assert np.unique(tables).size == nvar and np.abs(tables).max() <= 128
    y = x.astype(np.float64) @ w.astype(np.float64).T + tables.reshape(M, N).astype(np.float64)
    assert np.array_equal(y.astype(np.float32).astype(np.float64), y)   # exact in fp32
    return dict(x=x, w=w, tables=tables, y=y)


MAXPOOL_SHAPE = (2, 13, 17, 64)


def maxpool_recipe():
    """Values both element types hold exactly: integers in [-256, 255]; frame 1 all negative; one corner region at -61440 (-1.875 * 2^15),
    so that a window's maximum is far below zero and a wrong 'lowest' starting value shows."""
    B, H, W, Cc = MAXPOOL_SHAPE
    rng = np.random.default_rng(4)
    x = rng.integers(-256, 256, (B, H, W, Cc)).astype(np.float32)
    x[1] = -(np.abs(x[1]) % 256) - 1
    x[1, :4, :5] = -61440.0
    x[0, -3:, -3:, ::2] = -61440.0
    return dict(x=x, y=maxpool64(x))


REDUCE_ACT16 = (3, 8 * (3 * 256 + 5), 64)   # nsplit, n (four blocks of 256 threads x 8 elements, the last one partial), slab padding


def reduce_act16_recipe():
    nsplit, n, pad = REDUCE_ACT16
    rng = np.random.default_rng(30)
    part = rng.integers(-80, 81, (nsplit, n + pad)).astype(np.float32)
    part[:, n:] = 7777.0                       # the padding between slabs: must not be read
    part[1, 128:192] = -part[0, 128:192]       # exact cancellations
    part[2, 128:192] = 0.0
    return dict(part=part, y=part[:, :n].astype(np.float64).sum(0))


def exact_references():
    """name -> list of the tensors a kernel stores in that recipe (what the CPU test holds to EXACT_INT and to `nontrivial`; names ending in
    "/between": tensors that only pass from one launch of a route to the next, held to EXACT_INT alone)."""
    out = {}
    for case in TAIL_CASES:
        d = tail_recipe(case)
        out[f"tail{case}"] = [d["y"]] + ([d["z"]] if d["z"] is not None else [])
        out[f"tail{case}/between"] = [d["a1"]]
    d = tail_sc_recipe()
    out["tail_sc"] = [d["y"], d["z"]]
    out["tail_sc/between"] = [d["a1"], d["sc"]]
    for name in CONV_INT_CASES:
        out[f"conv_{name}"] = [conv_int_recipe(name)["y"]]
    out["dual"] = [dual_recipe()["y"]]
    out["splitk"] = [splitk_recipe()["y"]]
    out["k256"] = [k256_recipe()["y"]]
    out["alt"] = [alt_recipe()["y"]]
    out["reduce_act16"] = [reduce_act16_recipe()["y"]]
    return out


# ---- (c) bounds ------------------------------------------------------------------------------------------------------------------------------
def gemm_e(x, w, bias=None, res=None, K=None):
    """fp32 error of x . w^T + bias + res on exact 16-bit products: a sequential sum of K products, the bias and the residual has K + 1
    roundings, and every other order (MFMA blocks, k-slices, slabs added later) has a longest chain no longer:
    (K + 2) * U * (|x| . |w|^T + |bias| + |res|)."""
    x, w = np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(w, np.float64))
    s = x @ w.T
    if bias is not None:
        s = s + np.abs(np.asarray(bias, np.float64))
    if res is not None:
        s = s + np.abs(np.asarray(res, np.float64))
    return ((x.shape[-1] if K is None else K) + 2) * U * s


def conv_e(x_nhwc, w_nkkc, bias, stride, pad, K):
    """gemm_e for a convolution: |x| conv |w| + |bias|."""
    return (K + 2) * U * conv64(np.abs(x_nhwc), np.abs(w_nkkc), np.abs(bias), stride, pad)


def layernorm_bound(x, g, b, e_in=0.0, depth=255):
    """fp32 error of a two-pass LayerNorm (mean, centred variance, 1 / sqrtf(var + eps), (d rstd) g + b) whose input is within e_in
    (per row: the largest of the row) of the exact x, as reid_bounds.layernorm_bound carries it.  depth: the longest chain of additions of a row
    sum; 255 holds for every order in which 256 numbers can be added."""
    x = np.asarray(x, np.float64)
    g, b = np.asarray(g, np.float64), np.asarray(b, np.float64)
    e_in = np.broadcast_to(np.asarray(e_in, np.float64), x.shape).max(-1, keepdims=True)
    m = x.mean(-1, keepdims=True)
    dm = e_in + depth * U * (np.abs(x).mean(-1, keepdims=True) + e_in) + U * np.abs(m)
    d = x - m
    ed = e_in + dm + U * (np.abs(d) + e_in + dm)
    var = (d * d).mean(-1, keepdims=True)
    dq = (2 * np.abs(d) * ed + ed * ed).mean(-1, keepdims=True)
    dq = dq + (depth + 1) * U * (var + dq)
    v = var + 1e-5
    rel_r = 0.5 * (dq + 2 * U * v) / (v - np.minimum(dq, 0.5 * v)) + 2 * U
    r = 1 / np.sqrt(v)
    y = d * r * g + b
    return np.abs(g) * (ed * r * (1 + rel_r) + np.abs(d) * r * rel_r) + U * (2 * np.abs(d * r * g) + np.abs(y))


PRE_MEAN = np.array([0.485, 0.456, 0.406], np.float32).astype(np.float64)   # the kernel's fp32 constants, RGB
PRE_STD = np.array([0.229, 0.224, 0.225], np.float32).astype(np.float64)


def preprocess64(frames_bgr):
    """uint8 [..][3] BGR -> float64 RGB (v / 255 - mean) / std with the kernel's fp32 mean / std."""
    v = np.asarray(frames_bgr, np.float64)[..., ::-1]
    return (v / 255.0 - PRE_MEAN) / PRE_STD


def preprocess_e(frames_bgr):
    """fp32 error of ((float(v) * k - mean) / std), k = fl(1 / 255): k's rounding and the product (2 U v / 255), the difference, the quotient."""
    v = np.asarray(frames_bgr, np.float64)[..., ::-1]
    t2 = v / 255.0 - PRE_MEAN
    return (2 * U * v / 255.0 + U * np.abs(t2)) / PRE_STD + U * np.abs(t2 / PRE_STD)


def stem_pool_reference(x, w, bias, elem):
    """float64 stem (7x7 stride 2 pad 3, K padded to 256) + MaxPool2d(3, 2, 1) + ReLU and its bound: every convolution output is within
    round_bound(e, c) of c after its rounding to the element type; the maximum of a window moves by no more than the largest of its
    members' bounds, the ReLU by no more than that.  (Rounding before or after the pooling is the same thing: rounding is monotone.)"""
    c = conv64(x, w, bias, 2, 3)
    b = round_bound(conv_e(x, w, bias, 2, 3, 256), c, elem)
    return np.maximum(maxpool64(c), 0), maxpool64(b)


def softmax_weight_error(p, rho, extra_rel=0.0, sub=0.0):
    """|w - p| for weights w_k = t_k / sum_j t_j whose terms t_k are within a relative rho_k of (a common multiple of) p_k, plus an absolute
    `sub` (in units of the sum) each, and whose sum carries a relative error extra_rel:
    w_k = p_k (1 + d_k) / (1 + sum_j p_j d_j)  =>  |w_k - p_k| <= p_k (rho_k + sum_j p_j rho_j + extra) / (1 - that) + sub."""
    n = p.shape[-1]
    common = (p * rho).sum(-1, keepdims=True) + extra_rel + n * sub
    return p * (rho + common) / (1 - np.minimum(rho.max(-1, keepdims=True) + common, 0.5)) + sub


def attention64(q, k, v, scale, mask=None):
    """q [..][Lq][32], k / v [..][Lk][32] float64; mask [..][1 | Lq][Lk] bool (True: the key takes part) -> (P, P v)."""
    s = q @ np.swapaxes(k, -1, -2) * scale
    if mask is not None:
        s = np.where(mask, s, -np.inf)
    e = np.exp(s - s.max(-1, keepdims=True))
    p = e / e.sum(-1, keepdims=True)
    return p, p @ v


def attention_bound(q, k, v, scale, elem, mask=None, key_tile=64, out16=True):
    """attention_kernel (kernels_attn.hip), built as reid_bounds.attention_bound with the element ulp as a parameter.
    S = k q^T by one MFMA (32 fp32 accumulations); a = fma(s, scale log2 e, -m_ref) (the constant's and the product's roundings, the fma's own);
    t = exp2(a) (v_exp_f32: 2 U) with ONE reference per query, which cancels; t rounded to the element type UNNORMALISED (relative
    2^-(f+1); fp16 only: below 2^-14 the spacing is 2^-24, half of it 2^-25 in units of a row sum that is >= 1, because the reference is a
    score of the row and lags the maximum by 2^8 at most); O = sum t v and l = sum t by MFMA over the keys padded to the key tile, each
    rescaled once per tile at most; O / l; for a 16-bit output one rounding."""
    q, k, v = (np.asarray(a, np.float64) for a in (q, k, v))
    Lk = k.shape[-2]
    p, o = attention64(q, k, v, scale, mask)
    s = q @ np.swapaxes(k, -1, -2) * scale                            # natural-log domain
    ds = 32 * U * (np.abs(q) @ np.swapaxes(np.abs(k), -1, -2)) * scale
    smax = np.where(mask, s, -np.inf).max(-1, keepdims=True) if mask is not None else s.max(-1, keepdims=True)
    a = np.abs(s - smax) + 8.0 * np.log(2.0)                          # |a| <= |s - max| + the reference's lag
    rho = ds + 3 * U * np.abs(s) + U * a + 2 * U + 2.0 ** -(FRACTION_BITS[elem] + 1)
    ntiles = -(-Lk // key_tile)
    acc = (ntiles * key_tile + ntiles) * U
    sub = 2.0 ** -25 if elem == "fp16" else 0.0
    pz = np.where(mask, p, 0.0) if mask is not None else p
    rho = np.where(pz > 0, rho, 0.0)
    eP = softmax_weight_error(pz, rho, extra_rel=acc, sub=sub)
    if mask is not None:
        eP = np.where(mask, eP, 0.0)                                   # a masked key's weight is exactly zero
    av = np.abs(v)
    E = eP @ av + (acc + 2 * U) * ((pz + eP) @ av)
    return round_bound(E, o, elem) if out16 else E


def attention_map64(q, k, sel, heads, scale, valid=None, key_row=1):
    """q [rows][heads * 32], k [Lk][heads * 32] float64 -> (mean over the selected queries and the heads of softmax(q k^T scale) [Lk], its bound
    for attn_map_*_kernel)."""
    Lk = k.shape[0]
    qh = np.asarray(q, np.float64)[np.asarray(sel)].reshape(len(sel), heads, 32)
    kh = np.asarray(k, np.float64).reshape(Lk, heads, 32)
    x = np.einsum("qhd,khd->qhk", qh, kh) * scale
    ok = np.ones(Lk, bool)
    if valid is not None:
        idx = np.arange(Lk)
        ok = (idx // key_row < valid[0]) & (idx % key_row < valid[1])
    xm = np.where(ok, x, -np.inf)
    mx = xm.max(-1, keepdims=True)
    e = np.exp(xm - mx)
    p = e / e.sum(-1, keepdims=True)
    # 32 fmaf for the score, the fp32 scale and the product with it, x - max, expf (2 U); the row sum: ceil(Lk / 64) additions per lane and 6 shuffle
    # levels; the division; then rows additions per key and the division by their number
    dx = 32 * U * np.einsum("qhd,khd->qhk", np.abs(qh), np.abs(kh)) * scale + 2 * U * np.abs(x)
    rho = np.where(ok, dx + U * np.abs(x - mx) + 2 * U, 0.0)
    eP = softmax_weight_error(p, rho, extra_rel=(-(-Lk // 64) + 6 + 1) * U)
    rows = len(sel) * heads
    out = p.reshape(rows, Lk).mean(0)
    bound = eP.reshape(rows, Lk).mean(0) + (rows + 1) * U * (out + eP.reshape(rows, Lk).mean(0))
    return out, bound
