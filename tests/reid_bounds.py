"""Float64 references and derived error bounds of the Re-ID kernels (csrc/kernels_reid.hip, csrc/kernels_osnet.hip), shared by
tests/test_reid_kernels_gpu.py (the kernels against them) and tests/test_reid_bounds_cpu.py (the bounds against fp32 restatements of
the kernels, honest and with one-line mistakes).

Every bound is evaluated per output element from the operands and is the sum of three named terms, no round number picked by eye:
- fp16 rounding of a stored value: half an fp16 ulp of it (ulp16);
- fp32 accumulation: a sum whose longest chain of roundings is d long is within d * U * sum |terms| (U = 2^-24) of the exact sum, d
  read off the kernel's loop and reduction tree;
- in attention, the fp16 rounding of P: half an fp16 ulp of each probability, times |v|.
First-order error propagation (|f(x + e) - f(x)| <= |f'| e, with the largest slope over the interval where it matters: 1/4 for the
sigmoid) carries them through the later operations.
"""

from __future__ import annotations

import numpy as np

U = 2.0 ** -24   # fp32 unit roundoff


def ulp16(x):
    """The fp16 ulp at |x| (subnormals: 2^-24)."""
    a = np.maximum(np.abs(np.asarray(x, np.float64)), 2.0 ** -14)
    return 2.0 ** (np.floor(np.log2(a)) - 10)


def round16(e, x):
    """Bound of the fp16 rounding of a value within e of x."""
    return e + 0.5 * ulp16(np.abs(x) + e)


# ---- CLIP -------------------------------------------------------------------------------------------------------------------------------
def qgelu(z):
    z = np.asarray(z, np.float64)
    return z / (1.0 + np.exp(-1.702 * z))


def qgelu_fp32(z):
    """fp32 error of x * (1 / (1 + expf(-1.702f * x))) for an exact x: the product 1.702f * x (its rounding and the constant's, relative
    slope |t| at most), expf (2 U), the add, the reciprocal and the final product (U each)."""
    z = np.asarray(z, np.float64)
    return (2.1 * np.abs(z) + 8) * U * np.abs(qgelu(z))


def qgelu_bound(z):
    return round16(qgelu_fp32(z), qgelu(z))


def split_qkv(qkv, crops, T, H):
    """[crops * T][3H] -> q, k, v [crops][heads][T][64] float64."""
    t = np.asarray(qkv, np.float64).reshape(crops, T, 3, H // 64, 64)
    return tuple(np.ascontiguousarray(t[:, :, j].transpose(0, 2, 1, 3)) for j in range(3))


def heads_to_rows(out, crops, T, H):
    return np.asarray(out, np.float64).reshape(crops, T, H // 64, 64).transpose(0, 2, 1, 3)


def softmax(s):
    e = np.exp(s - s.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def attention(q, k, v):
    return softmax(q @ np.swapaxes(k, -1, -2)) @ v


def attention_bound(q, k, v):
    """S = q k^T by MFMA (64 fp32 accumulations); p = exp(s - max) / sum in fp32 (relative: twice the row's largest S error, the
    rounding of s - max, expf, T adds, the reciprocal and the product); P rounded to fp16; O = P v by MFMA (64 accumulations of exact
    fp16 products); O rounded to fp16."""
    T = q.shape[-2]
    s = q @ np.swapaxes(k, -1, -2)
    ds = 64 * U * (np.abs(q) @ np.swapaxes(np.abs(k), -1, -2))
    p = softmax(s)
    rel = 2 * ds.max(-1, keepdims=True) + (np.abs(s - s.max(-1, keepdims=True)) + T + 6) * U
    eP = p * rel + 0.5 * ulp16(p * (1 + rel))
    av = np.abs(v)
    E = eP @ av + 64 * U * ((p + eP) @ av)
    return round16(E, p @ v)


def layernorm(x, g, b):
    x = np.asarray(x, np.float64)
    m = x.mean(-1, keepdims=True)
    d = x - m
    return d / np.sqrt((d * d).mean(-1, keepdims=True) + 1e-5) * g + b


def layernorm_bound(x, g, b):
    """fp32 error of reid_layernorm_kernel (before the fp16 rounding): each lane sums 2 H / 128 values (pairs), then 6 shuffle levels,
    for the mean and for the squared deviations; 1 / sqrtf(var + eps); (d rstd) g + b."""
    x = np.asarray(x, np.float64)
    H = x.shape[-1]
    depth = 2 * (H // 128) + 6
    m = x.mean(-1, keepdims=True)
    dm = depth * U * np.abs(x).mean(-1, keepdims=True) + U * np.abs(m)
    d = x - m
    ed = dm + U * (np.abs(d) + dm)
    var = (d * d).mean(-1, keepdims=True)
    dq = (2 * np.abs(d) * ed + ed * ed).mean(-1, keepdims=True) + (depth + 1) * U * var
    v = var + 1e-5
    rel_r = 0.5 * (dq + 2 * U * v) / v + 2 * U
    r = 1 / np.sqrt(v)
    y = d * r * g + b
    return np.abs(g) * (ed * r + np.abs(d) * r * rel_r) + U * (2 * np.abs(d * r * g) + np.abs(y))


def l2norm(y):
    y = np.asarray(y, np.float64)
    return y / np.linalg.norm(y, axis=-1, keepdims=True)


def l2norm_bound(y):
    """reid_l2norm_kernel: each of 64 lanes sums ceil(E / 64) squares, 6 shuffle levels; 1 / sqrtf; the product."""
    E = y.shape[-1]
    depth = -(-E // 64) + 1 + 6
    return np.abs(l2norm(y)) * (0.5 * depth * U + 3 * U)


# ---- OSNet ------------------------------------------------------------------------------------------------------------------------------
def _streams(t, nb, HW, mid):
    return np.asarray(t, np.float64).reshape(nb, HW, 4, mid)


def gate(t, w1, b1, w2, b2, nb, HW, mid):
    """[nb][4][mid]: sigmoid(fc2(relu(fc1(mean over HW)))) of each stream."""
    p = _streams(t, nb, HW, mid).mean(1)
    h = np.maximum(p @ np.asarray(w1, np.float64).T + b1, 0)
    return 1 / (1 + np.exp(-(h @ np.asarray(w2, np.float64).T + b2)))


def gate_bound(t, w1, b1, w2, b2, nb, HW, mid):
    """osnet_gate_kernel: pooled sum in 256 / mid parts of ceil(HW / parts) rows, parts added in order, / HW; fc1 (mid products and
    adds), ReLU; fc2 (hid), sigmoid (slope <= 1/4; expf, add, reciprocal: 5 U relative)."""
    tt = _streams(t, nb, HW, mid)
    parts = 256 // mid
    rows = -(-HW // parts)
    w1, w2 = np.asarray(w1, np.float64), np.asarray(w2, np.float64)
    p = tt.mean(1)
    dp = (rows + parts + 1) * U * np.abs(tt).mean(1)
    h = np.maximum(p @ w1.T + b1, 0)
    dh = dp @ np.abs(w1).T + (mid + 2) * U * (np.abs(b1) + np.abs(p) @ np.abs(w1).T)
    hid = w1.shape[0]
    da = dh @ np.abs(w2).T + (hid + 2) * U * (np.abs(b2) + h @ np.abs(w2).T)
    g = 1 / (1 + np.exp(-(h @ w2.T + b2)))
    return 0.25 * da + 5 * U * g


def combine(t, g, nb, HW, mid):
    """x2 [nb * HW][mid] = sum over the four streams of gate * stream."""
    return (_streams(t, nb, HW, mid) * g[:, None]).sum(2).reshape(nb * HW, mid)


def combine_bound(t, g, dg, nb, HW, mid):
    tt = np.abs(_streams(t, nb, HW, mid))
    E = (tt * dg[:, None]).sum(2) + 5 * U * (tt * g[:, None]).sum(2)
    return round16(E.reshape(nb * HW, mid), combine(t, g, nb, HW, mid))


def head(x, wt, b):
    """osnet_head_kernel's operation: mean over HW, fc ([C][512]), ReLU, L2 normalisation."""
    y = np.maximum(np.asarray(x, np.float64).mean(1) @ np.asarray(wt, np.float64) + b, 0)
    return y / np.linalg.norm(y, axis=-1, keepdims=True)


def head_bound(x, wt, b):
    """the pooled mean (HW adds in row order, / HW), fc (C products and adds), ReLU, the sum of squares by a 9-level tree, sqrtf and
    the division."""
    x = np.asarray(x, np.float64)
    HW, C = x.shape[1], x.shape[2]
    wt = np.asarray(wt, np.float64)
    p = x.mean(1)
    dp = (HW + 1) * U * np.abs(x).mean(1)
    y = np.maximum(p @ wt + b, 0)
    dy = dp @ np.abs(wt) + (C + 2) * U * (np.abs(b) + np.abs(p) @ np.abs(wt))
    s = (y * y).sum(-1, keepdims=True)
    ds = (2 * y * dy).sum(-1, keepdims=True) + 10 * U * s
    n = np.sqrt(s)
    return dy / n + (y / n) * (0.5 * ds / s + 2 * U)
