"""The derived bounds of tests/reid_bounds.py on the CPU: an fp32 restatement of each Re-ID kernel's arithmetic (its summation order
and rounding points) stays within its bound, and the same restatement with one plausible one-line mistake breaks it.  So the
bounds test_reid_kernels_gpu.py holds the kernels to are neither slack nor tighter than fp32 allows."""

import numpy as np
import pytest

import reid_bounds as B

f32 = np.float32


def _excess(err, bound):
    """max err / bound: <= 1 within the bound."""
    return float((np.asarray(err, np.float64) / bound).max())


def _f16(a):
    return np.asarray(a, f32).astype(np.float16).astype(np.float64)


# ---- quick_gelu epilogue ------------------------------------------------------------------------------------------------------------------
def _qgelu32(z, alpha=1.702):
    x = z.astype(f32)
    with np.errstate(over="ignore"):   # (expf overflows to inf below x = -52, as on the device: the result is -0)
        return x * (f32(1) / (f32(1) + np.exp(-f32(alpha) * x)))


def test_qgelu_bound():
    z = np.arange(-16 * 64, 16 * 64 + 1) / 16.0   # the test's arguments: a 1/16 grid
    y = B.qgelu(z)
    bound = B.qgelu_bound(z)
    assert _excess(np.abs(_f16(_qgelu32(z)) - y), bound) <= 1
    # sigmoid(x) in place of sigmoid(1.702 x), or torch's erf GELU in place of quick_gelu
    assert _excess(np.abs(_f16(_qgelu32(z, 1.0)) - y), bound) > 10
    from math import erf
    gelu = np.array([0.5 * v * (1 + erf(v / np.sqrt(2))) for v in z])
    assert _excess(np.abs(_f16(gelu) - y), bound) > 5


# ---- attention ----------------------------------------------------------------------------------------------------------------------------
def _attn32(q, k, v, leak=0, drop_last=False):
    T = q.shape[-2]
    s = (q.astype(f32) @ np.swapaxes(k, -1, -2).astype(f32))
    if drop_last:
        s = s[..., :T - 1]
        v = v[..., :T - 1, :]
    mx = s.max(-1, keepdims=True)
    e = np.exp(s - mx)
    tot = e.sum(-1, keepdims=True, dtype=f32) + f32(leak) * np.exp(-mx)   # leak: zero-padded keys beyond T in the softmax
    P = (e * (f32(1) / tot)).astype(np.float16).astype(f32)
    return _f16(P @ v.astype(f32))


@pytest.mark.parametrize("T,peaked", [(50, False), (17, True), (5, False), (63, True)])
def test_attention_bound(T, peaked):
    rng = np.random.default_rng(T)
    crops, H = 3, 256
    qkv = rng.standard_normal((crops * T, 3 * H))
    if peaked:
        qkv[:, :H] *= 8.0
    q, k, v = B.split_qkv(qkv.astype(np.float16), crops, T, H)
    want, bound = B.attention(q, k, v), B.attention_bound(q, k, v)
    assert _excess(np.abs(_attn32(q, k, v) - want), bound) <= 1
    if not peaked:   # (a zero key's score is 0: next to peaked rows' maxima its exp(0 - max) is nothing)
        assert _excess(np.abs(_attn32(q, k, v, leak=64 - T) - want), bound) > 1   # a key beyond T leaks into the softmax
    assert _excess(np.abs(_attn32(q, k, v, drop_last=True) - want), bound) > 1   # the last key dropped


# ---- LayerNorm ----------------------------------------------------------------------------------------------------------------------------
def _ln32(x, g, b, mode="two_pass", eps=1e-5):
    x = x.astype(f32)
    H = x.shape[-1]
    m = x.sum(-1, keepdims=True, dtype=f32) / f32(H)
    if mode == "one_pass":
        var = (x * x).sum(-1, keepdims=True, dtype=f32) / f32(H) - m * m
    else:
        d = x - m
        var = (d * d).sum(-1, keepdims=True, dtype=f32) / f32(H - 1 if mode == "unbiased" else H)
    r = f32(1) / np.sqrt(np.maximum(var, 0) + f32(eps))
    return (x - m) * r * g + b


def _ln_rows(kind, H, rng, n=16):
    if kind == "offset":
        x = 1000.0 + rng.uniform(-3, 3, (n, 1)) + rng.standard_normal((n, H)) * rng.uniform(0.5, 3, (n, 1))
    else:
        x = rng.standard_normal((n, 1)) + rng.standard_normal((n, H)) * 3e-3
    return x.astype(f32)


@pytest.mark.parametrize("H", [128, 256, 768, 1024])
def test_layernorm_bound(H):
    rng = np.random.default_rng(H)
    g = (1 + 0.2 * rng.standard_normal(H)).astype(f32)
    b = (0.1 * rng.standard_normal(H)).astype(f32)
    for kind in ("offset", "narrow"):
        x = _ln_rows(kind, H, rng)
        want, bound = B.layernorm(x, g, b), B.layernorm_bound(x, g, b)
        b16 = bound + 0.5 * B.ulp16(np.abs(want) + bound)
        assert _excess(np.abs(_ln32(x, g, b) - want), bound) <= 1
        assert _excess(np.abs(_f16(_ln32(x, g, b)) - want), b16) <= 1
        if kind == "offset":   # E[x^2] - mean^2 in fp32
            assert _excess(np.abs(_f16(_ln32(x, g, b, "one_pass")) - want), b16) > 1
        else:   # epsilon 1e-6 in place of 1e-5
            assert _excess(np.abs(_f16(_ln32(x, g, b, eps=1e-6)) - want), b16) > 1
    # the unbiased variance (torch.var's default) in place of the biased one, on unit-scale rows: out of the fp32 bound and the fp16 one
    x = (rng.standard_normal((16, H)) * 1.5).astype(f32)
    want, bound = B.layernorm(x, g, b), B.layernorm_bound(x, g, b)
    assert _excess(np.abs(_ln32(x, g, b, "unbiased") - want), bound) > 1
    assert _excess(np.abs(_f16(_ln32(x, g, b, "unbiased")) - want), bound + 0.5 * B.ulp16(np.abs(want) + bound)) > 1


# ---- L2 norm --------------------------------------------------------------------------------------------------------------------------------
def _l2_32(y, lanes=64):
    y = y.astype(f32)
    E = y.shape[-1]
    part = np.zeros(y.shape[:-1] + (64,), f32)
    for c in range(E):
        part[..., c % 64] += y[..., c] * y[..., c]
    s = part[..., :lanes].sum(-1, keepdims=True, dtype=f32)   # lanes < 64: a shuffle level missing
    return y * (f32(1) / np.sqrt(s))


@pytest.mark.parametrize("E", [128, 256, 512, 100])
def test_l2norm_bound(E):
    rng = np.random.default_rng(E)
    y = (rng.standard_normal((37, E)) * rng.uniform(1e-2, 1e2, (37, 1))).astype(f32)
    want, bound = B.l2norm(y), B.l2norm_bound(y)
    assert _excess(np.abs(_l2_32(y) - want), bound) <= 1
    assert _excess(np.abs(_l2_32(y, 32) - want), bound) > 1


# ---- OSNet gate, combine, head --------------------------------------------------------------------------------------------------------------
def _gate32(t, w1, b1, w2, b2, nb, HW, mid, drop_tail=False, swap=False):
    tt = t.astype(f32).reshape(nb, HW, 4, mid)
    parts = 256 // mid
    rows = HW // parts if drop_tail else -(-HW // parts)   # drop_tail: floor instead of ceiling, the tail rows lost
    acc = np.zeros((nb, 4, mid), f32)
    for q in range(parts):
        acc += tt[:, q * rows:min(HW, (q + 1) * rows)].sum(1, dtype=f32)
    p = acc / f32(HW)
    h = np.maximum(p @ w1.T + b1, 0).astype(f32)
    g = f32(1) / (f32(1) + np.exp(-(h @ w2.T + b2).astype(f32)))
    return g[:, ::-1] if swap else g


@pytest.mark.parametrize("mid,HW", [(16, 2048), (48, 512), (80, 128), (256, 128)])
def test_gate_and_combine_bounds(mid, HW):
    rng = np.random.default_rng(mid)
    nb, hid = 2, max(1, mid // 16)
    t = np.abs(rng.standard_normal((nb * HW, 4 * mid)) * rng.uniform(0.2, 2, 4 * mid)).astype(np.float16).astype(f32)
    w1 = (rng.standard_normal((hid, mid)) * mid ** -0.5 * 2).astype(f32)
    b1 = (rng.standard_normal(hid) * 0.1).astype(f32)
    w2 = (rng.standard_normal((mid, hid)) * hid ** -0.5 * 2).astype(f32)
    b2 = (rng.standard_normal(mid) * 0.1).astype(f32)
    g, gb = B.gate(t, w1, b1, w2, b2, nb, HW, mid), B.gate_bound(t, w1, b1, w2, b2, nb, HW, mid)
    assert _excess(np.abs(_gate32(t, w1, b1, w2, b2, nb, HW, mid) - g), gb) <= 1
    if HW % (256 // mid):   # (the floor / ceiling rows differ only where parts does not divide HW)
        assert _excess(np.abs(_gate32(t, w1, b1, w2, b2, nb, HW, mid, drop_tail=True) - g), gb) > 1
    x, xb = B.combine(t, g, nb, HW, mid), B.combine_bound(t, g, gb, nb, HW, mid)
    g32 = _gate32(t, w1, b1, w2, b2, nb, HW, mid)
    tt = t.reshape(nb, HW, 4, mid)
    assert _excess(np.abs(_f16((tt * g32[:, None]).sum(2, dtype=f32).reshape(nb * HW, mid)) - x), xb) <= 1
    wrong = (tt * g32[:, None, ::-1]).sum(2, dtype=f32).reshape(nb * HW, mid)   # stream s takes another stream's gate
    assert _excess(np.abs(_f16(wrong) - x), xb) > 1


def _head32(x, wt, b, rows=None):
    x = x.astype(f32)
    p = x[:, :rows].sum(1, dtype=f32) / f32(x.shape[1])
    y = np.maximum(p @ wt + b, 0).astype(f32)
    return y / np.sqrt((y * y).sum(-1, keepdims=True, dtype=f32))


@pytest.mark.parametrize("C", [128, 256, 320, 512])
def test_head_bound(C):
    rng = np.random.default_rng(C)
    x = np.abs(rng.standard_normal((5, 128, C))).astype(np.float16).astype(f32)
    wt = (rng.standard_normal((C, 512)) * C ** -0.5).astype(f32)
    b = (rng.standard_normal(512) * 0.1).astype(f32)
    want, bound = B.head(x, wt, b), B.head_bound(x, wt, b)
    assert _excess(np.abs(_head32(x, wt, b) - want), bound) <= 1
    assert _excess(np.abs(_head32(x, wt, b, rows=127) - want), bound) > 1   # the last pooled row lost
