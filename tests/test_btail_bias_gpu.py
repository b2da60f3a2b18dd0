"""The fused tails' biases (kernels_btail.hip, kernels_btail3.hip), every channel observable exactly.

The tails load the biases of a whole tile once, packed over the sixteen lanes of a lane-row, and every chunk step takes its four floats
from one lane of the row (opd_kprims.h: row_bcast4).  The other tail tests draw biases from {-1, 0, 1} or from noise under a tolerance: a
wrong source lane can hide in both.  Here the GEMMs are switched off (zero weights) or reduced to a channel permutation (one-hot weights),
and every bias is a distinct small integer, so that an output element names the bias channel it was built from:

  expand bias   W1 = W2 = 0 (Wsc = 0):  y = relu(b2 + res),  z[n] = relu(y[(13 n + 7) mod C2] + b3[n])
  3x3 bias      W1 = 0, W2 one-hot n -> n mod C1:  y[n] = relu(b1[n mod C1] + b2[n] + res),  z[n] = relu(y[(13 n + 7) mod C2])
  rebuild pair  the same through stage 1's three tails, the second one rebuilding its residual from the first one's bias

with b2[c] = (37 c mod 251) - 100, b1[c] = c mod 61, b3[n] = n mod 97 and an integer residual in [-4, 4].  All values are integers of at most
250 in magnitude (asserted on the float64 reference): exact in fp16 (11 significand bits) and in bf16 (8), so bits are compared, for both
instantiations.  Shapes: B = 2, 9 x 13 -- 234 rows, one full and one ragged 128-pixel tile, all chunks; 15 x 13 under the stride-2 first
block of stage 2.
"""

import ctypes as C

import numpy as np
import pytest

import elem_common as E
from elem_common import to_bits
from office_person_detection_vit_amd import _capi

pytestmark = pytest.mark.gpu

f32 = np.float32
B, H, W = 2, 9, 13
SHAPE_SC2 = (2, 15, 13)
PAIRS = [(64, 64), (64, 128), (64, 0), (128, 128), (128, 0), (256, 256), (256, 0)]   # C1, C3; 256: the stage-3 kernel (kernels_btail3.hip)


@pytest.fixture(scope="module")
def lib():
    return _capi.load_library(test_hooks=True)


@pytest.fixture(params=E.ELEMS)
def elem(request, lib):
    lib.opd_test_set_elem_bf16(int(request.param == "bf16"))
    yield request.param
    lib.opd_test_set_elem_bf16(0)


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def bias2(C2, shift=0):
    return ((37 * np.arange(C2)) % 251 - 100 + shift).astype(f32)


def bias1(C1):
    return (np.arange(C1) % 61).astype(f32)


def bias3(C3):
    return (np.arange(C3) % 97).astype(f32)


def one_hot(rows, cols, col_of_row):
    w = np.zeros((rows, cols), f32)
    w[np.arange(rows), col_of_row(np.arange(rows)) % cols] = 1.0
    return w


def w3_perm(C3, C2):
    return one_hot(max(C3, 1), C2, lambda n: 13 * n + 7)[:C3] if C3 else None


def relu(a):
    return np.maximum(a, 0.0)


def tail64(b1, w2, b2, res, w3, b3):
    """float64 reference of a tail whose 3x3 weights are zero: a1 = relu(b1) at every pixel."""
    a1 = relu(np.asarray(b1, np.float64))[None, :]
    y = relu(a1 @ np.asarray(w2, np.float64).T + b2 + (0.0 if res is None else res))
    z = relu(y @ np.asarray(w3, np.float64).T + b3) if w3 is not None else None
    return y, z


def exact_bits(ref, elem):
    """The value-range precondition of a bit comparison, on the float64 reference; then its bit patterns."""
    ref = np.asarray(ref, np.float64)
    assert np.array_equal(ref, np.round(ref)) and np.abs(ref).max() < 2048 and np.abs(ref).max() <= E.EXACT_INT[elem], float(np.abs(ref).max())
    assert (ref > 0).mean() > 0.25 and ref.max() >= 16 and len(np.unique(ref)) > 30   # the biases show: many distinct values survive the ReLU
    return to_bits(ref + 0.0, elem)


def same(got, want, what):
    bad = np.argwhere(got != want)
    assert not len(bad), f"{what}: {len(bad)} of {want.size} elements differ, first at (row, channel) = {tuple(bad[0])}"


def int_rows(rng, shape, lo, hi):
    return rng.integers(lo, hi + 1, shape).astype(f32)


def run_btail(lib, elem, x1, w1, b1, w2, b2, res, w3, b3, C1, C3, shape=(B, H, W)):
    M = shape[0] * shape[1] * shape[2]
    y = np.full((M, 4 * C1), 0xFFFF, np.uint16)
    z = np.full((M, max(C3, 1)), 0xFFFF, np.uint16)
    bits = lambda a: to_bits(a, elem) if a is not None else None
    rc = lib.opd_test_btail(_p(bits(x1)), _p(bits(w1)), _p(b1), _p(bits(w2)), _p(b2), _p(bits(res)), _p(bits(w3)), _p(b3), _p(y), _p(z),
                            *shape, C1, C3, 1)
    _capi.check(rc, "opd_test_btail")
    return y, z


@pytest.mark.parametrize("C1,C3", PAIRS, ids=lambda v: str(v))
@pytest.mark.parametrize("kind", ["expand", "conv3x3"])
def test_tail_bias_per_channel(lib, elem, kind, C1, C3):
    """The residual tails (LDS-DMA residual): y and z name the channel of every bias they were built from."""
    rng = np.random.default_rng(100 * C1 + C3 + (kind == "conv3x3"))
    M, C2 = B * H * W, 4 * C1
    x1 = int_rows(rng, (B, H, W, C1), 0, 3)
    w1 = np.zeros((C1, 9 * C1), f32)
    res = int_rows(rng, (M, C2), -4, 4)
    b2 = bias2(C2)
    if kind == "expand":
        b1, w2, b3 = np.zeros(C1, f32), np.zeros((C2, C1), f32), (bias3(C3) if C3 else None)
    else:
        b1, w2, b3 = bias1(C1), one_hot(C2, C1, lambda n: n), (np.zeros(C3, f32) if C3 else None)
    w3 = w3_perm(C3, C2)
    want_y, want_z = tail64(b1, w2, b2, res, w3, b3)
    if kind == "expand":
        assert np.array_equal(want_y, relu(b2[None, :] + res))
    else:
        assert np.array_equal(want_y, relu(b1[np.arange(C2) % C1][None, :] + b2[None, :] + res))
    y, z = run_btail(lib, elem, x1, w1, b1, w2, b2, res, w3, b3, C1, C3)
    same(y, exact_bits(want_y, elem), "y")
    if C3:
        same(z, exact_bits(want_z, elem), "z")


def test_shortcut_tail_bias_per_channel(lib, elem):
    """First block of stage 1 (shortcut GEMM inside, Wsc = 0): y = relu(b2 + bsc) per channel, z through the permutation."""
    rng = np.random.default_rng(5)
    M = B * H * W
    b2, b3, w3 = bias2(256), bias3(64), w3_perm(64, 256)
    want_y, want_z = tail64(np.zeros(64), np.zeros((256, 64)), b2, None, w3, b3)
    want_y = np.broadcast_to(want_y, (M, 256))
    want_z = np.broadcast_to(want_z, (M, 64))
    y = np.full((M, 256), 0xFFFF, np.uint16)
    z = np.full((M, 64), 0xFFFF, np.uint16)
    bits = lambda a: to_bits(a, elem)
    args = [bits(int_rows(rng, (B, H, W, 64), 0, 3)), bits(np.zeros((64, 576), f32)), np.zeros(64, f32), bits(np.zeros((256, 64), f32)), b2,
            bits(int_rows(rng, (M, 64), 0, 3)), bits(np.zeros((256, 64), f32)), bits(w3), b3, y, z]
    _capi.check(lib.opd_test_btail_sc(*[_p(a) for a in args], B, H, W), "opd_test_btail_sc")
    same(y, exact_bits(want_y, elem), "y")
    same(z, exact_bits(want_z, elem), "z")


@pytest.mark.parametrize("C3", [128, 0])
@pytest.mark.parametrize("kind", ["expand", "conv3x3"])
def test_stride2_shortcut_tail_bias_per_channel(lib, elem, kind, C3):
    """First block of stage 2 (half steps, stride-2 shortcut over 256 channels, Wsc = 0): the same, eight chunks."""
    rng = np.random.default_rng(6 + C3)
    Bs, Hs, Ws = SHAPE_SC2
    M = Bs * ((Hs - 1) // 2 + 1) * ((Ws - 1) // 2 + 1)
    b2 = bias2(512)
    if kind == "expand":
        b1, w2, b3 = np.zeros(128, f32), np.zeros((512, 128), f32), bias3(128)
    else:
        b1, w2, b3 = bias1(128), one_hot(512, 128, lambda n: n), np.zeros(128, f32)
    w3 = w3_perm(128, 512)
    want_y, want_z = tail64(b1, w2, b2, None, w3, b3)
    want_y = np.broadcast_to(want_y, (M, 512))
    want_z = np.broadcast_to(want_z, (M, 128))
    y = np.full((M, 512), 0xFFFF, np.uint16)
    z = np.full((M, 128), 0xFFFF, np.uint16)
    bits = lambda a: to_bits(a, elem)
    args = [bits(int_rows(rng, (Bs, Hs, Ws, 128), 0, 3)), bits(np.zeros((128, 9 * 128), f32)), b1, bits(w2), b2,
            bits(int_rows(rng, (Bs, Hs, Ws, 256), 0, 3)), bits(np.zeros((512, 256), f32)), bits(w3), b3, y, z]
    _capi.check(lib.opd_test_btail_sc2(*[_p(a) for a in args], Bs, Hs, Ws, C3), "opd_test_btail_sc2")
    same(y, exact_bits(want_y, elem), "y")
    if C3:
        same(z, exact_bits(want_z, elem), "z")


def test_rebuild_pair_bias_per_channel(lib, elem):
    """Stage 1's three tails, both routes (residual read back / rebuilt from the first tail's bias `rc_b`): the first tail's output is
    y_a = relu(rc_b), rc_b[c] = (37 c mod 251) - 150; the second adds its own 3x3 and expand biases through the one-hot W2,
    y_b[n] = relu(b1[n mod 64] + b2[n] + y_a[n]) with b2 shifted by -60; the third, y_c = relu(b2 - 150 + y_b).  Every value <= 250."""
    rng = np.random.default_rng(7)
    M = B * H * W
    zero = lambda *s: np.zeros(s, f32)
    rc_b = bias2(256, -50)
    b1 = [zero(64), bias1(64), zero(64)]
    w2 = [zero(256, 64), one_hot(256, 64, lambda n: n), zero(256, 64)]
    b2 = [rc_b, bias2(256, -60), bias2(256, -150)]
    w3 = [zero(64, 256), w3_perm(64, 256), w3_perm(128, 256)]
    b3 = [zero(64), zero(64), zero(128)]
    ya, _ = tail64(b1[0], w2[0], b2[0], None, None, None)
    yb, zb = tail64(b1[1], w2[1], b2[1], np.broadcast_to(ya, (M, 256)), w3[1], b3[1])
    yc, zc = tail64(b1[2], w2[2], b2[2], yb, w3[2], b3[2])
    assert np.array_equal(ya[0], relu(rc_b)) and len(np.unique(ya)) > 90
    bits = lambda a: to_bits(a, elem)
    arr = lambda xs_: (C.c_void_p * len(xs_))(*[x.ctypes.data for x in xs_])
    w1b = [bits(zero(64, 576)) for _ in range(3)]
    w2b, w3b = [bits(a) for a in w2], [bits(a) for a in w3]
    x1, xs, wsc = bits(int_rows(rng, (B, H, W, 64), 0, 3)), bits(int_rows(rng, (M, 64), 0, 3)), bits(zero(256, 64))
    got_yb = [np.empty((M, 256), np.uint16) for _ in range(2)]
    got_zb = [np.empty((M, 64), np.uint16) for _ in range(2)]
    got_yc = [np.empty((B, H, W, 256), np.uint16) for _ in range(2)]
    got_zc = [np.empty((M, 128), np.uint16) for _ in range(2)]
    rc = lib.opd_test_btail_chain(_p(x1), _p(xs), arr(w1b), arr(b1), arr(w2b), arr(b2), _p(wsc), arr(w3b), arr(b3), arr(got_yb), arr(got_zb),
                                  arr(got_yc), arr(got_zc), B, H, W, 0xA5)
    _capi.check(rc, "opd_test_btail_chain")
    want_yb, want_zb = exact_bits(yb, elem), exact_bits(zb, elem)
    want_yc, want_zc = exact_bits(yc, elem).reshape(B, H, W, 256), exact_bits(zc, elem)
    for route, name in enumerate(("residual read back", "residual rebuilt")):
        same(got_yb[route], want_yb, f"second tail's y, {name}")
        same(got_zb[route], want_zb, f"second tail's z, {name}")
        same(got_zc[route], want_zc, f"third tail's z, {name}")
    same(got_yc[0].reshape(M, 256), want_yc.reshape(M, 256), "third tail's y")
    same(got_yc[1][:, ::2, ::2].reshape(-1, 256), want_yc[:, ::2, ::2].reshape(-1, 256), "third tail's y where a stride-2 1x1 reads it")
