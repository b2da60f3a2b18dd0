"""Stage 2's first block as ONE fused tail with its stride-2 shortcut convolution inside (GPU; kernels_btail.hip, SC2):

    a1 = relu(conv3x3_s2(x1, W1) + b1);  y0 = relu(W2 . a1 + Wsc . xs[2 oh, 2 ow] + (b2 + bsc));  z = relu(W3 . y0 + b3)

on x1 [B][H][W][128] and the block input xs [B][H][W][256].

 1. integer operands, both element types: y0 and z are the exact sums, and bit-identical to the three launches the tail replaces
    (3x3 -> dual-source expand -> reduce, through the hooks of those launchers);
 2. random fp16 operands against float64 on the same operands with a1 and y0 rounded to fp16 as the kernel rounds them, every element, at
    the bound of tests/test_kernels_gpu.py::test_btail_matches_torch (2e-3 of the tensor's scale + 2e-3 relative: one fp16 rounding of a1
    may differ by an ulp through accumulation order and propagates);
 3. one case under the race screen (launch_repeated, arch_common.RACE_REPS launches under memory noise): the same bits every time;
 4. end to end with OPD_SC2_TAIL = 0 / 1 at 256x320 and for the ragged pair 256x320 + 224x288: the bounds of tests/test_detector_gpu.py
    against the live oracle; eager, capture and replay agree bit for bit; a created handle and its clone agree bit for bit.

Shapes (input -> output map): 18x26 -> 9x13 at B = 2 (234 pixels: a full and a partial tile), 17x25 -> 9x13 (odd input: the last row and
column are the stride-2 edge), 5x7 -> 3x4 at B = 1 (one partial tile, every pixel on an edge), 22x30 -> 11x15 at B = 3 (495 pixels: tiles
spanning frames)."""

import ctypes as C
import functools

import numpy as np
import pytest

import elem_common as E
from arch_common import _p, race_screened
from elem_common import from_bits, to_bits
from office_person_detection_vit_amd import _capi
from office_person_detection_vit_amd.frames import structured_frames
from office_person_detection_vit_amd.weights import DetrArch, ensure_weight_file, load_safetensors

pytestmark = pytest.mark.gpu

C1, C2, CSC, C3 = 128, 512, 256, 128
SHAPES = [(2, 18, 26), (2, 17, 25), (1, 5, 7), (3, 22, 30)]
IDS = ["two_tiles_one_partial", "odd_input", "one_small_tile", "tile_spans_frames"]
c32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)


@pytest.fixture(scope="module")
def lib():
    return _capi.load_library(test_hooks=True)


@pytest.fixture(params=E.ELEMS)
def elem(request, lib):
    lib.opd_test_set_elem_bf16(int(request.param == "bf16"))
    yield request.param
    lib.opd_test_set_elem_bf16(0)


def _out_hw(H, W):
    return (H - 1) // 2 + 1, (W - 1) // 2 + 1


def block64(d, elem, rounded):
    """The block in float64 on the operands of `d`; rounded: a1 and y0 pass through the element type as the kernel stores them."""
    r = (lambda a: E.round_elem(a, elem).astype(np.float64)) if rounded else (lambda a: a)
    a1 = r(np.maximum(E.conv64(d["x1"], d["w1"].reshape(C1, 3, 3, C1), d["b1"], 2, 1), 0))
    sc = E.conv64(d["xs"], d["wsc"].reshape(C2, 1, 1, CSC), None, 2, 0)
    y = r(np.maximum(E.conv64(a1, d["w2"].reshape(C2, 1, 1, C1), d["b2sc"], 1, 0) + sc, 0))
    z = np.maximum(E.conv64(y, d["w3"].reshape(C3, 1, 1, C2), d["b3"], 1, 0), 0)
    return y, z


@functools.lru_cache(maxsize=None)
def integer_case(shape):
    """x1, xs in {0, 1, 2}; every weight row 4 non-zeros of +-1; biases in {-1, 0, 1}: a1 <= 9, y0 <= 45, z <= 181 -- every stored value an
    integer below EXACT_INT of both element types, every fp32 sum exact."""
    B, H, W = shape
    rng = np.random.default_rng(1000 * B + 10 * H + W)
    d = dict(x1=rng.integers(0, 3, (B, H, W, C1)).astype(np.float32), xs=rng.integers(0, 3, (B, H, W, CSC)).astype(np.float32),
             w1=E.sparse_int_rows(rng, C1, 9 * C1, 4, (-1, 1)), w2=E.sparse_int_rows(rng, C2, C1, 4, (-1, 1)),
             wsc=E.sparse_int_rows(rng, C2, CSC, 4, (-1, 1)), w3=E.sparse_int_rows(rng, C3, C2, 4, (-1, 1)),
             b1=rng.integers(-1, 2, C1).astype(np.float32), b2sc=rng.integers(-1, 2, C2).astype(np.float32), b3=rng.integers(-1, 2, C3).astype(np.float32))
    d["y"], d["z"] = block64(d, "fp16", rounded=False)
    return d


@functools.lru_cache(maxsize=None)
def random_case(shape):
    """The recipe of test_kernels_gpu.py::test_btail_matches_torch (non-negative activations, He-scaled weights), fp16-rounded operands."""
    B, H, W = shape
    rng = np.random.default_rng(77 + 1000 * B + 10 * H + W)
    h = lambda a: E.round_elem(a, "fp16")
    d = dict(x1=h(np.abs(rng.standard_normal((B, H, W, C1)))), xs=h(np.abs(rng.standard_normal((B, H, W, CSC)))),
             w1=h(rng.standard_normal((C1, 9 * C1)) * np.sqrt(2.0 / (9 * C1))), w2=h(rng.standard_normal((C2, C1)) * np.sqrt(2.0 / C1)),
             wsc=h(rng.standard_normal((C2, CSC)) * np.sqrt(2.0 / CSC)), w3=h(rng.standard_normal((C3, C2)) * np.sqrt(2.0 / C2)),
             b1=c32(rng.standard_normal(C1) * 0.1), b2sc=c32(rng.standard_normal(C2) * 0.1), b3=c32(rng.standard_normal(C3) * 0.1))
    y, z = block64(d, "fp16", rounded=True)
    d["y"], d["z"] = y, E.round_elem(z, "fp16").astype(np.float64)
    return d


def run_tail(lib, d, shape, elem, c3=C3):
    """The fused launch: (y0 bits [M][512], z bits [M][128]); c3 = 0: the form without the reduce (z comes back untouched)."""
    B, H, W = shape
    OH, OW = _out_hw(H, W)
    M = B * OH * OW
    y, z = np.full((M, C2), 0xFFFF, np.uint16), np.full((M, C3), 0xFFFF, np.uint16)
    b = lambda k: _p(to_bits(d[k], elem))
    rc = lib.opd_test_btail_sc2(b("x1"), b("w1"), _p(c32(d["b1"])), b("w2"), _p(c32(d["b2sc"])), b("xs"), b("wsc"), b("w3"), _p(c32(d["b3"])), _p(y), _p(z),
                                B, H, W, c3)
    _capi.check(rc, "opd_test_btail_sc2")
    return y, z


def run_chain(lib, d, shape, elem):
    """The three launches: 3x3 stride 2 -> dual-source expand over [a1 | xs at stride 2] -> 1x1 reduce; (y0 bits, z bits)."""
    B, H, W = shape
    OH, OW = _out_hw(H, W)
    M = B * OH * OW
    a1, y, z = (np.full((M, n), 0xFFFF, np.uint16) for n in (C1, C2, C3))
    b = lambda k: _p(to_bits(d[k], elem))
    _capi.check(lib.opd_test_conv_gemm(b("x1"), b("w1"), _p(c32(d["b1"])), None, None, _p(a1), B, H, W, C1, OH, OW, C1, 3, 3, 2, 1, 1, 0, 0, 0), "3x3")
    _capi.check(lib.opd_test_conv_dual(_p(a1), b("w2"), b("xs"), b("wsc"), _p(c32(d["b2sc"])), _p(y), B, OH, OW, C1, 1, 1, 0, C2, H, W, CSC, 2, 1), "dual expand")
    _capi.check(lib.opd_test_conv_gemm(_p(y), b("w3"), _p(c32(d["b3"])), None, None, _p(z), B, OH, OW, C2, OH, OW, C3, 1, 1, 1, 0, 1, 0, 0, 0), "reduce")
    return y, z


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_integer_operands_exact_and_bit_identical_to_the_three_launches(lib, elem, shape):
    d = integer_case(shape)
    assert max(np.abs(d["y"]).max(), np.abs(d["z"]).max()) < E.EXACT_INT[elem] and E.nontrivial(d["y"]) and E.nontrivial(d["z"])
    y, z = run_tail(lib, d, shape, elem)
    yc, zc = run_chain(lib, d, shape, elem)
    assert np.array_equal(y, yc), "y0: fused tail against 3x3 -> dual-source expand"
    assert np.array_equal(z, zc), "z: fused tail against 3x3 -> dual-source expand -> reduce"
    assert np.array_equal(from_bits(y, elem).reshape(d["y"].shape), d["y"]), "y0 against the exact sums"
    assert np.array_equal(from_bits(z, elem).reshape(d["z"].shape), d["z"]), "z against the exact sums"


def test_form_without_the_fused_reduce(lib, elem):
    """C3 = 0 (what plan_trunk takes when stage 2 has one block): the same y0, no z."""
    shape = SHAPES[1]
    d = integer_case(shape)
    y, z = run_tail(lib, d, shape, elem, c3=0)
    assert np.array_equal(y, run_chain(lib, d, shape, elem)[0])
    assert np.array_equal(from_bits(y, elem).reshape(d["y"].shape), d["y"]) and (z == 0xFFFF).all()


def _compare_random(lib, shape):
    d = random_case(shape)
    y, z = run_tail(lib, d, shape, "fp16")
    for name, got, want in (("y0", y, d["y"]), ("z", z, d["z"])):
        got = from_bits(got, "fp16").astype(np.float64).reshape(want.shape)
        scale = float(np.abs(want).max())
        err = np.abs(got - want)
        print(f"btail_sc2 {shape} {name}: max |err| {err.max():.3e}, scale {scale:.3f}, max err / bound {(err / (2e-3 * scale + 2e-3 * np.abs(want))).max():.3f}")
        assert scale > 0.5 and np.isfinite(got).all()
        np.testing.assert_allclose(got, want, atol=2e-3 * scale, rtol=2e-3)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_random_fp16_operands_match_float64(lib, shape):
    _compare_random(lib, shape)


def test_repeated_launches_are_bit_identical(lib):
    """The race screen on the case whose tiles span frames (tile walk direction alternating between the repetitions); the last
    repetition's outputs then meet the reference bound like any other launch."""
    race_screened(lib, _compare_random, lib, SHAPES[3])


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------
TOL_BOX, TOL_PROB, TOL_ENC = 2e-3, 4e-3, 3e-2   # tests/test_detector_gpu.py: TOL[1.0], small frames against the oracle / the golden vectors
E2E = {"256x320": [(256, 320), (256, 320)], "ragged_256x320_224x288": [(256, 320), (224, 288)]}


def _softmax(x):
    x = np.asarray(x, np.float64)
    e = np.exp(x - x.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


@functools.lru_cache(maxsize=None)
def _frames(tag):
    return tuple(structured_frames(1, h, w, seed=4100 + i)[0] for i, (h, w) in enumerate(E2E[tag]))


_ORACLE = {}


def _oracle(tag, path):
    if tag not in _ORACLE:
        from oracle import detr_oracle as O
        pv, pm = O.preprocess(list(_frames(tag)))
        _ORACLE[tag] = tuple(t.numpy() for t in O.forward(O.to_torch(load_safetensors(path)), pv, pm))
    return _ORACLE[tag]


def _forward(lib, handle, canvas, valid, Q, ncls, hw):
    B, H, W, _ = canvas.shape
    lg, bx, enc = np.empty((B, Q, ncls), np.float32), np.empty((B, Q, 4), np.float32), np.empty((B, hw, 256), np.float32)
    _capi.check(lib.opd_detr_forward_ragged(handle, _p(canvas), _capi.OPD_PIXELS_U8_BGR_HWC, _capi.OPD_MEM_HOST, B, H, W, _p(valid), _p(lg), _p(bx), _p(enc)),
                "opd_detr_forward_ragged")
    return lg, bx, enc


@pytest.mark.parametrize("sc2", [1, 0], ids=["sc2_tail", "dual_expand"])
@pytest.mark.parametrize("tag", list(E2E))
def test_end_to_end_both_routes(lib, weight_cache, monkeypatch, tag, sc2):
    monkeypatch.setenv("OPD_SC2_TAIL", str(sc2))
    path = ensure_weight_file(weight_cache, DetrArch(), 0, 1.0, "r50")
    frames = _frames(tag)
    canvas = np.zeros((2, 256, 320, 3), np.uint8)
    for i, f in enumerate(frames):
        canvas[i, :f.shape[0], :f.shape[1]] = f
    valid = np.asarray([f.shape[:2] for f in frames], np.int32)
    cfg = _capi.OpdConfig(struct_size=C.sizeof(_capi.OpdConfig), max_batch=2, max_height=256, max_width=320, flags=0)
    src, dup = C.c_void_p(), C.c_void_p()
    _capi.check(lib.opd_detr_create(C.byref(cfg), path.encode(), 0, C.byref(src)), "create")
    try:
        info = _capi.OpdModelInfo()
        _capi.check(lib.opd_detr_info(src, C.byref(info)), "info")
        shape = (info.num_queries, info.num_classes_plus1, 8 * 10)
        runs = [_forward(lib, src, canvas, valid, *shape) for _ in range(3)]   # eager, capture, replay
        _capi.check(lib.opd_detr_clone(src, C.byref(dup)), "clone")
        runs += [_forward(lib, dup, canvas, valid, *shape) for _ in range(3)]
    finally:
        if dup:
            lib.opd_detr_destroy(dup)
        lib.opd_detr_destroy(src)
    for k, name in enumerate(("capture", "replay", "clone eager", "clone capture", "clone replay"), 1):
        for a, b in zip(runs[0], runs[k]):
            assert np.array_equal(a, b), f"{name} differs from the created handle's eager forward"
    lg, bx, enc = runs[0]
    olg, obx, oenc = _oracle(tag, path)
    dbox, dprob, denc = float(np.abs(bx - obx).max()), float(np.abs(_softmax(lg) - _softmax(olg)).max()), float(np.abs(enc - oenc).max())
    print(f"btail_sc2 end to end {tag} OPD_SC2_TAIL={sc2}: |dbox| {dbox:.3e} |dprob| {dprob:.3e} |denc| {denc:.3e}")
    assert dbox <= TOL_BOX and dprob <= TOL_PROB and denc <= TOL_ENC


SC2_KERNEL = "btail_kernel<128, 128, false, true, false, 0>"


def test_the_switch_selects_the_kernel_and_the_routes_agree_bit_for_bit(lib, weight_cache, monkeypatch):
    """OPD_SC2_TAIL really selects the route: the kernel table of a profiled forward names the new instantiation once with the switch on and not
    at all with it off, where the dual-source expand appears instead.  Both routes round a1 and y0 once and sum the expand's products in the
    same order (bias, a1's k-blocks, then the block input's), so the model outputs come out with the same bits."""
    path = ensure_weight_file(weight_cache, DetrArch(), 0, 1.0, "r50")
    canvas = np.ascontiguousarray(np.stack(_frames("256x320")))
    out, names = {}, {}
    for sc2 in (0, 1):
        monkeypatch.setenv("OPD_SC2_TAIL", str(sc2))
        cfg = _capi.OpdConfig(struct_size=C.sizeof(_capi.OpdConfig), max_batch=2, max_height=256, max_width=320, flags=0)
        h = C.c_void_p()
        _capi.check(lib.opd_detr_create(C.byref(cfg), path.encode(), 0, C.byref(h)), "create")
        try:
            _capi.check(lib.opd_detr_set_profiling(h, 1), "opd_detr_set_profiling")
            out[sc2] = _forward(lib, h, canvas, None, 100, 92, 80)
            rows, n = (_capi.OpdKernelStat * 256)(), C.c_int()
            _capi.check(lib.opd_detr_kernel_table(h, rows, 256, C.byref(n)), "opd_detr_kernel_table")
            names[sc2] = {rows[i].name.decode(): int(rows[i].launches) for i in range(min(n.value, 256))}
        finally:
            lib.opd_detr_destroy(h)
    assert names[1].get(SC2_KERNEL) == 1 and SC2_KERNEL not in names[0], (sorted(names[0]), sorted(names[1]))
    assert sum(names[0].values()) == sum(names[1].values()) + 2   # 3x3, dual-source expand and reduce became one launch
    for a, b in zip(out[0], out[1]):
        assert np.array_equal(a, b)
