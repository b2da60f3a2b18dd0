"""CPU-only tests of the Re-ID path (no GPU): goldens reproduce from HF, the host-side crop geometry follows the reference's
expressions, the Pillow bicubic tables and the normalisation table match Pillow / HF, the host restatement of the pre-processing
kernel equals HF `pixel_values` in fp16 bit for bit, schema refusals need no device, DETR loading is unaffected."""

import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import reid_common as R
from office_person_detection_vit_amd import _capi
from office_person_detection_vit_amd.weights import ClipArch, save_safetensors, synth_clip_weights


@pytest.fixture(scope="module")
def lib():
    return _capi.load_library(test_hooks=True)


def _hook_geometry(lib, boxes, H, W):
    b = np.ascontiguousarray(np.asarray(boxes, np.float32).reshape(-1, 4))
    out = np.zeros((len(b), 13), np.int32)
    assert lib.opd_test_reid_geometry(b.ctypes.data, len(b), H, W, out.ctypes.data) == 0
    return b, out


def test_golden_reproduces_from_hf(golden_dir):
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    frames = R.golden_frames()
    for tag in ("mild", "sharp", "tiny", "p56"):
        g = np.load(os.path.join(golden_dir, f"reid_{tag}.npz"))
        assert int(g["frame_seed"]) == R.FRAME_SEED and tuple(g["frame_hw"]) == (R.FRAME_H, R.FRAME_W)
        boxes, owner = R.golden_boxes()
        np.testing.assert_array_equal(g["boxes"], boxes)
        np.testing.assert_array_equal(g["owner"], owner)
        model, _ = R.hf_model(tag)
        feats = R.hf_features(model, R.hf_pixel_values(frames, boxes, owner))
        np.testing.assert_array_equal(feats.astype(np.float32), g["features"])


def test_crop_geometry_matches_reference_expressions(lib):
    H, W = 720, 1280
    rng = np.random.default_rng(5)
    boxes = list(R.PIXEL_BOXES) + [(-5.0, -5.0, 3.0, 3.0), (1279.9, 719.9, 5.0, 5.0), (10.99, 20.01, 0.99, 100.0), (0.0, 0.0, 1.0, 1.0)]
    boxes += [tuple(v) for v in np.stack([rng.uniform(-100, 1300, 200), rng.uniform(-100, 800, 200), rng.uniform(0, 800, 200),
                                          rng.uniform(0, 800, 200)], 1)]
    b, out = _hook_geometry(lib, boxes, H, W)
    for i, (x, y, w, h) in enumerate(b.astype(np.float64)):   # the float32 boxes the C-ABI receives, widened as Python does
        x1, y1 = int(max(0, x)), int(max(0, y))
        x2, y2 = int(min(W, x + w)), int(min(H, y + h))
        zero = x2 <= x1 or y2 <= y1
        assert tuple(out[i, :5]) == (x1, y1, x2, y2, int(zero)), (i, b[i])
        if zero:
            continue
        ch, cw = y2 - y1, x2 - x1
        short, long = (cw, ch) if cw <= ch else (ch, cw)
        nl = int(224 * long / short)
        rh, rw = (nl, 224) if cw <= ch else (224, nl)
        assert tuple(out[i, 5:9]) == (rh, rw, (rh - 224) // 2, (rw - 224) // 2), (i, b[i])
        wy0, wx0, wy1, wx1 = out[i, 9:]
        assert y1 <= wy0 < wy1 <= y2 and x1 <= wx0 < wx1 <= x2   # the window lies inside the crop


def _pillow_coeffs(in_size, out_size, bicubic=True):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc (bicubic a = -0.5 or bilinear), restated in Python doubles."""
    def f(x):
        a = -0.5
        x = abs(x)
        if not bicubic:
            return 1.0 - x if x < 1.0 else 0.0
        if x < 1.0:
            return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
        if x < 2.0:
            return (((x - 5) * x + 8) * x - 4) * a
        return 0.0
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = (2.0 if bicubic else 1.0) * fs
    rows = []
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        k = [f((x + xmin - center + 0.5) / fs) for x in range(xmax)]
        ww = sum(k)
        k = [v / ww if ww != 0.0 else v for v in k]
        rows.append((xmin, xmax, [int(-0.5 + v * (1 << 22)) if v < 0 else int(0.5 + v * (1 << 22)) for v in k]))
    return rows


@pytest.mark.parametrize("in_size,out_size", [(40, 224), (700, 224), (1, 5), (300, 301), (1280, 398), (9, 224)])
def test_bicubic_tables_match_pillow_formula(lib, in_size, out_size):
    first, count = 0, out_size
    cap = 64
    bounds = np.zeros((count, 2), np.int32)
    coeffs = np.zeros((count, cap), np.int32)
    ks = lib.opd_test_reid_coeffs(in_size, out_size, first, count, bounds.ctypes.data, coeffs.ctypes.data, cap)
    assert ks > 0
    for i, (xmin, n, k) in enumerate(_pillow_coeffs(in_size, out_size)):
        assert (bounds[i, 0], bounds[i, 1]) == (xmin, n)
        assert list(coeffs[i, :n]) == k


def test_bilinear_tables_unchanged(lib):
    """The detector's bilinear tables come from the same (now filter-generic) routine: still Pillow's triangle filter."""
    for in_size, out_size in ((720, 800), (1280, 1333), (100, 37)):
        bounds = np.zeros((out_size, 2), np.int32)
        coeffs = np.zeros(out_size * 64, np.int32)
        ks = lib.opd_test_resize_coeffs(in_size, out_size, bounds.ctypes.data, coeffs.ctypes.data, coeffs.size)
        assert ks > 0
        coeffs = coeffs[:out_size * ks].reshape(out_size, ks)
        for i, (xmin, n, k) in enumerate(_pillow_coeffs(in_size, out_size, bicubic=False)):
            assert (bounds[i, 0], bounds[i, 1]) == (xmin, n)
            assert list(coeffs[i, :n]) == k


def test_normalisation_table_matches_hf(lib):
    from transformers import CLIPImageProcessorPil
    lut = np.zeros(768, np.uint16)
    assert lib.opd_test_reid_lut(lut.ctypes.data) == 0
    img = np.zeros((224, 224, 3), np.uint8)
    img.reshape(-1, 3)[:256] = np.arange(256, dtype=np.uint8)[:, None]
    pv = CLIPImageProcessorPil()(images=[img], return_tensors="pt")["pixel_values"][0]   # 224 x 224: no resize, no crop
    ref = pv.reshape(3, -1)[:, :256].numpy().astype(np.float16).view(np.uint16)
    np.testing.assert_array_equal(lut.reshape(3, 256), ref)


def test_host_preprocess_equals_hf_pixels_fp16(lib):
    frames = R.golden_frames()
    f = np.ascontiguousarray(frames[0])
    boxes = np.asarray(R.PIXEL_BOXES, np.float32)
    n = len(boxes)
    out = np.zeros((n, 50, 3072), np.uint16)
    assert lib.opd_test_reid_pixels_host(f.ctypes.data, f.shape[0], f.shape[1], boxes.ctypes.data, n, 32, 50, out.ctypes.data) == 0
    ref = R.to_patch_rows(R.hf_pixel_values(frames, boxes, np.zeros(n, np.int32))).numpy().astype(np.float16).view(np.uint16)
    for i in range(n):
        np.testing.assert_array_equal(out[i], ref[i], err_msg=f"box {i}: {R.PIXEL_BOXES[i]}")


def test_fp16_emulation_within_feature_bounds():
    """The bounds test_reid_gpu.py asserts (reid_common.FEAT_MAX_ABS / FEAT_MIN_COS on unit features) hold for the device's rounding
    points restated in torch (reid_common.emulate_device) against HF fp32, on both weight sets."""
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    frames = R.golden_frames()
    boxes, owner = R.golden_boxes(12)
    pv = R.hf_pixel_values(frames, boxes, owner)
    for tag in ("mild", "sharp"):
        model, w = R.hf_model(tag)
        d, cos = R.drift(R.emulate_device(w, pv), R.hf_features(model, pv))
        assert d <= R.FEAT_MAX_ABS and cos >= R.FEAT_MIN_COS, (tag, d, cos)


def test_fp16_emulation_within_feature_bounds_small_sets(golden_dir):
    """The per-set bounds of the tiny (hidden 128) and p56 (patch 56, 17 tokens) sets: emulate_device against their goldens, all 37
    boxes, within reid_common.EMU_BY_SET and not far below it (the constants are not slack)."""
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    frames = R.golden_frames()
    boxes, owner = R.golden_boxes()
    pv = R.hf_pixel_values(frames, boxes, owner)
    for tag, (emu_d, emu_c) in R.EMU_BY_SET.items():
        g = np.load(os.path.join(golden_dir, f"reid_{tag}.npz"))
        _, w = R.hf_model(tag)
        d, cos = R.drift(R.emulate_device(w, pv), g["features"])
        assert d <= emu_d and 1.0 - cos <= emu_c, (tag, d, 1.0 - cos)
        assert d >= emu_d / 2 and 1.0 - cos >= emu_c / 3, (tag, d, 1.0 - cos)


def _write_clip(tmp_path, cfg, name="model.safetensors", heads=None):
    d = tmp_path / name.replace(".", "_")
    d.mkdir()
    path = str(d / name)
    save_safetensors(synth_clip_weights(cfg, 1, 1.0), path)
    if heads is not None:
        (d / "config.json").write_text(json.dumps({"vision_config": {"num_attention_heads": heads}, "text_config": {"num_attention_heads": 8}}))
    return path


def _create(lib, path, max_crops=4):
    cfg = _capi.OpdReidConfig()
    cfg.struct_size = C.sizeof(_capi.OpdReidConfig)
    cfg.max_crops = max_crops
    h = C.c_void_p()
    rc = lib.opd_reid_create(C.byref(cfg), path.encode(), 0, C.byref(h))
    return rc, lib.opd_last_error().decode()


def test_schema_refusals_need_no_gpu(lib, tmp_path):
    # head_dim 80: hidden 160 with 2 heads named by config.json (hidden also not a multiple of 128)
    rc, msg = _create(lib, _write_clip(tmp_path, ClipArch(hidden=160, layers=1, heads=2, mlp=256, proj=128), heads=2))
    assert rc == _capi.OPD_ESCHEMA and "head_dim 80" in msg, msg
    # 197 tokens (ViT-B/16)
    rc, msg = _create(lib, _write_clip(tmp_path, ClipArch(hidden=128, layers=1, heads=2, mlp=256, patch=16, proj=128), "b16.safetensors"))
    assert rc == _capi.OPD_ESCHEMA and "197" in msg and "64 tokens" in msg, msg
    # hidden 192 = 3 heads of 64, not a multiple of 128
    rc, msg = _create(lib, _write_clip(tmp_path, ClipArch(hidden=192, layers=1, heads=3, mlp=256, proj=128), "h192.safetensors"))
    assert rc == _capi.OPD_ESCHEMA and "multiple of 128" in msg, msg
    # a missing tensor
    w = synth_clip_weights(ClipArch.tiny(), 1, 1.0)
    del w["vision_model.encoder.layers.1.mlp.fc2.bias"]
    p = str(tmp_path / "broken.safetensors")
    save_safetensors(w, p)
    rc, msg = _create(lib, p)
    assert rc == _capi.OPD_ESCHEMA and "fc2.bias" in msg, msg
    rc, msg = _create(lib, str(tmp_path / "absent.safetensors"))
    assert rc == _capi.OPD_EIO


def test_facade_refusals_without_gpu(tmp_path):
    from office_person_detection_vit_amd import HipReIDExtractor
    with pytest.raises(ValueError, match="osnet"):
        HipReIDExtractor(model_type="osnet")
    assert HipReIDExtractor(model_type="CLIP").model_type == "clip"   # case-insensitive, as the reference
    ex = HipReIDExtractor(model_path=str(tmp_path / "nope.safetensors"))
    with pytest.raises(FileNotFoundError, match="never downloads"):
        ex.load_model()
    assert not ex.is_loaded and ex.feature_dim == 512
    with pytest.raises(RuntimeError, match="load_model"):
        ex.extract_features(np.zeros((10, 10, 3), np.uint8), [(0, 0, 5, 5)])


def test_detr_keys_still_normalised(lib):
    """The raw-key option of the loader is the Re-ID path's only: DETR 4.x spellings are still renamed."""
    buf = C.create_string_buffer(256)
    assert lib.opd_test_normalise_key(b"model.encoder.layers.0.fc1.weight", buf, 256) >= 0
    assert buf.value.decode() == "model.encoder.layers.0.mlp.fc1.weight"
