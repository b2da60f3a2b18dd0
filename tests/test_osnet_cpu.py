"""CPU-only tests of the OSNet Re-ID model (no GPU): the goldens reproduce from the restatement, the restatement's key set is torchreid's,
the goldens discriminate crops far beyond the asserted bounds, the fp16 emulation the bounds come from stays within them, the host
restatement of the pre-processing kernel equals Pillow + torchvision in fp16 bit for bit, the loader's refusals need no device, and
the façade dispatches by model type."""

import ctypes as C
import os

import numpy as np
import pytest
import torch

import osnet_common as O
from office_person_detection_vit_amd import HipOSNetReIDExtractor, HipReIDExtractor, _capi, create_reid_extractor
from office_person_detection_vit_amd.reid import torchreid_state_dict
from office_person_detection_vit_amd.weights import OsnetArch, save_safetensors, synth_osnet_weights


@pytest.fixture(scope="module")
def lib():
    return _capi.load_library(test_hooks=True)


@pytest.fixture(scope="module")
def mild_weights():
    return synth_osnet_weights(*_set("mild"))


def _set(tag):
    from office_person_detection_vit_amd.weights import OSNET_SETS
    return OSNET_SETS[tag]


def test_golden_reproduces(golden_dir):
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    frames = O.golden_frames()
    for tag in ("mild", "sharp", "half", "odd"):
        g = np.load(os.path.join(golden_dir, f"osnet_{tag}.npz"))
        assert int(g["frame_seed"]) == O.R.FRAME_SEED and tuple(g["frame_hw"]) == (O.R.FRAME_H, O.R.FRAME_W)
        boxes, owner = O.golden_boxes()
        np.testing.assert_array_equal(g["boxes"], boxes)
        np.testing.assert_array_equal(g["owner"], owner)
        model, _ = O.osnet_model(tag)
        feats = O.osnet_features(model, O.reference_pixels(frames, boxes, owner))
        np.testing.assert_array_equal(feats.astype(np.float32), g["features"])


def _expected_keys():
    """torchreid osnet_x1_0's state dict without classifier.*, written out: (key, shape)."""
    keys = []

    def bn(p, c):
        keys.extend([(f"{p}.weight", (c,)), (f"{p}.bias", (c,)), (f"{p}.running_mean", (c,)), (f"{p}.running_var", (c,)),
                     (f"{p}.num_batches_tracked", ())])

    def convbn(p, cout, cin, k=1):
        keys.append((f"{p}.conv.weight", (cout, cin, k, k)))
        bn(f"{p}.bn", cout)

    def light(p, m):
        keys.append((f"{p}.conv1.weight", (m, m, 1, 1)))
        keys.append((f"{p}.conv2.weight", (m, 1, 3, 3)))
        bn(f"{p}.bn", m)

    convbn("conv1", 64, 3, 7)
    cin = 64
    for stage, cout, pool in (("conv2", 256, True), ("conv3", 384, True), ("conv4", 512, False)):
        m = cout // 4
        for i in range(2):
            p = f"{stage}.{i}"
            convbn(f"{p}.conv1", m, cin)
            light(f"{p}.conv2a", m)
            for s, d in (("b", 2), ("c", 3), ("d", 4)):
                for j in range(d):
                    light(f"{p}.conv2{s}.{j}", m)
            keys += [(f"{p}.gate.fc1.weight", (m // 16, m, 1, 1)), (f"{p}.gate.fc1.bias", (m // 16,)),
                     (f"{p}.gate.fc2.weight", (m, m // 16, 1, 1)), (f"{p}.gate.fc2.bias", (m,))]
            convbn(f"{p}.conv3", cout, m)
            if cin != cout:
                convbn(f"{p}.downsample", cout, cin)
            cin = cout
        if pool:
            convbn(f"{stage}.2.0", cout, cout)
    convbn("conv5", 512, 512)
    keys += [("fc.0.weight", (512, 512)), ("fc.0.bias", (512,))]
    bn("fc.1", 512)
    return dict(keys)


def test_restatement_keys_are_torchreids(mild_weights):
    sd = O.OSNet().state_dict()
    want = _expected_keys()
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    assert {k: v.shape for k, v in mild_weights.items()} == {k: s for k, s in want.items() if not k.endswith("num_batches_tracked")}


def test_goldens_discriminate(golden_dir):
    """The smallest 1 - cos between two different non-degenerate golden crops is >= 100x the asserted bound: the bound cannot pass a
    feature of the wrong crop."""
    for tag in ("mild", "sharp", "half", "odd"):
        f = np.load(os.path.join(golden_dir, f"osnet_{tag}.npz"))["features"].astype(np.float64)
        keep = [i for i in range(len(f)) if i != 5]   # box 5 is the degenerate one
        c = f[keep] @ f[keep].T
        np.fill_diagonal(c, -1.0)
        assert 1.0 - c.max() >= 100 * (1.0 - O.FEAT_MIN_COS), (tag, 1.0 - c.max())
        assert 1.0 - c.max() >= 100 * (1.0 - O.feat_bounds(tag)[1]), (tag, 1.0 - c.max())


def test_fp16_emulation_within_feature_bounds(golden_dir):
    """The bounds are 3x what the emulation of the device's rounding points measures: re-measure and hold them to it."""
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    frames = O.golden_frames()
    boxes, owner = O.golden_boxes()
    px = O.reference_pixels(frames, boxes, owner)
    worst_d, worst_c = 0.0, 0.0
    for tag in ("mild", "sharp"):
        g = np.load(os.path.join(golden_dir, f"osnet_{tag}.npz"))
        _, w = O.osnet_model(tag)
        d, cos = O.drift(O.emulate_device(w, px), g["features"])
        worst_d, worst_c = max(worst_d, d), max(worst_c, 1.0 - cos)
    assert worst_d <= O.EMU_MAX_ABS and worst_c <= O.EMU_ONE_MINUS_COS, (worst_d, worst_c)
    assert worst_d >= O.EMU_MAX_ABS / 2 and worst_c >= O.EMU_ONE_MINUS_COS / 3, (worst_d, worst_c)   # the constants are not slack
    from office_person_detection_vit_amd.weights import OSNET_SETS
    for tag in ("half", "odd"):   # the per-set rows of osnet_common.EMU_BY_SET, held the same way
        emu_d, emu_c = O.EMU_BY_SET[tag]
        g = np.load(os.path.join(golden_dir, f"osnet_{tag}.npz"))
        _, w = O.osnet_model(tag)
        d, cos = O.drift(O.emulate_device(w, px, OSNET_SETS[tag][0].blocks), g["features"])
        assert d <= emu_d and 1.0 - cos <= emu_c, (tag, d, 1.0 - cos)
        assert d >= emu_d / 2 and 1.0 - cos >= emu_c / 3, (tag, d, 1.0 - cos)


def test_host_pixels_equal_pil(lib):
    frames = O.golden_frames()
    f = np.ascontiguousarray(frames[0])
    boxes = np.asarray(list(O.PIXEL_BOXES) + [(10.0, 10.0, 128.0, 256.0), (3.0, 5.0, 700.0, 30.0)], np.float32)
    out = np.zeros((len(boxes), 256, 128, 4), np.uint16)
    assert lib.opd_test_osnet_pixels_host(f.ctypes.data, 720, 1280, boxes.ctypes.data, len(boxes), out.ctypes.data) == 0
    ref = O.to_device_layout(O.reference_pixels([f], boxes, np.zeros(len(boxes), np.int32)))
    for i in range(len(boxes)):
        np.testing.assert_array_equal(out[i], ref[i], err_msg=f"box {i}: {boxes[i]}")


def test_normalisation_table_is_torch_fp32(lib):
    lut = np.zeros(768, np.uint16)
    assert lib.opd_test_osnet_lut(lut.ctypes.data) == 0
    v = torch.arange(256, dtype=torch.uint8).to(torch.float32).div(255)
    for c in range(3):
        want = v.sub(torch.tensor(O.MEAN[c], dtype=torch.float32)).div(torch.tensor(O.STD[c], dtype=torch.float32))
        np.testing.assert_array_equal(lut[c * 256:(c + 1) * 256], want.numpy().astype(np.float16).view(np.uint16))


# ---- loader refusals -------------------------------------------------------------------------------------------------------------------
def _create(lib, path, model=_capi.OPD_REID_MODEL_OSNET):
    cfg = _capi.OpdReidConfig()
    cfg.struct_size = C.sizeof(_capi.OpdReidConfig)
    cfg.max_crops = 4
    cfg.model = model
    h = C.c_void_p()
    rc = lib.opd_reid_create(C.byref(cfg), path.encode(), 0, C.byref(h))
    if rc == 0:
        lib.opd_reid_destroy(h)
    return rc, _capi.last_error()


def _write(tmp_path, w, name):
    p = str(tmp_path / name)
    save_safetensors(w, p)
    return p


def test_loader_refusals_without_gpu(lib, tmp_path, mild_weights):
    w = dict(mild_weights)
    del w["conv3.1.conv2c.2.bn.running_var"]
    rc, msg = _create(lib, _write(tmp_path, w, "missing.safetensors"))
    assert rc == _capi.OPD_ESCHEMA and "conv3.1.conv2c.2.bn.running_var" in msg, msg
    # osnet_x0_75: stage widths 192, 288, 384 (288 / 4 = 72 channels per stream)
    w75 = synth_osnet_weights(OsnetArch(widths=(48, 192, 288, 384)), 1, 1.0)
    rc, msg = _create(lib, _write(tmp_path, w75, "x075.safetensors"))
    assert rc == _capi.OPD_ESCHEMA and "multiple of 16" in msg, msg
    w = dict(mild_weights)
    w["fc.0.weight"] = np.zeros((256, 512), np.float32)
    rc, msg = _create(lib, _write(tmp_path, w, "fc256.safetensors"))
    assert rc == _capi.OPD_ESCHEMA and "512" in msg, msg
    # instance norm (osnet_ain / ibn): conv1.bn with affine parameters and no running statistics
    w = {k: v for k, v in mild_weights.items() if not k.startswith("conv1.bn.running_")}
    rc, msg = _create(lib, _write(tmp_path, w, "ain.safetensors"))
    assert rc == _capi.OPD_ESCHEMA and "instance-norm" in msg, msg
    w = dict(mild_weights)
    w["conv2.0.IN.weight"] = np.ones(256, np.float32)
    w["conv2.0.IN.bias"] = np.zeros(256, np.float32)
    rc, msg = _create(lib, _write(tmp_path, w, "ibn.safetensors"))
    assert rc == _capi.OPD_ESCHEMA and "instance-norm" in msg, msg
    ok = _write(tmp_path, mild_weights, "mild.safetensors")
    for bad in (2, -1):
        rc, msg = _create(lib, ok, model=bad)
        assert rc == _capi.OPD_EINVAL and "OPD_REID_MODEL_OSNET" in msg, msg
    # a CLIP handle on an OSNet file names what it lacks
    rc, msg = _create(lib, ok, model=_capi.OPD_REID_MODEL_CLIP)
    assert rc == _capi.OPD_ESCHEMA and "CLIP" in msg, msg


def test_pth_checkpoint_loads_to_the_same_tensors(tmp_path, mild_weights):
    """A torchreid-style checkpoint (state_dict wrapped, DataParallel `module.` prefix, a 751-class classifier, integer counters) reads
    as the same tensors as the safetensors file."""
    sd = {"module." + k: torch.from_numpy(v.copy()) for k, v in mild_weights.items()}
    sd["module.classifier.weight"] = torch.zeros(751, 512)
    sd["module.classifier.bias"] = torch.zeros(751)
    sd["module.conv1.bn.num_batches_tracked"] = torch.tensor(7)
    p = str(tmp_path / "osnet.pth.tar")
    torch.save({"state_dict": sd, "epoch": 1}, p)
    got = torchreid_state_dict(p)
    assert set(got) == set(mild_weights)
    for k, v in mild_weights.items():
        np.testing.assert_array_equal(got[k], v)
    torch.save({k[7:]: v for k, v in sd.items()}, str(tmp_path / "plain.pth"))   # a bare state dict works too
    assert set(torchreid_state_dict(str(tmp_path / "plain.pth"))) == set(mild_weights)


# ---- façade --------------------------------------------------------------------------------------------------------------------------------
def test_facade_dispatch_and_refusals(tmp_path):
    assert isinstance(create_reid_extractor("clip"), HipReIDExtractor)
    assert type(create_reid_extractor("CLIP")) is HipReIDExtractor
    ex = create_reid_extractor("OSNet", model_path=str(tmp_path / "w.safetensors"))
    assert isinstance(ex, HipOSNetReIDExtractor) and ex.model_type == "osnet" and ex.feature_dim == 512 and not ex.is_loaded
    with pytest.raises(ValueError, match="'clip' or 'osnet'"):
        create_reid_extractor("resnet18")
    with pytest.raises(ValueError, match="osnet"):
        HipReIDExtractor(model_type="osnet")
    with pytest.raises(FileNotFoundError, match="never downloads"):
        HipOSNetReIDExtractor().load_model()
    with pytest.raises(FileNotFoundError, match="does not exist"):
        ex.load_model()
    with pytest.raises(RuntimeError, match="load_model"):
        ex.extract_features(np.zeros((10, 10, 3), np.uint8), [(0, 0, 5, 5)])
