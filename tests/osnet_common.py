"""Shared pieces of the OSNet Re-ID tests (test_osnet_cpu.py, test_osnet_gpu.py) and tools/gen_osnet_golden.py: an fp32 torch restatement
of torchreid's OSNet (eval mode, torchreid's module and state-dict names), the reference's crop + torchvision pre-processing written
with Pillow directly (ToPILImage -> Resize((256, 128)) bilinear -> ToTensor -> Normalize), and an fp16-emulating restatement of the
device forward (the rounding points of csrc/kernels_osnet.hip) that the feature bounds were set from."""

from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

import reid_common as R
from office_person_detection_vit_amd.weights import OSNET_SETS, synth_osnet_weights

OSNET_H, OSNET_W = 256, 128
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)

# Feature bounds of the device against the restatement's goldens (unit features).  emulate_device below measured max |d| = EMU_MAX_ABS and
# 1 - cos = EMU_ONE_MINUS_COS (the larger of the mild and sharp sets, 37 golden boxes); the bounds are 3x those and no looser, so that
# a misplaced rounding point, a wrong fold or a swapped stream shows.  test_osnet_cpu.py re-measures the emulation and checks it.
EMU_MAX_ABS, EMU_ONE_MINUS_COS = 1.7e-3, 1.2e-5
FEAT_MAX_ABS, FEAT_MIN_COS = 3 * EMU_MAX_ABS, 1.0 - 3 * EMU_ONE_MINUS_COS

# The same 3x rule per weight set: x1.0 (mild, sharp) above; the x0.5 widths (half) and the odd widths (odd) measured by emulate_device
# on their own goldens.  test_osnet_cpu.py re-measures every row.
EMU_BY_SET = {"mild": (EMU_MAX_ABS, EMU_ONE_MINUS_COS), "sharp": (EMU_MAX_ABS, EMU_ONE_MINUS_COS), "half": (1.6e-3, 8.5e-6),
              "odd": (1.3e-3, 8.0e-6)}


def feat_bounds(tag):
    """(max |d|, min cos) the device's features must meet against the golden of weight set `tag`."""
    d, c = EMU_BY_SET[tag]
    return 3 * d, 1.0 - 3 * c


# ---- the model: torchreid osnet.py restated (eval mode) -----------------------------------------------------------------------------
class ConvLayer(nn.Module):
    def __init__(self, cin, cout, k, stride=1, padding=0, groups=1):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, k, stride=stride, padding=padding, bias=False, groups=groups)
        self.bn = nn.BatchNorm2d(cout)
        self.relu = nn.ReLU(inplace=True)

    def forward(self, x):
        return self.relu(self.bn(self.conv(x)))


class Conv1x1(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, 1, bias=False)
        self.bn = nn.BatchNorm2d(cout)
        self.relu = nn.ReLU(inplace=True)

    def forward(self, x):
        return self.relu(self.bn(self.conv(x)))


class Conv1x1Linear(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, 1, bias=False)
        self.bn = nn.BatchNorm2d(cout)

    def forward(self, x):
        return self.bn(self.conv(x))


class LightConv3x3(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, cout, 1, bias=False)
        self.conv2 = nn.Conv2d(cout, cout, 3, padding=1, bias=False, groups=cout)
        self.bn = nn.BatchNorm2d(cout)
        self.relu = nn.ReLU(inplace=True)

    def forward(self, x):
        return self.relu(self.bn(self.conv2(self.conv1(x))))


class ChannelGate(nn.Module):
    def __init__(self, cin, reduction=16):
        super().__init__()
        self.global_avgpool = nn.AdaptiveAvgPool2d(1)
        self.fc1 = nn.Conv2d(cin, cin // reduction, 1, bias=True)
        self.relu = nn.ReLU(inplace=True)
        self.fc2 = nn.Conv2d(cin // reduction, cin, 1, bias=True)
        self.gate_activation = nn.Sigmoid()

    def forward(self, x):
        g = self.gate_activation(self.fc2(self.relu(self.fc1(self.global_avgpool(x)))))
        return x * g


class OSBlock(nn.Module):
    def __init__(self, cin, cout, bottleneck_reduction=4):
        super().__init__()
        mid = cout // bottleneck_reduction
        self.conv1 = Conv1x1(cin, mid)
        self.conv2a = LightConv3x3(mid, mid)
        self.conv2b = nn.Sequential(*[LightConv3x3(mid, mid) for _ in range(2)])
        self.conv2c = nn.Sequential(*[LightConv3x3(mid, mid) for _ in range(3)])
        self.conv2d = nn.Sequential(*[LightConv3x3(mid, mid) for _ in range(4)])
        self.gate = ChannelGate(mid)
        self.conv3 = Conv1x1Linear(mid, cout)
        self.downsample = Conv1x1Linear(cin, cout) if cin != cout else None

    def forward(self, x):
        identity = x
        x1 = self.conv1(x)
        x2 = self.gate(self.conv2a(x1)) + self.gate(self.conv2b(x1)) + self.gate(self.conv2c(x1)) + self.gate(self.conv2d(x1))
        x3 = self.conv3(x2)
        if self.downsample is not None:
            identity = self.downsample(identity)
        return F.relu(x3 + identity)


class OSNet(nn.Module):
    """torchreid OSNet with ``classifier`` replaced by nn.Identity (the reference's model): forward -> fc output (512)."""

    def __init__(self, widths=(64, 256, 384, 512), layers=(2, 2, 2), feature_dim=512):
        super().__init__()
        self.conv1 = ConvLayer(3, widths[0], 7, stride=2, padding=3)
        self.maxpool = nn.MaxPool2d(3, stride=2, padding=1)
        self.conv2 = self._make_layer(layers[0], widths[0], widths[1], True)
        self.conv3 = self._make_layer(layers[1], widths[1], widths[2], True)
        self.conv4 = self._make_layer(layers[2], widths[2], widths[3], False)
        self.conv5 = Conv1x1(widths[3], widths[3])
        self.global_avgpool = nn.AdaptiveAvgPool2d(1)
        self.fc = nn.Sequential(nn.Linear(widths[3], feature_dim), nn.BatchNorm1d(feature_dim), nn.ReLU(inplace=True))
        self.classifier = nn.Identity()

    @staticmethod
    def _make_layer(n, cin, cout, reduce):
        layers = [OSBlock(cin, cout)] + [OSBlock(cout, cout) for _ in range(1, n)]
        if reduce:
            layers.append(nn.Sequential(Conv1x1(cout, cout), nn.AvgPool2d(2, stride=2)))
        return nn.Sequential(*layers)

    def forward(self, x):
        x = self.maxpool(self.conv1(x))
        x = self.conv5(self.conv4(self.conv3(self.conv2(x))))
        v = self.global_avgpool(x).view(x.size(0), -1)
        return self.classifier(self.fc(v))


def osnet_model(tag):
    arch, seed, gain = OSNET_SETS[tag]
    w = synth_osnet_weights(arch, seed, gain)
    m = OSNet(arch.widths, (arch.blocks,) * 3, arch.feature_dim).eval()
    missing, unexpected = m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=False)
    assert not unexpected and all(k.endswith("num_batches_tracked") for k in missing), (missing, unexpected)
    return m, w


def osnet_features(model, pixels):
    """forward + L2 normalisation, as the reference (reid_feature_extractor.py:336-339), rounded to float32.  The module's fp32
    weights and the fp32 pixels are evaluated in float64: fp32 convolutions on the CPU sum in an order that depends on the instruction
    set and the thread count, so an fp32 forward does not reproduce bit for bit from one machine to the next, while the float64
    result rounded to float32 does (its own summation-order error is about 1e-16, far below half an fp32 ulp)."""
    import copy
    with torch.no_grad():
        f = copy.deepcopy(model).double()(pixels.double())
    return (f / f.norm(dim=-1, keepdim=True)).float().numpy()


# ---- the reference's pre-processing ---------------------------------------------------------------------------------------------------
def reference_crops(frame, boxes):
    """reid_feature_extractor.py:313-321: crop, BGR -> RGB; an empty crop is a 256 x 128 zero image."""
    crops = []
    H, W = frame.shape[:2]
    for x, y, w, h in boxes:
        x, y, w, h = float(x), float(y), float(w), float(h)
        x1, y1 = int(max(0, x)), int(max(0, y))
        x2, y2 = int(min(W, x + w)), int(min(H, y + h))
        if x2 <= x1 or y2 <= y1:
            crops.append(np.zeros((OSNET_H, OSNET_W, 3), np.uint8))
        else:
            crops.append(np.ascontiguousarray(frame[y1:y2, x1:x2][..., ::-1]))
    return crops


def pil_pixels(crops):
    """torchvision ToPILImage -> Resize((256, 128)) (PIL bilinear: img.resize((128, 256), BILINEAR)) -> ToTensor -> Normalize, fp32
    [n][3][256][128]."""
    from PIL import Image
    mean = torch.as_tensor(MEAN, dtype=torch.float32)[:, None, None]
    std = torch.as_tensor(STD, dtype=torch.float32)[:, None, None]
    out = []
    for c in crops:
        img = Image.fromarray(c).resize((OSNET_W, OSNET_H), Image.BILINEAR)
        t = torch.from_numpy(np.asarray(img).copy()).permute(2, 0, 1).contiguous().to(torch.float32).div(255)
        out.append(t.sub_(mean).div_(std))
    return torch.stack(out)


def reference_pixels(frames, boxes, owner):
    crops = []
    for i in range(len(boxes)):
        crops += reference_crops(frames[int(owner[i])], boxes[i:i + 1])
    return pil_pixels(crops)


def to_device_layout(pixels):
    """[n][3][256][128] fp32 -> the device's [n][256][128][4] fp16 bits (channel 3 zero)."""
    x = pixels.permute(0, 2, 3, 1).numpy().astype(np.float16)
    out = np.zeros(x.shape[:3] + (4,), np.float16)
    out[..., :3] = x
    return out.view(np.uint16)


# ---- fp16 emulation of the device forward ------------------------------------------------------------------------------------------------
def _h(t):
    return t.to(torch.float16).to(torch.float32)


def _fold(W, p):
    sc = W[p + ".weight"] / torch.sqrt(W[p + ".running_var"] + 1e-5)
    return sc, W[p + ".bias"] - W[p + ".running_mean"] * sc


def emulate_device(w, pixels, blocks=2):
    """The device forward with its rounding points (kernels_osnet.hip), fp32 torch on the CPU: BN folded in fp32, 1x1 and stem weights
    rounded to fp16, every stored activation rounded to fp16 (stem, max-pool, conv1, each LightConv's 1x1 and depthwise output, x2,
    block outputs, transitions and their pools, conv5), gates, depthwise weights, the head and the L2 norm in fp32."""
    W = {k: torch.from_numpy(v) for k, v in w.items()}

    def c1x1(x, p, bn_p=None):
        sc, sh = _fold(W, bn_p or p + ".bn")
        return F.conv2d(x, _h(W[p + ".conv.weight"] * sc[:, None, None, None])) + sh[None, :, None, None]

    def light(x, p):
        u = _h(F.conv2d(x, _h(W[p + ".conv1.weight"])))
        sc, sh = _fold(W, p + ".bn")
        return _h(F.relu(F.conv2d(u, W[p + ".conv2.weight"] * sc[:, None, None, None], padding=1, groups=u.shape[1]) + sh[None, :, None, None]))

    def gate(y, p):
        g = F.relu(F.conv2d(y.mean((2, 3), keepdim=True), W[p + ".fc1.weight"], W[p + ".fc1.bias"]))
        return torch.sigmoid(F.conv2d(g, W[p + ".fc2.weight"], W[p + ".fc2.bias"]))

    def block(x, p):
        x1 = _h(F.relu(c1x1(x, p + ".conv1")))
        x2 = 0
        for s, depth in (("a", 1), ("b", 2), ("c", 3), ("d", 4)):
            y = x1
            for j in range(depth):
                y = light(y, f"{p}.conv2a" if s == "a" else f"{p}.conv2{s}.{j}")
            x2 = x2 + gate(y, p + ".gate") * y
        x2 = _h(x2)
        z = c1x1(x2, p + ".conv3")
        z = z + (c1x1(x, p + ".downsample") if (p + ".downsample.conv.weight") in W else x)
        return _h(F.relu(z))

    with torch.no_grad():
        sc, sh = _fold(W, "conv1.bn")
        x = _h(pixels)
        x = _h(F.relu(F.conv2d(x, _h(W["conv1.conv.weight"] * sc[:, None, None, None]), stride=2, padding=3) + sh[None, :, None, None]))
        x = F.max_pool2d(x, 3, 2, 1)
        for s, pool in (("conv2", True), ("conv3", True), ("conv4", False)):
            for i in range(blocks):
                x = block(x, f"{s}.{i}")
            if pool:
                x = _h(F.avg_pool2d(_h(F.relu(c1x1(x, f"{s}.{blocks}.0"))), 2, 2))
        x = _h(F.relu(c1x1(x, "conv5"))).mean((2, 3))
        sc, sh = _fold(W, "fc.1")
        y = F.relu(F.linear(x, W["fc.0.weight"] * sc[:, None], (W["fc.0.bias"] - W["fc.1.running_mean"]) * sc + W["fc.1.bias"]))
        return (y / y.norm(dim=-1, keepdim=True)).numpy()


golden_frames = R.golden_frames
golden_boxes = R.golden_boxes
drift = R.drift
PIXEL_BOXES = R.PIXEL_BOXES
