"""Seeded synthetic DETR weights + the state-dict schema of the detect path.

Pretrained ``facebook/detr-resnet-50`` weights cannot be fetched here (no network), and
the reference loads them by NAME (``config.yaml.disabled:34``; deleted
``vit_detector.py`` ``load_model`` 81-99, see ``coverage.json:1``).  Parity work therefore
uses weights built locally from a seed.  HF default init is degenerate (every query emits
the same box), so the recipe below is engineered to be non-degenerate:

* zero-sum (per output channel) Kaiming conv kernels, FrozenBN with O(1) statistics and the
  last BN γ of every bottleneck scaled by 0.1 (mimics zero-init-γ training),
* an *attention gain* ``g_a`` multiplying every q/k projection so softmax is not uniform; residual-branch
  outputs (``o_proj``, ``fc2``) at half strength and a calibrated ``input_projection`` bias that centres the
  encoder tokens, so tokens and queries stay diverse through 6+6 post-LN layers,
* ``query_position_embeddings ~ N(0,1)``, classifier std ×2 with a bias towards the COCO
  "person" class (id 1) so that the reference's person filter has survivors.

* every tensor a GEMM consumes in fp16 is made exactly fp16-representable as the device sees it ("fold FBN
  in fp32 first, then round, so the CPU fp32 reference and the GPU use bit-identical weights and only activation rounding
  differs"): linear weights are rounded to fp16 values, convolution kernels are adjusted so that kernel x FrozenBN scale — the
  folded kernel the device stores — is an fp16 value (``make_device_exact``).  Without this the comparison measured mostly the
  fp16 rounding of the weights themselves, a systematic error a real checkpoint has too but one that says nothing about the
  kernels: at 800x1333 it was 5-7e-4 of the 6-8e-4 box error of the whole backbone (tools/drift_split.py).

Everything is drawn from ``numpy.random.default_rng`` (PCG64: bit-stable across machines), so
the exact same tensors are regenerated on the GPU box.  Tensor names/shapes follow the HF 5.x
``DetrForObjectDetection`` state dict; the file format is ``safetensors``, which
is what a real checkpoint ships as and what ``csrc/opd_loader.cpp`` parses natively.
"""

from __future__ import annotations

import json
import os
import struct
from collections import OrderedDict
from dataclasses import dataclass
from typing import Dict, Iterator, Tuple

import numpy as np

PERSON_LABEL = 1  # COCO id of "person" in DETR's 91(+1)-way label space


@dataclass(frozen=True)
class DetrArch:
    """Architecture hyper-parameters of the detect path (HF ``DetrConfig`` / ``ResNetConfig``)."""

    depths: Tuple[int, int, int, int] = (3, 4, 6, 3)  # r50; r101 = (3, 4, 23, 3)
    hidden_sizes: Tuple[int, int, int, int] = (256, 512, 1024, 2048)
    embedding_size: int = 64
    d_model: int = 256
    heads: int = 8
    ffn_dim: int = 2048
    encoder_layers: int = 6
    decoder_layers: int = 6
    num_queries: int = 100
    num_labels: int = 91

    @staticmethod
    def resnet50() -> "DetrArch":
        return DetrArch()

    @staticmethod
    def resnet101() -> "DetrArch":
        return DetrArch(depths=(3, 4, 23, 3))

    @staticmethod
    def tiny() -> "DetrArch":
        """Reduced-depth variant used by fast CPU tests (same kernels, fewer layers)."""
        return DetrArch(depths=(1, 1, 1, 1), encoder_layers=1, decoder_layers=1, num_queries=20)


_BN = ("weight", "bias", "running_mean", "running_var")


def param_specs(arch: DetrArch) -> Iterator[Tuple[str, Tuple[int, ...], str]]:
    """Yield ``(name, shape, kind)`` for every tensor of the detect path, in HF module order.

    kinds: conv_relu / conv_lin (backbone convs followed / not followed by ReLU), bn, bn_last
    (the third BN of a bottleneck), proj_w/proj_b, lin_relu/lin/lin_qk (+ ``_b`` biases), ln_w/ln_b,
    query_pos, cls_w/cls_b, box_last_w.
    """
    e = "model.backbone.model.embedder.embedder"
    yield f"{e}.convolution.weight", (arch.embedding_size, 3, 7, 7), "conv_relu"
    for s in _BN:
        yield f"{e}.normalization.{s}", (arch.embedding_size,), "bn:" + s
    cin = arch.embedding_size
    for si, (depth, cout) in enumerate(zip(arch.depths, arch.hidden_sizes)):
        mid = cout // 4
        for li in range(depth):
            p = f"model.backbone.model.encoder.stages.{si}.layers.{li}"
            stride = 2 if (li == 0 and si > 0) else 1
            if li == 0 and (cin != cout or stride != 1):
                yield f"{p}.shortcut.convolution.weight", (cout, cin, 1, 1), "conv_lin"
                for s in _BN:
                    yield f"{p}.shortcut.normalization.{s}", (cout,), "bn:" + s
            yield f"{p}.layer.0.convolution.weight", (mid, cin, 1, 1), "conv_relu"
            for s in _BN:
                yield f"{p}.layer.0.normalization.{s}", (mid,), "bn:" + s
            yield f"{p}.layer.1.convolution.weight", (mid, mid, 3, 3), "conv_relu"
            for s in _BN:
                yield f"{p}.layer.1.normalization.{s}", (mid,), "bn:" + s
            yield f"{p}.layer.2.convolution.weight", (cout, mid, 1, 1), "conv_lin"
            for s in _BN:
                yield f"{p}.layer.2.normalization.{s}", (cout,), "bn_last:" + s
            cin = cout
    d, f = arch.d_model, arch.ffn_dim
    yield "model.input_projection.weight", (d, arch.hidden_sizes[-1], 1, 1), "proj_w"
    yield "model.input_projection.bias", (d,), "bias"
    yield "model.query_position_embeddings.weight", (arch.num_queries, d), "query_pos"

    def attn(prefix: str):
        for nm in ("k_proj", "v_proj", "q_proj", "o_proj"):
            kind = "lin_qk" if nm in ("q_proj", "k_proj") else ("lin_branch" if nm == "o_proj" else "lin")
            yield f"{prefix}.{nm}.weight", (d, d), kind
            yield f"{prefix}.{nm}.bias", (d,), "bias"

    def ln(prefix: str):
        yield f"{prefix}.weight", (d,), "ln_w"
        yield f"{prefix}.bias", (d,), "ln_b"

    for i in range(arch.encoder_layers):
        p = f"model.encoder.layers.{i}"
        yield from attn(f"{p}.self_attn")
        yield from ln(f"{p}.self_attn_layer_norm")
        yield f"{p}.mlp.fc1.weight", (f, d), "lin_relu"
        yield f"{p}.mlp.fc1.bias", (f,), "bias"
        yield f"{p}.mlp.fc2.weight", (d, f), "lin_branch"
        yield f"{p}.mlp.fc2.bias", (d,), "bias"
        yield from ln(f"{p}.final_layer_norm")
    for i in range(arch.decoder_layers):
        p = f"model.decoder.layers.{i}"
        yield from attn(f"{p}.self_attn")
        yield from ln(f"{p}.self_attn_layer_norm")
        yield from attn(f"{p}.encoder_attn")
        yield from ln(f"{p}.encoder_attn_layer_norm")
        yield f"{p}.mlp.fc1.weight", (f, d), "lin_relu"
        yield f"{p}.mlp.fc1.bias", (f,), "bias"
        yield f"{p}.mlp.fc2.weight", (d, f), "lin_branch"
        yield f"{p}.mlp.fc2.bias", (d,), "bias"
        yield from ln(f"{p}.final_layer_norm")
    yield from ln("model.decoder.layernorm")
    yield "class_labels_classifier.weight", (arch.num_labels + 1, d), "cls_w"
    yield "class_labels_classifier.bias", (arch.num_labels + 1,), "cls_b"
    yield "bbox_predictor.layers.0.weight", (d, d), "lin_relu"
    yield "bbox_predictor.layers.0.bias", (d,), "bias"
    yield "bbox_predictor.layers.1.weight", (d, d), "lin_relu"
    yield "bbox_predictor.layers.1.bias", (d,), "bias"
    yield "bbox_predictor.layers.2.weight", (4, d), "box_last_w"
    yield "bbox_predictor.layers.2.bias", (4,), "bias"


def _round_mantissa(a: np.ndarray, bits: int = 12) -> np.ndarray:
    """Round fp32 values to ``bits`` explicit mantissa bits (round-to-nearest-even on the bit pattern)."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    drop = 23 - bits
    u = (u + ((1 << (drop - 1)) - 1) + ((u >> drop) & 1)) >> drop << drop
    return u.astype(np.uint32).view(np.float32)


def calibrate_frozen_bn(weights: "OrderedDict[str, np.ndarray]", arch: DetrArch, height: int = 320, width: int = 416,
                        n_frames: int = 2, frame_seed: int = 4321) -> None:
    """Set every FrozenBN's ``running_mean/var`` to the statistics of its own input on a calibration batch.

    Without this the synthetic backbone's stage-4 map is dominated by a spatially constant component and every
    encoder token (hence every query) collapses to the same value.  The pass runs in **fp64**
    (torch CPU) and the statistics are rounded to 12 mantissa bits, so the resulting fp32 tensors are
    bit-identical on any host: fp64 summation-order noise (1e-16) cannot move a 12-bit rounding.
    """
    import torch
    import torch.nn.functional as F

    from .frames import structured_frames

    frames = structured_frames(n_frames, height, width, seed=frame_seed)
    mean = np.array([0.485, 0.456, 0.406])
    std = np.array([0.229, 0.224, 0.225])
    x = np.stack([(f[:, :, ::-1].astype(np.float64) / 255.0 - mean) / std for f in frames]).transpose(0, 3, 1, 2)
    x = torch.from_numpy(np.ascontiguousarray(x))

    def conv_bn(x, prefix, stride, relu):
        cw = torch.from_numpy(weights[prefix + ".convolution.weight"]).double()
        y = F.conv2d(x, cw, None, stride=stride, padding=cw.shape[-1] // 2)
        m = y.mean(dim=(0, 2, 3))
        v = y.var(dim=(0, 2, 3), unbiased=False) + 1e-3
        m32 = _round_mantissa(m.numpy().astype(np.float32))
        v32 = _round_mantissa(v.numpy().astype(np.float32))
        weights[prefix + ".normalization.running_mean"] = m32
        weights[prefix + ".normalization.running_var"] = v32
        g = torch.from_numpy(weights[prefix + ".normalization.weight"]).double()
        b = torch.from_numpy(weights[prefix + ".normalization.bias"]).double()
        scale = g / torch.sqrt(torch.from_numpy(v32).double() + 1e-5)
        y = y * scale.view(1, -1, 1, 1) + (b - torch.from_numpy(m32).double() * scale).view(1, -1, 1, 1)
        return F.relu(y) if relu else y

    with torch.no_grad():
        x = conv_bn(x, "model.backbone.model.embedder.embedder", 2, True)
        x = F.max_pool2d(x, 3, 2, 1)
        for si, depth in enumerate(arch.depths):
            for li in range(depth):
                p = f"model.backbone.model.encoder.stages.{si}.layers.{li}"
                stride = 2 if (li == 0 and si > 0) else 1
                res = x
                if (p + ".shortcut.convolution.weight") in weights:
                    res = conv_bn(x, p + ".shortcut", stride, False)
                h = conv_bn(x, p + ".layer.0", 1, True)
                h = conv_bn(h, p + ".layer.1", stride, True)
                h = conv_bn(h, p + ".layer.2", 1, False)
                x = F.relu(h + res)
        # centre the encoder input: input_projection.bias -= W . E[stage-4 features]
        pw = torch.from_numpy(weights["model.input_projection.weight"][:, :, 0, 0]).double()
        shift = (pw @ x.mean(dim=(0, 2, 3))).numpy().astype(np.float32)
        weights["model.input_projection.bias"] = _round_mantissa(weights["model.input_projection.bias"] - shift)


def synth_weights(arch: DetrArch = DetrArch(), seed: int = 0, attention_gain: float = 2.0,
                  calibrate: bool = True, device_exact: bool = True) -> "OrderedDict[str, np.ndarray]":
    """Build the seeded, non-degenerate fp32 weight set (see module docstring).

    ``device_exact=False`` skips ``make_device_exact``: ordinary fp32 tensors, as a real checkpoint has them — the device
    then rounds every GEMM operand to fp16 itself, and the parity figure includes that weight rounding (the unfavourable case
    the tests report next to the device-exact one).

    One ``default_rng(seed)`` stream drives every tensor in ``param_specs`` order, then FrozenBN statistics are
    calibrated (``calibrate_frozen_bn``), so the result is a pure function of ``(arch, seed, attention_gain)``.
    """
    rng = np.random.default_rng(seed)
    out: "OrderedDict[str, np.ndarray]" = OrderedDict()

    def normal(shape, std):
        return (rng.standard_normal(shape, dtype=np.float32) * np.float32(std)).astype(np.float32)

    def uniform(shape, lo, hi):
        return (rng.random(shape, dtype=np.float32) * np.float32(hi - lo) + np.float32(lo)).astype(np.float32)

    for name, shape, kind in param_specs(arch):
        if kind in ("conv_relu", "conv_lin"):
            fan_in = shape[1] * shape[2] * shape[3]
            w = normal(shape, np.sqrt((2.0 if kind == "conv_relu" else 1.0) / fan_in))
            w -= w.mean(axis=(1, 2, 3), keepdims=True)  # zero-sum kernels: no mean/std cancellation in BN
            t = w
        elif kind.startswith("bn"):
            which = kind.split(":")[1]
            if which == "weight":
                t = uniform(shape, 0.8, 1.2)
                if kind.startswith("bn_last"):
                    t *= np.float32(0.1)
            elif which == "bias":
                t = normal(shape, 0.05)
            elif which == "running_mean":
                t = normal(shape, 0.05)
            else:  # running_var
                t = uniform(shape, 0.8, 1.2)
        elif kind == "proj_w":
            t = normal(shape, np.sqrt(1.0 / shape[1]))
        elif kind == "bias":
            t = normal(shape, 0.02)
        elif kind == "query_pos":
            t = normal(shape, 1.0)
        elif kind in ("lin", "lin_qk", "lin_relu", "lin_branch"):
            t = normal(shape, np.sqrt((2.0 if kind == "lin_relu" else 1.0) / shape[1]))
            if kind == "lin_qk":
                t *= np.float32(attention_gain)
            if kind == "lin_branch":  # residual-branch outputs at half strength keep tokens/queries diverse
                t *= np.float32(0.5)
        elif kind == "ln_w":
            t = uniform(shape, 0.8, 1.2)
        elif kind == "ln_b":
            t = normal(shape, 0.05)
        elif kind == "cls_w":
            t = normal(shape, 2.0 * np.sqrt(1.0 / shape[1]))
        elif kind == "cls_b":
            t = normal(shape, 0.02)
            t[PERSON_LABEL] += np.float32(6.0)
        elif kind == "box_last_w":
            t = normal(shape, 2.0 * np.sqrt(1.0 / shape[1]))
        else:  # pragma: no cover
            raise ValueError(kind)
        out[name] = np.ascontiguousarray(t, dtype=np.float32)
    if calibrate:
        calibrate_frozen_bn(out, arch)
    if device_exact:
        make_device_exact(out)
    return out


RECIPE_VERSION = 2   # bump when the tensors of a (arch, seed, gain) triple change: cached files of older recipes are not reused


def make_device_exact(weights: "OrderedDict[str, np.ndarray]") -> None:
    """Make every fp16 GEMM operand of the device path exactly representable (module docstring).

    * 2-D weights of the transformer linears and ``input_projection`` (consumed as fp16): rounded to the nearest fp16 value.
    * convolution kernels: the device folds FrozenBN in fp32, ``w * (gamma * 1/sqrt(var + 1e-5))`` (``csrc/opd_weights.cpp::make_conv``),
      and stores THAT in fp16.  The kernel is replaced by ``fp16(w * scale) / scale`` (fp64 division, stored fp32): the fold then
      lands within 2e-7 relative of an fp16 value and rounds to it, while the fp32 reference, which keeps kernel and scale apart,
      computes with the same number to fp32 accuracy.
    The fp32-consumed tensors (biases, norms, the heads' weights, the query embeddings) stay as drawn."""
    for name in list(weights):
        t = weights[name]
        if name.endswith(".convolution.weight"):
            pre = name[: -len(".convolution.weight")] + ".normalization"
            var = weights[pre + ".running_var"].astype(np.float32)
            scale = (weights[pre + ".weight"].astype(np.float32) * (np.float32(1.0) / np.sqrt(var + np.float32(1e-5)))).astype(np.float32)
            sc = scale.reshape(-1, 1, 1, 1)
            with np.errstate(over="ignore"):
                folded = (t * sc).astype(np.float32).astype(np.float16)
            weights[name] = np.ascontiguousarray((folded.astype(np.float64) / sc.astype(np.float64)).astype(np.float32))
        elif t.ndim >= 2 and name.endswith(".weight") and name.startswith(("model.encoder.", "model.decoder.", "model.input_projection.")):
            weights[name] = np.ascontiguousarray(t.astype(np.float16).astype(np.float32))


# ----------------------------------------------------------------------------------------------
# safetensors I/O (format: u64 LE header length, JSON header, raw little-endian tensor bytes).
# Written by hand (numpy only) so the byte layout the native loader parses is explicit here.
# ----------------------------------------------------------------------------------------------

def save_safetensors(weights: Dict[str, np.ndarray], path: str) -> None:
    header: Dict[str, dict] = {}
    off = 0
    for name, t in weights.items():
        assert t.dtype == np.float32
        n = t.size * 4
        header[name] = {"dtype": "F32", "shape": list(t.shape), "data_offsets": [off, off + n]}
        off += n
    hb = json.dumps(header, separators=(",", ":")).encode("utf-8")
    hb += b" " * ((8 - len(hb) % 8) % 8)
    tmp = path + f".tmp{os.getpid()}"
    with open(tmp, "wb") as f:
        f.write(struct.pack("<Q", len(hb)))
        f.write(hb)
        for t in weights.values():
            f.write(np.ascontiguousarray(t).tobytes())
    os.replace(tmp, path)


def load_safetensors(path: str) -> "OrderedDict[str, np.ndarray]":
    with open(path, "rb") as f:
        (hl,) = struct.unpack("<Q", f.read(8))
        header = json.loads(f.read(hl).decode("utf-8"))
        base = 8 + hl
        out: "OrderedDict[str, np.ndarray]" = OrderedDict()
        dt = {"F32": np.float32, "F16": np.float16, "F64": np.float64}
        for name, meta in header.items():
            if name == "__metadata__":
                continue
            a, b = meta["data_offsets"]
            f.seek(base + a)
            arr = np.frombuffer(f.read(b - a), dtype=dt[meta["dtype"]]).reshape(meta["shape"])
            out[name] = arr.astype(np.float32)
    return out


# HF 4.x checkpoint names -> 5.x names used throughout this repo (HF:conversion_mapping.py:1036-1041).
_RENAMES_4X = (
    ("model.backbone.conv_encoder.", "model.backbone."),
    (".out_proj.", ".o_proj."),
)


def rename_4x_key(name: str) -> str:
    for a, b in _RENAMES_4X:
        name = name.replace(a, b)
    for fc in ("fc1", "fc2"):
        tok = f".{fc}."
        if tok in name and ".mlp." not in name and ".layers." in name and name.startswith(("model.encoder", "model.decoder")):
            name = name.replace(tok, f".mlp.{fc}.")
    return name


def ensure_weight_file(cache_dir: str, arch: DetrArch = DetrArch(), seed: int = 0, attention_gain: float = 2.0,
                       tag: str = "r50", device_exact: bool = True) -> str:
    """Write (once) and return the path of the safetensors file for a seeded weight set."""
    os.makedirs(cache_dir, exist_ok=True)
    kind = "" if device_exact else "_raw"   # (part of the cache key: the two sets differ in every GEMM weight)
    path = os.path.join(cache_dir, f"detr_{tag}_seed{seed}_ga{attention_gain:g}_v{RECIPE_VERSION}{kind}.safetensors")
    if not os.path.exists(path):
        tmp = path + f".tmp{os.getpid()}"
        save_safetensors(synth_weights(arch, seed, attention_gain, device_exact=device_exact), tmp)
        os.replace(tmp, path)   # (atomic: several ranks may generate the same file at once)
    return path


# ----------------------------------------------------------------------------------------------
# CLIP ViT image tower (the Re-ID path, reid.py): seeded synthetic weights under the HF
# ``CLIPVisionModelWithProjection`` key names (``vision_model.*`` + ``visual_projection.weight``).
# ----------------------------------------------------------------------------------------------

@dataclass(frozen=True)
class ClipArch:
    hidden: int = 768
    layers: int = 12
    heads: int = 12
    mlp: int = 3072
    patch: int = 32
    image: int = 224
    proj: int = 512

    @staticmethod
    def vit_b32() -> "ClipArch":
        return ClipArch()

    @staticmethod
    def tiny() -> "ClipArch":   # kernel tests: 2 layers, hidden 128, 2 heads
        return ClipArch(hidden=128, layers=2, heads=2, mlp=512, proj=128)

    @staticmethod
    def p56() -> "ClipArch":   # patch 56 (17 tokens), hidden 256, 4 heads: the loader's non-B/32 shapes
        return ClipArch(hidden=256, layers=2, heads=4, mlp=1024, patch=56, proj=512)

    @property
    def tokens(self) -> int:
        return (self.image // self.patch) ** 2 + 1

    def hf_config(self):
        from transformers import CLIPVisionConfig
        return CLIPVisionConfig(hidden_size=self.hidden, intermediate_size=self.mlp, num_hidden_layers=self.layers,
                                num_attention_heads=self.heads, patch_size=self.patch, image_size=self.image, projection_dim=self.proj,
                                hidden_act="quick_gelu", layer_norm_eps=1e-5)


def synth_clip_weights(cfg: ClipArch = ClipArch(), seed: int = 0, attention_gain: float = 1.0) -> "OrderedDict[str, np.ndarray]":
    """Seeded fp32 CLIP vision weights.  Linear weights are N(0, 1/fan_in); q and k are multiplied by ``attention_gain``, so with
    LayerNorm'd tokens the attention logits have a standard deviation of about ``attention_gain ** 2``: 0.5 gives nearly uniform
    softmax rows ("mild"), 1.5 and above peaked ones ("sharp", where fp16 error in q / k / P shows).  Residual branches (out-proj,
    fc2) at half strength keep the stream from being dominated by one layer.  A pure function of ``(cfg, seed, attention_gain)``."""
    rng = np.random.default_rng(seed)
    out: "OrderedDict[str, np.ndarray]" = OrderedDict()
    H, F, P, T = cfg.hidden, cfg.mlp, cfg.patch, cfg.tokens

    def normal(shape, std):
        return (rng.standard_normal(shape, dtype=np.float32) * np.float32(std)).astype(np.float32)

    vm = "vision_model."
    out[vm + "embeddings.class_embedding"] = normal((H,), 1.0)
    out[vm + "embeddings.patch_embedding.weight"] = normal((H, 3, P, P), (3 * P * P) ** -0.5)
    out[vm + "embeddings.position_embedding.weight"] = normal((T, H), 0.5)
    out[vm + "pre_layrnorm.weight"] = 1.0 + normal((H,), 0.1)
    out[vm + "pre_layrnorm.bias"] = normal((H,), 0.05)
    for i in range(cfg.layers):
        p = f"{vm}encoder.layers.{i}."
        for n, gain in (("q_proj", attention_gain), ("k_proj", attention_gain), ("v_proj", 1.0), ("out_proj", 0.5)):
            out[p + f"self_attn.{n}.weight"] = normal((H, H), gain * H ** -0.5)
            out[p + f"self_attn.{n}.bias"] = normal((H,), 0.02)
        out[p + "layer_norm1.weight"] = 1.0 + normal((H,), 0.1)
        out[p + "layer_norm1.bias"] = normal((H,), 0.05)
        out[p + "mlp.fc1.weight"] = normal((F, H), H ** -0.5)
        out[p + "mlp.fc1.bias"] = normal((F,), 0.1)
        out[p + "mlp.fc2.weight"] = normal((H, F), 0.5 * F ** -0.5)
        out[p + "mlp.fc2.bias"] = normal((H,), 0.02)
        out[p + "layer_norm2.weight"] = 1.0 + normal((H,), 0.1)
        out[p + "layer_norm2.bias"] = normal((H,), 0.05)
    out[vm + "post_layernorm.weight"] = 1.0 + normal((H,), 0.1)
    out[vm + "post_layernorm.bias"] = normal((H,), 0.05)
    out["visual_projection.weight"] = normal((cfg.proj, H), H ** -0.5)
    return out


CLIP_SETS = {   # tag -> (arch, seed, attention_gain): the weight sets the Re-ID tests and goldens use
    "mild": (ClipArch.vit_b32(), 11, 0.5),
    "sharp": (ClipArch.vit_b32(), 12, 1.6),
    "tiny": (ClipArch.tiny(), 13, 1.0),
    "p56": (ClipArch.p56(), 14, 1.0),
}


def ensure_clip_weight_file(cache_dir: str, tag: str = "mild") -> str:
    """Write (once) and return the path of the safetensors file of one of ``CLIP_SETS``."""
    cfg, seed, gain = CLIP_SETS[tag]
    os.makedirs(cache_dir, exist_ok=True)
    path = os.path.join(cache_dir, f"clip_{tag}_seed{seed}_ga{gain:g}_h{cfg.hidden}_l{cfg.layers}.safetensors")
    if not os.path.exists(path):
        tmp = path + f".tmp{os.getpid()}"
        save_safetensors(synth_clip_weights(cfg, seed, gain), tmp)
        os.replace(tmp, path)
    return path


# ----------------------------------------------------------------------------------------------
# OSNet (the second Re-ID model, reid.py HipOSNetReIDExtractor): seeded synthetic weights under
# torchreid's ``osnet_x1_0`` key names, BN running statistics calibrated on frame crops.
# ----------------------------------------------------------------------------------------------

@dataclass(frozen=True)
class OsnetArch:
    widths: Tuple[int, int, int, int] = (64, 256, 384, 512)   # stem, conv2, conv3, conv4 (osnet_x1_0)
    blocks: int = 2                                             # OSBlocks per stage (torchreid: [2, 2, 2])
    feature_dim: int = 512

    @staticmethod
    def x1_0() -> "OsnetArch":
        return OsnetArch()

    @staticmethod
    def x0_5() -> "OsnetArch":
        return OsnetArch(widths=(32, 128, 192, 256))

    @staticmethod
    def odd() -> "OsnetArch":   # every branch osnet_x1_0 misses: stem 16, streams 16 / 48 / 80 wide, gate hidden 1 / 3 / 5, one block
        return OsnetArch(widths=(16, 64, 192, 320), blocks=1)


def osnet_param_specs(arch: OsnetArch) -> Iterator[Tuple[str, Tuple[int, ...], str]]:
    """(key, shape, kind) of every float tensor of torchreid's OSNet state dict without ``classifier.*``, in module order;
    kind is conv / bn / gate_w / gate_b / fc_w / fc_b."""
    def bn(p, c):
        for n in _BN:
            yield f"{p}.{n}", (c,), "bn"

    def conv(p, cout, cin, k=1, groups=1):
        yield f"{p}.weight", (cout, cin // groups, k, k), "conv"

    def conv_bn(p, cout, cin, k=1):
        yield from conv(p + ".conv", cout, cin, k)
        yield from bn(p + ".bn", cout)

    def light(p, m):
        yield from conv(p + ".conv1", m, m)
        yield from conv(p + ".conv2", m, m, 3, m)
        yield from bn(p + ".bn", m)

    def block(p, cin, cout):
        mid = cout // 4
        yield from conv_bn(p + ".conv1", mid, cin)
        yield from light(p + ".conv2a", mid)
        for s, depth in (("b", 2), ("c", 3), ("d", 4)):
            for j in range(depth):
                yield from light(f"{p}.conv2{s}.{j}", mid)
        yield f"{p}.gate.fc1.weight", (mid // 16, mid, 1, 1), "gate_w"
        yield f"{p}.gate.fc1.bias", (mid // 16,), "gate_b"
        yield f"{p}.gate.fc2.weight", (mid, mid // 16, 1, 1), "gate_w"
        yield f"{p}.gate.fc2.bias", (mid,), "gate_b"
        yield from conv_bn(p + ".conv3", cout, mid)
        if cin != cout:
            yield from conv_bn(p + ".downsample", cout, cin)

    c0, c2, c3, c4 = arch.widths
    yield from conv_bn("conv1", c0, 3, 7)
    cin = c0
    for s, cout, pool in (("conv2", c2, True), ("conv3", c3, True), ("conv4", c4, False)):
        for i in range(arch.blocks):
            yield from block(f"{s}.{i}", cin, cout)
            cin = cout
        if pool:
            yield from conv_bn(f"{s}.{arch.blocks}.0", cout, cout)
    yield from conv_bn("conv5", c4, c4)
    yield "fc.0.weight", (arch.feature_dim, c4), "fc_w"
    yield "fc.0.bias", (arch.feature_dim,), "fc_b"
    yield from bn("fc.1", arch.feature_dim)


def _osnet_calibrate(w: "OrderedDict[str, np.ndarray]", arch: OsnetArch, crops: np.ndarray) -> None:
    """Set every BN's running statistics to the batch statistics of its input on ``crops`` ([n][3][256][128] normalised), in fp64:
    each BN then maps its channels to about N(beta, gamma^2), so no channel is dead or saturated.  Statistics are rounded to 12
    mantissa bits so that the file does not depend on the last bit of a threaded fp64 reduction."""
    import torch
    import torch.nn.functional as F

    T = lambda k: torch.from_numpy(w[k]).double()

    def bn(x, p, relu):
        dims = [0, 2, 3] if x.dim() == 4 else [0]
        mean, var = x.mean(dims), x.var(dims, unbiased=False)
        w[p + ".running_mean"] = _round_mantissa(mean.float().numpy())
        w[p + ".running_var"] = _round_mantissa(var.float().numpy())
        shape = [1, -1] + [1] * (x.dim() - 2)
        y = (x - T(p + ".running_mean").view(shape)) / torch.sqrt(T(p + ".running_var").view(shape) + 1e-5)
        y = y * T(p + ".weight").view(shape) + T(p + ".bias").view(shape)
        return F.relu(y) if relu else y

    def conv_bn(x, p, relu=True, stride=1, pad=0):
        return bn(F.conv2d(x, T(p + ".conv.weight"), stride=stride, padding=pad), p + ".bn", relu)

    def light(x, p):
        m = x.shape[1]
        x = F.conv2d(x, T(p + ".conv1.weight"))
        return bn(F.conv2d(x, T(p + ".conv2.weight"), padding=1, groups=m), p + ".bn", True)

    def gate(x, p):
        g = F.relu(F.conv2d(x.mean((2, 3), keepdim=True), T(p + ".fc1.weight"), T(p + ".fc1.bias")))
        return x * torch.sigmoid(F.conv2d(g, T(p + ".fc2.weight"), T(p + ".fc2.bias")))

    def block(x, p):
        x1 = conv_bn(x, p + ".conv1")
        x2 = 0
        for s, depth in (("a", 1), ("b", 2), ("c", 3), ("d", 4)):
            y = x1
            for j in range(depth):
                y = light(y, f"{p}.conv2a" if s == "a" else f"{p}.conv2{s}.{j}")
            x2 = x2 + gate(y, p + ".gate")
        x3 = conv_bn(x2, p + ".conv3", relu=False)
        ident = conv_bn(x, p + ".downsample", relu=False) if (p + ".downsample.conv.weight") in w else x
        return F.relu(x3 + ident)

    with torch.no_grad():
        x = torch.from_numpy(crops).double()
        x = F.max_pool2d(conv_bn(x, "conv1", stride=2, pad=3), 3, 2, 1)
        for s, pool in (("conv2", True), ("conv3", True), ("conv4", False)):
            for i in range(arch.blocks):
                x = block(x, f"{s}.{i}")
            if pool:
                x = F.avg_pool2d(conv_bn(x, f"{s}.{arch.blocks}.0"), 2, 2)
        x = conv_bn(x, "conv5").mean((2, 3))
        bn(F.linear(x, T("fc.0.weight"), T("fc.0.bias")), "fc.1", True)


def osnet_calibration_crops(n: int = 8) -> np.ndarray:
    """n crops [n][3][256][128] (ImageNet-normalised fp32) of person-sized windows of structured frames: the BN calibration input."""
    from .frames import structured_frames
    frames = structured_frames(2, 512, 640, seed=97)
    mean = np.array([0.485, 0.456, 0.406], np.float32)[:, None, None]
    std = np.array([0.229, 0.224, 0.225], np.float32)[:, None, None]
    out = np.zeros((n, 3, 256, 128), np.float32)
    for i in range(n):
        f = frames[i % 2]
        y, x = 40 * (i // 2), 120 * (i // 2) + 20
        crop = f[y:y + 256, x:x + 128, ::-1].transpose(2, 0, 1).astype(np.float32) / np.float32(255)
        out[i] = (crop - mean) / std
    return out


def synth_osnet_weights(arch: OsnetArch = OsnetArch(), seed: int = 0, gain: float = 1.0) -> "OrderedDict[str, np.ndarray]":
    """Seeded fp32 OSNet weights under torchreid's key names.  Convolutions are N(0, 2 / fan_in); BN gammas are ``gain`` * (1 +
    0.1 N), betas 0.1 N, gate fc weights N(0, gain^2 / fan_in) with biases 0.1 N; running statistics are calibrated on frame crops
    (_osnet_calibrate).  The gamma of each block's conv3 BN (the residual branch) is quartered: at full strength the random network
    amplifies a 1e-4 input perturbation to 1e-4 in 1 - cos of the features, and no fp16 path could be told apart from a wrong one.  ``gain`` 1 gives a "mild" set; larger gains sharpen the gates towards 0 / 1 and widen the BN outputs, so a
    wrong gate, stream or fold shows in the features.  A pure function of ``(arch, seed, gain)``."""
    rng = np.random.default_rng(seed)
    out: "OrderedDict[str, np.ndarray]" = OrderedDict()

    def normal(shape, std):
        return (rng.standard_normal(shape, dtype=np.float32) * np.float32(std)).astype(np.float32)

    for key, shape, kind in osnet_param_specs(arch):
        if kind in ("conv", "fc_w"):
            fan_in = int(np.prod(shape[1:]))
            out[key] = normal(shape, (2.0 / fan_in) ** 0.5)
        elif kind == "gate_w":
            out[key] = normal(shape, gain * shape[1] ** -0.5)
        elif kind in ("gate_b", "fc_b"):
            out[key] = normal(shape, 0.1)
        elif key.endswith(".weight"):   # BN gamma; an OSBlock's conv3 (its residual branch) at quarter strength
            out[key] = gain * (1.0 + normal(shape, 0.1)) * np.float32(0.25 if key.endswith("conv3.bn.weight") else 1.0)
        elif key.endswith(".bias"):
            out[key] = normal(shape, 0.1)
        elif key.endswith(".running_mean"):
            out[key] = np.zeros(shape, np.float32)
        else:
            out[key] = np.ones(shape, np.float32)
    _osnet_calibrate(out, arch, osnet_calibration_crops())
    return out


OSNET_SETS = {   # tag -> (arch, seed, gain): the weight sets the OSNet tests and goldens use
    "mild": (OsnetArch.x1_0(), 21, 1.0),
    "sharp": (OsnetArch.x1_0(), 22, 2.5),
    "half": (OsnetArch.x0_5(), 23, 1.0),
    "odd": (OsnetArch.odd(), 24, 1.0),
}


def ensure_osnet_weight_file(cache_dir: str, tag: str = "mild") -> str:
    """Write (once) and return the path of the safetensors file of one of ``OSNET_SETS``."""
    arch, seed, gain = OSNET_SETS[tag]
    os.makedirs(cache_dir, exist_ok=True)
    path = os.path.join(cache_dir, f"osnet_{tag}_seed{seed}_g{gain:g}_w{'-'.join(map(str, arch.widths))}.safetensors")
    if not os.path.exists(path):
        tmp = path + f".tmp{os.getpid()}"
        save_safetensors(synth_osnet_weights(arch, seed, gain), tmp)
        os.replace(tmp, path)
    return path
