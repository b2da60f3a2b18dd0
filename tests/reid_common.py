"""Shared pieces of the Re-ID tests (test_reid_cpu.py, test_reid_gpu.py) and tools/gen_reid_golden.py: the frames and boxes of the
goldens, the reference's crop + CLIPImageProcessor + CLIPVisionModelWithProjection path in fp32 on the CPU, and an fp16-emulating
restatement of the device forward (the rounding points of csrc/kernels_reid.hip) that the feature bounds were set from."""

from __future__ import annotations

import numpy as np
import torch

from office_person_detection_vit_amd.frames import structured_frames
from office_person_detection_vit_amd.weights import CLIP_SETS, synth_clip_weights

FRAME_H, FRAME_W = 720, 1280

# Feature bounds of the device against HF fp32 (unit features): emulate_device below measured max |d| <= 1.9e-4 and 1 - cos <= 6e-7 on
# the mild and sharp sets; the bounds allow about 3x / 5x that for the device's different accumulation order, and no more, so that a
# misplaced rounding point or a wrong epsilon shows.
FEAT_MAX_ABS, FEAT_MIN_COS = 6e-4, 0.999997
# The same rule (3x max |d|, 5x 1 - cos) for the small sets, from emulate_device against their goldens (37 boxes): tiny (hidden 128,
# patch 32) measured 1.2e-4 / 9.4e-8, p56 (hidden 256, patch 56, 17 tokens) 7.9e-5 / 1.0e-7.  test_reid_cpu.py re-measures them.
EMU_BY_SET = {"tiny": (1.2e-4, 9.4e-8), "p56": (7.9e-5, 1.0e-7)}


def feat_bounds(tag):
    """(max |d|, min cos) the device's features must meet against the golden of weight set `tag`."""
    if tag not in EMU_BY_SET:
        return FEAT_MAX_ABS, FEAT_MIN_COS
    d, c = EMU_BY_SET[tag]
    return 3 * d, 1.0 - 5 * c
FRAME_SEED = 4321
N_GOLDEN = 37

# boxes (x, y, w, h) of the pixel-exactness test: upscale, heavy downscale, 1-pixel-wide, partly off-frame, degenerate, full frame
PIXEL_BOXES = [(600.3, 300.7, 40.2, 90.9), (100.0, 20.0, 500.0, 690.0), (900.0, 100.0, 1.0, 300.0), (-30.5, 600.2, 120.0, 200.0),
               (400.0, 300.0, 0.4, 50.0), (0.0, 0.0, 1280.0, 720.0), (1250.6, -10.0, 80.0, 40.0), (700.0, 710.5, 30.0, 9.9)]


def golden_frames():
    return structured_frames(2, FRAME_H, FRAME_W, seed=FRAME_SEED)


def golden_boxes(n=N_GOLDEN, seed=77):
    """n person-like boxes over the two golden frames (a few partly off-frame, one degenerate): boxes [n][4] f32, owner frame [n]."""
    rng = np.random.default_rng(seed)
    h = rng.uniform(40, 500, n)
    w = h * rng.uniform(0.25, 0.7, n)
    x = rng.uniform(-40, FRAME_W - 20, n)
    y = rng.uniform(-30, FRAME_H - 30, n)
    boxes = np.stack([x, y, w, h], 1).astype(np.float32)
    boxes[5] = (300.0, 200.0, 0.5, 0.5)   # degenerate: a zero image
    owner = (np.arange(n) % 2).astype(np.int32)
    return boxes, owner


def reference_crops(frame, boxes):
    """The reference's cropping (reid_feature_extractor.py:124-134), BGR -> RGB via channel reversal (= cv2.COLOR_BGR2RGB)."""
    crops = []
    H, W = frame.shape[:2]
    for x, y, w, h in boxes:
        x, y, w, h = float(x), float(y), float(w), float(h)
        x1, y1 = int(max(0, x)), int(max(0, y))
        x2, y2 = int(min(W, x + w)), int(min(H, y + h))
        if x2 <= x1 or y2 <= y1:
            crop = np.zeros((224, 224, 3), dtype=np.uint8)
        else:
            crop = np.ascontiguousarray(frame[y1:y2, x1:x2][..., ::-1])
        crops.append(crop)
    return crops


def hf_pixel_values(frames, boxes, owner):
    from transformers import CLIPImageProcessorPil
    proc = CLIPImageProcessorPil()
    crops = []
    for i in range(len(boxes)):
        crops += reference_crops(frames[int(owner[i])], boxes[i:i + 1])
    return proc(images=crops, return_tensors="pt")["pixel_values"].float()


def to_patch_rows(pixel_values, patch=32):
    """[n][3][224][224] -> the device's patch rows [n][tokens][3 P P] (k = (kh, kw, c)), row 0 zero."""
    n = pixel_values.shape[0]
    g = 224 // patch
    x = pixel_values.reshape(n, 3, g, patch, g, patch).permute(0, 2, 4, 3, 5, 1).reshape(n, g * g, 3 * patch * patch)
    return torch.cat([torch.zeros(n, 1, x.shape[2], dtype=x.dtype), x], 1)


def hf_model(tag):
    from transformers import CLIPVisionModelWithProjection
    cfg, seed, gain = CLIP_SETS[tag]
    w = synth_clip_weights(cfg, seed, gain)
    m = CLIPVisionModelWithProjection(cfg.hf_config()).eval()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    return m, w


def hf_features(model, pixel_values):
    """`get_image_features` + L2 normalisation, as the reference (reid_feature_extractor.py:141-145)."""
    with torch.no_grad():
        out = model(pixel_values=pixel_values).image_embeds
    return (out / out.norm(dim=-1, keepdim=True)).numpy()


def _h(t):
    return t.to(torch.float16).to(torch.float32)


def emulate_device(w, pixel_values, heads_dim=64):
    """The device forward with its fp16 rounding points (kernels_reid.hip), in fp32 torch on the CPU: weights and every GEMM
    operand rounded to fp16, fp32 accumulation, fp32 residual stream, LayerNorm / softmax statistics in fp32."""
    vm = "vision_model."
    W = {k: torch.from_numpy(v) for k, v in w.items()}
    pe = W[vm + "embeddings.patch_embedding.weight"]
    H, P = pe.shape[0], pe.shape[2]
    pw = _h(pe.permute(0, 2, 3, 1).reshape(H, -1))
    x16 = _h(to_patch_rows(pixel_values, P))
    n, T = x16.shape[0], x16.shape[1]
    bias = W[vm + "embeddings.position_embedding.weight"].clone()
    bias[0] += W[vm + "embeddings.class_embedding"]
    x = x16 @ pw.T + bias
    ln = lambda t, p: torch.nn.functional.layer_norm(t, (H,), W[p + ".weight"], W[p + ".bias"], 1e-5)
    x = ln(x, vm + "pre_layrnorm")
    L = 0
    while f"{vm}encoder.layers.{L}.self_attn.q_proj.weight" in W:
        L += 1
    nh = H // heads_dim
    for i in range(L):
        p = f"{vm}encoder.layers.{i}."
        xn = _h(ln(x, p + "layer_norm1"))
        q = _h(xn @ _h(W[p + "self_attn.q_proj.weight"] * 0.125).T + W[p + "self_attn.q_proj.bias"] * 0.125)
        k = _h(xn @ _h(W[p + "self_attn.k_proj.weight"]).T + W[p + "self_attn.k_proj.bias"])
        v = _h(xn @ _h(W[p + "self_attn.v_proj.weight"]).T + W[p + "self_attn.v_proj.bias"])
        sp = lambda t: t.reshape(n, T, nh, heads_dim).transpose(1, 2)
        s = sp(q) @ sp(k).transpose(-1, -2)
        pr = _h(torch.softmax(s, -1))
        o = _h((pr @ sp(v)).transpose(1, 2).reshape(n, T, H))
        x = x + (o @ _h(W[p + "self_attn.out_proj.weight"]).T + W[p + "self_attn.out_proj.bias"])
        xn = _h(ln(x, p + "layer_norm2"))
        hdn = xn @ _h(W[p + "mlp.fc1.weight"]).T + W[p + "mlp.fc1.bias"]
        hdn = _h(hdn * torch.sigmoid(1.702 * hdn))
        x = x + (hdn @ _h(W[p + "mlp.fc2.weight"]).T + W[p + "mlp.fc2.bias"])
    cls = _h(ln(x[:, 0], vm + "post_layernorm"))
    f = cls @ _h(W["visual_projection.weight"]).T
    return (f / f.norm(dim=-1, keepdim=True)).numpy()


def drift(a, b):
    """max |a - b| and the smallest per-row cosine of two sets of unit rows."""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    cos = (a * b).sum(1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))
    return float(np.abs(a - b).max()), float(cos.min())
