"""Colour-histogram appearance features on one MI355X: opd_color_features on 1280 x 720 frames at 1, 21 and 160 person-sized crops per
call (21.25 detections per frame is the reference's published session average), frames in host memory and in device memory, next to
the host restatement (FeatureExtractor.extract_batch on crop_boxes, numpy) on the same box; then detect_with_features(frame) with
features="color" next to the encoder-feature mode.  Host clock around calls that end in a device wait.

    python tools/bench_color_features.py [--iters 200] [--json out.json]
"""

from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from office_person_detection_vit_amd import HipDetrDetector, _capi  # noqa: E402
from office_person_detection_vit_amd.feature_extractor import FeatureExtractor, crop_boxes  # noqa: E402
from office_person_detection_vit_amd.frames import structured_frames  # noqa: E402
from office_person_detection_vit_amd.weights import DetrArch, ensure_weight_file  # noqa: E402


def timed(call, warmup, iters):
    for _ in range(warmup):
        call()
    t = time.perf_counter()
    for _ in range(iters):
        call()
    return (time.perf_counter() - t) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--sizes", default="1,21,160")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch
    lib = _capi.load_library()
    H, W = 720, 1280
    frame = np.ascontiguousarray(structured_frames(1, H, W, seed=99)[0])
    dev_frame = torch.from_numpy(frame).cuda()
    torch.cuda.synchronize()
    hw = np.array([H, W], np.int32)
    rng = np.random.default_rng(0)
    fx = FeatureExtractor()
    rows = []
    for n in [int(s) for s in args.sizes.split(",")]:
        bw, bh = rng.uniform(40, 140, n), rng.uniform(120, 320, n)   # person-sized crops
        boxes = np.ascontiguousarray(np.stack([rng.uniform(0, W - 140, n), rng.uniform(0, H - 320, n), bw, bh], 1).astype(np.float32))
        out = np.zeros((n, 256), np.float32)
        for kind, name, ptr in ((_capi.OPD_MEM_HOST, "host", frame.ctypes.data), (_capi.OPD_MEM_DEVICE, "device", dev_frame.data_ptr())):
            ptrs = (C.c_void_p * 1)(ptr)
            call = lambda: _capi.check(lib.opd_color_features(0, ptrs, hw.ctypes.data, 1, kind, boxes.ctypes.data, None, n, out.ctypes.data),
                                       "opd_color_features")
            ms = timed(call, args.warmup, args.iters)
            rows.append({"what": "opd_color_features", "frames": name, "n": n, "ms_per_call": round(ms, 4), "crops_per_s": round(n / ms * 1e3, 1)})
            print(json.dumps(rows[-1]), flush=True)
        ms = timed(lambda: fx.extract_batch(crop_boxes(frame, boxes)), 1, max(3, args.iters // 20))
        want = fx.extract_batch(crop_boxes(frame, boxes))
        rows.append({"what": "host restatement (numpy)", "n": n, "ms_per_call": round(ms, 4), "crops_per_s": round(n / ms * 1e3, 1),
                     "max_abs_device_minus_host": float(np.abs(out.astype(np.float64) - want).max())})
        print(json.dumps(rows[-1]), flush=True)
    path = ensure_weight_file(os.environ.get("OPD_WEIGHT_CACHE", "/tmp/opd_weights"), DetrArch(), 0, 1.0, "r50")
    det = HipDetrDetector(model_path=path, max_batch=1, confidence_threshold=0.05)
    det.load_model()
    for mode in ("encoder", "color", "encoder", "color"):   # alternated: the two modes share everything but the feature kernels
        ndet = len(det.detect_with_features(frame, features=mode)[0])
        ms = timed(lambda: det.detect_with_features(frame, features=mode), args.warmup, args.iters)
        rows.append({"what": "detect_with_features", "features": mode, "frame": [H, W], "detections": ndet, "ms_per_frame": round(ms, 4)})
        print(json.dumps(rows[-1]), flush=True)
    det.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
