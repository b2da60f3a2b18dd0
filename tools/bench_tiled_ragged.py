"""Tiled detection of one 2160 x 3840 frame on a grid whose tiles differ in size (2 x 3, overlap 1/8: 6 tiles of 1215 x 1440 and 1215 x 1600, model
sizes 800 x 948 and 800 x 1053) on one handle of one MI355X: the native call (TiledDetector(native=True, mixed_sizes=True):
opd_detr_detect_tiled_ragged, the frame uploaded once, every tile resampled on the device into one zero-padded canvas, a ragged forward, the seam
merge in a kernel) against the host path it replaces (native=False: contiguous tile copies, a PIL resize per tile, the canvas built and uploaded,
suppression and merge in Python), same detector, same build, in interleaved rounds.  Both paths run the ragged forward eagerly.  The lists of the
two are asserted identical before anything is timed.  Host clock around calls that end in a device wait.  Then one profiled native call per round
for the split by stage from opd_detr_kernel_table.  --grid 3x3 runs the 9-tile grid (six window sizes) on a max_batch=9 handle instead.

    python tools/bench_tiled_ragged.py [--grid 2x3] [--rounds 7] [--iters 5] [--warmup 2] [--threshold 0.05] [--json out.json]
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

from office_person_detection_vit_amd import HipDetrDetector, TiledDetector, _capi  # noqa: E402
from office_person_detection_vit_amd.frames import structured_frames  # noqa: E402
from office_person_detection_vit_amd.tiling import tile_grid  # noqa: E402
from office_person_detection_vit_amd.weights import DetrArch, ensure_weight_file  # noqa: E402

H, W, OVERLAP = 2160, 3840, 0.125


def timed(call, iters):
    t = time.perf_counter()
    for _ in range(iters):
        call()
    return (time.perf_counter() - t) / iters * 1e3


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def fields(dets):
    return [[(d.bbox, d.confidence, d.class_id, d.camera_coords, d.query_index) for d in f] for f in dets]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", default="2x3", choices=["2x3", "3x3"])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--threshold", type=float, default=0.05)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    lib = _capi.load_library()
    cache = os.environ.get("OPD_WEIGHT_CACHE", "/tmp/opd_weights")
    rows_, cols_ = (int(v) for v in args.grid.split("x"))
    grid = tile_grid(H, W, rows_, cols_, OVERLAP)
    frames = [np.ascontiguousarray(f) for f in structured_frames(1, H, W, seed=99)]
    # the seeded weights with attention gain 2 (the tests' `sharp` set): a tile keeps several boxes and the seam merge absorbs some
    det = HipDetrDetector(model_path=ensure_weight_file(cache, DetrArch(), 0, 2.0, "r50"), max_batch=max(8, len(grid)), confidence_threshold=args.threshold)
    det.load_model()
    sizes = det.tile_model_sizes(grid)
    host = TiledDetector(det, rows_, cols_, overlap=OVERLAP, native=False)
    native = TiledDetector(det, rows_, cols_, overlap=OVERLAP, native=True, mixed_sizes=True)
    for _ in range(args.warmup):
        want = host.detect_batch(frames)
        got = native.detect_batch(frames)
    assert fields(want) == fields(got), "the native lists differ from the host path's"
    th, tn = [], []
    for _ in range(args.rounds):   # interleaved: drift of the machine lands on both
        th.append(timed(lambda: host.detect_batch(frames), args.iters))
        tn.append(timed(lambda: native.detect_batch(frames), args.iters))
    pairs = sum(n < h for n, h in zip(tn, th))
    canvas = (max(s[0] for s in sizes), max(s[1] for s in sizes))
    row = {"what": "python", "grid": args.grid, "frame": [H, W], "tile_sizes": sorted({(t[2], t[3]) for t in grid}), "model_sizes": sorted(set(sizes)), "canvas": canvas,
           "detections": [len(f) for f in want], "lists_identical": True, "native=False": stats(th), "native=True,mixed_sizes=True": stats(tn),
           "host_path_spread_ms": round(max(th) - min(th), 4), "saved_ms": round(float(np.median(th) - np.median(tn)), 4),
           "pairs_native_faster": f"{pairs} of {args.rounds}", "upload_bytes_native=False": len(grid) * canvas[0] * canvas[1] * 3, "upload_bytes_native=True": H * W * 3,
           "host_tile_copy_bytes_native=False": sum(t[2] * t[3] * 3 for t in grid)}
    print(json.dumps(row), flush=True)
    rows = [row]
    # the split by stage: profiled calls (eager launches, an event pair around each)
    _capi.check(lib.opd_detr_set_profiling(C.c_void_p(det.model), 1), "opd_detr_set_profiling")
    split = {"resize": [], "forward": [], "postprocess+nms": [], "merge": []}
    stage = {"tile_resize_ragged_u8_kernel": "resize", "tile_merge_kernel": "merge", "person_nms_kernel": "postprocess+nms", "postprocess_kernel": "postprocess+nms"}
    for r in range(1 + args.rounds):
        native.detect_batch(frames)
        tab, n = (_capi.OpdKernelStat * 256)(), C.c_int(0)
        _capi.check(lib.opd_detr_kernel_table(C.c_void_p(det.model), tab, 256, C.byref(n)), "opd_detr_kernel_table")
        acc = dict.fromkeys(split, 0.0)
        for i in range(min(n.value, 256)):
            acc[stage.get(tab[i].name.decode(), "forward")] += tab[i].ms
        if r:
            for k, v in acc.items():
                split[k].append(v)
    _capi.check(lib.opd_detr_set_profiling(C.c_void_p(det.model), 0), "opd_detr_set_profiling")
    rows.append({"what": "kernel table, native=True, mixed_sizes=True", "grid": args.grid, **{k: stats(v) for k, v in split.items()}})
    print(json.dumps(rows[-1]), flush=True)
    det.close()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump({"rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
