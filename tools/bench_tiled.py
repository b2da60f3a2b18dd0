"""Tiled detection of 2160 x 3840 frames (2 x 2 tiles, overlap 1/8: BASELINE.json configs[4]) on one handle of one MI355X: the native call
(TiledDetector(native=True): opd_detr_detect_tiled, frames uploaded once, tiles resampled in place, seam merge in a kernel) against the host
path it replaces (native=False: contiguous tile copies, their upload, per-tile lists and the Python merge), same detector, same build, in
interleaved rounds.  The host path is the yardstick and its own round-to-round spread the margin.  Host clock around calls that end in a
device wait.  Then one profiled native call per round (an event pair around every launch) for the split by stage from
opd_detr_kernel_table: resize, forward, post-process + per-tile suppression, merge; the upload is a copy, not a launch, and appears as
the bytes each path sends.  Last, tile_merge_kernel alone on synthetic loads of 100 to 1024 candidates per frame (opd_detr_merge_tiles).

    python tools/bench_tiled.py [--frames 2] [--rounds 5] [--iters 10] [--warmup 3] [--threshold 0.05] [--json out.json]
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

H, W, ROWS, COLS, OVERLAP = 2160, 3840, 2, 2, 0.125


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
    ap.add_argument("--frames", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--threshold", type=float, default=0.05)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    lib = _capi.load_library()
    cache = os.environ.get("OPD_WEIGHT_CACHE", "/tmp/opd_weights")
    grid = tile_grid(H, W, ROWS, COLS, OVERLAP)
    frames = [np.ascontiguousarray(f) for f in structured_frames(args.frames, H, W, seed=99)]
    det = HipDetrDetector(model_path=ensure_weight_file(cache, DetrArch(), 0, 1.0, "r50"), max_batch=args.frames * len(grid), confidence_threshold=args.threshold)
    det.load_model()
    host, native = TiledDetector(det, ROWS, COLS, overlap=OVERLAP, native=False), TiledDetector(det, ROWS, COLS, overlap=OVERLAP, native=True)
    for _ in range(args.warmup):
        want = host.detect_batch(frames)
        got = native.detect_batch(frames)
    same = fields(want) == fields(got)
    th, tn = [], []
    for _ in range(args.rounds):   # interleaved: drift of the machine lands on both
        th.append(timed(lambda: host.detect_batch(frames), args.iters))
        tn.append(timed(lambda: native.detect_batch(frames), args.iters))
    pairs = sum(n < h for n, h in zip(tn, th))
    row = {"what": "python", "frames": args.frames, "frame": [H, W], "tiles": [list(t) for t in grid], "detections": [len(f) for f in want], "lists_identical": same,
           "native=False": stats(th), "native=True": stats(tn), "host_path_spread_ms": round(max(th) - min(th), 4),
           "saved_ms": round(float(np.median(th) - np.median(tn)), 4), "pairs_native_faster": f"{pairs} of {args.rounds}",
           "upload_bytes_native=False": args.frames * sum(t[2] * t[3] * 3 for t in grid), "upload_bytes_native=True": args.frames * H * W * 3,
           "host_tile_copy_bytes_native=False": args.frames * sum(t[2] * t[3] * 3 for t in grid)}
    print(json.dumps(row), flush=True)
    rows = [row]
    # the split by stage: profiled calls (eager launches, an event pair around each)
    _capi.check(lib.opd_detr_set_profiling(C.c_void_p(det.model), 1), "opd_detr_set_profiling")
    split = {"resize": [], "forward": [], "postprocess+nms": [], "merge": []}
    stage = {"tile_resize_u8_kernel": "resize", "tile_merge_kernel": "merge", "person_nms_kernel": "postprocess+nms", "postprocess_kernel": "postprocess+nms"}
    for r in range(1 + args.rounds):
        native.detect_batch(frames)
        tab, n = (_capi.OpdKernelStat * 256)(), C.c_int(0)
        _capi.check(lib.opd_detr_kernel_table(C.c_void_p(det.model), tab, 256, C.byref(n)), "opd_detr_kernel_table")
        acc = dict.fromkeys(split, 0.0)
        for i in range(min(n.value, 256)):
            acc[stage.get(tab[i].name.decode(), "forward")] += tab[i].ms
        if r:   # (the first profiled call drops the captured graph)
            for k, v in acc.items():
                split[k].append(v)
    _capi.check(lib.opd_detr_set_profiling(C.c_void_p(det.model), 0), "opd_detr_set_profiling")
    rows.append({"what": "kernel table, native=True", "frames": args.frames, **{k: stats(v) for k, v in split.items()}})
    print(json.dumps(rows[-1]), flush=True)
    # the merge kernel alone under load (opd_detr_merge_tiles on synthetic per-tile records, its row of the kernel table): the calls above give it
    # a handful of candidates; here every slot of every tile holds a small random box, few of which absorb each other
    _capi.check(lib.opd_detr_set_profiling(C.c_void_p(det.model), 1), "opd_detr_set_profiling")
    rec = np.dtype([("x1", "<f4"), ("y1", "<f4"), ("x2", "<f4"), ("y2", "<f4"), ("score", "<f4"), ("label", "<i4"), ("query_index", "<i4"), ("frame", "<i4")])
    win = np.asarray(grid, np.int32)
    for stride, box in ((25, 400.0), (100, 400.0), (100, 150.0), (256, 150.0)):
        rng = np.random.RandomState(stride)
        recs, cnt = np.zeros((len(grid), stride), rec), np.full(len(grid), stride, np.int32)
        for t, (_, _, th_, tw_) in enumerate(grid):
            wh = rng.uniform(0.4 * box, box, (stride, 2))
            xy = rng.uniform(0, 1, (stride, 2)) * ([tw_, th_] - wh)
            recs[t]["x1"], recs[t]["y1"], recs[t]["x2"], recs[t]["y2"] = xy[:, 0], xy[:, 1], xy[:, 0] + wh[:, 0], xy[:, 1] + wh[:, 1]
            recs[t]["score"], recs[t]["label"], recs[t]["query_index"] = rng.uniform(0.05, 0.99, stride), 1, np.arange(stride)
        p = _capi.OpdTileParams(struct_size=C.sizeof(_capi.OpdTileParams), person_label=1, tile_nms_threshold=0.4, merge_nms_threshold=0.4, merge_threshold=0.5,
                                edge_tolerance=0.01)
        out, counts = (_capi.OpdTileDet * (len(grid) * stride))(), (C.c_int32 * 1)()
        ms = []
        for _ in range(2 + args.rounds):
            _capi.check(lib.opd_detr_merge_tiles(C.c_void_p(det.model), recs.ctypes.data, cnt.ctypes.data, 1, len(grid), stride, win.ctypes.data, H, W, C.byref(p), out, counts),
                        "opd_detr_merge_tiles")
            tab, n = (_capi.OpdKernelStat * 256)(), C.c_int(0)
            _capi.check(lib.opd_detr_kernel_table(C.c_void_p(det.model), tab, 256, C.byref(n)), "opd_detr_kernel_table")
            ms += [tab[i].ms for i in range(min(n.value, 256)) if tab[i].name.decode() == "tile_merge_kernel"]
        rows.append({"what": "kernel", "name": "tile_merge_kernel", "candidates": len(grid) * stride, "box_edge_px": box, "kept": int(counts[0]), "event_pair": stats(ms[2:])})
        print(json.dumps(rows[-1]), flush=True)
    _capi.check(lib.opd_detr_set_profiling(C.c_void_p(det.model), 0), "opd_detr_set_profiling")
    det.close()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump({"rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
