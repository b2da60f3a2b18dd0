"""Re-ID throughput on one MI355X: opd_reid_extract on 1280x720 host frames at n = 1, 8, 20 and 160 crops per call, captured graph
against eager launches, ms per call, crops/s and achieved TFLOP/s from the ViT-B/32 count (4.41 G multiply-adds = 8.83 GFLOP per crop:
12 x (QKV 88.5 M + out-proj 29.5 M + MLP 235.9 M + attention 3.8 M) + patch embedding 115.6 M; the projection is left out), or with
--model osnet the OSNet x1.0 count (0.979 G multiply-adds = 1.96 GFLOP per crop at 256 x 128).
The per-kernel table comes from a rocprofv3 --kernel-trace --stats pass over this script (profiles/NOTES.md).

    python tools/bench_reid.py [--model clip|osnet] [--iters 50] [--json out.json]
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

from office_person_detection_vit_amd import _capi  # noqa: E402
from office_person_detection_vit_amd.frames import structured_frames  # noqa: E402
from office_person_detection_vit_amd.weights import ensure_clip_weight_file, ensure_osnet_weight_file  # noqa: E402

GFLOP_PER_CROP = {"clip": 2 * (12 * (88.5e6 + 29.5e6 + 235.9e6 + 3.8e6) + 115.6e6) / 1e9, "osnet": 1.96}


def kernel_table(lib, h, ptrs, hw, n_frames, boxes, owner, n, iters):
    cap = 32
    rows = (_capi.OpdKernelStat * cap)()
    count = C.c_int()
    _capi.check(lib.opd_test_reid_kernel_table(h, ptrs, hw.ctypes.data, n_frames, boxes.ctypes.data, owner.ctypes.data, n, iters, rows, cap,
                                               C.byref(count)), "opd_test_reid_kernel_table")
    out = [{"kernel": rows[i].name.decode(), "launches_per_forward": rows[i].launches // iters, "ms_per_forward": rows[i].ms / iters,
            "tflops": (rows[i].flops / (rows[i].ms * 1e-3) / 1e12) if rows[i].flops and rows[i].ms > 0 else None}
           for i in range(min(count.value, cap))]
    out.sort(key=lambda r: -r["ms_per_forward"])
    tot = sum(r["ms_per_forward"] for r in out)
    print(f"  per-kernel, n = {n} (bucket of the call), eager forwards with events around every launch: {tot:.3f} ms of kernel time, "
          f"{sum(r['launches_per_forward'] for r in out)} launches per forward")
    for r in out:
        tf = f"{r['tflops']:7.1f}" if r["tflops"] else "      -"
        print(f"  {r['kernel']:48s} {r['launches_per_forward']:4d} x  {r['ms_per_forward']:8.4f} ms  {100 * r['ms_per_forward'] / tot:5.1f} %  "
              f"{tf} TFLOP/s", flush=True)
    return {"kernel_ms_per_forward": tot, "kernels": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=("clip", "osnet"), default="clip")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sizes", default="1,8,20,160")
    ap.add_argument("--json", default=None)
    ap.add_argument("--no-table", action="store_true", help="skip the per-kernel table")
    args = ap.parse_args()
    lib = _capi.load_library(test_hooks=True)
    cache = os.environ.get("OPD_WEIGHT_CACHE", "/tmp/opd_weights")
    path = ensure_osnet_weight_file(cache, "mild") if args.model == "osnet" else ensure_clip_weight_file(cache, "mild")
    gflop = GFLOP_PER_CROP[args.model]
    frames = [np.ascontiguousarray(f) for f in structured_frames(4, 720, 1280, seed=99)]
    hw = np.array([f.shape[:2] for f in frames], np.int32)
    ptrs = (C.c_void_p * len(frames))(*[f.ctypes.data for f in frames])
    rng = np.random.default_rng(0)
    sizes = [int(s) for s in args.sizes.split(",")]
    rows = []
    for mode, flags in (("graph", 0), ("eager", _capi.OPD_FLAG_NO_GRAPH)):
        cfg = _capi.OpdReidConfig()
        cfg.struct_size = C.sizeof(_capi.OpdReidConfig)
        cfg.max_crops = max(sizes)
        cfg.flags = flags
        cfg.model = _capi.OPD_REID_MODEL_OSNET if args.model == "osnet" else _capi.OPD_REID_MODEL_CLIP
        h = C.c_void_p()
        _capi.check(lib.opd_reid_create(C.byref(cfg), path.encode(), 0, C.byref(h)), "opd_reid_create")
        for n in sizes:
            hgt = rng.uniform(120, 420, n)   # person-sized boxes on a 1280 x 720 frame
            boxes = np.stack([rng.uniform(0, 1100, n), rng.uniform(0, 300, n), hgt * rng.uniform(0.3, 0.6, n), hgt], 1).astype(np.float32)
            owner = (np.arange(n) % len(frames)).astype(np.int32)
            out = np.zeros((n, 512), np.float32)
            call = lambda: _capi.check(lib.opd_reid_extract(h, ptrs, hw.ctypes.data, len(frames), _capi.OPD_MEM_HOST, boxes.ctypes.data,
                                                            owner.ctypes.data, n, out.ctypes.data), "opd_reid_extract")
            for _ in range(args.warmup):
                call()
            t = time.perf_counter()
            for _ in range(args.iters):
                call()
            ms = (time.perf_counter() - t) / args.iters * 1e3
            row = {"model": args.model, "mode": mode, "n": n, "ms_per_call": round(ms, 4), "crops_per_s": round(n / ms * 1e3, 1),
                   "tflops": round(n * gflop / ms, 2)}
            print(json.dumps(row), flush=True)
            if mode == "graph" and not args.no_table:
                row["table"] = kernel_table(lib, h, ptrs, hw, len(frames), boxes, owner, n, 10)
            rows.append(row)
        lib.opd_reid_destroy(h)
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"model": args.model, "gflop_per_crop": gflop, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
