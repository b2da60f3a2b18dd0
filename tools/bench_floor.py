"""The floor map on one MI355X: ms per opd_floor_transform call at 21, 100 and 800 boxes (21.25 detections per frame is the reference's
published session average) for the homography, a 40-point piecewise affine and a 40-point thin-plate spline with the configuration's
three zones, next to the numpy restatement (tests/floor_common.py) on the same box; then opd_detr_detect_frames_floor against
opd_detr_detect_frames as interleaved pairs on the handle and frame of tools/bench_color_features.py.  Host clock around calls that
end in a device wait.

    python tools/bench_floor.py [--iters 200] [--json out.json]
"""

from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

import floor_common as F  # noqa: E402
from office_person_detection_vit_amd import HipDetrDetector, _capi  # noqa: E402
from office_person_detection_vit_amd import floor as FL  # noqa: E402
from office_person_detection_vit_amd.frames import structured_frames  # noqa: E402
from office_person_detection_vit_amd.weights import DetrArch, ensure_weight_file  # noqa: E402

FM = (1878, 1369, 28.1926406926406, 28.241430700447)
ZONES = [{"id": "zone_1", "polygon": [[859, 912], [1095, 912], [1095, 1350], [859, 1350]], "priority": 1},
         {"id": "zone_2", "polygon": [[1095, 912], [1331, 912], [1331, 1350], [1095, 1350]], "priority": 2},
         {"id": "zone_3", "polygon": [[1331, 912], [1567, 912], [1567, 1350], [1331, 1350]], "priority": 3}]
H = [[-0.8795888447, -2.8974379541, 417.8510123786], [-1.5459702925, -3.4570021203, 1054.0107447082], [-0.0011928509, -0.0035480452, 1.0]]


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
    ap.add_argument("--sizes", default="21,100,800")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    lib = _capi.load_library()
    rng = np.random.default_rng(0)
    src = np.round(rng.uniform((40, 40), (1240, 680), (40, 2)), 2)
    dst = np.stack([1.4 * src[:, 0] + 40 + 25 * np.sin(src[:, 1] / 150.0), 1.8 * src[:, 1] + 30 + 20 * np.cos(src[:, 0] / 200.0)], 1)
    models = {"homography": FL.model_homography(H, FM, ZONES), "piecewise_affine": FL.model_piecewise_affine(src, dst, FM, ZONES),
              "thin_plate_spline": FL.model_thin_plate_spline(src, dst, FM, ZONES)}
    rows = []
    for method, model in models.items():
        h = F.create(lib, model)
        for n in [int(s) for s in args.sizes.split(",")]:
            bw, bh = rng.uniform(40, 140, n), rng.uniform(120, 320, n)
            boxes = np.ascontiguousarray(np.stack([rng.uniform(0, 1140, n), rng.uniform(0, 400, n), bw, bh], 1).astype(np.float32))
            out = np.zeros(n, F.REC_DTYPE)
            call = lambda: _capi.check(lib.opd_floor_transform(h, boxes.ctypes.data, n, _capi.OPD_MEM_HOST, out.ctypes.data), "opd_floor_transform")
            ms = timed(call, args.warmup, args.iters)
            ms_np = timed(lambda: F.run(model, boxes=boxes), 1, max(3, args.iters // 20))
            px = F.run(model, boxes=boxes)[0]
            rows.append({"what": "opd_floor_transform", "method": method, "n": n, "triangles": int(len(model.get("triangles", ()))), "ms_per_call": round(ms, 4),
                         "us_per_record": round(ms / n * 1e3, 3), "numpy_restatement_ms": round(ms_np, 4), "max_abs_device_minus_numpy": float(np.abs(out["px"] - px).max())})
            print(json.dumps(rows[-1]), flush=True)
        lib.opd_floor_destroy(h)
    Hf, Wf = 720, 1280
    frame = np.ascontiguousarray(structured_frames(1, Hf, Wf, seed=99)[0])
    path = ensure_weight_file(os.environ.get("OPD_WEIGHT_CACHE", "/tmp/opd_weights"), DetrArch(), 0, 1.0, "r50")
    det = HipDetrDetector(model_path=path, max_batch=1, confidence_threshold=0.05)
    det.load_model()
    fmap = F.create(lib, models["piecewise_affine"])
    Q = det.num_queries
    th, tw = det._frame_list_target([frame])
    recs, counts, floor = (_capi.OpdDet * Q)(), (C.c_int32 * 1)(), np.zeros(Q, F.REC_DTYPE)
    ptrs = (C.c_void_p * 1)(frame.ctypes.data)
    plain = lambda: _capi.check(lib.opd_detr_detect_frames(C.c_void_p(det.model), ptrs, _capi.OPD_MEM_HOST, 1, Hf, Wf, th, tw, 0.05, recs, counts), "detect_frames")
    fused = lambda: _capi.check(lib.opd_detr_detect_frames_floor(C.c_void_p(det.model), fmap, ptrs, 1, Hf, Wf, th, tw, 0.05, 1, recs, counts, floor.ctypes.data),
                                "detect_frames_floor")
    for _ in range(args.warmup):
        plain(), fused()
    t_plain = t_fused = 0.0
    for _ in range(args.iters):   # interleaved pairs: both see the same clocks and the same neighbours
        t0 = time.perf_counter(); plain(); t1 = time.perf_counter(); fused(); t2 = time.perf_counter()
        t_plain += t1 - t0
        t_fused += t2 - t1
    persons = sum(1 for r in recs[:int(counts[0])] if r.label == 1)
    rows.append({"what": "detect_frames vs detect_frames_floor", "frame": [Hf, Wf], "records": int(counts[0]), "person_records": persons,
                 "ms_plain": round(t_plain / args.iters * 1e3, 4), "ms_fused": round(t_fused / args.iters * 1e3, 4),
                 "added_ms": round((t_fused - t_plain) / args.iters * 1e3, 4)})
    print(json.dumps(rows[-1]), flush=True)
    lib.opd_floor_destroy(fmap)
    det.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
