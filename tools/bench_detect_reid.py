"""Detect + Re-ID features of one 720 x 1280 frame on one MI355X: the fused call (opd_detr_detect_frames_reid) against the two calls it
replaces (opd_detr_detect_frames, then opd_reid_extract on the boxes of the first `slots` person records), same handles, same build,
in interleaved rounds.  The two-call sequence is the yardstick and its own round-to-round spread the margin.  The person count is
whatever the frame yields at each threshold.  Then the Python surface: detect_with_features(features="reid") against detect() +
extract_features().  Host clock around calls that end in a device wait.  --device-nms: the Python rows in both suppression modes
(host NMS behind the call / opd_detr_set_nms inside it) on the same handles, all four sequences interleaved in every round, and a row
with person_nms_kernel's own time from opd_detr_kernel_table.

    python tools/bench_detect_reid.py [--model osnet|clip] [--slots 8,32] [--thresholds 0.05,0.45] [--rounds 5] [--iters 100] [--device-nms]
                                      [--json out.json]
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

from office_person_detection_vit_amd import HipDetrDetector, HipOSNetReIDExtractor, HipReIDExtractor, _capi  # noqa: E402
from office_person_detection_vit_amd.frames import structured_frames  # noqa: E402
from office_person_detection_vit_amd.weights import DetrArch, ensure_clip_weight_file, ensure_osnet_weight_file, ensure_weight_file  # noqa: E402

PERSON = 1
REC = np.dtype([("x1", "<f4"), ("y1", "<f4"), ("x2", "<f4"), ("y2", "<f4"), ("score", "<f4"), ("label", "<i4"), ("query_index", "<i4"), ("frame", "<i4")])


def timed(call, iters):
    t = time.perf_counter()
    for _ in range(iters):
        call()
    return (time.perf_counter() - t) / iters * 1e3


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="osnet", choices=["osnet", "clip"])
    ap.add_argument("--slots", default="8,32")
    ap.add_argument("--thresholds", default="0.05,0.45")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--device-nms", action="store_true")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    lib = _capi.load_library()
    cache = os.environ.get("OPD_WEIGHT_CACHE", "/tmp/opd_weights")
    H, W = 720, 1280
    frame = np.ascontiguousarray(structured_frames(1, H, W, seed=99)[0])
    det = HipDetrDetector(model_path=ensure_weight_file(cache, DetrArch(), 0, 1.0, "r50"), max_batch=1, confidence_threshold=0.05)
    det.load_model()
    if args.model == "osnet":
        ext = HipOSNetReIDExtractor(model_path=ensure_osnet_weight_file(cache, "mild"), max_crops=64)
    else:
        ext = HipReIDExtractor(model_path=ensure_clip_weight_file(cache, "mild"), max_crops=64)
    ext.load_model()
    Q, E = det.num_queries, ext.feature_dim
    th, tw = det._frame_list_target([frame])
    ptrs = (C.c_void_p * 1)(frame.ctypes.data)
    hw = np.array([H, W], np.int32)
    recs, counts = np.zeros(Q, REC), np.zeros(1, np.int32)
    rp, cp = recs.ctypes.data_as(C.POINTER(_capi.OpdDet)), counts.ctypes.data_as(C.POINTER(C.c_int32))
    rows = []
    for thr in [float(t) for t in args.thresholds.split(",")]:
        for slots in [int(s) for s in args.slots.split(",")]:
            feats, slot_map, n_person = np.zeros((slots, E), np.float32), np.zeros(slots, np.int32), C.c_int32(0)
            out2 = np.zeros((slots, E), np.float32)
            seen = {}

            def fused():
                _capi.check(lib.opd_detr_detect_frames_reid(C.c_void_p(det.model), ext._handle, ptrs, 1, H, W, th, tw, thr, PERSON, slots, rp, cp,
                                                            feats.ctypes.data, slot_map.ctypes.data, C.byref(n_person)), "opd_detr_detect_frames_reid")

            def two_calls():
                _capi.check(lib.opd_detr_detect_frames(C.c_void_p(det.model), ptrs, _capi.OPD_MEM_HOST, 1, H, W, th, tw, thr, rp, cp), "opd_detr_detect_frames")
                r = recs[:int(counts[0])]
                r = r[r["label"] == PERSON][:slots]
                seen["n"] = len(r)
                if len(r) == 0:
                    return
                x1, y1 = r["x1"].astype(np.float64), r["y1"].astype(np.float64)
                boxes = np.ascontiguousarray(np.stack([x1, y1, r["x2"].astype(np.float64) - x1, r["y2"].astype(np.float64) - y1], 1).astype(np.float32))
                _capi.check(lib.opd_reid_extract(ext._handle, ptrs, hw.ctypes.data, 1, _capi.OPD_MEM_HOST, boxes.ctypes.data, None, len(r), out2.ctypes.data),
                            "opd_reid_extract")

            for _ in range(args.warmup):
                two_calls()
                fused()
            n = min(int(n_person.value), slots)
            same = bool(n == seen["n"] and np.array_equal(feats[:n], out2[:n]))
            t2, tf = [], []
            for _ in range(args.rounds):   # interleaved: drift of the machine lands on both
                t2.append(timed(two_calls, args.iters))
                tf.append(timed(fused, args.iters))
            rows.append({"what": "C-ABI", "model": args.model, "threshold": thr, "slots": slots, "n_person": int(n_person.value), "rows": n,
                         "rows_bit_identical": same, "two_calls": stats(t2), "fused": stats(tf),
                         "two_calls_spread_ms": round(max(t2) - min(t2), 4), "saved_ms": round(float(np.median(t2) - np.median(tf)), 4)})
            print(json.dumps(rows[-1]), flush=True)
    # the Python surface, twice: as configured (suppression discards most of this frame's overlapping records, so the fused call computes
    # rows nobody reads), and with a threshold and an IoU limit at which every record is kept (both ways then compute the same rows)
    nms0 = det.nms_threshold
    for conf, nms in ((0.05, nms0), (float(args.thresholds.split(",")[-1]), 1.0)):
        det.confidence_threshold, det.nms_threshold = conf, nms
        for slots in [int(s) for s in args.slots.split(",")]:
            ndet = len(det.detect(frame))
            two = lambda: ext.extract_features(frame, [d.bbox for d in det.detect(frame)])
            one = lambda: det.detect_with_features(frame, features="reid", reid=ext, reid_slots=slots)
            for _ in range(args.warmup):
                two()
                one()
            same = bool(np.array_equal(two(), one()[1]))
            t2, tf = [], []
            for _ in range(args.rounds):
                t2.append(timed(two, args.iters))
                tf.append(timed(one, args.iters))
            rows.append({"what": "python", "model": args.model, "threshold": conf, "nms_threshold": nms, "slots": slots, "detections": ndet,
                         "rows_bit_identical": same, "detect+extract_features": stats(t2), "detect_with_features(reid)": stats(tf),
                         "two_calls_spread_ms": round(max(t2) - min(t2), 4), "saved_ms": round(float(np.median(t2) - np.median(tf)), 4)})
            print(json.dumps(rows[-1]), flush=True)
            if not args.device_nms:
                continue

            def in_mode(on, call):   # (the switch is one host call on the handle: outside the clock)
                det.device_nms = on
                det._sync_nms()
                return call()

            for _ in range(args.warmup):
                in_mode(True, two)
                in_mode(True, one)
            same = bool(np.array_equal(in_mode(False, one)[1], in_mode(True, one)[1]) and np.array_equal(in_mode(True, two), in_mode(True, one)[1]))
            ts = {"host:detect+extract_features": [], "host:detect_with_features(reid)": [], "device:detect+extract_features": [],
                  "device:detect_with_features(reid)": []}
            for _ in range(args.rounds):   # four sequences, interleaved: drift of the machine lands on all of them
                for key, on, call in (("host:detect+extract_features", False, two), ("host:detect_with_features(reid)", False, one),
                                      ("device:detect+extract_features", True, two), ("device:detect_with_features(reid)", True, one)):
                    ts[key].append(in_mode(on, lambda: timed(call, args.iters)))
            in_mode(False, lambda: None)
            med = {k: float(np.median(v)) for k, v in ts.items()}
            pairs = sum(a < b for a, b in zip(ts["device:detect_with_features(reid)"], ts["host:detect+extract_features"]))
            rows.append({"what": "python device_nms", "model": args.model, "threshold": conf, "nms_threshold": nms, "slots": slots, "detections": ndet,
                         "rows_bit_identical": same, **{k: stats(v) for k, v in ts.items()},
                         "two_calls_spread_ms": round(max(ts["host:detect+extract_features"]) - min(ts["host:detect+extract_features"]), 4),
                         "fused_device_vs_two_calls_host_ms": round(med["device:detect_with_features(reid)"] - med["host:detect+extract_features"], 4),
                         "fused_device_vs_fused_host_ms": round(med["device:detect_with_features(reid)"] - med["host:detect_with_features(reid)"], 4),
                         "two_calls_device_vs_two_calls_host_ms": round(med["device:detect+extract_features"] - med["host:detect+extract_features"], 4),
                         "pairs_fused_device_faster_than_two_calls_host": f"{pairs} of {args.rounds}"})
            print(json.dumps(rows[-1]), flush=True)
    if args.device_nms:   # the kernel's own time: one profiled call (event pair around every launch) per confidence threshold
        det.nms_threshold, det.device_nms = nms0, True
        _capi.check(lib.opd_detr_set_profiling(C.c_void_p(det.model), 1), "opd_detr_set_profiling")
        for conf in (0.05, float(args.thresholds.split(",")[-1])):
            det.confidence_threshold = conf
            ms = []
            for _ in range(1 + args.rounds):
                nrec = len(det.detect(frame))
                tab, n = (_capi.OpdKernelStat * 256)(), C.c_int(0)
                _capi.check(lib.opd_detr_kernel_table(C.c_void_p(det.model), tab, 256, C.byref(n)), "opd_detr_kernel_table")
                ms += [tab[i].ms / max(tab[i].launches, 1) for i in range(min(n.value, 256)) if tab[i].name.decode() == "person_nms_kernel"]
            rows.append({"what": "kernel", "name": "person_nms_kernel", "threshold": conf, "kept": nrec, "calls": len(ms), "event_pair": stats(ms[1:]) if len(ms) > 1 else None})
            print(json.dumps(rows[-1]), flush=True)
        _capi.check(lib.opd_detr_set_profiling(C.c_void_p(det.model), 0), "opd_detr_set_profiling")
        det.device_nms = False
        det._sync_nms()
    ext.cleanup()
    det.close()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump({"rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
