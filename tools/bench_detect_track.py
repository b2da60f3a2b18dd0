"""Detect + track one 720 x 1280 frame per call on one MI355X: the fused call (HipDetrDetector.detect_and_track, one
opd_detr_detect_frames_track with one host wait) against the two calls it replaces (detect_with_features, then HipTracker.update) on twin
trackers, same detector handle (device_nms=True), same build, in interleaved pairs.  The two-call sequence is the yardstick and its own
round-to-round spread the margin.  Per feature kind, at nms_threshold 0.4 (few kept records) and 1.0 (all kept).  The same frame goes in
every call, so after the first few calls every kept record matches its track: the steady state of a camera on a still scene.  Host clock
around calls that end in a device wait; the commit launch of either form is not waited for and overlaps the next call's upload.

    python tools/bench_detect_track.py [--kinds none,encoder,color,reid] [--nms 0.4,1.0] [--rounds 7] [--iters 60] [--json out.json]
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from office_person_detection_vit_amd import HipDetrDetector, HipOSNetReIDExtractor, HipTracker  # noqa: E402
from office_person_detection_vit_amd.frames import structured_frames  # noqa: E402
from office_person_detection_vit_amd.weights import DetrArch, ensure_osnet_weight_file, ensure_weight_file  # noqa: E402


def timed(call, iters):
    t = time.perf_counter()
    for _ in range(iters):
        call()
    return (time.perf_counter() - t) / iters * 1e3


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kinds", default="none,encoder,color,reid")
    ap.add_argument("--nms", default="0.4,1.0")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--slots", type=int, default=32)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    cache = os.environ.get("OPD_WEIGHT_CACHE", "/tmp/opd_weights")
    H, W = 720, 1280
    frame = np.ascontiguousarray(structured_frames(1, H, W, seed=99)[0])
    det = HipDetrDetector(model_path=ensure_weight_file(cache, DetrArch(), 0, 1.0, "r50"), max_batch=1, confidence_threshold=0.05, device_nms=True)
    det.load_model()
    ext = None
    rows = []
    for name in args.kinds.split(","):
        features = None if name == "none" else name
        if features == "reid" and ext is None:
            ext = HipOSNetReIDExtractor(model_path=ensure_osnet_weight_file(cache, "mild"), max_crops=64)
            ext.load_model()
        D = {"none": 64, "encoder": 256, "color": 256, "reid": ext.feature_dim if ext else 0}[name]
        for nms in [float(t) for t in args.nms.split(",")]:
            det.nms_threshold = nms
            # (the seeded detector's scores on this frame stay below the reference's high_conf_threshold of 0.5, at which no track would ever start)
            a, b = (HipTracker(feature_dim=D, max_tracks=256, max_dets=128, min_hits=1, high_conf_threshold=0.06) for _ in range(2))
            seen = {}

            def fused():
                seen["fused"] = det.detect_and_track(frame, a, features=features, reid=ext, reid_slots=args.slots)

            def two_calls():
                dets = det.detect_with_features(frame, features=features, reid=ext, reid_slots=args.slots)[0] if features else det.detect(frame)
                seen["two"] = b.update(dets)

            for _ in range(args.warmup):
                two_calls()
                fused()
            same = [(d.track_id, d.bbox) for d in seen["fused"]] == [(d.track_id, d.bbox) for d in seen["two"]]
            t2, tf = [], []
            for _ in range(args.rounds):   # interleaved: drift of the machine lands on both
                t2.append(timed(two_calls, args.iters))
                tf.append(timed(fused, args.iters))
            pairs = sum(f < t for f, t in zip(tf, t2))
            rows.append({"features": name, "nms_threshold": nms, "tracked": len(seen["fused"]), "tracks": len(a.get_tracks()), "ids_identical": bool(same),
                         "two_calls": stats(t2), "fused": stats(tf), "two_calls_spread_ms": round(max(t2) - min(t2), 4),
                         "saved_ms": round(float(np.median(t2) - np.median(tf)), 4), "pairs_fused_faster": f"{pairs} of {args.rounds}"})
            print(json.dumps(rows[-1]), flush=True)
            a.close()
            b.close()
    if ext is not None:
        ext.cleanup()
    det.close()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump({"rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
