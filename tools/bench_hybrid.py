"""Hybrid tracking of 720 x 1280 frames on one MI355X: the fused calls against the per-frame calls they replace, on twin trackers, same
detector handle (device_nms=True), same build, in interleaved pairs.  The per-frame loop is the yardstick and its own round-to-round
spread the margin.  Results are asserted identical inside the tool.

  (a) a detection frame: ``detect`` + ``HipLightweightTracker.update_with_detections`` against ``detect_and_track_hybrid``
      (opd_detr_detect_frames_hybrid), at nms_threshold 0.4 (one kept record) and 1.0 (all 100 kept);
  (b) one key frame followed by 1, 4 and 9 in-between frames: the loop of (a)'s two calls and ``interpolate`` against
      ``track_hybrid_batch`` (opd_detr_detect_sequence_hybrid), per frame.

Host clock around calls that end in a device wait.

    python tools/bench_hybrid.py [--nms 0.4,1.0] [--runs 1,4,9] [--rounds 7] [--iters 40] [--json out.json]
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

from office_person_detection_vit_amd import HipDetrDetector, HipLightweightTracker  # noqa: E402
from office_person_detection_vit_amd.frames import structured_frames  # noqa: E402
from office_person_detection_vit_amd.weights import DetrArch, ensure_weight_file  # noqa: E402


def timed(call, iters):
    t = time.perf_counter()
    for _ in range(iters):
        call()
    return (time.perf_counter() - t) / iters * 1e3


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def plain(entry):
    """A frame's result without object identity: (id, bbox) pairs of a key frame's detections or of an in-between frame's records."""
    return [(d.track_id, d.bbox) if hasattr(d, "bbox") else (d[0], d[1]) for d in entry]


def compare(rows, what, args, loop, fused, seen, per_frame, extra):
    for _ in range(args.warmup):
        loop()
        fused()
    assert seen["fused"] == seen["loop"], f"{what}: the fused call and the loop disagree"
    tl, tf = [], []
    for _ in range(args.rounds):   # interleaved: drift of the machine lands on both
        tl.append(timed(loop, args.iters) / per_frame)
        tf.append(timed(fused, args.iters) / per_frame)
    assert seen["fused"] == seen["loop"], f"{what}: the fused call and the loop disagree"
    pairs = sum(f < t for f, t in zip(tf, tl))
    rows.append(dict(extra, what=what, identical=True, loop=stats(tl), fused=stats(tf), loop_spread_ms=round(max(tl) - min(tl), 4),
                     saved_ms=round(float(np.median(tl) - np.median(tf)), 4), pairs_fused_faster=f"{pairs} of {args.rounds}"))
    print(json.dumps(rows[-1]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nms", default="0.4,1.0")
    ap.add_argument("--runs", default="1,4,9")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    cache = os.environ.get("OPD_WEIGHT_CACHE", "/tmp/opd_weights")
    H, W = 720, 1280
    frames = [np.ascontiguousarray(f) for f in structured_frames(10, H, W, seed=99)]
    det = HipDetrDetector(model_path=ensure_weight_file(cache, DetrArch(), 0, 1.0, "r50"), max_batch=1, confidence_threshold=0.05, device_nms=True)
    det.load_model()
    rows = []

    def trackers():   # (a short max_age: tracks that LK carried off their boxes die instead of filling the handle over thousands of calls)
        return HipLightweightTracker(max_age=3, max_tracks=512), HipLightweightTracker(max_age=3, max_tracks=512)

    for nms in [float(t) for t in args.nms.split(",")]:
        det.nms_threshold = nms
        a, b = trackers()
        seen = {}

        def fused():
            seen["fused"] = plain(det.detect_and_track_hybrid(frames[0], a))

        def loop():
            seen["loop"] = plain(b.update_with_detections(frames[0], det.detect(frames[0])))

        compare(rows, "detection frame", args, loop, fused, seen, 1, {"nms_threshold": nms})
        rows[-1]["kept"] = len(seen["fused"])
        a.close()
        b.close()
        for n in [int(t) for t in args.runs.split(",")]:
            a, b = trackers()
            run, keys = frames[:n + 1], [True] + [False] * n

            def fused_run():
                seen["fused"] = [plain(e) for e in det.track_hybrid_batch(run, a, keys)]

            def loop_run():
                seen["loop"] = [plain(b.update_with_detections(run[0], det.detect(run[0])))] + [plain(b.interpolate(f)) for f in run[1:]]

            compare(rows, f"key + {n} in between, per frame", args, loop_run, fused_run, seen, n + 1, {"nms_threshold": nms, "in_between": n})
            rows[-1]["points_left"] = int(a.info().n_points)
            a.close()
            b.close()
    det.close()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump({"rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
