"""Hybrid tracking on a tiled camera: one 2160 x 3840 camera, 2 x 2 tiles (overlap 1/8), seeded `sharp` weights (attention gain 2: the seam merge has
boxes to absorb), one handle of one MI355X.  Each case runs the separate calls and the fused call in interleaved rounds on twin trackers and asserts
identical results; the separate calls are the yardstick and their own round-to-round spread the margin.  Host clock around calls that end in a device
wait.

  detection frame   detect_tiled + lwt.update_with_detections (the frame uploaded twice, two waits) against detect_tiled_hybrid
                    (opd_detr_detect_tiled_hybrid: one upload, one wait), with and without optical flow
  key + n between   the per-frame loop (that detection frame, then lwt.interpolate per in-between frame) against track_tiled_hybrid_batch
                    (opd_detr_detect_tiled_sequence_hybrid), per frame
  --reid            2 x 3 tiles (two window sizes), OSNet x1.0, 8 and 32 slots: detect_tiled_ragged + reid.extract_features (+ floor_map.apply)
                    against detect_tiled_ragged_reid

    python tools/bench_tiled_hybrid.py [--reid] [--rounds 7] [--iters 10] [--warmup 3] [--runs 1,4] [--slots 8,32] [--json out.json]
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

from office_person_detection_vit_amd import HipDetrDetector, HipFloorMapper, HipLightweightTracker, HipOSNetReIDExtractor  # noqa: E402
from office_person_detection_vit_amd.frames import structured_frames  # noqa: E402
from office_person_detection_vit_amd.tiling import tile_grid  # noqa: E402
from office_person_detection_vit_amd.weights import DetrArch, ensure_osnet_weight_file, ensure_weight_file  # noqa: E402

H, W, OVERLAP = 2160, 3840, 0.125
FLOORMAP = (1878, 1369, 28.1926406926406, 28.241430700447)
ZONES = [{"id": "zone_1", "polygon": [[859, 912], [1095, 912], [1095, 1350], [859, 1350]], "priority": 1},
         {"id": "zone_2", "polygon": [[1095, 912], [1331, 912], [1331, 1350], [1095, 1350]], "priority": 2}]
HOMOGRAPHY = [[0.45, 0.02, 10.0], [0.01, 0.6, 20.0], [0.00001, 0.00002, 1.0]]   # the 4K frame onto the floor map, mildly projective


def timed(call, iters):
    t = time.perf_counter()
    for _ in range(iters):
        call()
    return (time.perf_counter() - t) / iters * 1e3


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def plain(entry):
    """A frame's result as comparable values: detections of a key frame, (id, box) pairs of an in-between frame."""
    return [e if isinstance(e, tuple) else (e.bbox, e.confidence, e.track_id, e.query_index, e.floor_coords, None if e.features is None else e.features.tobytes())
            for e in entry]


def compare(rows, what, args, separate, fused, seen, per_frame, extra):
    for _ in range(args.warmup):
        separate()
        fused()
    assert seen["separate"] == seen["fused"], f"{what}: the fused call and the separate calls differ"
    ts, tf = [], []
    for _ in range(args.rounds):   # interleaved: drift of the machine lands on both
        ts.append(timed(separate, args.iters) / per_frame)
        tf.append(timed(fused, args.iters) / per_frame)
        assert seen["separate"] == seen["fused"], f"{what}: the fused call and the separate calls differ"
    pairs = sum(f < s for f, s in zip(tf, ts))
    rows.append(dict(extra, what=what, results_identical=True, separate_calls=stats(ts), fused_call=stats(tf), separate_spread_ms=round(max(ts) - min(ts), 4),
                     saved_ms=round(float(np.median(ts) - np.median(tf)), 4), pairs_fused_faster=f"{pairs} of {args.rounds}"))
    print(json.dumps(rows[-1]), flush=True)


def shifted(frame, k):
    """The scene moved by k x (2, 1) pixels, edge pixels repeated: consecutive frames of one camera for Lucas-Kanade to follow."""
    ys, xs = np.clip(np.arange(H) - 2 * k, 0, H - 1), np.clip(np.arange(W) - k, 0, W - 1)
    return np.ascontiguousarray(frame[ys][:, xs])


def hybrid_cases(args, cache, rows):
    grid = tile_grid(H, W, 2, 2, OVERLAP)
    base = np.ascontiguousarray(structured_frames(1, H, W, seed=99)[0])
    frames = [base] + [shifted(base, k) for k in range(1, max(args.runs) + 1)]
    det = HipDetrDetector(model_path=ensure_weight_file(cache, DetrArch(), 0, 2.0, "r50"), max_batch=len(grid), confidence_threshold=args.threshold)
    det.load_model()

    def trackers(flow=True):   # (a short max_age: tracks that LK carried off their boxes die instead of filling the handle over hundreds of calls)
        return tuple(HipLightweightTracker(max_age=3, max_tracks=1024, use_optical_flow=flow) for _ in range(2))

    for flow in (True, False):
        a, b = trackers(flow)
        seen = {}

        def fused():
            seen["fused"] = plain(det.detect_tiled_hybrid([base], grid, [a])[0])

        def separate():
            seen["separate"] = plain(b.update_with_detections(base, det.detect_tiled([base], grid)[0]))

        compare(rows, "detection frame", args, separate, fused, seen, 1, {"optical_flow": flow, "frame": [H, W], "tiles": len(grid)})
        rows[-1]["kept"] = len(seen["fused"])
        assert a.info().last_waits == 0
        a.close()
        b.close()
    for n in args.runs:
        a, b = trackers()
        run, keys = frames[:n + 1], [True] + [False] * n
        seen = {}

        def fused_run():
            seen["fused"] = [plain(e) for e in det.track_tiled_hybrid_batch(run, grid, a, keys)]

        def loop_run():
            seen["separate"] = [plain(b.update_with_detections(run[0], det.detect_tiled([run[0]], grid)[0]))] + [plain(b.interpolate(f)) for f in run[1:]]

        compare(rows, f"key + {n} in between, per frame", args, loop_run, fused_run, seen, n + 1, {"in_between": n, "frame": [H, W], "tiles": len(grid)})
        rows[-1]["kept"], rows[-1]["points_left"] = len(seen["fused"][0]), int(a.info().n_points)
        a.close()
        b.close()
    det.close()


def reid_cases(args, cache, rows):
    grid = tile_grid(H, W, 2, 3, OVERLAP)
    assert len({(t[2], t[3]) for t in grid}) > 1
    frame = np.ascontiguousarray(structured_frames(1, H, W, seed=99)[0])
    det = HipDetrDetector(model_path=ensure_weight_file(cache, DetrArch(), 0, 2.0, "r50"), max_batch=max(8, len(grid)), confidence_threshold=args.threshold)
    det.load_model()
    reid = HipOSNetReIDExtractor(model_path=ensure_osnet_weight_file(cache, "mild"), max_crops=max(64, max(args.slots)))
    reid.load_model()
    fmap = HipFloorMapper.homography(HOMOGRAPHY, FLOORMAP, ZONES)
    for slots in args.slots:
        for floor in (False, True):
            seen = {}

            def separate():
                dets = det.detect_tiled_ragged([frame], grid)[0]
                for d, row in zip(dets, reid.extract_features(frame, [d.bbox for d in dets])):
                    d.features = row
                if floor:
                    fmap.apply(dets)
                seen["separate"] = plain(dets)

            def fused():
                seen["fused"] = plain(det.detect_tiled_ragged_reid([frame], grid, reid, reid_slots=slots, floor_map=fmap if floor else None)[0])

            compare(rows, "ragged Re-ID", args, separate, fused, seen, 1, {"slots": slots, "floor": floor, "frame": [H, W], "tiles": len(grid)})
            rows[-1]["kept"] = len(seen["fused"])
    fmap.close()
    reid.cleanup()
    det.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reid", action="store_true")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", default="1,4")
    ap.add_argument("--slots", default="8,32")
    ap.add_argument("--threshold", type=float, default=0.05)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    args.runs, args.slots = [int(t) for t in args.runs.split(",")], [int(t) for t in args.slots.split(",")]
    cache = os.environ.get("OPD_WEIGHT_CACHE", "/tmp/opd_weights")
    rows = []
    (reid_cases if args.reid else hybrid_cases)(args, cache, rows)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump({"rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
