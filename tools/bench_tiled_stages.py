"""The feature, floor and track stages of a tiled call on one 2160 x 3840 frame (2 x 2 tiles, overlap 1/8) on one handle of one MI355X, seeded
`sharp` weights (attention gain 2: the seam merge has boxes to absorb): the fused call (detect_tiled_stages(features="color", floor_map=, trackers=):
opd_detr_detect_tiled_stages, ONE host wait, no box or feature row crossing the bus twice) against the separate calls it replaces on the same
handle (detect_tiled + extract_color_features, which uploads the frame a second time, + floor_map.apply + tracker.update), in interleaved rounds,
with and without the tracker.  The separate calls are the yardstick and their own round-to-round spread the margin.  Host clock around calls
that end in a device wait.

    python tools/bench_tiled_stages.py [--rounds 7] [--iters 10] [--warmup 3] [--threshold 0.05] [--json out.json]
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

from office_person_detection_vit_amd import HipDetrDetector, HipFloorMapper, HipTracker  # noqa: E402
from office_person_detection_vit_amd.frames import structured_frames  # noqa: E402
from office_person_detection_vit_amd.tiling import tile_grid  # noqa: E402
from office_person_detection_vit_amd.weights import DetrArch, ensure_weight_file  # noqa: E402

H, W, ROWS, COLS, OVERLAP = 2160, 3840, 2, 2, 0.125
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


def fields(dets):
    return [(d.bbox, d.confidence, d.camera_coords, d.floor_coords, d.floor_coords_mm, tuple(d.zone_ids), d.track_id, d.query_index) for d in dets]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--threshold", type=float, default=0.05)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    cache = os.environ.get("OPD_WEIGHT_CACHE", "/tmp/opd_weights")
    grid = tile_grid(H, W, ROWS, COLS, OVERLAP)
    frame = np.ascontiguousarray(structured_frames(1, H, W, seed=99)[0])
    det = HipDetrDetector(model_path=ensure_weight_file(cache, DetrArch(), 0, 2.0, "r50"), max_batch=len(grid), confidence_threshold=args.threshold)
    det.load_model()
    fmap = HipFloorMapper.homography(HOMOGRAPHY, FLOORMAP, ZONES)
    S = len(grid) * det.num_queries
    rows = []
    for tracked in (False, True):
        make = lambda: HipTracker(feature_dim=256, max_dets=S, max_tracks=1024, min_hits=1) if tracked else None   # noqa: E731
        ta, tb = make(), make()

        def separate():
            dets = det.detect_tiled([frame], grid)[0]
            for d, row in zip(dets, det.extract_color_features(frame, dets)):
                d.features = row
            fmap.apply(dets)
            if tracked:
                ta.update(dets)
            return dets

        def fused():
            return det.detect_tiled_stages([frame], grid, features="color", floor_map=fmap, trackers=[tb] if tracked else None)[0]

        for _ in range(args.warmup):
            want, got = separate(), fused()
        same = fields(want) == fields(got) and (tracked or all(np.array_equal(a.features, b.features) for a, b in zip(want, got)))
        ts, tf = [], []
        for _ in range(args.rounds):   # interleaved: drift of the machine lands on both
            ts.append(timed(separate, args.iters))
            tf.append(timed(fused, args.iters))
        pairs = sum(f < s for f, s in zip(tf, ts))
        rows.append({"what": "tiled stages", "tracker": tracked, "frame": [H, W], "tiles": len(grid), "detections": len(want), "results_identical": bool(same),
                     "separate_calls": stats(ts), "fused_call": stats(tf), "separate_spread_ms": round(max(ts) - min(ts), 4),
                     "saved_ms": round(float(np.median(ts) - np.median(tf)), 4), "pairs_fused_faster": f"{pairs} of {args.rounds}"})
        print(json.dumps(rows[-1]), flush=True)
        for t in (ta, tb):
            if t is not None:
                t.close()
    fmap.close()
    det.close()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump({"rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
