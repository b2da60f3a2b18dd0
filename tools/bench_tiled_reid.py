"""The Re-ID stage of a tiled call on one 2160 x 3840 frame (2 x 2 tiles, overlap 1/8) on one handle of one MI355X, seeded `sharp` detector weights
(attention gain 2: the seam merge has boxes to absorb) and OSNet x1.0: the fused call (detect_tiled_reid(reid=, floor_map=, trackers=):
opd_detr_detect_tiled_reid, ONE host wait, crops cut on the device from the frame where the source step left it) against the separate calls it
replaces on the same handles (detect_tiled + reid.extract_features, which stages the crop windows on the host and uploads them, + floor_map.apply
+ tracker.update), in interleaved rounds, with and without the tracker, at 8 and 32 crop slots.  The Re-ID forward of the fused call is sized from
the slots before the person count is known, so a large slot count can lose: both are reported, whatever the outcome.  The separate calls are the
yardstick and their own round-to-round spread the margin.  Host clock around calls that end in a device wait.

    python tools/bench_tiled_reid.py [--rounds 7] [--iters 10] [--warmup 3] [--threshold 0.05] [--slots 8 32] [--json out.json]
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

from office_person_detection_vit_amd import HipDetrDetector, HipFloorMapper, HipOSNetReIDExtractor, HipTracker  # noqa: E402
from office_person_detection_vit_amd.frames import structured_frames  # noqa: E402
from office_person_detection_vit_amd.tiling import tile_grid  # noqa: E402
from office_person_detection_vit_amd.weights import DetrArch, ensure_osnet_weight_file, ensure_weight_file  # noqa: E402

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
    ap.add_argument("--slots", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    cache = os.environ.get("OPD_WEIGHT_CACHE", "/tmp/opd_weights")
    grid = tile_grid(H, W, ROWS, COLS, OVERLAP)
    frame = np.ascontiguousarray(structured_frames(1, H, W, seed=99)[0])
    det = HipDetrDetector(model_path=ensure_weight_file(cache, DetrArch(), 0, 2.0, "r50"), max_batch=len(grid), confidence_threshold=args.threshold)
    det.load_model()
    reid = HipOSNetReIDExtractor(model_path=ensure_osnet_weight_file(cache, "mild"), max_crops=max(64, max(args.slots)))
    reid.load_model()
    fmap = HipFloorMapper.homography(HOMOGRAPHY, FLOORMAP, ZONES)
    S = len(grid) * det.num_queries
    rows = []
    for slots in args.slots:
        for tracked in (False, True):
            make = lambda: HipTracker(feature_dim=reid.feature_dim, max_dets=S, max_tracks=1024, min_hits=1) if tracked else None   # noqa: E731
            ta, tb = make(), make()

            def separate():
                dets = det.detect_tiled([frame], grid)[0]
                feats = reid.extract_features(frame, [d.bbox for d in dets])
                for k, d in enumerate(dets):   # (what the fused tracked call does with a record beyond the slots: it enters without a row)
                    d.features = feats[k] if (not tracked or k < slots) else None
                fmap.apply(dets)
                if tracked:
                    ta.update(dets)
                return dets

            def fused():
                return det.detect_tiled_reid([frame], grid, reid, reid_slots=slots, floor_map=fmap, trackers=[tb] if tracked else None)[0]

            for _ in range(args.warmup):
                want, got = separate(), fused()
            same = fields(want) == fields(got) and (tracked or all(np.array_equal(a.features, b.features) for a, b in zip(want, got)))
            if tracked:
                same = same and [bytes(r) for r in ta._records()] == [bytes(r) for r in tb._records()]
            assert same, f"slots = {slots}, tracker = {tracked}: the fused call and the separate calls differ"
            ts, tf = [], []
            for _ in range(args.rounds):   # interleaved: drift of the machine lands on both
                ts.append(timed(separate, args.iters))
                tf.append(timed(fused, args.iters))
            pairs = sum(f < s for f, s in zip(tf, ts))
            rows.append({"what": "tiled reid", "slots": slots, "tracker": tracked, "frame": [H, W], "tiles": len(grid), "detections": len(want),
                         "results_identical": bool(same), "separate_calls": stats(ts), "fused_call": stats(tf), "separate_spread_ms": round(max(ts) - min(ts), 4),
                         "saved_ms": round(float(np.median(ts) - np.median(tf)), 4), "pairs_fused_faster": f"{pairs} of {args.rounds}"})
            print(json.dumps(rows[-1]), flush=True)
            for t in (ta, tb):
                if t is not None:
                    t.close()
    fmap.close()
    reid.cleanup()
    det.close()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump({"rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
