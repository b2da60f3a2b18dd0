"""Time the hybrid tracker's two calls on 720 x 1280 frames at 21 and 100 tracks, from host frames and from device frames:
``HipLightweightTracker.interpolate`` and ``.update_with_detections`` (one native call and one host wait each) next to what the package
prescribed before: ``HipOpticalFlowTracker`` inside the numpy restatement of the reference's ``LightweightTracker``
(tests/lwt_common.py) -- a blocking ``opd_flow_track``, the points and status on the host, numpy Kalman algebra per track, the
surviving points uploaded again by the next call.

    python tools/bench_lwt.py [--pairs 7] [--frames 20] [--out FILE.json]

Both run in ONE process, alternating window by window (fused, baseline, fused, ...); a window is one detection frame followed by
``--frames`` in-between frames, every call ends in its own host wait inside the timed span, and the spread over the windows is reported
next to the median.  The two paths see the same frames and hold the same tracks (their records are compared once, untimed).
No GPU: the tool fails."""

import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import flow_common as FC  # noqa: E402
import lwt_common as LC  # noqa: E402
from office_person_detection_vit_amd import HipLightweightTracker, HipOpticalFlowTracker  # noqa: E402

F32 = np.float32
H, W = 720, 1280


def boxes_on_grid(n):
    cols = int(np.ceil(np.sqrt(n * W / H)))
    rows = int(np.ceil(n / cols))
    k = np.arange(n)
    cx, cy = (k % cols + 0.5) * (W / cols), (k // cols + 0.5) * (H / rows)
    w, h = np.full(n, 30.0), np.full(n, 50.0)
    return (np.round(np.stack([cx - w / 2, cy - h / 2, w, h], 1) * 4) / 4).astype(F32)


class Baseline:
    """The reference class restated in numpy with the device's LK plugged in as its ``of_tracker``."""

    def __init__(self):
        self.r = LC.Restatement()
        self.of = HipOpticalFlowTracker()

    def update_with_detections(self, frame, dets):
        ids = self.r.update(np.array([d.bbox for d in dets], F32))
        for d, i in zip(dets, ids):
            d.track_id = i
        self.of.initialize(frame, dets)
        return dets

    def interpolate(self, frame):
        tracked = self.of.track(frame)
        ids = self.r.pt_ids
        nxt = np.array([tracked.get(i, (0.0, 0.0)) for i in ids], F32).reshape(-1, 2)
        return self.r.interpolate(nxt, np.array([i in tracked for i in ids], np.uint8))

    def close(self):
        self.of.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the rows as JSON to this file")
    args = ap.parse_args()
    assert args.pairs >= 5
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_lwt: no GPU visible; nothing is measured without one")
    host = FC.structured_pair(H, W, 502, (2, 1))
    dev = [torch.from_numpy(f).to("cuda") for f in host]
    torch.cuda.synchronize()
    rows = []
    for n in (21, 100):
        boxes = boxes_on_grid(n)
        for where, frames in (("host", host), ("device", dev)):
            paths = {"fused": HipLightweightTracker(max_tracks=256), "baseline": Baseline()}

            def window(path):
                """One detection frame, then in-between frames going back and forth between the two frames; seconds per call of each kind."""
                dets = [SimpleNamespace(bbox=tuple(float(v) for v in b), track_id=None, features=None) for b in boxes]
                t0 = time.perf_counter()
                path.update_with_detections(frames[0], dets)
                t1 = time.perf_counter()
                for f in range(args.frames):
                    recs = path.interpolate(frames[(f + 1) % 2])
                t2 = time.perf_counter()
                return t1 - t0, (t2 - t1) / args.frames, recs

            got = {k: window(p)[2] for k, p in paths.items()}   # warm-up, and the two paths agree
            assert [q[0] for q in got["fused"]] == [q[0] for q in got["baseline"]] and np.array_equal(np.array([q[1] for q in got["fused"]]), np.array([q[1] for q in got["baseline"]]))
            times = {k: [] for k in paths}
            for _ in range(args.pairs):
                for k, p in paths.items():
                    times[k].append(window(p)[:2])
            followed = paths["fused"].info().n_points
            for p in paths.values():
                p.close()
            row = {"tracks": n, "frames_from": where, "size": [H, W], "pairs": args.pairs, "in_between_frames_per_window": args.frames, "points_followed": int(followed)}
            for k, v in times.items():
                v = np.array(v) * 1e3
                for j, call in enumerate(("update", "interpolate")):
                    row[f"{k}_{call}_ms_median"] = round(float(np.median(v[:, j])), 4)
                    row[f"{k}_{call}_ms_min_max"] = [round(float(v[:, j].min()), 4), round(float(v[:, j].max()), 4)]
            for call in ("update", "interpolate"):
                row[f"{call}_speedup_of_medians"] = round(row[f"baseline_{call}_ms_median"] / row[f"fused_{call}_ms_median"], 2)
            rows.append(row)
            print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
