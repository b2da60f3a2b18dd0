"""A run of frames of one camera through detector and tracker on one MI355X: ``HipDetrDetector.detect_and_track_batch`` (one
opd_detr_detect_sequence_track per chunk of B frames: one batched forward, the association on the device, one host wait) against the loop of B
``detect_and_track`` calls it replaces, on twin trackers, same detector handle (device_nms=True, max_batch = B), same build, in interleaved
rounds.  The loop is the yardstick and its own round-to-round spread the margin.  At nms_threshold 0.4 (one kept record a frame) and 1.0 (all
100 kept), features "color" and None, 720 x 1280 frames.  Host clock around calls that end in a device wait.

Then the association alone: ``track_assoc_kernel`` (between two device events per launch) against the host's ``associate()`` (its own clock) on
the same T x N matrices, through the test library's opd_track_test_bench_assoc.  A figure where the device is slower is printed like any other.

    python tools/bench_track_sequence.py [--batch 8] [--kinds color,none] [--nms 0.4,1.0] [--rounds 7] [--iters 12] [--json out.json]
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

from office_person_detection_vit_amd import HipDetrDetector, HipTracker, _capi  # noqa: E402
from office_person_detection_vit_amd.frames import structured_frames  # noqa: E402
from office_person_detection_vit_amd.weights import DetrArch, ensure_weight_file  # noqa: E402


def timed(call, iters):
    t = time.perf_counter()
    for _ in range(iters):
        call()
    return (time.perf_counter() - t) / iters * 1e3


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def bench_calls(args, rows):
    cache = os.environ.get("OPD_WEIGHT_CACHE", "/tmp/opd_weights")
    H, W, B = 720, 1280, args.batch
    frames = [np.ascontiguousarray(f) for f in structured_frames(B, H, W, seed=99)]
    det = HipDetrDetector(model_path=ensure_weight_file(cache, DetrArch(), 0, 1.0, "r50"), max_batch=B, confidence_threshold=0.05, device_nms=True)
    det.load_model()
    for name in args.kinds.split(","):
        features = None if name == "none" else name
        D = 64 if features is None else 256
        for nms in [float(t) for t in args.nms.split(",")]:
            det.nms_threshold = nms
            # (the seeded detector's scores on these frames stay below the reference's high_conf_threshold of 0.5, at which no track would ever start)
            a, b = (HipTracker(feature_dim=D, max_tracks=256, max_dets=128, min_hits=1, high_conf_threshold=0.06) for _ in range(2))
            seen = {}

            def sequence():
                seen["sequence"] = det.detect_and_track_batch(frames, a, features=features)

            def loop():
                seen["loop"] = [det.detect_and_track(f, b, features=features) for f in frames]

            for _ in range(args.warmup):
                loop()
                sequence()
            key = lambda run: [[(d.track_id, d.bbox) for d in f] for f in run]   # noqa: E731
            same = key(seen["sequence"]) == key(seen["loop"])
            tl, ts = [], []
            for _ in range(args.rounds):   # interleaved: drift of the machine lands on both
                tl.append(timed(loop, args.iters) / B)
                ts.append(timed(sequence, args.iters) / B)
            pairs = sum(s < l for s, l in zip(ts, tl))
            rows.append({"what": "ms per frame", "batch": B, "features": name, "nms_threshold": nms, "tracked_per_frame": len(seen["sequence"][-1]),
                         "tracks": len(a.get_tracks()), "ids_identical": bool(same), "loop": stats(tl), "sequence": stats(ts),
                         "loop_spread_ms": round(max(tl) - min(tl), 4), "saved_ms_per_frame": round(float(np.median(tl) - np.median(ts)), 4),
                         "frames_per_s_loop": round(1e3 / float(np.median(tl)), 1), "frames_per_s_sequence": round(1e3 / float(np.median(ts)), 1),
                         "rounds_sequence_faster": f"{pairs} of {args.rounds}"})
            print(json.dumps(rows[-1]), flush=True)
            a.close()
            b.close()
    det.close()


def bench_association(args, rows):
    lib = _capi.load_library(test_hooks=True)
    rng = np.random.default_rng(11)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    for T, N in ((12, 16), (30, 21), (100, 100)):
        for kind in ("uniform", "ties"):
            draw = (lambda: rng.random((T, N), dtype=np.float32)) if kind == "uniform" else (lambda: rng.choice(np.array([0.25, 0.5, 1.0], np.float32), size=(T, N)))
            app, iou, comb = (np.ascontiguousarray(draw()) for _ in range(3))
            hits, conf = rng.integers(0, 6, T).astype(np.int32), rng.uniform(0.2, 0.9, N).astype(np.float32)
            ks, hs = [], []
            for _ in range(args.rounds):
                k, h = C.c_float(), C.c_float()
                _capi.check(lib.opd_track_test_bench_assoc(0, p(app), p(iou), p(comb), T, N, p(hits), p(conf), 3, 0.5, N, 50, C.byref(k), C.byref(h)), "opd_track_test_bench_assoc")
                ks.append(k.value)
                hs.append(h.value)
            rows.append({"what": "association alone, ms", "T": T, "N": N, "costs": kind, "kernel": stats(ks), "host": stats(hs)})
            print(json.dumps(rows[-1]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--kinds", default="color,none")
    ap.add_argument("--nms", default="0.4,1.0")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    os.environ.setdefault("OPD_TEST_HOOKS", "1")   # (one process, one library: the association figures need the test build's hook)
    rows = []
    bench_calls(args, rows)
    bench_association(args, rows)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump({"rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
