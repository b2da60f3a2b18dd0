"""K frames each of C cameras through detector and trackers on one MI355X: ``HipDetrDetector.detect_and_track_streams`` (one
opd_detr_detect_streams_track: one forward at batch C x K, the cameras' tracker steps side by side, one host wait) against what the callers had
before, on twin trackers, same detector handle (device_nms=True, max_batch = 8), same build, in interleaved rounds:

  (a) C calls of ``detect_and_track_batch`` of K frames each (C forwards at batch K, C waits, C x K serial steps);
  (b) for K = 1, one opd_detr_detect_frames_track call over the C frames (one forward, one wait, the association on the host behind it).

720 x 1280 frames, seeded weights, colour features; at one kept record a frame (suppression at 0.4) and at about 20 (the reference's own density:
the suppression threshold nearest to it is searched for).  Results are asserted identical before anything is timed.  A shape where the new call is
slower is printed like any other.  Host clock around calls that end in a device wait.

    python tools/bench_track_streams.py [--shapes 2x4,4x2,8x1] [--rounds 7] [--iters 8] [--json out.json]
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

H, W, MAX_BATCH, PERSON = 720, 1280, 8, 1


def timed(call, iters):
    t = time.perf_counter()
    for _ in range(iters):
        call()
    return (time.perf_counter() - t) / iters * 1e3


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def nms_for_density(det, frames, target):
    """The suppression threshold in 0.4 .. 1.0 whose mean kept count over `frames` is nearest to `target` (the count grows with the threshold)."""
    def kept(thr):
        det.nms_threshold = thr
        return float(np.mean([len(d) for d in det.detect_batch(frames)]))
    lo, hi = 0.4, 1.0
    for _ in range(10):
        mid = (lo + hi) / 2
        lo, hi = (mid, hi) if kept(mid) < target else (lo, mid)
    return min((lo, hi), key=lambda t: abs(kept(t) - target))


def trackers(n):
    # (the seeded detector's scores on these frames stay below the reference's high_conf_threshold of 0.5, at which no track would ever start)
    return [HipTracker(feature_dim=256, max_tracks=256, max_dets=128, min_hits=1, high_conf_threshold=0.06) for _ in range(n)]


def frames_track(det, handles, frames):
    """(b): one opd_detr_detect_frames_track over one frame of each camera; the ids of the kept records per frame."""
    n, Q = len(frames), det.num_queries
    recs, counts = (_capi.OpdDet * (n * Q))(), (C.c_int32 * n)()
    ids, nf = np.full((n, Q), -1, np.int32), np.zeros(n, np.int32)
    ptrs = (C.c_void_p * n)(*[f.ctypes.data for f in frames])
    hs = (C.c_void_p * n)(*[t._h.value for t in handles])
    target = det._frame_list_target(frames)
    _capi.check(det._lib.opd_detr_detect_frames_track(C.c_void_p(det.model), None, hs, ptrs, n, H, W, target[0], target[1], float(det.confidence_threshold), PERSON,
                                                      _capi.OPD_TRACK_FEAT_COLOR, 0, recs, counts, ids.ctypes.data, nf.ctypes.data), "opd_detr_detect_frames_track")
    return [[int(i) for i in ids[b, :counts[b]] if i >= 0] for b in range(n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="2x4,4x2,8x1")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    cache = os.environ.get("OPD_WEIGHT_CACHE", "/tmp/opd_weights")
    pool = [np.ascontiguousarray(f) for f in structured_frames(MAX_BATCH, H, W, seed=99)]
    det = HipDetrDetector(model_path=ensure_weight_file(cache, DetrArch(), 0, 1.0, "r50"), max_batch=MAX_BATCH, confidence_threshold=0.05, device_nms=True)
    det.load_model()
    dense = nms_for_density(det, pool, 20.0)
    rows = []
    for shape in args.shapes.split(","):
        n_cams, K = (int(v) for v in shape.split("x"))
        per_camera = [pool[c * K:(c + 1) * K] for c in range(n_cams)]
        for nms in (0.4, dense):
            det.nms_threshold = nms
            a, b, d = trackers(n_cams), trackers(n_cams), trackers(n_cams)
            seen = {}

            def streams():
                seen["streams"] = det.detect_and_track_streams(per_camera, a, features="color")

            def per_cam():
                seen["per_camera"] = [det.detect_and_track_batch(f, t, features="color") for f, t in zip(per_camera, b)]

            def one_frames_call():
                seen["frames_track"] = frames_track(det, d, [cam[0] for cam in per_camera])

            sides = [("per_camera", per_cam)] + ([("frames_track", one_frames_call)] if K == 1 else [])
            for t in d:
                t._ensure()
            for _ in range(args.warmup):
                for _, call in sides:
                    call()
                streams()
            key = lambda run: [[[(x.track_id, x.bbox) for x in f] for f in cam] for cam in run]   # noqa: E731
            assert key(seen["streams"]) == key(seen["per_camera"]), "the streams call and the per-camera calls disagree"
            if K == 1:
                assert [[x.track_id for x in cam[0]] for cam in seen["streams"]] == seen["frames_track"], "the streams call and the frames call disagree"
            times = {name: [] for name, _ in sides + [("streams", streams)]}
            for _ in range(args.rounds):   # interleaved: drift of the machine lands on all sides
                for name, call in sides + [("streams", streams)]:
                    times[name].append(timed(call, args.iters))
            info = _capi.OpdTrackStatus()
            _capi.check(a[0]._lib.opd_track_info(a[0]._h, C.byref(info)), "opd_track_info")
            row = {"what": "ms per call set", "cameras": n_cams, "frames_per_camera": K, "nms_threshold": round(nms, 4),
                   "kept_per_frame": round(float(np.mean([len(f) for cam in seen["streams"] for f in cam])), 1), "results_identical": True,
                   "streams_launches": int(info.last_launches), "streams": stats(times["streams"])}
            for name, _ in sides:
                won = sum(s < o for s, o in zip(times["streams"], times[name]))
                row[name] = stats(times[name])
                row[f"streams_faster_than_{name}"] = f"{won} of {args.rounds}"
                row[f"saved_ms_vs_{name}"] = round(float(np.median(times[name]) - np.median(times["streams"])), 4)
            rows.append(row)
            print(json.dumps(row), flush=True)
            for t in a + b + d:
                t.close()
    det.close()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump({"rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
