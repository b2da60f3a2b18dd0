"""Time one tracker update on the device (``opd_track_update``) at (tracks, detections) = (12, 16), (30, 21) and (100, 100) with D = 512,
features handed over from host memory and from device memory, next to the per-pair numpy restatement (tests/track_common.py, float32) of the
same frames on the same machine.

    python tools/bench_track.py [--updates 200] [--windows 5] [--out FILE.json]

An update ends in a host wait, but its second launch is only enqueued, so a window of ``--updates`` consecutive updates is timed with a
host clock and closed by ``opd_track_get`` (which waits for the stream).  Every shape is warmed up first; the two feature sources alternate
window by window in one process, and the spread over the windows is reported next to the median.  No GPU: the tool fails."""

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import track_common as TC  # noqa: E402
from office_person_detection_vit_amd import _capi  # noqa: E402

F32 = np.float32
D = 512


def scene(T, N, n_frames, seed):
    """T slow walkers on a grid; each frame shows the first min(T, N) of them, and N - T low-confidence detections when N > T."""
    rng = np.random.default_rng(seed)
    cols = int(np.ceil(np.sqrt(T)))
    pos = np.stack([100 + 260.0 * (np.arange(T) % cols), 200 + 300.0 * (np.arange(T) // cols)], 1)
    vel = rng.uniform(-1.5, 1.5, (T, 2))
    base = rng.standard_normal((T, D))
    base /= np.linalg.norm(base, axis=1, keepdims=True)
    extra = max(N - T, 0)
    frames = []
    for f in range(n_frames):
        shown = T if f == 0 else min(T, N)   # the first frame starts every track
        p = pos[:shown] + vel[:shown] * (f % 40)
        boxes = np.concatenate([np.stack([p[:, 0] - 30, p[:, 1] - 150, np.full(shown, 60.0), np.full(shown, 150.0)], 1),
                                np.stack([rng.uniform(0, 3000, extra), rng.uniform(3000, 4000, extra), np.full(extra, 50.0), np.full(extra, 120.0)], 1)]).astype(F32)
        if f == 0:
            boxes = boxes[:T]
        feats = base[:shown] + rng.standard_normal((shown, D)) * (0.2 / np.sqrt(D))
        feats = np.concatenate([feats, rng.standard_normal((len(boxes) - shown, D))])
        feats = (feats / np.linalg.norm(feats, axis=1, keepdims=True)).astype(F32)
        conf = np.concatenate([np.full(shown, 0.9), np.full(len(boxes) - shown, 0.3)]).astype(F32)
        foot = np.stack([boxes[:, 0] + boxes[:, 2] / F32(2), boxes[:, 1] + boxes[:, 3]], 1).astype(F32)
        frames.append((boxes, foot, conf, feats))
    return frames


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--updates", type=int, default=200)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the rows as JSON to this file")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_track: no GPU visible; nothing is measured without one")
    lib = _capi.load_library()
    rows = []
    for T, N in ((12, 16), (30, 21), (100, 100)):
        frames = scene(T, N, 1 + args.warmup + args.updates, seed=T * 1000 + N)
        dev_feats = [torch.from_numpy(fr[3]).to("cuda") for fr in frames]
        torch.cuda.synchronize()
        handles = {k: TC.create(lib, _capi, D, max_tracks=128, max_dets=128, max_age=1 << 20) for k in ("host", "device")}
        n = C.c_int()

        def window(kind, lo, hi):
            h = handles[kind]
            t0 = time.perf_counter()
            for f in range(lo, hi):
                b, ft, cf, fe = frames[f]
                rc, _ = TC.device_update(lib, _capi, h, b, ft, cf, fe if kind == "host" else None, feat_ptr=dev_feats[f].data_ptr() if kind == "device" else None)
                if rc != 0:
                    sys.exit(f"opd_track_update failed: {_capi.last_error()}")
            _capi.check(lib.opd_track_get(h, None, 0, C.byref(n)), "opd_track_get")
            recs = (_capi.OpdTrackRec * n.value)()
            _capi.check(lib.opd_track_get(h, recs, n.value, C.byref(n)), "opd_track_get")   # waits for the last commit launch
            return (time.perf_counter() - t0) / (hi - lo)

        times = {"host": [], "device": []}
        for kind in times:
            window(kind, 0, 1 + args.warmup)
            assert n.value == T, (n.value, T)
        for _ in range(args.windows):
            for kind in times:   # alternating; every window replays the same frames (the tracks follow: positions are periodic)
                times[kind].append(window(kind, 1 + args.warmup, 1 + args.warmup + args.updates))
        for h in handles.values():
            lib.opd_track_destroy(h)
        r = TC.Restatement(D, np.float32, max_age=1 << 20)
        for f in range(3):
            b, ft, cf, fe = frames[f]
            r.update(b, ft, cf, fe)
        t0 = time.perf_counter()
        for f in range(3, 6):
            b, ft, cf, fe = frames[f]
            r.update(b, ft, cf, fe)
        numpy_ms = (time.perf_counter() - t0) / 3 * 1e3
        row = {"tracks": T, "detections": N, "D": D, "updates_per_window": args.updates, "windows": args.windows, "numpy_restatement_ms": round(numpy_ms, 3)}
        for kind, v in times.items():
            v = np.array(v) * 1e3
            row[f"{kind}_features_ms_median"] = round(float(np.median(v)), 4)
            row[f"{kind}_features_ms_min_max"] = [round(float(v.min()), 4), round(float(v.max()), 4)]
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
