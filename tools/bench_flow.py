"""Optical flow on one MI355X: milliseconds per opd_flow_track call on 720 x 1280 frames with 21 and 100 points (21.25 detections per
frame is the reference's published session average; 100 is its max_corners), frames in host memory and in device memory, next to the
numpy restatement of the same arithmetic (tests/flow_common.py) on the same box for context.  Host clock around calls that end in a
device wait.  A call is gray + a 4-level pyramid of the new frame + the LK launch.

    python tools/bench_flow.py [--iters 200] [--json out.json]
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import flow_common as F  # noqa: E402
from office_person_detection_vit_amd import _capi  # noqa: E402


def timed(call, warmup, iters):
    for _ in range(warmup):
        call()
    t = time.perf_counter()
    for _ in range(iters):
        call()
    return (time.perf_counter() - t) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--sizes", default="21,100")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch
    lib = _capi.load_library()
    H, W = 720, 1280
    f0, f1 = F.structured_pair(H, W, seed=99)
    dev = [torch.from_numpy(f).cuda() for f in (f0, f1)]
    torch.cuda.synchronize()
    rng = np.random.default_rng(0)
    rows = []
    handle = F.flow_create(lib, H, W, 128)
    for n in [int(s) for s in args.sizes.split(",")]:
        pts = np.stack([rng.uniform(40, W - 40, n), rng.uniform(40, H - 40, n)], 1).astype(np.float32)
        for kind, name, frames in ((_capi.OPD_MEM_HOST, "host", (f0, f1)), (_capi.OPD_MEM_DEVICE, "device", [(t.data_ptr(), H, W) for t in dev])):
            F.flow_set_reference(lib, handle, frames[0], kind)
            state = {"k": 0}

            def call():   # alternate the two frames: every call sees a new frame, as a video does
                state["k"] ^= 1
                return F.flow_track(lib, handle, frames[state["k"]], pts, kind)

            ms = timed(call, args.warmup, args.iters)
            rows.append({"what": "opd_flow_track", "frames": name, "n": n, "ms_per_call": round(ms, 4)})
            print(json.dumps(rows[-1]), flush=True)
        p0, p1 = F.pyramid(f0), F.pyramid(f1)
        t = time.perf_counter()
        reps = max(2, args.iters // 50)
        for _ in range(reps):
            want, st = F.lk_pyramids(p0, F.pyramid(f1), pts, dtype=np.float32)
        ms = (time.perf_counter() - t) / reps * 1e3
        F.flow_set_reference(lib, handle, f0)
        got, gst = F.flow_track(lib, handle, f1, pts)
        same = st == gst
        rows.append({"what": "numpy restatement (float32; gray + pyramid of one frame + LK)", "n": n, "ms_per_call": round(ms, 3),
                     "status_equal": int(same.sum()), "found": int(gst.sum()),
                     "max_abs_device_minus_numpy_found": float(np.abs(got - want)[same & (gst == 1)].max()) if (same & (gst == 1)).any() else None})
        print(json.dumps(rows[-1]), flush=True)
    lib.opd_flow_destroy(handle)
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
