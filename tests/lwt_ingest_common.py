"""The ingest launch of the fused hybrid detect call (``lwt_ingest_kernel``, csrc/kernels_lwt.hip) restated in numpy: one frame's kept
records -> the float32 ``[n][4]`` xywh image ``HipLightweightTracker.update_with_detections`` builds as
``np.array([d.bbox for d in dets], np.float32)``.  ``detector.py::_postprocess_batch`` takes the corners as they are and the width and
height as differences of the float32 corners in Python floats (float64); the float32 array rounds each once.  That is the box rule of
``track_ingest_kernel`` (track_ingest_common.py), without its foot points, flags and feature rows."""

import numpy as np

import track_ingest_common as TI

DET = TI.DET


def pack(records):
    """boxes xywh [n][4] float32 of `records` (a DET array)."""
    return TI.pack(records)[0]


def ingest(records, n, Q, boxes):
    """What the launch does to the staging array (in place; it arrives holding the caller's sentinels) and the count it publishes."""
    n = max(0, min(int(n), Q))
    boxes[:n] = pack(records[:n])
    return n


def edge_records(h=720, w=1280):
    """Records touching 0 and the frame edge, degenerate ones, and corners whose difference is no float32 number; then TI.hard_records()
    and as many regular ones as fill 100."""
    f = np.float32
    rows = [
        (f(0.0), f(0.0), f(w), f(h)),                                   # the whole frame
        (f(0.0), f(10.5), f(33.3), f(h)),                               # left and bottom edge
        (f(w) - f(0.1), f(0.0), f(w), f(0.7)),                          # right and top edge, a difference that needs rounding
        (f(w), f(h), f(w), f(h)),                                       # empty, at the far corner
        (f(0.0), f(0.0), f(0.0), f(0.0)),                               # empty, at the origin
        (f(np.nextafter(f(0.0), f(1.0))), f(0.0), f(1.0), f(1e-30)),    # a subnormal corner
        (f(1279.9999), f(719.99994), f(w), f(h)),                       # the last representable numbers below the edge
    ]
    hard = TI.hard_records()
    recs = np.zeros(100, DET)
    for i, (x1, y1, x2, y2) in enumerate(rows):
        recs[i] = (x1, y1, x2, y2, f(0.99) - f(0.001) * f(i), 1, i, 0)
    recs[len(rows):len(rows) + len(hard)] = hard
    rng = np.random.default_rng(23)
    for i in range(len(rows) + len(hard), 100):
        x1, y1 = f(rng.uniform(0, w - 2)), f(rng.uniform(0, h - 2))
        recs[i] = (x1, y1, f(min(w, x1 + f(rng.uniform(0, 300)))), f(min(h, y1 + f(rng.uniform(0, 500)))), f(0.5), 1, i, 0)
    recs["query_index"] = np.random.default_rng(5).permutation(100).astype(np.int32)
    return recs
