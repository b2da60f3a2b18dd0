"""Shared by tests/test_tile_hybrid_cpu.py and tests/test_tile_hybrid_gpu.py: the numpy restatement of ``lwt_ingest_kernel`` on the MERGED records
of a tiled call (``opd_tile_det``: float64 x, y, w, h in frame pixels), the merged detections of ``tile_common``'s cases as the Python path holds
them, and hand-made merged records for the kernel alone.  The restatement is held to ``np.array([d.bbox for d in dets], np.float32)``, what
``HipLightweightTracker.update_with_detections`` hands ``opd_lwt_update``, by the CPU file; the kernel to the restatement by the GPU file."""

import numpy as np

from office_person_detection_vit_amd.data_models import Detection
from office_person_detection_vit_amd.tiling import merge_tile_detections
from tile_common import TILE_DET

F32 = np.float32


def ingest_merged(merged, n, S, boxes):
    """lwt_ingest_kernel on a view of merged records: the count clamped to 0 .. S, rows [0, n) of `boxes` written with x, y, w, h each rounded from
    float64 to float32 ONCE (nothing is re-derived), the rows behind left alone.  Returns the clamped count."""
    n = max(0, min(int(n), int(S)))
    for k, name in enumerate(("x", "y", "w", "h")):
        boxes[:n, k] = merged[name][:n].astype(F32)
    return n


def merged_detections(case):
    """``tiling.merge_tile_detections`` on a case of tile_common.cases(), per frame: the Detection list the host path hands the tracker."""
    T = len(case["tiles"])
    origins = [(int(t[0]), int(t[1])) for t in case["tiles"]]
    sizes = [(int(t[2]), int(t[3])) for t in case["tiles"]]
    out = []
    for f in range(case["n_frames"]):
        per_tile = []
        for t in range(T):
            dets = []
            for i in range(max(0, int(case["counts"][f * T + t]))):
                r = case["recs"][f * T + t, i]
                x1, y1, x2, y2 = float(r["x1"]), float(r["y1"]), float(r["x2"]), float(r["y2"])
                bbox = (x1, y1, float(x2 - x1), float(y2 - y1))   # HipDetrDetector._postprocess_batch
                dets.append(Detection(bbox=bbox, confidence=float(r["score"]), class_id=int(r["label"]), class_name="person",
                                      camera_coords=(bbox[0] + bbox[2] / 2, bbox[1] + bbox[3]), query_index=int(r["query_index"])))
            per_tile.append(dets)
        out.append(merge_tile_detections(per_tile, origins, case["nms"], sizes, case["frame"], case["merge"], case["tol"]))
    return out


def as_merged(dets, S):
    """[S] merged records as tile_merge_kernel leaves the detections `dets` of one frame; slots behind them hold decoys."""
    recs = decoys(S)
    for k, d in enumerate(dets):
        recs[k] = (*d.bbox, F32(d.confidence), d.class_id, d.query_index, 0)
    return recs


def decoys(S):
    recs = np.zeros(S, TILE_DET)
    recs["x"], recs["y"], recs["w"], recs["h"], recs["score"], recs["label"], recs["query_index"], recs["tile"] = -1e6, -1e6, 2e6, 2e6, 2.0, 1, -7, 0
    return recs


def edge_merged(S, h=2160, w=3840, seed=11):
    """[S] merged records whose doubles are NOT float32 numbers (each of the four rounds, and x + w rounded differs from the rounded x plus the
    rounded w for most), and among the first ones: boxes touching 0 and the frame edge, a zero width, a zero area, a negative width, values one
    float32 step apart, a box far outside."""
    rng = np.random.RandomState(seed)
    recs = decoys(S)
    x, y = rng.uniform(0, w - 50, S), rng.uniform(0, h - 50, S)
    bw, bh = rng.uniform(0.5, 400, S), rng.uniform(0.5, 900, S)
    recs["x"], recs["y"], recs["w"], recs["h"] = x, y, np.minimum(bw, w - x), np.minimum(bh, h - y)
    recs["score"], recs["query_index"], recs["tile"] = np.sort(rng.uniform(0.05, 0.99, S).astype(F32))[::-1], np.arange(S) % 100, np.arange(S) % 4
    up = float(np.nextafter(F32(1000), F32(2000)))
    special = [(0.0, 0.0, float(w), float(h)), (0.0, 17.3, 20.7, h - 17.3), (w - 33.3, h - 77.7, 33.3, 77.7), (100.1, 200.2, 0.0, 50.5),
               (5.5, 5.5, 0.0, 0.0), (300.3, 300.3, -10.1, 20.2), (1000.0, (1000.0 + up) / 2, up, 1000.0 + 1e-9), (-1e5, 3e6, 1e-30, 1e30),
               (15.99999999, 7.99999999, 23.5, 17.25)]
    for k, b in enumerate(special[:S]):
        recs["x"][k], recs["y"][k], recs["w"][k], recs["h"][k] = b
    return recs


def python_boxes(dets):
    """What HipLightweightTracker.update_with_detections builds from a Detection list."""
    return np.array([d.bbox for d in dets], F32).reshape(len(dets), 4)
