"""Shared by tests/test_records_cpu.py and tests/test_record_view_gpu.py: the hand-made records of tests/tile_stages_common.py in BOTH forms a sink
stage reads them in (csrc/opd_records.h), with what separates the stages' filter and key rules: two records of another label, and (post-process form
only: a merged record is named by its position) one ``query_index`` at the stride and one below zero."""

import numpy as np

import tile_stages_common as TS
from tile_common import TILE_DET
from track_ingest_common import DET

S = TS.S
LABEL = 1                       # the label of the hand-made records, and the stage label of the hooks
OTHER = ((0, 1, 0), (1, 2, 3))  # (frame, record, label): inside the counts of the run [8, 3]
QUERY = ([3, 0, 6, 1, S, 2, 5, 4], [7, -1, 0, 4, 2, 6, 1, 3])   # post-process form: distinct per frame; (0, 4) and (1, 1) name no row


def merged(counts):
    recs = TS.merged(counts)
    for f, k, label in OTHER:
        recs[f, k]["label"] = label
    return recs


def dets(counts):
    """[2][S] post-process records of the same boxes: float32 corners, QUERY as query_index; slots at and behind a count hold decoys."""
    src = merged(counts)
    recs = np.zeros((2, S), DET)
    f32 = np.float32
    recs["x1"], recs["y1"] = src["x"].astype(f32), src["y"].astype(f32)
    recs["x2"], recs["y2"] = (src["x"] + src["w"]).astype(f32), (src["y"] + src["h"]).astype(f32)
    recs["score"], recs["label"] = src["score"], src["label"]
    recs["query_index"] = np.asarray(QUERY, np.int32)
    recs["frame"] = np.arange(2, dtype=np.int32)[:, None]
    return recs


def box64(recs):
    """The float64 box x, y, w, h of every record, [..][4]: Detection.bbox as Python holds it."""
    if recs.dtype == TILE_DET:
        return np.stack([recs["x"], recs["y"], recs["w"], recs["h"]], -1).astype(np.float64)
    x1, y1 = recs["x1"].astype(np.float64), recs["y1"].astype(np.float64)
    return np.stack([x1, y1, recs["x2"].astype(np.float64) - x1, recs["y2"].astype(np.float64) - y1], -1)
