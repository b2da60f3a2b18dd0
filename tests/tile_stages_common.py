"""Shared by tests/test_tile_stages_cpu.py and tests/test_tile_stages_gpu.py: the hand-made MERGED records of a tiled call (``opd_tile_det``:
float64 x, y, w, h in frame pixels) on which the merged-record readers of the colour, floor and tracker-ingest kernels are held to the separate
calls, what those separate calls are handed (the host arrays ``extract_color_features``, ``HipFloorMapper`` and ``HipTracker.update`` build), and
the field-for-field comparison of detection lists.  Every comparison is an equality."""

import numpy as np

from tile_common import TILE_DET

FRAME_HW = (48, 64)   # h, w of the two hand-made frames
S = 8                 # record slots per frame (n_tiles x num_queries of a real call)
RUNS = ([5, 0], [8, 3])   # counts of the two runs

# (x, y, w, h) in float64.  What each is for:
BOXES = [
    (10.3, 5.7, 20.45, 30.9),              # fractional sides
    (50.2, 30.1, 30.5, 40.0),              # partly outside the frame (clipped right and below)
    (15.99999999, 7.99999999, 23.5, 17.25),   # float32 rounding moves the integer crop edge: int(15.99999999) = 15, int(float32(..)) = 16
    (7.7, 10.1, 3.3, 7.3),                 # x + w / 2 and y + h in float64 round to other float32 than the foot point of the rounded box
    (-5.5, 3.25, 20.75, 20.5),             # negative x
    (20.0, 10.0, 0.0, 15.5),               # w = 0: the reference's dummy crop
    (100.0, 100.0, 10.0, 10.0),            # wholly outside: dummy crop
    (0.0, 0.0, 64.0, 48.0),                # the whole frame
]
assert int(BOXES[2][0]) == 15 and int(float(np.float32(BOXES[2][0]))) == 16
_x, _y, _w, _h = BOXES[3]
assert np.float32(_x + _w / 2) != np.float32(float(np.float32(_x)) + float(np.float32(_w)) / 2.0)
assert np.float32(_y + _h) != np.float32(float(np.float32(_y)) + float(np.float32(_h)))


def frames(seed=17):
    """Two 48 x 64 BGR frames of random bytes, one block [2][48][64][3]."""
    return np.random.RandomState(seed).randint(0, 256, size=(2, FRAME_HW[0], FRAME_HW[1], 3)).astype(np.uint8)


def merged(counts):
    """[2][S] merged records: frame 0 takes BOXES in order, frame 1 in reversed order; slots at and behind a count hold decoys (a box over everything,
    score 2, query_index -7).  query_index repeats between records, as it does between two tiles of a frame: it names no row."""
    recs = np.zeros((2, S), TILE_DET)
    recs["x"], recs["y"], recs["w"], recs["h"], recs["score"], recs["label"], recs["query_index"], recs["tile"] = -1e6, -1e6, 2e6, 2e6, 2.0, 1, -7, 0
    for f, order in enumerate((BOXES, BOXES[::-1])):
        for k in range(counts[f]):
            recs[f, k] = (*order[k], np.float32(0.95 - 0.07 * k - 0.01 * f), 1, k % 3, k % 4)
    return recs


def host_arrays(recs_f, n):
    """What the separate calls are handed for the first n records of one frame: float32 boxes (np.asarray(d.bbox, np.float32)), the tracker's foot
    points (camera_coords in float64 from the unrounded doubles, stored as float32) and confidences."""
    bbox = [(float(r["x"]), float(r["y"]), float(r["w"]), float(r["h"])) for r in recs_f[:n]]
    boxes = np.ascontiguousarray(np.asarray(bbox, dtype=np.float32).reshape(-1, 4))
    foot = np.zeros((n, 2), np.float32)
    for j, (x, y, w, h) in enumerate(bbox):
        foot[j] = (x + w / 2, y + h)
    conf = np.asarray([float(r["score"]) for r in recs_f[:n]], np.float32)
    return bbox, boxes, foot, conf


FIELDS = ("bbox", "confidence", "class_id", "class_name", "camera_coords", "floor_coords", "floor_coords_mm", "zone_ids", "track_id", "features", "appearance_score",
          "query_index")


def fields(d):
    return (d.bbox, d.confidence, d.class_id, d.class_name, d.camera_coords, d.floor_coords, d.floor_coords_mm, tuple(d.zone_ids), d.track_id,
            None if d.features is None else np.asarray(d.features).tobytes(), d.appearance_score, d.query_index)


def same(a, b, what, skip_features=False):
    """Two lists of per-frame detection lists, field for field (`skip_features`: all but det.features, which a fused tracked call leaves on the device)."""
    assert len(a) == len(b), what
    for f, (x, y) in enumerate(zip(a, b)):
        fa, fb = [fields(d) for d in x], [fields(d) for d in y]
        if skip_features:
            fa, fb = [t[:9] + t[10:] for t in fa], [t[:9] + t[10:] for t in fb]
        if fa != fb:   # name the first field that differs
            names = [n for i, n in enumerate(FIELDS) if not (skip_features and i == 9)]
            diff = [(k, names[i]) for k, (p, q) in enumerate(zip(fa, fb)) for i in range(len(names)) if p[i] != q[i]]
            assert False, f"{what}: frame {f}: {len(fa)} and {len(fb)} detections, first differences (detection, field) {diff[:4]}"
