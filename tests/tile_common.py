"""Shared by tests/test_tile_cpu.py and tests/test_tile_gpu.py: ONE generator of tiled-detection merge cases (tile-local ``opd_det`` records per
tile, the way the post-process and the per-tile suppression leave them), the expected result of each from the Python rule itself
(``tiling.merge_tile_detections`` on ``Detection``s built the way ``HipDetrDetector._postprocess_batch`` builds them), and the helpers that
run a case through a routine with ``opd_detr_merge_tiles``'s arguments and compare.

Every comparison is exact: the four float64 of a box with ``==``, the score, the label, the ``query_index`` and the tile of the record that
opened the kept slot, the order and the counts.  Slots at and beyond a tile's count hold decoys (score 2, a box over everything,
``query_index`` -7): a routine that reads them shows."""

import ctypes as C

import numpy as np

from nms_common import DET   # the 32-byte opd_det
from office_person_detection_vit_amd import _capi
from office_person_detection_vit_amd.data_models import Detection
from office_person_detection_vit_amd.tiling import merge_tile_detections, tile_grid

TILE_DET = np.dtype([("x", "<f8"), ("y", "<f8"), ("w", "<f8"), ("h", "<f8"), ("score", "<f4"), ("label", "<i4"), ("query_index", "<i4"), ("tile", "<i4")])
assert DET.itemsize == C.sizeof(_capi.OpdDet) == 32 and TILE_DET.itemsize == C.sizeof(_capi.OpdTileDet) == 48

FRAME = (200, 300)                                # h, w
GRID = tile_grid(200, 300, 2, 2, 0.125)           # (0,0) (0,131) (88,0) (88,131), every tile 112 x 169: tx = 1.69, ty = 1.12
assert GRID == [(0, 0, 112, 169), (0, 131, 112, 169), (88, 0, 112, 169), (88, 131, 112, 169)]
RANDOM_SEEDS = (3, 4, 5, 6)


def _local(tile, box):
    """A frame-space xyxy box as the float32 tile-local record box of `tile`."""
    y0, x0 = tile[0], tile[1]
    return [box[0] - x0, box[1] - y0, box[2] - x0, box[3] - y0]


def _case(name, tiles, frame, per_tile, stride=None, nms=0.4, merge=0.5, tol=0.01, n_frames=1, counts=None, expect=None):
    """per_tile: for every (frame, tile) in order a list of (local xyxy, score); query_index: a permutation of the slots that is not the identity."""
    T = len(tiles)
    assert len(per_tile) == n_frames * T
    stride = stride or max(1, max(len(p) for p in per_tile))
    recs = np.zeros((n_frames * T, stride), DET)
    recs["x1"], recs["y1"], recs["x2"], recs["y2"], recs["score"], recs["label"], recs["query_index"] = -1e6, -1e6, 1e6, 1e6, 2.0, 1, -7
    cnt = np.zeros(n_frames * T, np.int32)
    for i, p in enumerate(per_tile):
        n = len(p)
        assert n <= stride
        cnt[i] = n
        for k, (box, score) in enumerate(p):
            recs[i, k] = (*np.float32(box), np.float32(score), 1, (k * 7 + 3) % stride, i // T)
    if counts is not None:
        cnt[:] = counts
    return {"name": name, "tiles": np.asarray(tiles, np.int32).reshape(T, 4), "frame": frame, "recs": recs, "counts": cnt, "stride": stride,
            "n_frames": n_frames, "nms": float(nms), "merge": float(merge), "tol": float(tol), "expect": expect}


def _bodies(rng, tiles, frame, n_bodies, jitter=True):
    """Random bodies on the frame, each seen by every tile that holds at least 6 x 6 pixels of it: the visible part as that tile's record."""
    h, w = frame
    per = [[] for _ in tiles]
    for _ in range(n_bodies):
        bw, bh = rng.uniform(15, 70), rng.uniform(25, 95)
        x1, y1 = rng.uniform(-10, w - 10), rng.uniform(-10, h - 10)
        body = [max(0.0, x1), max(0.0, y1), min(float(w), x1 + bw), min(float(h), y1 + bh)]
        for t, (y0, x0, th, tw) in enumerate(tiles):
            part = [max(body[0], x0), max(body[1], y0), min(body[2], x0 + tw), min(body[3], y0 + th)]
            if part[2] - part[0] < 6 or part[3] - part[1] < 6:
                continue
            j = rng.normal(0, 0.8, 4) * (np.asarray(part) != np.asarray([x0, y0, x0 + tw, y0 + th])) if jitter else np.zeros(4)   # (a clipped side stays on the edge)
            per[t].append((_local(tiles[t], np.asarray(part) + j), np.float32(rng.choice([rng.uniform(0.05, 0.99), 0.5, 0.75]))))
    return per


def _random(name, seed, tiles, frame, n_bodies, stride=None, n_frames=1, **kw):
    rng = np.random.RandomState(seed)
    per = []
    for _ in range(n_frames):
        per += _bodies(rng, tiles, frame, n_bodies)
    if stride:
        per = [p[:stride] for p in per]
    return _case(name, tiles, frame, per, stride=stride, n_frames=n_frames, **kw)


def _full(name, seed, stride):
    """4 tiles x `stride` records: every slot of every tile in use (small boxes all over each tile, a third of them on a tile edge)."""
    rng = np.random.RandomState(seed)
    per = []
    for (y0, x0, th, tw) in GRID:
        p = []
        for k in range(stride):
            bw, bh = rng.uniform(8, 40), rng.uniform(8, 50)
            x, y = rng.uniform(0, tw - bw), rng.uniform(0, th - bh)
            box = [x, y, x + bw, y + bh]
            if k % 3 == 0:
                side = rng.randint(4)
                box[side] = [0.0, 0.0, float(tw), float(th)][side]
            p.append((box, np.float32(rng.uniform(0.05, 0.99))))
        per.append(p)
    return _case(name, GRID, FRAME, per, stride=stride)


def cases():
    """Every case of the generator, in a fixed order with unique names (`case["mixed"]`: its tiles differ in size)."""
    T0, T1, T2, T3 = GRID
    out = []
    out.append(_case("no_records", GRID, FRAME, [[], [], [], []], stride=100, expect=[0]))
    out.append(_case("one_tile_only", GRID, FRAME, [[], [], [([20, 20, 60, 90], 0.9), ([22, 24, 61, 88], 0.8), ([90, 10, 130, 70], 0.7), ([5, 60, 30, 100], 0.85)], []],
                     stride=100, expect=[3]))
    # a body over the vertical seam: frame x 120 .. 200, seen as 120 .. 169 by tile 0 and 131 .. 200 by tile 1 -> ONE union
    out.append(_case("vertical_seam", GRID, FRAME, [[(_local(T0, [120, 20, 169, 90]), 0.9)], [(_local(T1, [131, 20, 200, 90]), 0.8)], [], []], expect=[1]))
    out.append(_case("horizontal_seam", GRID, FRAME, [[(_local(T0, [30, 80, 80, 112]), 0.6)], [], [(_local(T2, [30, 88, 80, 150]), 0.95)], []], expect=[1]))
    # a body at the corner where the four tiles meet
    out.append(_case("corner_four_tiles", GRID, FRAME, [[(_local(T0, [120, 70, 169, 112]), 0.9)], [(_local(T1, [131, 70, 180, 112]), 0.8)],
                                                        [(_local(T2, [120, 88, 169, 130]), 0.7)], [(_local(T3, [131, 88, 180, 130]), 0.6)]], expect=[1]))
    # growth chain: A (tile 0, cut) absorbs part B (tile 1) and grows to x 100 .. 220; C (tile 1, x 180 .. 250) does not touch the original A
    A, B, Cc = (_local(T0, [100, 20, 169, 90]), 0.9), (_local(T1, [131, 20, 220, 90]), 0.8), (_local(T1, [180, 20, 250, 90]), 0.7)
    out.append(_case("growth_chain", GRID, FRAME, [[A], [B, Cc], [], []], expect=[1]))
    out.append(_case("growth_chain_without_b", GRID, FRAME, [[A], [Cc], [], []], expect=[2]))
    # fails the merge test (same tile) but passes the IoU test -> dropped; and the reverse (parts of one body, IoU 0.2375) -> merged
    out.append(_case("iou_only", GRID, FRAME, [[(_local(T0, [100, 20, 169, 90]), 0.9), (_local(T0, [104, 22, 169, 88]), 0.8)], [], [], []], expect=[1]))
    out.append(_case("merge_only", GRID, FRAME, [[(_local(T0, [100, 20, 169, 90]), 0.9)], [(_local(T1, [131, 20, 260, 90]), 0.8)], [], []], expect=[1]))
    # two UNCUT boxes of different tiles inside the overlap band: iomin = 1, no merge; IoU alone decides (0.6: dropped; 0.3: both stay)
    out.append(_case("uncut_pair_iou_high", GRID, FRAME, [[(_local(T0, [135, 30, 165, 80]), 0.9)], [(_local(T1, [135, 30, 165, 60]), 0.8)], [], []], expect=[1]))
    out.append(_case("uncut_pair_iou_low", GRID, FRAME, [[(_local(T0, [135, 30, 165, 80]), 0.9)], [(_local(T1, [135, 30, 165, 45]), 0.8)], [], []], expect=[2]))
    # iomin exactly 0.5 (38 x 70 of 76 x 70): `>` keeps the two apart at 0.5 (IoU 1/3), merges one ulp below
    half = [[(_local(T0, [93, 20, 169, 90]), 0.9)], [(_local(T1, [131, 20, 207, 90]), 0.8)], [], []]
    out.append(_case("iomin_at_threshold", GRID, FRAME, half, merge=0.5, expect=[2]))
    out.append(_case("iomin_ulp_above_threshold", GRID, FRAME, half, merge=np.nextafter(0.5, 0.0), expect=[1]))
    # IoU exactly 0.5
    edge = [[([0, 0, 20, 20], 0.9), ([0, 0, 20, 10], 0.8)], [], [], []]
    out.append(_case("iou_at_threshold", GRID, FRAME, edge, nms=0.5, expect=[2]))
    out.append(_case("iou_ulp_above_threshold", GRID, FRAME, edge, nms=np.nextafter(0.5, 0.0), expect=[1]))
    # a side exactly at tx = 2^-7 x 256 = 2 (cut: `<=`) and one float32 step beyond (not cut: IoU 70/150 then drops B instead of merging it)
    two = [(0, 0, 100, 256), (0, 128, 100, 256)]
    up = float(np.nextafter(np.float32(2), np.float32(3)))
    for tag, x, n in (("at", 2.0, 1), ("beyond", up, 1)):
        out.append(_case(f"left_side_{tag}_tx", two, (100, 384), [[([100, 10, 200, 80], 0.9)], [([x, 10, 122, 80], 0.8)]], tol=2.0 ** -7, expect=[n]))
    dn = float(np.nextafter(np.float32(254), np.float32(0)))
    for tag, x in (("at", 254.0), ("beyond", dn)):
        out.append(_case(f"right_side_{tag}_tw_minus_tx", two, (100, 384), [[([150, 10, x, 80], 0.8)], [([60, 10, 160, 80], 0.9)]], tol=2.0 ** -7, expect=[1]))
    # equal scores across tiles: ties keep (tile, record) order, and the first of a tie opens the slot
    tie = [[(_local(T0, [120, 20, 169, 90]), 0.5), ([10, 10, 40, 60], 0.5)], [(_local(T1, [131, 20, 200, 90]), 0.5), (_local(T1, [240, 10, 280, 60]), 0.5)],
           [([12, 0, 41, 30], 0.5)], [(_local(T3, [240, 100, 280, 170]), 0.5)]]
    out.append(_case("equal_scores", GRID, FRAME, tie))
    out.append(_case("equal_scores_reversed_tiles", GRID, FRAME, [tie[1], tie[0], tie[3], tie[2]]))
    # merge_nms_threshold >= 1: nothing is absorbed, not even the parts of one body
    for thr in (1.0, 2.0):
        out.append(_case(f"nms_{thr}", GRID, FRAME, [[(_local(T0, [120, 20, 169, 90]), 0.9)], [(_local(T1, [131, 20, 200, 90]), 0.8)], [], []], nms=thr, expect=[2]))
        out.append(_random(f"random_nms_{thr}", 71, GRID, FRAME, 25, nms=thr))
    out.append(_random("thresholds_zero", 72, GRID, FRAME, 25, nms=0.0, merge=0.0, tol=0.0))
    out.append(_random("tolerance_large", 73, GRID, FRAME, 25, tol=0.2))
    # degenerate boxes: zero width, x2 < x1, zero area on a seam
    deg = [[([160, 20, 160, 90], 0.9), ([100, 20, 90, 60], 0.8), ([120, 20, 169, 90], 0.7), ([169, 0, 169, 112], 0.65)],
           [([0, 20, 0, 90], 0.85), ([0, 20, 69, 90], 0.6), ([30, 50, 10, 40], 0.5)], [([0, 0, 0, 0], 0.4)], [([5, 5, 5, 5], 0.3), ([0, 0, 169, 112], 0.2)]]
    out.append(_case("degenerate", GRID, FRAME, deg))
    out.append(_case("degenerate_thr0", GRID, FRAME, deg, nms=0.0, merge=0.0))
    # full load
    out.append(_full("full_load_s100", 81, 100))
    out.append(_full("full_load_s128", 82, 128))
    # other grids
    out.append(_random("grid_1x2", 91, tile_grid(120, 300, 1, 2, 0.125), (120, 300), 20))
    out.append(_random("grid_2x1", 92, tile_grid(240, 150, 2, 1, 0.125), (240, 150), 20))
    out.append(_random("grid_1x1", 93, tile_grid(100, 100, 1, 1, 0.0), (100, 100), 12))
    out.append(_random("grid_3x3_mixed_sizes", 94, tile_grid(203, 299, 3, 3, 0.125), (203, 299), 40))
    # several frames in one call, a negative tile count (taken as zero)
    out.append(_random("three_frames", 95, GRID, FRAME, 18, stride=100, n_frames=3))
    neg = _random("negative_count", 96, GRID, FRAME, 18, stride=100, n_frames=2)
    neg["counts"][1] = -1
    neg["counts"][6] = -5
    out.append(neg)
    for seed in RANDOM_SEEDS:
        out.append(_random(f"random_{seed}", seed, GRID, FRAME, 30, stride=100))
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names)
    for c in out:
        c["mixed"] = len({(int(t[2]), int(t[3])) for t in c["tiles"]}) > 1
    assert any(c["mixed"] for c in out)
    return out


def expected(case):
    """The Python rule on the case: per frame a list of (x, y, w, h, score, label, query_index, tile).  The tile travels in class_name."""
    T, S = len(case["tiles"]), case["stride"]
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
                dets.append(Detection(bbox=bbox, confidence=float(r["score"]), class_id=int(r["label"]), class_name=str(t),
                                      camera_coords=(bbox[0] + bbox[2] / 2, bbox[1] + bbox[3]), query_index=int(r["query_index"])))
            per_tile.append(dets)
        merged = merge_tile_detections(per_tile, origins, case["nms"], sizes, case["frame"], case["merge"], case["tol"])
        out.append([(*d.bbox, d.confidence, d.class_id, d.query_index, int(d.class_name)) for d in merged])
    return out


def params(case):
    return _capi.OpdTileParams(struct_size=C.sizeof(_capi.OpdTileParams), person_label=1, tile_nms_threshold=0.4, merge_nms_threshold=case["nms"],
                               merge_threshold=case["merge"], edge_tolerance=case["tol"])


def run(fn, case, handle=None):
    """A routine with opd_detr_merge_tiles's arguments (`handle`: the model handle in front, None: the host hook) on the case: (rc, out, counts)."""
    T, S, F = len(case["tiles"]), case["stride"], case["n_frames"]
    recs, cnt, tiles = case["recs"].copy(), case["counts"].copy(), np.ascontiguousarray(case["tiles"])
    out, counts = np.zeros((F, T * S), TILE_DET), np.full(F, -99, np.int32)
    out["query_index"] = -9
    p = params(case)
    args = [C.c_void_p(recs.ctypes.data), C.c_void_p(cnt.ctypes.data), F, T, S, C.c_void_p(tiles.ctypes.data), case["frame"][0], case["frame"][1], C.byref(p),
            out.ctypes.data_as(C.POINTER(_capi.OpdTileDet)), counts.ctypes.data_as(C.POINTER(C.c_int32))]
    rc = fn(*args) if handle is None else fn(C.c_void_p(handle), *args)
    assert np.array_equal(recs, case["recs"]) and np.array_equal(cnt, case["counts"]), f"{case['name']}: the inputs were written"
    return rc, out, counts


def assert_same(case, out, counts, want):
    name = case["name"]
    assert counts.tolist() == [len(w) for w in want], f"{name}: counts {counts.tolist()} != {[len(w) for w in want]}"
    for f, w in enumerate(want):
        got = [(float(r["x"]), float(r["y"]), float(r["w"]), float(r["h"]), float(r["score"]), int(r["label"]), int(r["query_index"]), int(r["tile"])) for r in out[f, :len(w)]]
        for k, (a, b) in enumerate(zip(got, w)):
            assert a == b, f"{name}: frame {f}, record {k} of {len(w)}: {a} != {b}"
    if case["expect"] is not None:
        assert counts.tolist() == case["expect"], f"{name}: kept {counts.tolist()}, the case was built for {case['expect']}"
    for f in range(len(want)):
        assert (out[f, :counts[f]]["query_index"] >= 0).all(), f"{name}: a decoy slot was read"
