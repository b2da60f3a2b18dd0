"""Shared by tests/test_nms_cpu.py and tests/test_nms_gpu.py: ONE generator of record sets for the person filter + greedy IoU-NMS
(opd_person_nms on the host, person_nms_kernel on the device), and the helpers that run a case through a routine and compare bytes.

A case is a few frames of fixed-slot records, ``dets`` ``[n_frames, stride]`` of ``DET`` (the 32-byte ``opd_det``) and ``counts``
``[n_frames]``, with a person label and a threshold.  Slots at and beyond a frame's count hold decoy records (high scores, the person
label, boxes over everything): a routine that reads them shows.  Every comparison is bytewise over the first ``counts[f]`` records of
each frame, and of the counts."""

import ctypes as C
import hashlib

import numpy as np

from office_person_detection_vit_amd import _capi

DET = np.dtype([("x1", "<f4"), ("y1", "<f4"), ("x2", "<f4"), ("y2", "<f4"), ("score", "<f4"), ("label", "<i4"), ("query_index", "<i4"),
                ("frame", "<i4")])
assert DET.itemsize == C.sizeof(_capi.OpdDet) == 32

SIZES = (0, 1, 2, 63, 64, 65, 100, 127, 128)
STRIDES = (100, 128)
THRESHOLDS = (0.0, 0.4, 1.0, 2.0)
RANDOM_SEEDS = (11, 12, 13)


def _frame(boxes, scores, labels=None, stride=None, frame=0):
    """One frame's slots: the given records first (query_index = a permutation that is not the identity), decoys behind."""
    boxes = np.asarray(boxes, np.float32).reshape(-1, 4)
    n = len(boxes)
    stride = stride or max(n, 1)
    assert n <= stride
    out = np.zeros(stride, DET)
    out["x1"][:n], out["y1"][:n], out["x2"][:n], out["y2"][:n] = boxes.T
    out["score"][:n] = np.asarray(scores, np.float32)
    out["label"][:n] = 1 if labels is None else np.asarray(labels, np.int32)
    out["query_index"][:n] = (np.arange(n) * 7 + 3) % max(n, 1) if n % 7 else np.arange(n)[::-1]
    out["frame"] = frame
    out["x1"][n:], out["y1"][n:], out["x2"][n:], out["y2"][n:] = -1e6, -1e6, 1e6, 1e6   # decoys
    out["score"][n:] = 2.0
    out["label"][n:] = 1
    out["query_index"][n:] = -7
    return out, n


def _case(name, frames, label=1, thr=0.4, expect_counts=None):
    """frames: list of (slots, n) from _frame, or None for the padding slot of an uneven shard (count -1)."""
    stride = max(len(f[0]) for f in frames if f is not None)
    dets = np.zeros((len(frames), stride), DET)
    counts = np.zeros(len(frames), np.int32)
    for i, f in enumerate(frames):
        if f is None:
            dets[i] = _frame(np.zeros((0, 4)), [], stride=stride, frame=i)[0]
            counts[i] = -1
        else:
            assert len(f[0]) == stride
            dets[i], counts[i] = f
    return {"name": name, "dets": dets, "counts": counts, "stride": stride, "label": int(label), "thr": np.float32(thr),
            "expect_counts": expect_counts}


def _cluster_boxes(rng, n, centres=6, spread=30.0, jitter=6.0, size=(40.0, 90.0)):
    """n float boxes around a few centres on a 640 x 480 canvas: within a centre most pairs overlap above 0.4, across centres few do."""
    c = rng.uniform([40, 40], [600, 440], size=(centres, 2))
    k = rng.randint(0, centres, size=n)
    xy = c[k] + rng.normal(0.0, jitter, size=(n, 2)) + rng.uniform(-spread, spread, size=(n, 2)) * (rng.rand(n, 1) < 0.3)
    wh = np.asarray(size) * rng.uniform(0.8, 1.25, size=(n, 2))
    return np.concatenate([xy - wh / 2, xy + wh / 2], axis=1).astype(np.float32)


def _random_frame(seed, n, stride, frame=0, labels=False):
    rng = np.random.RandomState(seed)
    boxes = _cluster_boxes(rng, n)
    scores = rng.uniform(0.05, 0.999, size=n).astype(np.float32)
    lab = rng.choice([1, 1, 1, 3, 17], size=n) if labels else None
    return _frame(boxes, scores, lab, stride, frame)


def cases():
    """Every case of the generator, in a fixed order with unique names (the data depends on nothing but this file)."""
    out = []
    # sizes: one frame of n clustered records, both strides
    for stride in STRIDES:
        for n in SIZES:
            if n <= stride:
                out.append(_case(f"size_n{n}_s{stride}", [_random_frame(1000 + n, n, stride)]))
    # batches: 1 and 3 frames with different counts, one of them the padding slot
    out.append(_case("batch1_s100", [_random_frame(21, 37, 100)]))
    out.append(_case("batch3_s100", [_random_frame(22, 37, 100, 0), None, _random_frame(23, 100, 100, 2)]))
    out.append(_case("batch3_s128", [_random_frame(24, 128, 128, 0), _random_frame(25, 0, 128, 1), _random_frame(26, 65, 128, 2)]))
    # ties: all scores equal / runs of equal scores, boxes shuffled: the order must be record order
    rng = np.random.RandomState(31)
    far = np.stack([np.arange(50) * 100.0, np.zeros(50), np.arange(50) * 100.0 + 50, np.full(50, 50.0)], 1)[rng.permutation(50)]
    out.append(_case("ties_all_equal_far", [_frame(far, np.full(50, 0.5))], expect_counts=[50]))
    out.append(_case("ties_all_equal_cluster", [_frame(_cluster_boxes(rng, 128), np.full(128, 0.25), stride=128)]))
    runs = np.repeat(np.float32([0.9, 0.3, 0.7, 0.3, 0.9, 0.5, 0.7, 0.1]), 16)
    out.append(_case("ties_runs", [_frame(_cluster_boxes(rng, 128, centres=20), runs, stride=128)]))
    out.append(_case("ties_signed_zero_scores", [_frame(far[:8], np.float32([0.0, -0.0, 0.0, -0.0, 0.5, -0.0, 0.5, 0.0]))], expect_counts=[8]))
    # chain: A suppresses B, B alone would suppress C, A does not touch C -> A and C (records in the order C, A, B)
    A, B_, C_ = [0, 0, 10, 10], [4, 0, 14, 10], [8, 0, 18, 10]   # IoU(A, B) = IoU(B, C) = 60 / 140, IoU(A, C) = 20 / 180
    out.append(_case("chain", [_frame([C_, A, B_], [0.7, 0.9, 0.8])], expect_counts=[2]))
    out.append(_case("chain_long", [_frame([[4 * i, 0, 4 * i + 10, 10] for i in range(100)], 0.99 - 0.005 * np.arange(100), stride=100)], expect_counts=[50]))
    # threshold edge: IoU([0,0,2,2], [0,0,2,1]) = 2 / 4 = 0.5 exactly; the test is `>`
    edge = [[0, 0, 2, 2], [0, 0, 2, 1]]
    out.append(_case("edge_at_threshold", [_frame(edge, [0.9, 0.8])], thr=0.5, expect_counts=[2]))
    out.append(_case("edge_below_threshold", [_frame(edge, [0.9, 0.8])], thr=np.nextafter(np.float32(0.5), np.float32(0)), expect_counts=[1]))
    grid = [[x, y, x + w, y + h] for x in range(0, 4) for y in range(0, 3) for w in (1, 2, 4) for h in (2, 3)]
    out.append(_case("edge_grid_quarter", [_frame(grid, 0.9 - 0.01 * np.arange(len(grid)), stride=100)], thr=0.25))
    out.append(_case("edge_grid_half", [_frame(grid, 0.9 - 0.01 * np.arange(len(grid)), stride=100)], thr=0.5))
    # degenerate boxes: x2 < x1, zero area, identical boxes, far apart
    deg = [[10, 10, 5, 20], [10, 10, 5, 20], [3, 3, 3, 9], [3, 3, 3, 9], [0, 0, 8, 8], [0, 0, 8, 8], [0, 0, 8, 8], [5, 5, 2, 2], [0, 0, 0, 0], [1, 1, 7, 7]]
    out.append(_case("degenerate", [_frame(deg, [0.5, 0.6, 0.7, 0.2, 0.9, 0.8, 0.95, 0.4, 0.3, 0.1])]))
    out.append(_case("degenerate_thr0", [_frame(deg, [0.5, 0.6, 0.7, 0.2, 0.9, 0.8, 0.95, 0.4, 0.3, 0.1])], thr=0.0))
    out.append(_case("identical_boxes", [_frame([[2, 3, 50, 80]] * 64, np.linspace(0.1, 0.9, 64))], expect_counts=[1]))
    out.append(_case("identical_boxes_thr1", [_frame([[2, 3, 50, 80]] * 64, np.linspace(0.1, 0.9, 64))], thr=1.0, expect_counts=[64]))
    out.append(_case("far_apart", [_frame(far, rng.uniform(0.1, 0.9, 50))], expect_counts=[50]))
    # dense cluster: 128 jittered copies of one box, 1 of 128 survives
    dense = np.float32([100, 100, 300, 500]) + rng.uniform(-3, 3, size=(128, 4)).astype(np.float32)
    out.append(_case("dense_cluster", [_frame(dense, rng.uniform(0.1, 0.99, 128), stride=128)], expect_counts=[1]))
    # labels: a mixture, with person_label 1 and -1
    for label in (1, -1):
        tag = "person" if label == 1 else "all"
        out.append(_case(f"labels_{tag}", [_random_frame(41, 100, 100, labels=True)], label=label))
        out.append(_case(f"labels_{tag}_s128", [_random_frame(42, 128, 128, labels=True), _random_frame(43, 5, 128, 1, labels=True)], label=label))
    out.append(_case("labels_none_match", [_random_frame(44, 64, 100)], label=5, expect_counts=[0]))
    # thresholds: >= 1 disables suppression
    for thr in THRESHOLDS:
        out.append(_case(f"thr_{thr}", [_random_frame(51, 100, 100, labels=True), _random_frame(53, 77, 100, 1)], thr=thr))
    # random float boxes: some pairs above the threshold, some below (assert_random_cases_mixed checks it on the host routine)
    for seed in RANDOM_SEEDS:
        out.append(_case(f"random_{seed}", [_random_frame(seed, 100, 100), _random_frame(seed + 200, 90, 100, 1)]))
        out.append(_case(f"random_{seed}_s128", [_random_frame(seed + 300, 128, 128)]))
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names)
    return out


def input_digest(case):
    h = hashlib.sha256()
    h.update(case["dets"].tobytes()); h.update(case["counts"].tobytes())
    h.update(np.int32([case["stride"], case["label"]]).tobytes()); h.update(np.float32(case["thr"]).tobytes())
    return h.hexdigest()


def run_host(fn, case):
    """A host routine with opd_person_nms_batch's signature, on a copy of the case: (rc, dets, counts)."""
    dets, counts = case["dets"].copy(), case["counts"].copy()
    rc = fn(dets.ctypes.data_as(C.POINTER(_capi.OpdDet)), counts.ctypes.data_as(C.POINTER(C.c_int32)), len(counts), case["stride"], case["label"],
            C.c_float(float(case["thr"])))
    return rc, dets, counts


def run_single(lib, case):
    """opd_person_nms frame by frame, on a copy of the case: (dets, counts)."""
    dets, counts = case["dets"].copy(), case["counts"].copy()
    for f in range(len(counts)):
        if counts[f] < 0:
            continue
        row = dets[f]
        kept = lib.opd_person_nms(row.ctypes.data_as(C.POINTER(_capi.OpdDet)), int(counts[f]), case["label"], C.c_float(float(case["thr"])))
        assert kept >= 0
        counts[f] = kept
    return dets, counts


def kept_bytes(dets, counts):
    """The bytes a comparison looks at: per frame, the first counts[f] records."""
    return [dets[f, :max(int(counts[f]), 0)].tobytes() for f in range(len(counts))]


def assert_same(name, got, want):
    (gd, gc), (wd, wc) = got, want
    assert np.array_equal(gc, wc), f"{name}: counts {gc.tolist()} != {wc.tolist()}"
    for f, (a, b) in enumerate(zip(kept_bytes(gd, gc), kept_bytes(wd, wc))):
        if a != b:
            ga, wa = np.frombuffer(a, DET), np.frombuffer(b, DET)
            bad = int(np.nonzero(ga != wa)[0][0])
            raise AssertionError(f"{name}: frame {f}, record {bad} of {len(ga)}: {ga[bad]} != {wa[bad]}")


def assert_expectations(case, dets, counts):
    """What a case states about its own result, beyond equality with another routine."""
    if case["expect_counts"] is not None:
        assert counts.tolist() == case["expect_counts"], f"{case['name']}: kept {counts.tolist()}, expected {case['expect_counts']}"
    if case["name"] == "chain":
        assert dets[0, :2]["score"].tolist() == [np.float32(0.9), np.float32(0.7)]
    if case["name"].startswith("ties_all_equal_far") or case["name"] == "ties_signed_zero_scores":
        n = int(case["counts"][0])
        want = case["dets"][0, :n]
        if case["name"] == "ties_signed_zero_scores":   # 0.5 twice in record order, then the six zeros in record order
            want = want[[4, 6, 0, 1, 2, 3, 5, 7]]
        assert dets[0, :n].tobytes() == want.tobytes(), f"{case['name']}: ties must keep record order"
    for f in range(len(counts)):
        if counts[f] > 0:
            k = dets[f, :counts[f]]
            assert (np.diff(k["score"]) <= 0).all(), f"{case['name']}: frame {f} is not in descending score order"
            assert (k["query_index"] >= 0).all(), f"{case['name']}: a decoy slot was read"
            if case["label"] >= 0:
                assert (k["label"] == case["label"]).all()


def assert_random_cases_mixed(lib, all_cases):
    """On the host routine's own output: every random case keeps some records and suppresses some, in every frame."""
    for case in all_cases:
        if case["name"].startswith("random_"):
            _, counts = run_single(lib, case)
            for f in range(len(counts)):
                assert 0 < counts[f] < case["counts"][f], f"{case['name']}: frame {f} kept {counts[f]} of {case['counts'][f]}"
