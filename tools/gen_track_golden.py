"""Write tests/golden/track_sequences.npz: seeded detection sequences, the ids the reference's own ``Tracker`` gave them frame by frame,
and its final per-track counters and Kalman states.  Only data is recorded.

    python tools/gen_track_golden.py --reference DIR        (a checkout of the reference project; also $OPD_REFERENCE_ROOT)

The reference's ``cv2`` import is satisfied by an empty placeholder module: ``Tracker`` reaches no cv2 function.

Conditions, checked here and not loosened.  A drawn sequence is DROPPED when the reference's ids differ from those of the float64
restatement (tests/track_common.py), or when a thresholded quantity comes too close to its threshold on any frame: an appearance cost within
1e-3 of 0.3, a combined cost within 1e-3 of 0.5, an IoU distance within 1e-3 of 0.5 or 0.6, a gate distance within 0.5 px of
max_position_distance, a confidence within 1e-3 of the high-confidence threshold.  (The quantities are read from the float64 restatement
of the same run, whose ids are the reference's.)  At most 10 % of the drawn sequences may be dropped and every scenario class must keep
one; otherwise the tool fails and the seeds, not the caps, are changed.

``kalman_tol``: the largest difference, over every frame of the kept sequences, between the reference's float32 Kalman states and the
float64 restatement: x relative to max(1, |x|), P relative to max |P|.  The tests assert 8 x that value (profiles/NOTES.md)."""

import argparse
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import track_common as TC  # noqa: E402

F32 = np.float32
MARGIN_COST, MARGIN_GATE, MARGIN_CONF = 1e-3, 0.5, 1e-3
CLASSES = ("steady", "occlusion", "lowconf", "nofeat", "mixed", "maxage", "gate", "ring", "empty")
# (class, D, walkers, frames, seeds)
PLAN = [("steady", 37, 10, 30, (1, 2)), ("steady", 256, 3, 10, (3,)), ("steady", 512, 3, 8, (4, 5)),
        ("occlusion", 37, 4, 24, (6, 7)), ("occlusion", 256, 3, 14, (8,)),
        ("lowconf", 37, 4, 20, (9, 10)), ("lowconf", 512, 2, 10, (11,)),
        ("nofeat", 37, 6, 20, (12, 13)),
        ("mixed", 37, 5, 20, (14,)), ("mixed", 256, 3, 12, (15, 16)),
        ("maxage", 37, 6, 30, (17, 18, 19)),
        ("gate", 37, 3, 10, (20, 21)), ("gate", 256, 2, 8, (22,)),
        ("ring", 37, 3, 16, (23,)), ("ring", 256, 2, 14, (24, 25)),
        ("empty", 37, 4, 16, (26, 27)), ("empty", 512, 2, 8, (28,))]


def unit(v):
    return (v / np.linalg.norm(v)).astype(F32)


def draw(kind, D, K, n_frames, seed):
    """One sequence: params and per frame [(box xywh, conf, feature or None)] -- quarter-pixel boxes, so foot points are exact in float32."""
    rng = np.random.default_rng(1000 + seed)
    params = {}
    if kind == "maxage":
        params["max_age"] = 3
    # walkers: start points on a coarse grid (at least 260 px apart), slow velocities, a base feature each
    cells = rng.permutation(16)[:K]
    pos = np.stack([150 + 300.0 * (cells % 4), 200 + 260.0 * (cells // 4)], 1) + rng.uniform(-20, 20, (K, 2))
    vel = rng.uniform(-4, 4, (K, 2))
    size = np.stack([rng.uniform(48, 80, K), rng.uniform(110, 190, K)], 1)
    base = [unit(rng.standard_normal(D)) for _ in range(K)]
    use_feats = kind != "nofeat"
    first = np.zeros(K, int)   # the frame a walker enters, and the frames it is hidden
    hidden = [set() for _ in range(K)]
    lowconf = [set() for _ in range(K)]
    if kind == "occlusion":
        hidden[0] = set(range(5, 5 + int(rng.integers(3, 6))))
        hidden[1] = set(range(10, 13)) if K > 1 else set()
    if kind == "lowconf":
        lowconf[0] = set(range(5, 8))
        lowconf[1] = {9, 10}
    if kind == "maxage":
        for k in range(K):
            first[k] = 0 if k < 3 else int(rng.integers(6, 18))
        hidden[0] = set(range(4, n_frames))          # leaves for good: dies after three frames, its slot is used again
        hidden[1] = set(range(8, 10))                # two frames: survives
        hidden[2] = set(range(12, n_frames))
    if kind == "empty":
        first[:] = 1
        for k in range(K):
            hidden[k] = {5, 6, 11}                   # frames 0, 5, 6 and 11 have no detections at all
    frames = []
    for f in range(n_frames):
        dets = []
        for k in range(K):
            p = pos[k] + vel[k] * f
            if f < first[k] or f in hidden[k]:
                continue
            w, h = size[k] + rng.uniform(-2, 2, 2)
            box = np.round(np.array([p[0] - w / 2, p[1] - h, w, h]) * 2) / 2
            conf = rng.uniform(0.2, 0.4) if f in lowconf[k] else rng.uniform(0.6, 0.95)
            feat = unit(base[k] + rng.standard_normal(D) * (0.25 / np.sqrt(D))) if use_feats else None
            if kind == "mixed" and rng.random() < 0.4:
                feat = None
            dets.append((box.astype(F32), F32(conf), feat))
        if kind == "lowconf" and f in (6, 12):       # a low-confidence detection near nobody: it gets no id and starts no track
            dets.append((np.array([1300.0, 40.0, 50.0, 120.0], F32), F32(rng.uniform(0.2, 0.4)), unit(rng.standard_normal(D))))
        if kind == "gate" and f == 1:
            # walker 0 (tentative: one hit) is missing; a detection 500 px away carries the very feature it was created with
            dets = [d for i, d in enumerate(dets) if i != 0]
            b0 = frames[0][0][0]
            dets.append((np.array([b0[0] + 500.0, b0[1] + 8.0, b0[2], b0[3]], F32), F32(0.9), frames[0][0][2].copy()))
        frames.append(dets)
    return params, use_feats, frames


def arrays(frames, D):
    out = []
    for dets in frames:
        n = len(dets)
        boxes = np.array([d[0] for d in dets], F32).reshape(n, 4)
        foot = np.stack([boxes[:, 0] + boxes[:, 2] / F32(2), boxes[:, 1] + boxes[:, 3]], 1).astype(F32).reshape(n, 2)
        conf = np.array([d[1] for d in dets], F32)
        has = np.array([d[2] is not None for d in dets], bool)
        feats = np.array([d[2] if d[2] is not None else np.zeros(D, F32) for d in dets], F32).reshape(n, D)
        out.append((boxes, foot, conf, feats, has))
    return out


def load_reference(ref_root):
    if "cv2" not in sys.modules:
        sys.modules["cv2"] = types.ModuleType("cv2")
    sys.path.insert(0, ref_root)
    from src.models.data_models import Detection
    from src.tracking.tracker import Tracker
    return Tracker, Detection


def run_one(Tracker, Detection, params, use_feats, D, frames):
    """Reference and float64 restatement side by side.  Returns (ok, reason, ids per frame, counters, x, P, kalman error)."""
    ref = Tracker(**params)
    r64 = TC.Restatement(D, np.float64, **params)
    md, hc = r64.p["max_position_distance"], r64.p["high_conf_threshold"]
    all_ids, err = [], 0.0
    for boxes, foot, conf, feats, has in frames:
        dets = [Detection(bbox=tuple(float(v) for v in boxes[j]), confidence=float(conf[j]), class_id=1, class_name="person",
                          camera_coords=(float(foot[j, 0]), float(foot[j, 1])), features=feats[j].copy() if use_feats and has[j] else None)
                for j in range(len(conf))]
        ref.update(dets)
        ids_ref = [d.track_id if d.track_id is not None else -1 for d in dets]
        ids64 = r64.update(boxes, foot, conf, feats if use_feats else None, has if use_feats else None)
        if ids_ref != ids64:
            return False, "ids differ from the float64 restatement", None, None, None, None, None
        m = r64.last
        if m["app"].size:
            near = min(np.abs(m["app"] - 0.3).min(), np.abs(m["comb"] - 0.5).min(), np.abs(m["iou"] - 0.5).min(), np.abs(m["iou"] - 0.6).min())
            if near < MARGIN_COST:
                return False, f"a cost {near:.2e} from its threshold", None, None, None, None, None
        if len(conf) and np.abs(conf.astype(np.float64) - hc).min() < MARGIN_CONF:
            return False, "a confidence at the threshold", None, None, None, None, None
        if m["gate_dist"].size and md > 0 and np.abs(m["gate_dist"] - md).min() < MARGIN_GATE:
            return False, "a gate distance at the threshold", None, None, None, None, None
        assert [t.track_id for t in ref.tracks] == [t["id"] for t in r64.tracks]
        if ref.tracks:
            xr = np.array([t.kalman_filter.x for t in ref.tracks])
            Pr = np.array([t.kalman_filter.P for t in ref.tracks])
            assert xr.dtype == np.float32 and Pr.dtype == np.float32
            x64, P64 = r64.states()
            err = max(err, TC.state_error(xr, Pr, x64, P64))
        all_ids.append(np.array(ids_ref, np.int32))
    counters = np.array([[t.track_id, t.age, t.hits, t.time_since_update] for t in ref.tracks], np.int32).reshape(-1, 4)
    assert np.array_equal(counters, r64.counters())
    x = np.array([t.kalman_filter.x for t in ref.tracks], F32).reshape(-1, 4)
    P = np.array([t.kalman_filter.P for t in ref.tracks], F32).reshape(-1, 4, 4)
    return True, "", all_ids, counters, x, P, err


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("OPD_REFERENCE_ROOT"))
    ap.add_argument("--out", default=TC.GOLDEN)
    args = ap.parse_args()
    if not args.reference:
        sys.exit("the recorded ids are the reference's own: pass --reference DIR")
    Tracker, Detection = load_reference(args.reference)
    out, names, kept_classes, drawn, dropped, tol = {}, [], set(), 0, 0, 0.0
    for kind, D, K, n_frames, seeds in PLAN:
        for seed in seeds:
            drawn += 1
            name = f"{kind}_d{D}_s{seed}"
            params, use_feats, frames = draw(kind, D, K, n_frames, seed)
            fr = arrays(frames, D)
            ok, why, ids, counters, x, P, err = run_one(Tracker, Detection, params, use_feats, D, fr)
            if not ok:
                dropped += 1
                print(f"{name}: DROPPED ({why})")
                continue
            full = dict(TC.DEFAULTS, **params)
            counts = np.array([len(f[2]) for f in fr], np.int32)
            assert counts.max() <= 16 and len(fr) <= 40 and len(counters) <= 12
            out.update({f"{name}_D": np.int32(D), f"{name}_param_names": np.array(list(full)), f"{name}_params": np.array(list(full.values()), np.float64),
                        f"{name}_use_feats": np.bool_(use_feats), f"{name}_counts": counts, f"{name}_boxes": np.concatenate([f[0] for f in fr]),
                        f"{name}_foot": np.concatenate([f[1] for f in fr]), f"{name}_conf": np.concatenate([f[2] for f in fr]),
                        f"{name}_has": np.concatenate([f[4] for f in fr]), f"{name}_ids": np.concatenate(ids), f"{name}_counters": counters,
                        f"{name}_x": x, f"{name}_P": P})
            if use_feats:
                out[f"{name}_feats"] = np.concatenate([f[3] for f in fr])
            names.append(name)
            kept_classes.add(kind)
            tol = max(tol, err)
            print(f"{name}: {len(fr)} frames, {int(counts.sum())} detections, ids up to {int(np.concatenate(ids).max())}, {len(counters)} tracks at the end, "
                  f"reference vs float64 {err:.3e}")
    print(f"dropped {dropped} of {drawn} drawn sequences; kalman_tol = {tol:.6e} (asserted bound: 8 x = {8 * tol:.3e})")
    assert dropped <= 0.1 * drawn, "more than 10 % of the drawn sequences were dropped: draw other seeds"
    assert kept_classes == set(CLASSES), f"no sequence left of: {sorted(set(CLASSES) - kept_classes)}"
    out["names"] = np.array(names)
    out["kalman_tol"] = np.float64(tol)
    np.savez_compressed(args.out, **out)
    size = os.path.getsize(args.out)
    print(f"wrote {args.out}: {len(names)} sequences, {size} bytes")
    assert size < (1 << 20)


if __name__ == "__main__":
    main()
