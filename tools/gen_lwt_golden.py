"""Write tests/golden/lwt_sequences.npz: seeded hybrid-tracking sequences run through the reference's own ``LightweightTracker`` (with its
real ``OpticalFlowTracker`` bookkeeping), frame by frame: the ids of every detection frame, the records of every in-between frame, the
counters after every frame, and the final Kalman states with their element types.  Only data is recorded.

    python tools/gen_lwt_golden.py --reference DIR        (a checkout of the reference project; also $OPD_REFERENCE_ROOT)

The reference's ``cv2`` import is satisfied by a small stand-in module: ``cvtColor`` returns its input and ``calcOpticalFlowPyrLK``
returns the points and status the generator scripted for that frame (the walkers' true centres plus quarter-pixel noise, a share of them
lost), so the sequences pin the track logic and not LK's numerics.  A detection frame comes every 4th frame.

Conditions, checked here and not loosened.  A drawn sequence is DROPPED when the reference's ids, counters, element types or records
differ from those of the restatement (tests/lwt_common.py) -- of a record whose point was followed every number bit for bit; of a record
that reports a Kalman-predicted centre the id, width and height (its x and y are measured, see record_tol) -- or when a maximum the
greedy matching looked at lies within 1e-3 of the threshold or is tied.  At most 10 % of the drawn sequences may be dropped and every class must keep one; otherwise the tool fails and
the seeds, not the caps, are changed.

``kalman_tol``: the largest difference, over every frame of the kept sequences, between the reference's Kalman states and the
all-float64 restatement: x relative to max(1, |x|), P relative to max |P| (track_common.state_error).  It is dominated by the float32
``P`` of tracks predicted many frames in a row.  ``record_tol``: the same for the x and y of the Kalman-PREDICTED interpolate records
(a predicted position minus half the size), relative to max(1, |value|) (lwt_common.records_error): pixel coordinates get a tolerance
measured on pixel coordinates.  The CPU test holds the restatement's states to kalman_tol itself; the device tests assert 8 x either
value (profiles/NOTES.md)."""

import argparse
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import lwt_common as LC  # noqa: E402
import track_common as TC  # noqa: E402

F32, F64 = np.float32, np.float64
MARGIN = 1e-3
N_FRAMES, PERIOD = 24, 4
# (class, walkers, seeds)
PLAN = [("flowoff", 6, (1, 2, 3)), ("lost", 8, (4, 5, 6, 7)), ("alllost", 5, (8, 9)), ("occlusion", 6, (10, 11, 12)), ("empty", 5, (13, 14)),
        ("moredets", 9, (15, 16)), ("moretracks", 9, (17, 18)), ("shuffled", 8, (19, 20, 21))]
SCRIPT = []   # what the stand-in's calcOpticalFlowPyrLK returns next: (next [n][1][2] float32, status [n][1] uint8)


def make_cv2():
    cv2 = types.ModuleType("cv2")
    cv2.COLOR_BGR2GRAY, cv2.TERM_CRITERIA_EPS, cv2.TERM_CRITERIA_COUNT = 6, 2, 1
    cv2.cvtColor = lambda frame, code: frame

    def lk(prev_gray, gray, prev_points, next_points, **kw):
        nxt, status = SCRIPT.pop(0)
        assert nxt.shape == prev_points.shape
        return nxt, status, None
    cv2.calcOpticalFlowPyrLK = lk
    return cv2


def load_reference(ref_root):
    sys.modules["cv2"] = make_cv2()
    sys.path.insert(0, ref_root)
    from src.models.data_models import Detection
    from src.tracking.lightweight_tracker import LightweightTracker
    return LightweightTracker, Detection


def quarter(v):
    return np.round(np.asarray(v, F64) * 4) / 4


def draw(kind, K, seed):
    """params and per frame the walkers visible: [(walker, box xywh float32)] on detection frames; walker centres on every frame."""
    rng = np.random.default_rng(2000 + seed)
    params = dict(max_age=30, iou_threshold=0.3, use_optical_flow=kind != "flowoff")
    if kind in ("occlusion", "flowoff"):
        params["max_age"] = 3 if kind == "occlusion" else 6
    if kind == "shuffled":
        params["iou_threshold"] = 0.4
    cells = rng.permutation(16)[:K]
    pos = np.stack([150 + 300.0 * (cells % 4), 200 + 260.0 * (cells // 4)], 1) + rng.uniform(-20, 20, (K, 2))
    vel = rng.uniform(-3, 3, (K, 2))
    size = np.stack([rng.uniform(48, 80, K), rng.uniform(110, 190, K)], 1)
    first, last = np.zeros(K, int), np.full(K, N_FRAMES)
    hidden = [set() for _ in range(K)]
    if kind == "occlusion":
        hidden[0] = set(range(4, 16))    # away over three detection frames: its track dies, a new one starts
        hidden[1] = {8}                  # one detection frame: survives when its point is followed
        last[2] = 8
    if kind == "flowoff":
        hidden[0] = {4, 8}
        last[1] = 4
    if kind == "empty":
        for k in range(K):
            hidden[k] = {0, 8, 12}
    if kind == "moredets":
        first[K // 2:] = 8               # more detections than tracks from frame 8 on
    if kind in ("moredets", "lost"):
        first[-1] = 20                   # its track is made on the last detection frame: x is still float32 at the end
    if kind == "moretracks":
        last[K // 2:] = 8                # ... and the reverse
    centres = np.stack([pos + vel * f for f in range(N_FRAMES)])
    frames = []
    for f in range(N_FRAMES):
        dets = []
        if f % PERIOD == 0:
            for k in range(K):
                if f < first[k] or f >= last[k] or f in hidden[k]:
                    continue
                w, h = quarter(size[k] + rng.uniform(-2, 2, 2))
                x, y = quarter(centres[f, k] - np.array([w, h]) / 2)
                dets.append((k, np.array([x, y, w, h], F32)))
            if kind == "shuffled":
                dets = [dets[i] for i in rng.permutation(len(dets))]
        frames.append(dets)
    lose = {"lost": 0.25, "alllost": 1.0, "flowoff": 0.0}.get(kind, 0.15)
    return params, frames, centres, lose, rng


def run_one(LightweightTracker, Detection, kind, K, seed):
    params, frames, centres, lose, rng = draw(kind, K, seed)
    ref = LightweightTracker(**params)
    r32, r64 = LC.Restatement(**params), LC.Restatement(wide=True, **params)
    frame = LC.DUMMY_FRAME
    walker_of, rec, err, rerr = {}, [], 0.0, 0.0
    for f, dets in enumerate(frames):
        fr = {}
        if f % PERIOD == 0:
            boxes = np.array([b for _, b in dets], F32).reshape(-1, 4)
            objs = [Detection(bbox=tuple(float(v) for v in b), confidence=0.9, class_id=1, class_name="person", camera_coords=(0.0, 0.0)) for b in boxes]
            ref.update_with_detections(frame, objs)
            ids = [d.track_id for d in objs]
            if ids != r32.update(boxes) or ids != r64.update(boxes):
                return None, "ids differ from the restatement", 0.0, 0.0
            for (k, _), i in zip(dets, ids):
                walker_of[i] = k
            fr.update(kind=1, boxes=boxes, ids=np.array(ids, np.int32))
        else:
            nxt, status = np.zeros((0, 2), F32), np.zeros(0, np.uint8)
            of = ref.of_tracker
            if of is not None and of.prev_points is not None and len(of.prev_points):
                n = len(of.prev_track_ids)
                assert of.prev_track_ids == r32.pt_ids and np.array_equal(of.prev_points.reshape(-1, 2), r32.pts)
                nxt = np.array([quarter(centres[f, walker_of[i]] + rng.uniform(-0.75, 0.75, 2)) for i in of.prev_track_ids], F32).reshape(n, 2)
                status = (rng.random(n) >= lose).astype(np.uint8)
                SCRIPT.append((nxt.reshape(n, 1, 2).copy(), status.reshape(n, 1).copy()))
            out = ref.interpolate(frame)
            assert not SCRIPT
            good = {i for i, st in zip(r32.pt_ids, status) if st == 1}
            got, wide = r32.interpolate(nxt, status), r64.interpolate(nxt, status)
            rec_ids = np.array([o[0] for o in out], np.int32)
            rec_boxes = np.array([o[1] for o in out], F64).reshape(-1, 4)
            followed = np.array([i in good for i in rec_ids], bool)
            # a followed point's box, every id, width and height: bit for bit.  The x and y of a PREDICTED box are a Kalman position minus
            # half the size: they get a tolerance of their own, record_tol
            if not LC.records_equal(got, rec_ids, rec_boxes, followed, np.inf) or not LC.records_equal(wide, rec_ids, rec_boxes, followed, np.inf):
                return None, "interpolate records differ from the restatement", 0.0, 0.0
            rerr = max(rerr, LC.records_error(wide, rec_boxes))
            fr.update(kind=0, next=nxt, status=status, rec_ids=rec_ids, rec_boxes=rec_boxes, rec_followed=followed)
        counters = np.array([[t.track_id, t.age, t.hits, t.time_since_update] for t in ref.tracks], np.int32).reshape(-1, 4)
        is32 = np.array([t.kalman.x.dtype == F32 for t in ref.tracks], bool)
        if not np.array_equal(counters, r32.counters()) or ref.next_id != r32.next_id or not np.array_equal(is32, r32.states()[2]):
            return None, "counters or element types differ from the restatement", 0.0, 0.0
        assert all(t.kalman.P.dtype == F32 for t in ref.tracks)
        if ref.tracks:
            xr = np.array([t.kalman.x.astype(F64) for t in ref.tracks])
            Pr = np.array([t.kalman.P for t in ref.tracks])
            x64, P64 = r64.states()[:2]
            err = max(err, TC.state_error(xr, Pr, x64, P64))
        fr.update(counters=counters, next_id=ref.next_id)
        rec.append(fr)
    if r32.margin < MARGIN or r64.margin < MARGIN:
        return None, f"a greedy maximum {min(r32.margin, r64.margin):.2e} from the threshold", 0.0, 0.0
    if r32.tied:
        return None, "a tied greedy maximum", 0.0, 0.0
    final = dict(x=np.array([t.kalman.x.astype(F64) for t in ref.tracks], F64).reshape(-1, 4), P=np.array([t.kalman.P for t in ref.tracks], F32).reshape(-1, 4, 4),
                 is32=np.array([t.kalman.x.dtype == F32 for t in ref.tracks], bool), bbox=np.array([t.bbox for t in ref.tracks], F64).reshape(-1, 4))
    return (params, rec, final), "", err, rerr


def pack(name, params, rec, final):
    cat = lambda key, empty, frames: np.concatenate([fr[key] for fr in frames] or [empty])   # noqa: E731
    det, itp = [fr for fr in rec if fr["kind"]], [fr for fr in rec if not fr["kind"]]
    out = {f"{name}_max_age": np.int32(params["max_age"]), f"{name}_iou_threshold": F64(params["iou_threshold"]), f"{name}_use_flow": np.bool_(params["use_optical_flow"]),
           f"{name}_kinds": np.array([fr["kind"] for fr in rec], np.uint8),
           f"{name}_n_dets": np.array([len(fr["ids"]) if fr["kind"] else 0 for fr in rec], np.int32),
           f"{name}_n_points": np.array([0 if fr["kind"] else len(fr["status"]) for fr in rec], np.int32),
           f"{name}_n_recs": np.array([0 if fr["kind"] else len(fr["rec_ids"]) for fr in rec], np.int32),
           f"{name}_n_tracks": np.array([len(fr["counters"]) for fr in rec], np.int32),
           f"{name}_next_ids": np.array([fr["next_id"] for fr in rec], np.int32),
           f"{name}_counters": cat("counters", np.zeros((0, 4), np.int32), rec),
           f"{name}_boxes": cat("boxes", np.zeros((0, 4), F32), det), f"{name}_ids": cat("ids", np.zeros(0, np.int32), det),
           f"{name}_next": cat("next", np.zeros((0, 2), F32), itp), f"{name}_status": cat("status", np.zeros(0, np.uint8), itp),
           f"{name}_rec_ids": cat("rec_ids", np.zeros(0, np.int32), itp), f"{name}_rec_boxes": cat("rec_boxes", np.zeros((0, 4), F64), itp),
           f"{name}_rec_followed": cat("rec_followed", np.zeros(0, bool), itp)}
    out.update({f"{name}_final_{k}": v for k, v in final.items()})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("OPD_REFERENCE_ROOT"))
    ap.add_argument("--out", default=LC.GOLDEN)
    args = ap.parse_args()
    if not args.reference:
        sys.exit("the recorded ids are the reference's own: pass --reference DIR")
    LightweightTracker, Detection = load_reference(args.reference)
    out, names, kept, drawn, dropped, tol, rtol = {}, [], set(), 0, 0, 0.0, 0.0
    for kind, K, seeds in PLAN:
        for seed in seeds:
            drawn += 1
            name = f"{kind}_s{seed}"
            got, why, err, rerr = run_one(LightweightTracker, Detection, kind, K, seed)
            if got is None:
                dropped += 1
                print(f"{name}: DROPPED ({why})")
                continue
            params, rec, final = got
            out.update(pack(name, params, rec, final))
            names.append(name)
            kept.add(kind)
            tol, rtol = max(tol, err), max(rtol, rerr)
            print(f"{name}: {len(rec)} frames, ids up to {rec[-1]['next_id'] - 1}, {len(final['x'])} tracks at the end ({int(final['is32'].sum())} with a float32 x), "
                  f"{sum(int((fr['status'] == 0).sum()) for fr in rec if not fr['kind'])} points lost, reference vs float64: states {err:.3e}, predicted records {rerr:.3e}")
    print(f"dropped {dropped} of {drawn} drawn sequences; kalman_tol = {tol:.6e}, record_tol = {rtol:.6e} (the device tests assert 8 x each)")
    assert dropped <= 0.1 * drawn, "more than 10 % of the drawn sequences were dropped: draw other seeds"
    assert kept == set(LC.CLASSES), f"no sequence left of: {sorted(set(LC.CLASSES) - kept)}"
    out["names"] = np.array(names)
    out["kalman_tol"], out["record_tol"] = F64(tol), F64(rtol)
    out["drawn"], out["dropped"] = np.int32(drawn), np.int32(dropped)
    np.savez_compressed(args.out, **out)
    size = os.path.getsize(args.out)
    print(f"wrote {args.out}: {len(names)} sequences, {size} bytes")
    assert size < (1 << 20)


if __name__ == "__main__":
    main()
