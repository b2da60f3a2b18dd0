"""The hybrid tracker of ``csrc/kernels_lwt.hip`` restated in numpy, for the tests, tools/gen_lwt_golden.py and tools/bench_lwt.py.

``Restatement`` is the reference's ``LightweightTracker`` + ``LightweightTrack`` + the bookkeeping of ``OpticalFlowTracker`` with the Kalman
recurrences evaluated elementwise in the kernel's stated order (track_common's ``kalman_predict`` / ``kalman_update``) and every cast
written out, so that nothing depends on the numpy version's promotion rules:

  * P, S, K are float32 always; x is a float32 array until the first update with a float64 centre (a detection-frame match) and a
    float64 array from then on: y = z - x[:2] and x + K y are then evaluated in float64 on the float32 K;
  * the box a followed point gives is (float32(c) - float32(w / 2), ...): a float32 scalar minus a Python float is float32 in numpy 2;
  * IoU in Python floats on float32-valued boxes.

Its ``x``, ``P`` and ``bbox`` are what the device must hold bit for bit.  ``wide=True`` evaluates the same formulas with everything in
float64: the yardstick ``kalman_tol`` is measured against."""

import ctypes as C
import os

import numpy as np

import track_common as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "lwt_sequences.npz")
F32, F64 = np.float32, np.float64
DEFAULTS = dict(max_age=30, iou_threshold=0.3, use_optical_flow=True)
CLASSES = ("flowoff", "lost", "alllost", "occlusion", "empty", "moredets", "moretracks", "shuffled")


# ---- the arithmetic ---------------------------------------------------------------------------------------------------------------------
def predict(x, P):
    """x in its own element type, P in its own."""
    xn = x.copy()
    xn[0] = x[0] + x[2]
    xn[1] = x[1] + x[3]
    return xn, TC.kalman_predict(np.zeros(4, P.dtype), P)[1]


def gain(P):
    ft = P.dtype
    one = ft.type(1)
    s00, s01, s10, s11 = P[0, 0] + one, P[0, 1], P[1, 0], P[1, 1] + one
    det = s00 * s11 - s01 * s10
    i00, i01, i10, i11 = s11 / det, (-s01) / det, (-s10) / det, s00 / det
    K = np.empty((4, 2), ft)
    K[:, 0] = P[:, 0] * i00 + P[:, 1] * i10
    K[:, 1] = P[:, 0] * i01 + P[:, 1] * i11
    return K


def update(x, P, z):
    """z: a float32 or float64 pair.  Same element type as x: track_common's update; else the mixed one (float64 x, float32 P)."""
    if x.dtype == z.dtype == P.dtype:
        return TC.kalman_update(x, P, z)
    Pn = TC.kalman_update(np.zeros(4, P.dtype), P, np.zeros(2, P.dtype))[1]
    K = gain(P).astype(F64)
    x64, z64 = x.astype(F64), z.astype(F64)
    y0, y1 = z64[0] - x64[0], z64[1] - x64[1]
    return x64 + (K[:, 0] * y0 + K[:, 1] * y1), Pn


def iou(b1, b2):
    x1, y1, w1, h1 = (float(v) for v in b1)
    x2, y2, w2, h2 = (float(v) for v in b2)
    xi1, yi1 = (x2 if x2 > x1 else x1), (y2 if y2 > y1 else y1)
    r1, r2, e1, e2 = x1 + w1, x2 + w2, y1 + h1, y2 + h2
    xi2, yi2 = (r2 if r2 < r1 else r1), (e2 if e2 < e1 else e1)
    dw, dh = xi2 - xi1, yi2 - yi1
    inter = (dw if dw > 0.0 else 0.0) * (dh if dh > 0.0 else 0.0)
    uni = (w1 * h1 + w2 * h2) - inter
    return 0.0 if uni <= 0.0 else inter / uni


class Restatement:
    def __init__(self, max_age=30, iou_threshold=0.3, use_optical_flow=True, wide=False):
        self.max_age, self.thr, self.use_flow, self.wide = int(max_age), float(iou_threshold), bool(use_optical_flow), wide
        self.reset()

    def reset(self):
        self.tracks, self.next_id = [], 1
        self.pts, self.pt_ids = np.zeros((0, 2), F32), []
        self.margin, self.tied = np.inf, False   # over the whole run: the closest a greedy maximum came to the threshold; a tied maximum was taken

    def _match(self, boxes):
        T, N = len(self.tracks), len(boxes)
        if T == 0 or N == 0:
            return []
        m = np.zeros((T, N))
        for t, tr in enumerate(self.tracks):
            for d in range(N):
                m[t, d] = iou(tr["bbox"], boxes[d])
        out = []
        while True:
            top = m.max()
            self.margin = min(self.margin, abs(top - self.thr))
            if top < self.thr:
                break
            self.tied = self.tied or int((m == top).sum()) > 1
            t, d = divmod(int(m.argmax()), N)
            out.append((t, d))
            m[t, :] = 0
            m[:, d] = 0
        return out

    def _kalman_update(self, tr, z):
        if self.wide:
            z = z.astype(F64)
        tr["x"], tr["P"] = update(tr["x"], tr["P"], z)

    def update(self, boxes):
        """``update_with_detections`` on float32 boxes [N][4]; returns the id of every detection."""
        boxes = np.asarray(boxes, F32).reshape(-1, 4)
        N = len(boxes)
        for tr in self.tracks:
            tr["x"], tr["P"] = predict(tr["x"], tr["P"])
            tr["age"] += 1
            tr["tsu"] += 1
        ids = [-1] * N
        centres = np.stack([boxes[:, 0].astype(F64) + boxes[:, 2].astype(F64) / 2.0, boxes[:, 1].astype(F64) + boxes[:, 3].astype(F64) / 2.0], 1)
        for t, d in self._match(boxes):
            tr = self.tracks[t]
            tr["bbox"], tr["center"] = boxes[d].copy(), centres[d].copy()
            self._kalman_update(tr, centres[d])
            tr["tsu"] = 0
            tr["hits"] += 1
            ids[d] = tr["id"]
        ft = F64 if self.wide else F32
        for d in range(N):
            if ids[d] >= 0:
                continue
            c32 = centres[d].astype(F32)
            self.tracks.append(dict(id=self.next_id, bbox=boxes[d].copy(), center=centres[d].copy(), x=np.array([c32[0], c32[1], 0, 0], ft),
                                    P=np.diag([100.0, 100.0, 1000.0, 1000.0]).astype(ft), age=0, hits=1, tsu=0))
            ids[d] = self.next_id
            self.next_id += 1
        self.tracks = [tr for tr in self.tracks if tr["tsu"] <= self.max_age]
        if self.use_flow:
            self.pts, self.pt_ids = centres.astype(F32), list(ids)
        return ids

    def interpolate(self, next_xy=None, status=None):
        """``interpolate`` with LK's results for the points held (``next_xy`` [n][2] float32, ``status`` [n]); returns [(id, (x, y, w, h))]."""
        followed = {}
        if self.use_flow and len(self.pt_ids):
            next_xy, status = np.asarray(next_xy, F32).reshape(-1, 2), np.asarray(status).reshape(-1)
            assert len(next_xy) == len(status) == len(self.pt_ids)
            good = np.flatnonzero(status == 1)
            followed = {self.pt_ids[j]: next_xy[j] for j in good}
            self.pts, self.pt_ids = next_xy[good].copy(), [self.pt_ids[j] for j in good]
        out = []
        for tr in self.tracks:
            w, h = tr["bbox"][2], tr["bbox"][3]
            hw, hh = float(w) / 2.0, float(h) / 2.0
            c = followed.get(tr["id"])
            if c is not None:
                bx, by = F32(c[0]) - F32(hw), F32(c[1]) - F32(hh)
                tr["bbox"], tr["center"] = np.array([bx, by, w, h], F32), c.astype(F64)
                self._kalman_update(tr, c.astype(F32))
                tr["tsu"] = 0
                tr["hits"] += 1
            else:
                tr["x"], tr["P"] = predict(tr["x"], tr["P"])
                tr["age"] += 1
                tr["tsu"] += 1
                if tr["x"].dtype == F32:
                    bx, by = tr["x"][0] - F32(hw), tr["x"][1] - F32(hh)
                else:
                    bx, by = float(tr["x"][0]) - hw, float(tr["x"][1]) - hh
            out.append((tr["id"], (float(bx), float(by), float(w), float(h))))
        return out

    def counters(self):
        return np.array([[tr["id"], tr["age"], tr["hits"], tr["tsu"]] for tr in self.tracks], np.int32).reshape(-1, 4)

    def states(self):
        """x [T][4] float64 (holding float32 values where is32), P [T][4][4] float32 (float64 when wide), is32 [T], bbox [T][4] float32."""
        x = np.array([tr["x"].astype(F64) for tr in self.tracks], F64).reshape(-1, 4)
        P = np.array([tr["P"] for tr in self.tracks], F64 if self.wide else F32).reshape(-1, 4, 4)
        is32 = np.array([tr["x"].dtype == F32 for tr in self.tracks], bool)
        return x, P, is32, np.array([tr["bbox"] for tr in self.tracks], F32).reshape(-1, 4)


# ---- the fixture ------------------------------------------------------------------------------------------------------------------------
def sequence_names(g):
    return [str(n) for n in g["names"]]


def sequence(g, name):
    """(params, frames): a frame is a dict with kind 'det' (boxes, ids) or 'interp' (next, status, rec_ids, rec_boxes, rec_followed), and the counters
    [T][4] and next_id after it."""
    params = dict(max_age=int(g[f"{name}_max_age"]), iou_threshold=float(g[f"{name}_iou_threshold"]), use_optical_flow=bool(g[f"{name}_use_flow"]))
    kinds, nd, npts, nrec, ntr = (g[f"{name}_{k}"] for k in ("kinds", "n_dets", "n_points", "n_recs", "n_tracks"))
    od, op, orc, ot = (np.concatenate([[0], np.cumsum(a)]) for a in (nd, npts, nrec, ntr))
    frames = []
    for f, kind in enumerate(kinds):
        fr = dict(kind="det" if kind else "interp", counters=g[f"{name}_counters"][ot[f]:ot[f + 1]], next_id=int(g[f"{name}_next_ids"][f]))
        if kind:
            fr.update(boxes=g[f"{name}_boxes"][od[f]:od[f + 1]], ids=g[f"{name}_ids"][od[f]:od[f + 1]])
        else:
            fr.update(next=g[f"{name}_next"][op[f]:op[f + 1]], status=g[f"{name}_status"][op[f]:op[f + 1]],
                      rec_ids=g[f"{name}_rec_ids"][orc[f]:orc[f + 1]], rec_boxes=g[f"{name}_rec_boxes"][orc[f]:orc[f + 1]],
                      rec_followed=g[f"{name}_rec_followed"][orc[f]:orc[f + 1]])
        frames.append(fr)
    return params, frames


def records_error(recs, boxes):
    """The largest distance of the records' x and y from ``boxes`` [n][4], relative to max(1, |value|): the measure of ``kalman_tol``."""
    got, want = np.array([r[1] for r in recs], F64).reshape(-1, 4)[:, :2], np.asarray(boxes, F64).reshape(-1, 4)[:, :2]
    return float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max()) if got.size else 0.0


def records_equal(recs, ids, boxes, followed=None, tol=0.0):
    """[(id, (x, y, w, h))] against recorded ids [n] and boxes [n][4] float64, as bit patterns.  With ``followed`` [n]: x and y of the
    other records (a Kalman-predicted centre minus half the size) may lie ``tol`` away in the measure of records_error."""
    got_ids = np.array([r[0] for r in recs], np.int32)
    got, want = np.array([r[1] for r in recs], F64).reshape(-1, 4), np.ascontiguousarray(boxes, F64).reshape(-1, 4)
    if not np.array_equal(got_ids, np.asarray(ids, np.int32)):
        return False
    same = got.view(np.uint64) == want.view(np.uint64)
    if followed is None:
        return bool(same.all())
    followed = np.asarray(followed, bool)
    predicted = [r for r, f in zip(recs, followed) if not f]
    return bool(same[:, 2:].all() and same[followed].all() and records_error(predicted, want[~followed]) <= tol)


# ---- the C-ABI --------------------------------------------------------------------------------------------------------------------------
DUMMY_FRAME = np.zeros((24, 32, 3), np.uint8)   # what a flow-on handle is fed where only the track logic is under test


def create(lib, capi, max_tracks=32, max_dets=32, max_h=24, max_w=32, device=0, flow=None, **params):
    """``flow``: further fields of opd_lwt_config.flow (win, max_level, max_iter, epsilon, min_eig_threshold; absent = the defaults)."""
    p = dict(DEFAULTS, **params)
    cfg = capi.OpdLwtConfig(struct_size=C.sizeof(capi.OpdLwtConfig), max_tracks=max_tracks, max_dets=max_dets, max_age=p["max_age"],
                            use_optical_flow=int(p["use_optical_flow"]), iou_threshold=p["iou_threshold"],
                            flow=capi.OpdFlowConfig(max_h=max_h, max_w=max_w, max_points=1, **(flow or {})))
    h = C.c_void_p()
    capi.check(lib.opd_lwt_create(C.byref(cfg), device, C.byref(h)), "opd_lwt_create")
    return h


def info(lib, capi, h):
    st = capi.OpdLwtStatus()
    capi.check(lib.opd_lwt_info(h, C.byref(st)), "opd_lwt_info")
    return st


def _frame_args(frame):
    """(pointer, mem_kind, h, w) of None, a host array or (device pointer, h, w)."""
    if frame is None:
        return None, 0, 0, 0
    if isinstance(frame, tuple):
        return C.c_void_p(int(frame[0])), 1, frame[1], frame[2]
    assert frame.dtype == np.uint8 and frame.flags.c_contiguous
    return C.c_void_p(frame.ctypes.data), 0, frame.shape[0], frame.shape[1]


def device_update(lib, capi, h, boxes, frame=None):
    """opd_lwt_update; returns (rc, ids)."""
    boxes = np.ascontiguousarray(boxes, F32).reshape(-1, 4)
    n = len(boxes)
    ids = np.full(max(n, 1), -7, np.int32)
    ptr, kind, fh, fw = _frame_args(frame)
    rc = lib.opd_lwt_update(h, ptr, kind, fh, fw, TC.ptr(boxes), n, TC.ptr(ids))
    return rc, ids[:n]


def _recs(capi, recs, n):
    return [(recs[i].track_id, tuple(float(v) for v in recs[i].bbox)) for i in range(n)]


def device_interpolate(lib, capi, h, frame=None):
    """opd_lwt_interpolate; returns [(id, (x, y, w, h))]."""
    cap = info(lib, capi, h).n_tracks
    recs, n = (capi.OpdLwtRec * max(cap, 1))(), C.c_int()
    ptr, kind, fh, fw = _frame_args(frame)
    capi.check(lib.opd_lwt_interpolate(h, ptr, kind, fh, fw, recs, cap, C.byref(n)), "opd_lwt_interpolate")
    return _recs(capi, recs, n.value)


def device_scripted(lib, capi, h, next_xy, status):
    """The in-between frame on dictated LK results (opd_test_lwt_interpolate_scripted)."""
    cap = info(lib, capi, h).n_tracks
    recs, n = (capi.OpdLwtRec * max(cap, 1))(), C.c_int()
    nxt, st = np.ascontiguousarray(next_xy, F32).reshape(-1, 2), np.ascontiguousarray(status, np.uint8)
    capi.check(lib.opd_test_lwt_interpolate_scripted(h, TC.ptr(nxt), TC.ptr(st), recs, cap, C.byref(n)), "opd_test_lwt_interpolate_scripted")
    return _recs(capi, recs, n.value)


def device_tracks(lib, capi, h):
    n = C.c_int()
    capi.check(lib.opd_lwt_get(h, None, 0, C.byref(n)), "opd_lwt_get")
    out = (capi.OpdLwtTrack * max(n.value, 1))()
    capi.check(lib.opd_lwt_get(h, out, n.value, C.byref(n)), "opd_lwt_get")
    return [out[i] for i in range(n.value)]


def device_states(lib, capi, h):
    """The device's tracks in the shape of ``Restatement.states`` + counters: x, P, is32, bbox, counters, centers."""
    tr = device_tracks(lib, capi, h)
    x = np.array([list(t.x) for t in tr], F64).reshape(-1, 4)
    P = np.array([list(t.P) for t in tr], F32).reshape(-1, 4, 4)
    is32 = np.array([bool(t.x_is_float32) for t in tr], bool)
    bbox = np.array([list(t.bbox) for t in tr], F64).reshape(-1, 4)
    counters = np.array([[t.track_id, t.age, t.hits, t.time_since_update] for t in tr], np.int32).reshape(-1, 4)
    return x, P, is32, bbox, counters, np.array([list(t.center) for t in tr], F64).reshape(-1, 2)
