"""The tracker of ``csrc/kernels_track.hip`` / ``csrc/opd_assoc.cpp`` restated in numpy, for the tests and tools/gen_track_golden.py.

``Restatement(D, dtype=np.float32)`` evaluates the Kalman recurrences elementwise in exactly the kernel's stated order (numpy rounds every
elementwise operation to the array's type and fuses nothing, as the kernel file built with -ffp-contract=off does): its ``x`` and ``P``
are what the device must hold bit for bit.  ``dtype=np.float64`` evaluates the same formulas, on the same float32-valued constants, in
float64: the yardstick for the reference's own float32 rounding (``kalman_tol``) and for the features and appearance costs.  The
association runs over the three matrices with ``scipy.optimize.linear_sum_assignment``.

One deliberate difference from the reference: with no live track the reference starts a track from EVERY detection; here, as with live
tracks, only a high-confidence detection starts one."""

import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "track_sequences.npz")
RING = 10
DEFAULTS = dict(max_age=30, min_hits=3, iou_threshold=0.3, appearance_weight=0.7, motion_weight=0.3, max_position_distance=150.0, high_conf_threshold=0.5)
F32 = np.float32


# ---- (c) the association over given matrices --------------------------------------------------------------------------------------------
def _stage(m, tracks, dets, thr, inclusive, remove, matches):
    from scipy.optimize import linear_sum_assignment
    if not tracks or not dets:
        return tracks, dets
    sub = np.asarray(m, np.float64)[np.ix_(tracks, dets)]
    rows, cols = linear_sum_assignment(sub)
    col_of = dict(zip(rows.tolist(), cols.tolist()))
    left, taken = [], set()
    for i, t in enumerate(tracks):
        j = col_of.get(i, -1)
        if j >= 0 and (sub[i, j] <= thr if inclusive else sub[i, j] < thr):
            matches.append((t, dets[j]))
            taken.add(j)
        else:
            left.append(t)
    return left, ([d for k, d in enumerate(dets) if k not in taken] if remove else dets)


def associate(app, iou, comb, hits, conf, min_hits, high_conf):
    """(matches [(track, detection)], detections that start tracks, unmatched tracks) of one frame."""
    T, N = len(hits), len(conf)
    high = [j for j in range(N) if float(conf[j]) >= high_conf]
    low = [j for j in range(N) if not float(conf[j]) >= high_conf]
    if T == 0:
        return [], high, []
    if N == 0:
        return [], [], list(range(T))
    tracks = [t for t in range(T) if hits[t] >= min_hits]
    tentative = [t for t in range(T) if hits[t] < min_hits]
    matches = []
    tracks, high = _stage(app, tracks, high, 0.3, True, True, matches)
    tracks, high = _stage(comb, tracks, high, 1.0 - 0.5, False, True, matches)
    tracks, high = _stage(iou, tracks, high, 1.0 - 0.4, False, True, matches)
    tracks, low = _stage(iou, tracks, low, 1.0 - 0.5, False, False, matches)
    tentative, high = _stage(comb, tentative, high, 1.0 - 0.5, False, True, matches)
    return matches, high, tracks + tentative


# ---- (a) / (b) the arithmetic -----------------------------------------------------------------------------------------------------------
def _q(ft):
    q = F32(0.1)
    q4, q2 = F32(0.25) * q, F32(0.5) * q
    return np.array([[q4, 0, q2, 0], [0, q4, 0, q2], [q2, 0, q, 0], [0, q2, 0, q]], F32).astype(ft)


def kalman_predict(x, P):
    ft = x.dtype
    x = x.copy()
    x[0] = x[0] + x[2]
    x[1] = x[1] + x[3]
    A = P.copy()
    A[0] = P[0] + P[2]
    A[1] = P[1] + P[3]
    B = A.copy()
    B[:, 0] = A[:, 0] + A[:, 2]
    B[:, 1] = A[:, 1] + A[:, 3]
    return x, B + _q(ft)


def kalman_update(x, P, z):
    ft = x.dtype
    one = ft.type(1)
    y0, y1 = z[0] - x[0], z[1] - x[1]
    s00, s01, s10, s11 = P[0, 0] + one, P[0, 1], P[1, 0], P[1, 1] + one
    det = s00 * s11 - s01 * s10
    i00, i01, i10, i11 = s11 / det, (-s01) / det, (-s10) / det, s00 / det
    K = np.empty((4, 2), ft)
    K[:, 0] = P[:, 0] * i00 + P[:, 1] * i10
    K[:, 1] = P[:, 0] * i01 + P[:, 1] * i11
    x = x + (K[:, 0] * y0 + K[:, 1] * y1)
    KH = np.zeros((4, 4), ft)
    KH[:, :2] = K
    M = np.eye(4, dtype=ft) - KH
    Pn = ((M[:, 0:1] * P[0:1, :] + M[:, 1:2] * P[1:2, :]) + M[:, 2:3] * P[2:3, :]) + M[:, 3:4] * P[3:4, :]
    return x, Pn


def smoothed(ring, ft):
    """EMA over the stored features in age order, then the L2 normalisation when the norm exceeds 1e-6; None for an empty ring."""
    if not ring:
        return None
    a, b = ft.type(F32(0.9)), ft.type(F32(0.1))
    e = ring[0].astype(ft)
    for f in ring[1:]:
        e = a * f.astype(ft) + b * e
    norm = np.sqrt(np.sum(e * e, dtype=ft))
    return e / norm if norm > ft.type(F32(1e-6)) else e


def iou_distance(b1, b2):
    """In Python floats (double) on the float32 boxes: the arithmetic of similarity_matrix_kernel."""
    x1, y1, w1, h1 = (float(v) for v in b1)
    x2, y2, w2, h2 = (float(v) for v in b2)
    ix0, iy0 = max(x1, x2), max(y1, y2)
    ix1, iy1 = min(x1 + w1, x2 + w2), min(y1 + h1, y2 + h2)
    iou = 0.0
    if ix1 > ix0 and iy1 > iy0:
        inter = (ix1 - ix0) * (iy1 - iy0)
        uni = w1 * h1 + w2 * h2 - inter
        if uni > 0.0:
            iou = min(max(inter / uni, 0.0), 1.0)
    return 1.0 - iou


class Restatement:
    def __init__(self, D, dtype=np.float32, **params):
        unknown = set(params) - set(DEFAULTS)
        assert not unknown, unknown
        self.D, self.ft = D, np.dtype(dtype)
        self.p = dict(DEFAULTS, **params)
        self.tracks, self.next_id = [], 1
        self.last = None   # of the last update: app / iou / comb [T][N] (float64 arrays holding this dtype's values), gate [T][N], smooth [T],
        #                          ids_before [T] (the tracks the rows belong to)

    def matrices(self, boxes, foot, feats, has):
        ft, T, N = self.ft, len(self.tracks), len(boxes)
        app, iou, comb = np.ones((T, N)), np.ones((T, N)), np.ones((T, N))
        gate, gate_dist = np.zeros((T, N), bool), np.zeros((T, N))
        smooth = []
        aw0, mw, md = self.p["appearance_weight"], self.p["motion_weight"], self.p["max_position_distance"]
        for t, tr in enumerate(self.tracks):
            s = smoothed(tr["ring"], ft)
            smooth.append(s)
            for j in range(N):
                iou[t, j] = iou_distance(tr["box"], boxes[j])
                d = tr["x"][:2].astype(F32) - foot[j]
                gate_dist[t, j] = np.sqrt(d[0] * d[0] + d[1] * d[1])   # (float32)
                gate[t, j] = md > 0 and gate_dist[t, j] > F32(md)
                both = s is not None and feats is not None and bool(has[j])
                if both:
                    dot = np.sum(s * feats[j].astype(ft), dtype=ft)
                    a = 1.0 - float(min(max(dot, ft.type(-1)), ft.type(1)))
                    app[t, j] = a
                aw = aw0 if both else 0.0
                total = aw + mw
                c = 0.0
                if both:
                    c += aw * a
                c += mw * iou[t, j]
                comb[t, j] = 1.0 if gate[t, j] or total == 0 else c / total
        if ft == np.float32:   # the matrices are float32 arrays in the reference and on the device
            app, comb = app.astype(F32).astype(np.float64), comb.astype(F32).astype(np.float64)
        return dict(app=app, iou=iou, comb=comb, iou32=iou.astype(F32), gate=gate, gate_dist=gate_dist, smooth=smooth,
                    ids_before=[tr["id"] for tr in self.tracks])

    def update(self, boxes, foot, conf, feats=None, has=None):
        """One frame; returns the id given to every detection (-1: none)."""
        ft = self.ft
        boxes, foot = np.asarray(boxes, F32).reshape(-1, 4), np.asarray(foot, F32).reshape(-1, 2)
        N = len(boxes)
        if feats is not None and has is None:
            has = np.ones(N, bool)
        for tr in self.tracks:
            tr["x"], tr["P"] = kalman_predict(tr["x"], tr["P"])
            tr["tsu"] += 1
        m = self.last = self.matrices(boxes, foot, feats, has)
        use = (m["app"], m["iou32"] if ft == np.float32 else m["iou"], m["comb"])
        matches, new, _ = associate(*use, [tr["hits"] for tr in self.tracks], conf, self.p["min_hits"], self.p["high_conf_threshold"])
        ids = [-1] * N
        for t, j in matches:
            tr = self.tracks[t]
            z = foot[j].astype(ft)
            if tr["tsu"] >= 3:
                n = tr["tsu"]
                for i in range(1, n + 1):
                    w = ft.type(F32(i / (n + 1)))
                    tr["x"], tr["P"] = kalman_predict(tr["x"], tr["P"])
                    tr["x"], tr["P"] = kalman_update(tr["x"], tr["P"], tr["last"] + w * (z - tr["last"]))
            tr["x"], tr["P"] = kalman_update(tr["x"], tr["P"], z)
            tr["last"], tr["box"] = z, boxes[j].copy()
            tr["age"] += 1
            tr["hits"] += 1
            tr["tsu"] = 0
            if feats is not None and has[j]:
                tr["ring"] = (tr["ring"] + [np.asarray(feats[j], F32).copy()])[-RING:]
            ids[j] = tr["id"]
        for j in new:
            z = foot[j].astype(ft)
            tr = dict(id=self.next_id, age=1, hits=1, tsu=0, x=np.array([z[0], z[1], 0, 0], ft), P=np.diag([100.0, 100.0, 1000.0, 1000.0]).astype(ft),
                      last=z, box=boxes[j].copy(), ring=[np.asarray(feats[j], F32).copy()] if feats is not None and has[j] else [])
            self.next_id += 1
            self.tracks.append(tr)
            ids[j] = tr["id"]
        self.tracks = [tr for tr in self.tracks if tr["tsu"] < self.p["max_age"]]
        return ids

    def counters(self):
        return np.array([[tr["id"], tr["age"], tr["hits"], tr["tsu"]] for tr in self.tracks], np.int32).reshape(-1, 4)

    def states(self):
        return (np.array([tr["x"] for tr in self.tracks], self.ft).reshape(-1, 4), np.array([tr["P"] for tr in self.tracks], self.ft).reshape(-1, 4, 4))


# ---- the fixture ------------------------------------------------------------------------------------------------------------------------
def sequence_names(g):
    return [str(n) for n in g["names"]]


def sequence(g, name):
    """A recorded sequence: params, D and per frame (boxes, foot, conf, feats or None, has or None, reference ids)."""
    D = int(g[f"{name}_D"])
    params = {k: (int(v) if k in ("max_age", "min_hits") else float(v)) for k, v in zip(g[f"{name}_param_names"], g[f"{name}_params"])}
    counts = g[f"{name}_counts"]
    off = np.concatenate([[0], np.cumsum(counts)])
    use_feats = bool(g[f"{name}_use_feats"])
    frames = []
    for f in range(len(counts)):
        s = slice(off[f], off[f + 1])
        frames.append((g[f"{name}_boxes"][s], g[f"{name}_foot"][s], g[f"{name}_conf"][s], g[f"{name}_feats"][s] if use_feats else None,
                       g[f"{name}_has"][s].astype(bool) if use_feats else None, g[f"{name}_ids"][s]))
    return params, D, frames


def state_error(x, P, x_ref, P_ref):
    """x relative to max(1, |x|), P relative to max |P|: the measure kalman_tol is stated in."""
    x, P, x_ref, P_ref = (np.asarray(a, np.float64) for a in (x, P, x_ref, P_ref))
    if x.size == 0:
        return 0.0
    ex = np.abs(x - x_ref) / np.maximum(1.0, np.abs(x_ref))
    eP = np.abs(P - P_ref) / np.abs(P_ref).max(axis=(-2, -1), keepdims=True)
    return float(max(ex.max(), eP.max()))


# ---- the C-ABI --------------------------------------------------------------------------------------------------------------------------
def make_config(capi, D, max_tracks=16, max_dets=16, **params):
    p = dict(params)
    if "max_position_distance" in p and p["max_position_distance"] <= 0:
        p["max_position_distance"] = -1.0
    return capi.OpdTrackConfig(struct_size=C.sizeof(capi.OpdTrackConfig), max_tracks=max_tracks, max_dets=max_dets, feature_dim=D, **p)


def create(lib, capi, D, device=0, **kw):
    h = C.c_void_p()
    cfg = make_config(capi, D, **kw)
    capi.check(lib.opd_track_create(C.byref(cfg), device, C.byref(h)), "opd_track_create")
    return h


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def device_update(lib, capi, h, boxes, foot, conf, feats=None, has=None, feat_ptr=None):
    """opd_track_update on host arrays (``feat_ptr``: a device address used instead of ``feats``); returns (rc, ids)."""
    boxes, foot, conf = (np.ascontiguousarray(a, F32) for a in (boxes, foot, conf))
    n = len(conf)
    feats = None if feats is None else np.ascontiguousarray(feats, F32)
    has8 = None if has is None else np.ascontiguousarray(has, np.uint8)
    ids = np.full(max(n, 1), -7, np.int32)
    if feat_ptr is not None:
        rc = lib.opd_track_update(h, ptr(boxes), ptr(foot), ptr(conf), C.c_void_p(feat_ptr), ptr(has8), capi.OPD_MEM_DEVICE, n, ptr(ids))
    else:
        rc = lib.opd_track_update(h, ptr(boxes), ptr(foot), ptr(conf), ptr(feats), ptr(has8), capi.OPD_MEM_HOST, n, ptr(ids))
    return rc, ids[:n]


def device_tracks(lib, capi, h):
    n = C.c_int()
    capi.check(lib.opd_track_get(h, None, 0, C.byref(n)), "opd_track_get")
    recs = (capi.OpdTrackRec * max(n.value, 1))()
    capi.check(lib.opd_track_get(h, recs, n.value, C.byref(n)), "opd_track_get")
    return [recs[i] for i in range(n.value)]


def device_matrices(lib, capi, h):
    T, N = C.c_int(), C.c_int()
    capi.check(lib.opd_track_test_matrices(h, None, None, None, 0, C.byref(T), C.byref(N)), "opd_track_test_matrices")
    out = [np.zeros((T.value, N.value), F32) for _ in range(3)]
    capi.check(lib.opd_track_test_matrices(h, ptr(out[0]), ptr(out[1]), ptr(out[2]), T.value * N.value, C.byref(T), C.byref(N)), "opd_track_test_matrices")
    return out


def device_state(lib, capi, h, index, D):
    x, P, sm, n = np.zeros(4, F32), np.zeros((4, 4), F32), np.zeros(D, F32), C.c_int32()
    capi.check(lib.opd_track_test_state(h, index, ptr(x), ptr(P), C.byref(n), ptr(sm)), "opd_track_test_state")
    return x, P, n.value, (sm if n.value else None)
