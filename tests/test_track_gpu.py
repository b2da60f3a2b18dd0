"""The tracker on the device: ``opd_track_update`` and ``HipTracker`` against the fixture the reference's own ``Tracker`` recorded
(tests/golden/track_sequences.npz, tools/gen_track_golden.py) and the numpy restatement in track_common.py.

The bounds.
  * Kalman x and P after every frame equal the float32 restatement BIT FOR BIT: the kernel file is built without fused multiply-adds and
    the restatement evaluates the same operations in the same order.  Against the reference's recorded final states they lie within
    8 x kalman_tol, the distance the generator measured between the reference's float32 states and the float64 restatement.
  * Smoothed features and appearance costs lie within (2 D + 8) 2^-24 of the float64 restatement on the same inputs: the worst case of a
    float32 dot product of two unit vectors in any order (D products and D - 1 sums, each within 2^-24 of a partial sum that is at most 1 in
    magnitude) plus one float32 normalisation; 6.2e-5 at D = 512.  The combined cost is a convex combination of the appearance cost and the
    exactly evaluated IoU distance, so the same bound holds for it.
  * The IoU distance is evaluated in double on float32 boxes by the same operations as the restatement: equal.  Where the gate fires the
    combined cost is exactly 1.0.
  * Ids per frame and the final counters equal the reference's."""

import ctypes as C
import faulthandler

import numpy as np
import pytest
import torch

import track_common as TC
from office_person_detection_vit_amd import Detection, HipTracker, _capi

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(autouse=True)
def _time_limit():
    """Every test runs under its own limit: a hang ends the process (with a traceback) instead of holding the GPU."""
    faulthandler.dump_traceback_later(120, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def lib():
    return _capi.load_library()


@pytest.fixture(scope="module")
def golden():
    return np.load(TC.GOLDEN)


def _info(lib, h):
    info = _capi.OpdTrackStatus()
    _capi.check(lib.opd_track_info(h, C.byref(info)), "opd_track_info")
    return info


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _same_bits(a, b, what):
    assert np.array_equal(_bits(a), _bits(b)), (what, np.asarray(a).ravel()[:8], np.asarray(b).ravel()[:8])


@pytest.mark.parametrize("name", TC.sequence_names(np.load(TC.GOLDEN)))
def test_golden_sequences_through_the_c_abi(lib, golden, name):
    params, D, frames = TC.sequence(golden, name)
    bound = (2 * D + 8) * 2.0 ** -24
    r32, r64 = TC.Restatement(D, np.float32, **params), TC.Restatement(D, np.float64, **params)
    h = TC.create(lib, _capi, D, max_tracks=12, max_dets=16, **params)
    worst_app = worst_sm = 0.0
    try:
        for f, (boxes, foot, conf, feats, has, want) in enumerate(frames):
            T = len(r32.tracks)
            rc, ids = TC.device_update(lib, _capi, h, boxes, foot, conf, feats, has)
            assert rc == 0, _capi.last_error()
            info = _info(lib, h)
            assert info.last_waits == 1 and info.last_launches <= 2 and (info.last_launches >= 1) == (T > 0 or (ids >= 0).any())
            assert ids.tolist() == want.tolist(), f
            assert r32.update(boxes, foot, conf, feats, has) == want.tolist() == r64.update(boxes, foot, conf, feats, has)
            app, iou, comb = TC.device_matrices(lib, _capi, h)
            m32, m64 = r32.last, r64.last
            assert app.shape == (T, len(conf))
            if app.size:
                assert np.array_equal(iou, m32["iou32"]), f
                assert np.all(comb[m32["gate"]] == 1.0) and np.array_equal(m32["gate"], m64["gate"])
                worst_app = max(worst_app, float(np.abs(app - m64["app"]).max()), float(np.abs(comb - m64["comb"]).max()))
            assert info.n_tracks == len(r32.tracks) and info.next_id == r32.next_id
            live = {tr["id"]: i for i, tr in enumerate(r32.tracks)}
            for i, tr in enumerate(r32.tracks):
                x, P, n_ring, sm = TC.device_state(lib, _capi, h, i, D)
                _same_bits(x, tr["x"], (f, i, "x"))
                _same_bits(P, tr["P"], (f, i, "P"))
                assert n_ring == len(tr["ring"])
            # the smoothed features this frame's rows were computed with (tracks that were alive before the frame and still are)
            for t, s64 in enumerate(m64["smooth"]):
                tid = m64["ids_before"][t]
                if s64 is not None and tid in live:
                    sm = TC.device_state(lib, _capi, h, live[tid], D)[3]
                    worst_sm = max(worst_sm, float(np.abs(sm - s64).max()))
        print(f"{name}: D = {D}, max |app, comb - float64| = {worst_app:.3e}, max |smoothed - float64| = {worst_sm:.3e} (bound {bound:.3e})")
        assert worst_app <= bound and worst_sm <= bound
        recs = TC.device_tracks(lib, _capi, h)
        got = np.array([[r.track_id, r.age, r.hits, r.time_since_update] for r in recs], np.int32).reshape(-1, 4)
        assert np.array_equal(got, golden[f"{name}_counters"])
        x = np.array([list(r.x) for r in recs], F32).reshape(-1, 4)
        P = np.array([TC.device_state(lib, _capi, h, i, D)[1] for i in range(len(recs))], F32).reshape(-1, 4, 4)
        err, limit = TC.state_error(x, P, golden[f"{name}_x"], golden[f"{name}_P"]), 8 * float(golden["kalman_tol"])
        print(f"{name}: final device states {err:.3e} from the reference's (bound {limit:.3e})")
        assert err <= limit
        for r, tr in zip(recs, r32.tracks):
            _same_bits(list(r.box), tr["box"], "box")
    finally:
        lib.opd_track_destroy(h)


@pytest.mark.parametrize("name", TC.sequence_names(np.load(TC.GOLDEN)))
def test_golden_sequences_through_hip_tracker(golden, name):
    params, D, frames = TC.sequence(golden, name)
    t = HipTracker(feature_dim=D, max_tracks=12, max_dets=16, **params)
    try:
        for f, (boxes, foot, conf, feats, has, want) in enumerate(frames):
            dets = [Detection(bbox=tuple(float(v) for v in boxes[j]), confidence=float(conf[j]), class_id=1, class_name="person",
                              camera_coords=(float(foot[j, 0]), float(foot[j, 1])), features=feats[j] if feats is not None and has[j] else None)
                    for j in range(len(conf))]
            out = t.update(dets)
            assert [d.track_id if d.track_id is not None else -1 for d in dets] == want.tolist(), f
            assert out == [d for d in dets if d.track_id is not None]
        got = np.array([[tr.track_id, tr.age, tr.hits, tr.time_since_update] for tr in t.tracks], np.int32).reshape(-1, 4)
        assert np.array_equal(got, golden[f"{name}_counters"])
        assert t.next_id == int(golden[f"{name}_ids"].max()) + 1
        assert [tr.track_id for tr in t.get_confirmed_tracks()] == [int(c[0]) for c in golden[f"{name}_counters"] if c[2] >= t.min_hits]
        for tr, x in zip(t.get_tracks(), golden[f"{name}_x"]):
            st = tr.get_state()
            assert st["track_id"] == tr.track_id and st["trajectory_length"] == tr.hits == len(tr.trajectory)
            assert np.all(np.abs(np.array(st["position"] + st["velocity"]) - x) <= 8 * float(golden["kalman_tol"]) * np.maximum(1.0, np.abs(x)))
        t.reset()
        assert t.tracks == [] and t.next_id == 1
    finally:
        t.close()


# ---- a track's numbers do not depend on the launch ------------------------------------------------------------------------------------
def _unit(v):
    return (v / np.linalg.norm(v)).astype(F32)


def _probe_history(D, rng, n_frames=14):
    """A walker seen on frames 0 .. n - 1 except 5, 6, 7 (the re-update path), more than ten times in all (the ring overflows)."""
    base = _unit(rng.standard_normal(D))
    out = []
    for f in range(n_frames):
        if f in (5, 6, 7):
            out.append(None)
            continue
        box = np.array([700.0 + 3.5 * f, 420.0 - 2.0 * f, 60.0, 150.5], F32)
        out.append((box, _unit(base + rng.standard_normal(D) * (0.25 / np.sqrt(D)))))
    return out


def _foot(boxes):
    return np.stack([boxes[:, 0] + boxes[:, 2] / F32(2), boxes[:, 1] + boxes[:, 3]], 1).astype(F32)


def _others(f):
    """Eleven slow walkers far from the probe and from one another; `f` moves them."""
    return np.array([[40.0 + 290.0 * (k % 6) + 1.5 * f, 900.0 + 320.0 * (k // 6) + 0.5 * f, 50.0 + k, 140.0] for k in range(11)], F32)


@pytest.mark.parametrize("D", [37, 512])
def test_rows_and_state_do_not_depend_on_the_launch(lib, D):
    rng = np.random.default_rng(D)
    hist = _probe_history(D, rng)
    other_feats = [_unit(rng.standard_normal(D)) for _ in range(11)]
    # the last frame: the probe's detection, the others', and four low-confidence detections (they start nothing)
    last_box = np.array([700.0 + 3.5 * 14, 420.0 - 2.0 * 14, 61.0, 149.0], F32)
    last_feat = _unit(hist[-1][1] + rng.standard_normal(D) * (0.2 / np.sqrt(D)))
    low_boxes = np.array([[690.0, 380.0, 70.0, 160.0], [1500.0, 100.0, 40.0, 90.0], [760.0, 300.0, 55.0, 150.0], [20.0, 20.0, 30.0, 60.0]], F32)
    low_feats = np.stack([_unit(rng.standard_normal(D)) for _ in range(4)])

    def run(crowd, max_tracks, final):
        """final: 'one' = the probe's detection alone; 'all' = all sixteen, the probe's last.  Returns rows [3][N], x, P, smoothed."""
        h = TC.create(lib, _capi, D, max_tracks=max_tracks, max_dets=16)
        try:
            for f, item in enumerate(hist):
                boxes = [*_others(f)] if crowd else []
                feats = list(other_feats) if crowd else []
                if item is not None:   # (among others the probe is the LAST detection of frame 0: it gets the last slot)
                    boxes.append(item[0])
                    feats.append(item[1])
                b = np.array(boxes, F32).reshape(-1, 4)
                rc, ids = TC.device_update(lib, _capi, h, b, _foot(b), np.full(len(b), 0.9, F32), np.array(feats, F32).reshape(-1, D) if len(b) else None)
                assert rc == 0, _capi.last_error()
                probe_id = 12 if crowd else 1
                assert (probe_id in ids.tolist()) == (item is not None), (f, ids)
            row = [r.track_id for r in TC.device_tracks(lib, _capi, h)].index(probe_id)
            if final == "one":
                b, ft, conf = last_box[None], last_feat[None], np.array([0.9], F32)
            else:
                ob = _others(len(hist))
                b = np.concatenate([ob, low_boxes, last_box[None]])
                ft = np.concatenate([np.array(other_feats, F32), low_feats, last_feat[None]])
                conf = np.array([0.9] * 11 + [0.3] * 4 + [0.9], F32)
            rc, ids = TC.device_update(lib, _capi, h, b, _foot(b), conf, ft)
            assert rc == 0 and ids[-1] == probe_id, (_capi.last_error(), ids)
            rows = np.stack([m[row] for m in TC.device_matrices(lib, _capi, h)])
            row = [r.track_id for r in TC.device_tracks(lib, _capi, h)].index(probe_id)
            x, P, n_ring, sm = TC.device_state(lib, _capi, h, row, D)
            assert n_ring == 10
            return rows, x, P, sm
        finally:
            lib.opd_track_destroy(h)

    alone_one = run(False, 16, "one")     # slot 0, T = 1, N = 1
    alone_all = run(False, 16, "all")     # slot 0, T = 1, N = 16
    crowd_all = run(True, 12, "all")      # the last slot of twelve, T = 12, N = 16
    _same_bits(alone_all[0], crowd_all[0], "rows: alone / among eleven others, slot 0 / the last slot")
    _same_bits(alone_one[0][:, 0], alone_all[0][:, 15], "rows: N = 1 / N = 16")
    for k, what in ((1, "x"), (2, "P"), (3, "smoothed feature")):
        _same_bits(alone_one[k], alone_all[k], what)
        _same_bits(alone_all[k], crowd_all[k], what)
    assert alone_all[0][0, 15] < 0.3 and (alone_all[0][0, :11] > 0.3).all()   # the probe's own detection is close in appearance, the others are not
    # the tail lanes: the smoothed feature is a unit vector and matches a plain float64 evaluation
    assert abs(float(np.sum(alone_one[3].astype(np.float64) ** 2)) - 1.0) <= (2 * D + 8) * 2.0 ** -24


# ---- edge cases -----------------------------------------------------------------------------------------------------------------------
def _three(D, rng):
    boxes = np.array([[100.0, 100.0, 50.0, 120.0], [600.0, 200.0, 60.0, 150.0], [1100.0, 400.0, 55.0, 140.0]], F32)
    feats = np.stack([_unit(rng.standard_normal(D)) for _ in range(3)])
    return boxes, _foot(boxes), feats


def test_no_detections_still_predicts_and_no_tracks_start_from_high_confidence_only(lib):
    D = 37
    boxes, foot, feats = _three(D, np.random.default_rng(1))
    h = TC.create(lib, _capi, D)
    r = TC.Restatement(D, np.float32)
    try:
        conf = np.array([0.9, 0.3, 0.8], F32)
        rc, ids = TC.device_update(lib, _capi, h, boxes, foot, conf, feats)
        assert rc == 0 and ids.tolist() == [1, -1, 2] == r.update(boxes, foot, conf, feats)
        assert (_info(lib, h).last_launches, _info(lib, h).last_waits, _info(lib, h).n_tracks) == (1, 1, 2)
        for _ in range(2):
            rc, ids = TC.device_update(lib, _capi, h, boxes[:0], foot[:0], conf[:0])
            assert rc == 0 and len(ids) == 0
            r.update(boxes[:0], foot[:0], conf[:0])
            assert (_info(lib, h).last_launches, _info(lib, h).last_waits) == (1, 1)
        recs = TC.device_tracks(lib, _capi, h)
        assert [(q.track_id, q.age, q.hits, q.time_since_update) for q in recs] == [(1, 1, 1, 2), (2, 1, 1, 2)]
        for i, tr in enumerate(r.tracks):
            x, P, n_ring, _ = TC.device_state(lib, _capi, h, i, D)
            _same_bits(x, tr["x"], "x")
            _same_bits(P, tr["P"], "P")
            assert n_ring == 1 and P[0, 0] > 100.0
    finally:
        lib.opd_track_destroy(h)


def test_device_features_equal_host_features_and_a_host_pointer_is_refused_as_device_memory(lib):
    D = 256
    rng = np.random.default_rng(2)
    boxes, foot, feats = _three(D, rng)
    conf = np.array([0.9, 0.8, 0.7], F32)
    frames = [(boxes + F32(2 * f), _foot(boxes + F32(2 * f)), np.stack([_unit(v + rng.standard_normal(D) * 0.01) for v in feats])) for f in range(5)]
    hh, hd = TC.create(lib, _capi, D), TC.create(lib, _capi, D)
    try:
        for b, ft_pts, ft in frames:
            dev = torch.from_numpy(ft).to("cuda")
            torch.cuda.synchronize()
            rc_h, ids_h = TC.device_update(lib, _capi, hh, b, ft_pts, conf, ft)
            rc_d, ids_d = TC.device_update(lib, _capi, hd, b, ft_pts, conf, feat_ptr=dev.data_ptr())
            assert rc_h == 0 and rc_d == 0, _capi.last_error()
            assert ids_h.tolist() == ids_d.tolist() == [1, 2, 3]
            for mh, md in zip(TC.device_matrices(lib, _capi, hh), TC.device_matrices(lib, _capi, hd)):
                _same_bits(mh, md, "matrices")
        for i in range(3):
            (xh, Ph, nh, sh), (xd, Pd, nd, sd) = TC.device_state(lib, _capi, hh, i, D), TC.device_state(lib, _capi, hd, i, D)
            assert nh == nd == 5
            for a, b in ((xh, xd), (Ph, Pd), (sh, sd)):
                _same_bits(a, b, "state")
        before = [(q.track_id, q.hits, list(q.x)) for q in TC.device_tracks(lib, _capi, hd)]
        b, ft_pts, ft = frames[-1]
        rc, _ = TC.device_update(lib, _capi, hd, b, ft_pts, conf, feat_ptr=ft.ctypes.data)   # pageable host memory called device memory
        assert rc == _capi.OPD_EINVAL and "not device-accessible" in _capi.last_error()
        assert [(q.track_id, q.hits, list(q.x)) for q in TC.device_tracks(lib, _capi, hd)] == before   # nothing was touched
    finally:
        lib.opd_track_destroy(hh)
        lib.opd_track_destroy(hd)


def test_reset_and_the_error_paths(lib):
    D = 37
    boxes, foot, feats = _three(D, np.random.default_rng(3))
    conf = np.array([0.9, 0.8, 0.7], F32)
    h = TC.create(lib, _capi, D, max_tracks=2, max_dets=4)
    try:
        rc, ids = TC.device_update(lib, _capi, h, boxes, foot, conf, feats)          # three new tracks, two slots
        assert rc == _capi.OPD_EINVAL and "max_tracks = 2" in _capi.last_error() and ids.tolist() == [-1, -1, -1]
        assert _info(lib, h).n_tracks == 0
        five = np.concatenate([boxes, boxes[:2] + F32(300)])
        rc, _ = TC.device_update(lib, _capi, h, five, _foot(five), np.full(5, 0.9, F32))   # five detections, room for four
        assert rc == _capi.OPD_EINVAL and "max_dets = 4" in _capi.last_error() and _info(lib, h).n_tracks == 0
        rc, ids = TC.device_update(lib, _capi, h, boxes[:2], foot[:2], conf[:2], feats[:2])
        assert rc == 0 and ids.tolist() == [1, 2]
        rc, ids = TC.device_update(lib, _capi, h, boxes, foot, conf, feats)          # two matched, the third finds no slot: the frame ages the tracks
        assert rc == _capi.OPD_EINVAL and ids.tolist() == [-1, -1, -1]
        assert [(q.track_id, q.hits, q.time_since_update) for q in TC.device_tracks(lib, _capi, h)] == [(1, 1, 1), (2, 1, 1)]
        rc, ids = TC.device_update(lib, _capi, h, boxes[:2], foot[:2], conf[:2], feats[:2])
        assert rc == 0 and ids.tolist() == [1, 2]
        n = C.c_int()
        assert lib.opd_track_get(h, (_capi.OpdTrackRec * 1)(), 1, C.byref(n)) == _capi.OPD_EINVAL and n.value == 2
        _capi.check(lib.opd_track_reset(h), "opd_track_reset")
        info = _info(lib, h)
        assert (info.n_tracks, info.next_id, info.max_tracks, info.max_dets, info.feature_dim, info.max_age, info.min_hits) == (0, 1, 2, 4, D, 30, 3)
        rc, ids = TC.device_update(lib, _capi, h, boxes[1:], foot[1:], conf[1:], feats[1:])
        assert rc == 0 and ids.tolist() == [1, 2]
        x, P, n_ring, _ = TC.device_state(lib, _capi, h, 0, D)
        assert x.tolist() == [float(foot[1, 0]), float(foot[1, 1]), 0.0, 0.0] and np.array_equal(P, np.diag([100.0, 100.0, 1000.0, 1000.0])) and n_ring == 1
    finally:
        lib.opd_track_destroy(h)
