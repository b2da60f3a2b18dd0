"""The hybrid tracker on the device: ``opd_lwt_update`` / ``opd_lwt_interpolate`` and ``HipLightweightTracker`` against the fixture the
reference's own ``LightweightTracker`` recorded (tests/golden/lwt_sequences.npz, tools/gen_lwt_golden.py) and the numpy restatement in
lwt_common.py.

The bounds.
  * Kalman x (as uint64 views of the doubles), P and the box (uint32 views) after EVERY frame, and every interpolate record, equal the
    restatement BIT FOR BIT: the kernel file is built without fused multiply-adds and the restatement evaluates the same operations in the
    same order with the same element types.
  * Ids, counters, next ids, the number of flow points and the element type of every x equal the reference's.  Of the reference's
    interpolate records every id, width and height, and the whole box of a track whose point was followed, are equal bit for bit; the x
    and y of a Kalman-PREDICTED record lie within 8 x record_tol and the final states within 8 x kalman_tol, the distances the generator
    measured on those very numbers between the reference and the all-float64 restatement (test_lwt_cpu.py says why these cannot be equal).
  * The fused interpolate on real frames equals ``opd_flow_track`` on a second flow handle fed into the restatement, bit for bit."""

import ctypes as C
import faulthandler

import numpy as np
import pytest
import torch

import flow_common as FC
import lwt_common as LC
import track_common as TC
from office_person_detection_vit_amd import Detection, HipLightweightTracker, _capi

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64


@pytest.fixture(autouse=True)
def _time_limit():
    """Every test runs under its own limit: a hang ends the process (with a traceback) instead of holding the GPU."""
    faulthandler.dump_traceback_later(120, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def lib():
    return _capi.load_library(test_hooks=True)


@pytest.fixture(scope="module")
def golden():
    return np.load(LC.GOLDEN)


def _same(r, lib, h, what):
    """The device's tracks equal the restatement's: counters, element types, and x / P / box as bit patterns."""
    x, P, is32, bbox, counters, centers = LC.device_states(lib, _capi, h)
    rx, rP, ris32, rbbox = r.states()
    assert np.array_equal(counters, r.counters()), (what, counters, r.counters())
    assert np.array_equal(is32, ris32), what
    assert np.array_equal(x.view(np.uint64), rx.view(np.uint64)), (what, "x", x, rx)
    assert np.array_equal(P.view(np.uint32), rP.view(np.uint32)), (what, "P")
    assert np.array_equal(bbox.astype(F32).view(np.uint32), rbbox.view(np.uint32)) and np.array_equal(bbox, rbbox.astype(F64)), (what, "bbox")
    assert np.array_equal(centers, np.array([tr["center"] for tr in r.tracks], F64).reshape(-1, 2)), (what, "center")
    info = LC.info(lib, _capi, h)
    assert (info.n_tracks, info.next_id, info.n_points) == (len(r.tracks), r.next_id, len(r.pt_ids)), what
    return info


def _recs_same(got, want, what):
    assert [q[0] for q in got] == [q[0] for q in want], what
    a, b = np.array([q[1] for q in got], F64).reshape(-1, 4), np.array([q[1] for q in want], F64).reshape(-1, 4)
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), (what, a, b)


# ---- 1. the fixture -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LC.sequence_names(np.load(LC.GOLDEN)))
def test_golden_sequences_through_the_c_abi(lib, golden, name):
    params, frames = LC.sequence(golden, name)
    bound, rec_bound = 8 * float(golden["kalman_tol"]), 8 * float(golden["record_tol"])
    r = LC.Restatement(**params)
    h = LC.create(lib, _capi, max_tracks=16, max_dets=16, **params)
    frame = LC.DUMMY_FRAME if params["use_optical_flow"] else None
    try:
        for f, fr in enumerate(frames):
            if fr["kind"] == "det":
                rc, ids = LC.device_update(lib, _capi, h, fr["boxes"], frame)
                assert rc == 0, _capi.last_error()
                assert ids.tolist() == fr["ids"].tolist() == r.update(fr["boxes"]), f
            else:
                assert LC.info(lib, _capi, h).n_points == len(fr["status"]), f
                got = LC.device_scripted(lib, _capi, h, fr["next"], fr["status"]) if params["use_optical_flow"] else LC.device_interpolate(lib, _capi, h)
                _recs_same(got, r.interpolate(fr["next"], fr["status"]), (f, "records"))
                assert LC.records_equal(got, fr["rec_ids"], fr["rec_boxes"], fr["rec_followed"], rec_bound), f
            info = _same(r, lib, h, f)
            assert info.last_waits == 1 and info.last_launches >= 1, f
            assert np.array_equal(r.counters(), fr["counters"]) and info.next_id == fr["next_id"], f
        x, P, is32, bbox, _, _ = LC.device_states(lib, _capi, h)
        assert np.array_equal(is32, golden[f"{name}_final_is32"]) and np.array_equal(bbox[:, 2:], golden[f"{name}_final_bbox"][:, 2:])
        err = TC.state_error(x, P, golden[f"{name}_final_x"], golden[f"{name}_final_P"])
        print(f"{name}: final device states {err:.3e} from the reference's (bound {bound:.3e})")
        assert err <= bound
    finally:
        lib.opd_lwt_destroy(h)


# ---- 2. shapes where the kernel can go wrong -----------------------------------------------------------------------------------------------
def _grid(n, dx=0.0, dy=0.0, cols=20):
    """n quarter-pixel boxes 100 px apart (no two overlap), moved by (dx, dy)."""
    k = np.arange(n)
    return np.stack([50.0 + 100.0 * (k % cols) + dx, 30.25 + 120.0 * (k // cols) + dy, 40.0 + (k % 7) * 0.5, 80.0 + (k % 5) * 0.25], 1).astype(F32)


def _both(lib, h, r, boxes, frame=None, what=""):
    rc, ids = LC.device_update(lib, _capi, h, boxes, frame)
    assert rc == 0, _capi.last_error()
    assert ids.tolist() == r.update(boxes), what
    info = _same(r, lib, h, what)
    assert info.last_waits == 1
    return ids.tolist()


def _interp_both(lib, h, r, what=""):
    _recs_same(LC.device_interpolate(lib, _capi, h), r.interpolate(), what)
    assert _same(r, lib, h, what).last_waits == 1


@pytest.mark.parametrize("T,N,picks", [(1, 1, [0]), (65, 3, [64, 0, 33]), (3, 65, [2, 0, 1]), (257, 5, [256, 0, 100])])
def test_matrix_shapes_across_wave_and_workgroup(lib, T, N, picks):
    """T tracks, then N detections of which len(picks) overlap tracks `picks` (out of order); the others start tracks."""
    p = dict(max_age=30, iou_threshold=0.3, use_optical_flow=False)
    r = LC.Restatement(**p)
    h = LC.create(lib, _capi, max_tracks=T + N, max_dets=T + N, **p)
    try:
        assert _both(lib, h, r, _grid(T), what="first") == list(range(1, T + 1))
        _interp_both(lib, h, r, "predict")
        first = _grid(T + N, 3.25, -2.5)
        rows = picks + [T + i for i in range(N - len(picks))]   # tracks' own boxes moved a little, and boxes where no track is
        ids = _both(lib, h, r, first[rows], what="second")
        assert ids[:len(picks)] == [k + 1 for k in picks] and ids[len(picks):] == list(range(T + 1, T + 1 + N - len(picks)))
        _interp_both(lib, h, r, "predict again")
        _both(lib, h, r, _grid(T + N, 5.0, 1.75)[::-1], what="reversed order")
    finally:
        lib.opd_lwt_destroy(h)


def _pile(n, step, x0=300.0, y0=200.0):
    """n quarter-pixel boxes piled on one another: box k lies (step, step / 2) * k from the first, so each overlaps many others."""
    k = np.arange(n)
    return np.stack([x0 + step * k, y0 + 0.5 * step * k, np.full(n, 60.0), np.full(n, 120.0)], 1).astype(F32)


@pytest.mark.parametrize("T,N", [(12, 70), (70, 12), (70, 70)])
def test_rows_competing_for_the_same_detections_are_scanned_again(lib, T, N):
    """Tracks piled tightly on one another and detections fanned out over them: many rows have their maximum in the column a match takes,
    so several waves scan their rows again in one iteration of the greedy loop (over more than one lane stride of columns at N = 70),
    and equal IoUs (the piles are regular) are decided by the row-major tie rule across waves."""
    p = dict(max_age=30, iou_threshold=0.3, use_optical_flow=False)
    r = LC.Restatement(**p)
    h = LC.create(lib, _capi, max_tracks=T + N, max_dets=max(T, N), **p)
    try:
        tracks = _pile(T, 0.25)                                                                    # a tight pile: the tracks want the same few detections
        dets = np.concatenate([_pile(N - 2, 2.0, 301.0, 200.5), _pile(2, 0.0, 301.0, 200.5)])   # the last two equal the first: tied columns
        assert _both(lib, h, r, tracks, what="the pile of tracks") == list(range(1, T + 1))
        m = np.array([[LC.iou(a, b) for b in dets] for a in tracks])
        assert np.bincount(m.argmax(1)).max() > 4, "more rows than the workgroup has waves share one best column"
        assert (m >= 0.3).sum(1).min() >= 12           # every row has a dozen acceptable columns to fall back on
        ids = _both(lib, h, r, dets, what="the pile of detections")
        assert sum(i <= T for i in ids) >= 12 and r.tied      # a dozen rounds of the loop at least, and tied maxima were taken
        _interp_both(lib, h, r, "predict")
        _both(lib, h, r, dets[::-1] + np.array([0.5, 0.25, 0.0, 0.0], F32), what="reversed")
    finally:
        lib.opd_lwt_destroy(h)


def test_empty_sides_ties_and_ageing_out(lib):
    p = dict(max_age=1, iou_threshold=0.3, use_optical_flow=False)
    r = LC.Restatement(**p)
    h = LC.create(lib, _capi, max_tracks=8, max_dets=8, **p)
    try:
        none = np.zeros((0, 4), F32)
        assert _both(lib, h, r, none, what="no tracks, no detections") == []
        _interp_both(lib, h, r, "nothing to interpolate")
        a = np.array([100.0, 100.0, 50.0, 120.0], F32)
        # no tracks: two identical boxes start two tracks with identical boxes
        assert _both(lib, h, r, np.stack([a, a]), what="two identical detections, no tracks") == [1, 2]
        # one detection, both rows have the same IoU: the lower row takes it (argmax over the row-major matrix)
        assert _both(lib, h, r, a[None] + F32(1.0), what="tied rows") == [1]
        # two identical detections: both columns of row 0 are tied, the lower one wins; the other detection goes to the second track
        b = a + F32(2.0)
        assert _both(lib, h, r, np.stack([b, b]), what="tied columns") == [1, 2]
        assert _both(lib, h, r, none, what="no detections: every track predicted") == []
        assert len(r.tracks) == 2
        assert _both(lib, h, r, none, what="every track aged out in one call") == []
        assert len(r.tracks) == 0 and LC.info(lib, _capi, h).n_tracks == 0
        assert _both(lib, h, r, a[None], what="ids go on") == [3]
    finally:
        lib.opd_lwt_destroy(h)


def test_filling_the_handle_exactly_and_the_refusals_that_change_nothing(lib):
    p = dict(max_age=30, iou_threshold=0.3, use_optical_flow=True)
    r = LC.Restatement(**p)
    h = LC.create(lib, _capi, max_tracks=8, max_dets=9, **p)
    fr = LC.DUMMY_FRAME
    try:
        _both(lib, h, r, _grid(5), fr, "five")
        assert _both(lib, h, r, _grid(8, 2.0, 1.0), fr, "five matched and three new fill the handle") == [1, 2, 3, 4, 5, 6, 7, 8]
        got = LC.device_scripted(lib, _capi, h, r.pts + F32(1.5), np.array([1, 0, 1, 1, 0, 1, 1, 1], np.uint8))
        _recs_same(got, r.interpolate(r.pts + F32(1.5), np.array([1, 0, 1, 1, 0, 1, 1, 1])), "scripted")
        before = _same(r, lib, h, "before the refusals")
        assert before.n_points == 6
        rc, _ = LC.device_update(lib, _capi, h, _grid(9, 3.0, 1.0), fr)           # eight matched, the ninth finds no room
        assert rc == _capi.OPD_EINVAL and "max_tracks = 8" in _capi.last_error()
        _same(r, lib, h, "after an update that did not fit")
        rc, _ = LC.device_update(lib, _capi, h, _grid(10), fr)                    # ten detections, room for nine
        assert rc == _capi.OPD_EINVAL and "max_dets = 9" in _capi.last_error()
        rc, _ = LC.device_update(lib, _capi, h, _grid(2), None)                   # optical flow, no frame
        assert rc == _capi.OPD_EINVAL and "null frame" in _capi.last_error()
        big = np.zeros((25, 32, 3), np.uint8)
        rc, _ = LC.device_update(lib, _capi, h, _grid(2), big)                    # a frame larger than the handle was made for
        assert rc == _capi.OPD_EINVAL
        n = C.c_int()
        assert lib.opd_lwt_interpolate(h, TC.ptr(fr), 0, 24, 32, (_capi.OpdLwtRec * 2)(), 2, C.byref(n)) == _capi.OPD_EINVAL and n.value == 8
        _same(r, lib, h, "after every refusal")
        # the points are still the six followed ones: the next scripted frame takes six results
        got = LC.device_scripted(lib, _capi, h, r.pts - F32(0.25), np.ones(6, np.uint8))
        _recs_same(got, r.interpolate(r.pts - F32(0.25), np.ones(6, np.uint8)), "scripted after the refusals")
        _same(r, lib, h, "scripted after the refusals")
        _capi.check(lib.opd_lwt_reset(h), "opd_lwt_reset")
        r.reset()
        info = _same(r, lib, h, "reset")
        assert (info.max_tracks, info.max_dets, info.max_age, info.use_optical_flow, info.iou_threshold) == (8, 9, 30, 1, 0.3)
        assert _both(lib, h, r, _grid(3), fr, "after reset") == [1, 2, 3]
    finally:
        lib.opd_lwt_destroy(h)


# ---- 3. the fused interpolate on real frames ---------------------------------------------------------------------------------------------
def _three_frames(hh, ww, seed):
    """A structured frame and two more, each the one before moved by an integer shift (flow_common.structured_pair's construction)."""
    f0, f1 = FC.structured_pair(hh, ww, seed, (2, 1))
    ys, xs = np.clip(np.arange(hh) - 2, 0, hh - 1), np.clip(np.arange(ww) - 1, 0, ww - 1)
    f2 = f1[ys][:, xs].copy()
    y0, y1, x0, x1 = FC.flat_rect(hh, ww)
    f2[y0:y1, x0:x1] = FC.FLAT_BGR
    return f0, f1, np.ascontiguousarray(f2)


def _boxes_21(hh, ww):
    """21 boxes whose centres lie on a 7 x 3 grid inside the frame; the flat rectangle holds some of them (points LK loses)."""
    cx, cy = np.meshgrid(np.linspace(ww * 0.12, ww * 0.88, 7), np.linspace(hh * 0.2, hh * 0.8, 3))
    c = np.round(np.stack([cx.ravel(), cy.ravel()], 1) * 4) / 4
    y0, y1, x0, x1 = FC.flat_rect(hh, ww)
    c[0] = [(x0 + x1) / 2.0, (y0 + y1) / 2.0]   # no texture: LK loses it
    w, h = 8.0 + 0.5 * (np.arange(21) % 4), 12.0 + 0.25 * (np.arange(21) % 3)
    return np.stack([c[:, 0] - w / 2, c[:, 1] - h / 2, w, h], 1).astype(F32)


@pytest.mark.parametrize("hw,seed,on_device,flow_cfg", [((97, 131), 501, False, {}), ((97, 131), 501, True, {}), ((720, 1280), 502, False, {}),
                                                        ((97, 131), 501, False, dict(win=9, max_level=5))],
                         ids=["hw0-501-False", "hw1-501-True", "hw2-502-False", "hw0-501-False-win9-level5"])   # (the first three: their ids from before flow_cfg)
def test_fused_interpolate_equals_flow_track_fed_into_the_restatement(lib, hw, seed, on_device, flow_cfg):
    """``flow_cfg``: fields of opd_lwt_config.flow other than the defaults (window 21, max_level 3), given to the tracker and to the
    stand-alone flow handle alike."""
    hh, ww = hw
    top = FC.top_level(hh, ww, flow_cfg.get("win", 21), flow_cfg.get("max_level", 3))
    assert top == {(97, 131, 21): 2, (720, 1280, 21): 3, (97, 131, 9): 3}[(hh, ww, flow_cfg.get("win", 21))]
    frames = _three_frames(hh, ww, seed)
    keep = [torch.from_numpy(f).to("cuda") for f in frames] if on_device else None
    torch.cuda.synchronize()
    arg = (lambda i: (keep[i].data_ptr(), hh, ww)) if on_device else (lambda i: frames[i])
    p = dict(max_age=30, iou_threshold=0.3, use_optical_flow=True)
    r = LC.Restatement(**p)
    h = LC.create(lib, _capi, max_tracks=32, max_dets=32, max_h=hh, max_w=ww, flow=flow_cfg, **p)
    flow = FC.flow_create(lib, hh, ww, max_points=32, **flow_cfg)
    try:
        boxes = _boxes_21(hh, ww)
        rc, ids = LC.device_update(lib, _capi, h, boxes, arg(0))
        assert rc == 0 and ids.tolist() == r.update(boxes) == list(range(1, 22)), _capi.last_error()
        FC.flow_set_reference(lib, flow, frames[0])
        lost_total = 0
        for i in (1, 2):   # two consecutive in-between frames: the second starts from the first one's compacted points
            n_before = len(r.pt_ids)
            nxt, status = FC.flow_track(lib, flow, frames[i], r.pts)
            got = LC.device_interpolate(lib, _capi, h, arg(i))
            _recs_same(got, r.interpolate(nxt, status), (i, "records"))
            info = _same(r, lib, h, (i, "states"))
            assert info.last_waits == 1 and info.last_launches == 1 + top + 1 + 1   # gray, one launch per pyramid level above 0, LK, the tracks
            assert info.n_points == int((status == 1).sum()) <= n_before
            lost_total += n_before - info.n_points
        assert 0 < lost_total < 21 and 0 < len(r.pt_ids)   # points were lost (the flat rectangle) and the compacted list carried over
        assert any(tr["tsu"] == 2 for tr in r.tracks) and any(tr["tsu"] == 0 and tr["hits"] == 3 for tr in r.tracks)
        # the next detection frame makes the frame the new reference and every detection a point again
        b2 = boxes + np.array([1.0, 1.0, 0.0, 0.0], F32)
        rc, ids = LC.device_update(lib, _capi, h, b2, arg(2))
        want = r.update(b2)   # (a point LK carried away from its box leaves a track that no longer matches: a new id, here as there)
        assert rc == 0 and ids.tolist() == want and sum(i <= 21 for i in want) >= 15, (ids, want)
        assert _same(r, lib, h, "second detection frame").n_points == 21
    finally:
        lib.opd_lwt_destroy(h)
        lib.opd_flow_destroy(flow)


def test_a_refused_update_leaves_the_reference_usable_on_real_pixels(lib):
    """An update the kernel refuses has built its frame's pyramid (of ITS size and level count) into the slot the flow handle's reference
    does not use and never reaches the finish: handle A, which sees refused updates -- one of the reference's size (97 x 131, three
    levels), one after a frame of another size (64 x 80, two levels) -- and handle B, which sees only the accepted calls, agree bit for
    bit in LK's interpolation of real frames, in every number of every track and in opd_lwt_info."""
    f0, f1 = FC.structured_pair(97, 131, 503, (2, 1))
    g0, g1 = FC.structured_pair(64, 80, 504, (1, 1))
    four = np.array([[56, 43, 12, 14], [61, 14, 10, 12], [90, 20, 14, 16], [100, 60, 12, 18]], F32)   # the first two lie inside 64 x 80 as well
    five = np.concatenate([four, np.array([[20, 70, 10, 12]], F32)])                                  # ... and one box that overlaps none
    p = dict(max_age=30, iou_threshold=0.3, use_optical_flow=True)

    def observe(h):
        st = LC.info(lib, _capi, h)
        return [a.tobytes() for a in LC.device_states(lib, _capi, h)], tuple(getattr(st, n) for n, _ in st._fields_)

    def run(refusals):
        h = LC.create(lib, _capi, max_tracks=4, max_dets=5, max_h=97, max_w=131, **p)
        seen = []

        def refused():
            rc, _ = LC.device_update(lib, _capi, h, five, f1)
            assert rc == _capi.OPD_EINVAL and "max_tracks = 4" in _capi.last_error(), _capi.last_error()

        def interpolate(frame):
            recs = LC.device_interpolate(lib, _capi, h, frame)
            seen.append(([q[0] for q in recs], np.array([q[1] for q in recs], F64).tobytes(), observe(h)))
            return LC.info(lib, _capi, h).n_points

        try:
            rc, ids = LC.device_update(lib, _capi, h, four, f0)
            assert rc == 0 and ids.tolist() == [1, 2, 3, 4], _capi.last_error()
            if refusals:
                refused()
            assert 0 < interpolate(f1) <= 4   # LK ran against f0's pyramid and followed points
            rc, ids = LC.device_update(lib, _capi, h, four[:2], g0)
            assert rc == 0 and ids.tolist() == [1, 2], _capi.last_error()
            if refusals:
                refused()   # (97 x 131 into the other slot: the reference's 64 x 80 geometry is its own)
            assert 0 < interpolate(g1) <= 2
            n = C.c_int()   # and a frame that is not the reference's size is refused with the reference's size in the text, here as there
            ptr, kind, fh, fw = LC._frame_args(f1)
            assert lib.opd_lwt_interpolate(h, ptr, kind, fh, fw, (_capi.OpdLwtRec * 4)(), 4, C.byref(n)) == _capi.OPD_EINVAL
            seen.append((_capi.last_error(), observe(h)))
            assert "the reference has 64 x 80" in seen[-1][0]
            return seen
        finally:
            lib.opd_lwt_destroy(h)

    a, b = run(True), run(False)
    assert len(a) == len(b) == 3
    for k, (x, y) in enumerate(zip(a, b)):
        assert x == y, k


# ---- 4. independence ----------------------------------------------------------------------------------------------------------------------
def test_a_track_does_not_depend_on_the_others_or_on_its_row(lib):
    p = dict(max_age=30, iou_threshold=0.3, use_optical_flow=True)

    def walker(f):
        return np.array([900.25 + 2.75 * f, 700.5 - 1.5 * f, 60.0, 150.5], F32)

    def run(crowd):
        h = LC.create(lib, _capi, max_tracks=192, max_dets=64, **p)
        out = []
        try:
            for f in range(12):
                others = list(_grid(40, 1.5 * f, 0.5 * f, cols=8)[:, :]) if crowd else []
                if f % 4 == 0:
                    if f == 8:
                        boxes = np.array(others, F32).reshape(-1, 4)    # the walker is not detected on frame 8: predicted
                    else:
                        boxes = np.array(others + [walker(f)], F32).reshape(-1, 4)    # the walker is the LAST detection: the last row
                    rc, ids = LC.device_update(lib, _capi, h, boxes, LC.DUMMY_FRAME)
                    assert rc == 0, _capi.last_error()
                    wid = int(ids[-1]) if f == 0 else wid
                    recs = None
                else:
                    n = LC.info(lib, _capi, h).n_points
                    nxt = np.array([[5.25 + 3.0 * j, 7.5 + 2.0 * j] for j in range(n)], F32).reshape(n, 2)
                    status = (np.arange(n) % 3 != 1).astype(np.uint8)
                    if n and f < 8:    # the walker's point is the last one of the list; it is followed except on frame 7
                        c = walker(f)
                        nxt[-1] = [c[0] + c[2] / 2 + 0.25, c[1] + c[3] / 2 - 0.5]
                        status[-1] = f != 7
                    recs = LC.device_scripted(lib, _capi, h, nxt, status)
                tr = [t for t in LC.device_tracks(lib, _capi, h) if t.track_id == wid][0]
                out.append((np.array(list(tr.x)).view(np.uint64).tolist(), np.array(list(tr.P), F32).view(np.uint32).tolist(), list(tr.bbox), list(tr.center),
                            (tr.age, tr.hits, tr.time_since_update, tr.x_is_float32), None if recs is None else [q[1] for q in recs if q[0] == wid]))
            return wid, out
        finally:
            lib.opd_lwt_destroy(h)

    (id_alone, alone), (id_crowd, crowd) = run(False), run(True)
    assert (id_alone, id_crowd) == (1, 41)
    for f, (a, b) in enumerate(zip(alone, crowd)):
        assert a == b, f
    assert alone[-1][4][3] == 0 and alone[1][4][3] == 1   # float32 until the first detection-frame match, float64 after it


# ---- 5. the class -------------------------------------------------------------------------------------------------------------------------
def _dets(boxes):
    return [Detection(bbox=tuple(float(v) for v in b), confidence=0.9, class_id=1, class_name="person", camera_coords=(0.0, 0.0)) for b in boxes]


def test_hip_lightweight_tracker_against_the_recorded_sequence(golden):
    name = [n for n in LC.sequence_names(golden) if n.startswith("flowoff")][0]
    params, frames = LC.sequence(golden, name)
    bound, rec_bound = 8 * float(golden["kalman_tol"]), 8 * float(golden["record_tol"])
    t = HipLightweightTracker(max_tracks=16, **params)
    r = LC.Restatement(**params)
    try:
        for f, fr in enumerate(frames):
            if fr["kind"] == "det":
                dets = _dets(fr["boxes"])
                feat = np.full(4, f, F32)
                if dets:
                    dets[0].features = feat
                assert t.update_with_detections(None, dets) is dets
                assert [d.track_id for d in dets] == fr["ids"].tolist() == r.update(fr["boxes"]), f
                assert len(t._features) <= t.info().n_tracks, f   # the features of tracks that died are forgotten without anyone reading `tracks`
            else:
                got = t.interpolate(None)
                _recs_same(got, r.interpolate(), f)
                assert all(isinstance(v, float) for q in got for v in q[1]) and all(isinstance(q[0], int) for q in got)
                assert LC.records_equal(got, fr["rec_ids"], fr["rec_boxes"], fr["rec_followed"], rec_bound), f
            info = t.info()
            assert info.last_waits == 1 and info.last_launches == 1 and t.next_id == fr["next_id"], f
            tracks = t.tracks
            got = np.array([[q.track_id, q.age, q.hits, q.time_since_update] for q in tracks], np.int32).reshape(-1, 4)
            assert np.array_equal(got, fr["counters"]), f
            assert [q.track_id for q in t.get_active_tracks()] == [int(c[0]) for c in fr["counters"] if c[3] == 0]
        first = [q for q in t.tracks if q.track_id == int(frames[0]["ids"][0])]
        assert not first or np.array_equal(first[0].features, np.zeros(4, F32))   # a track keeps the features it was created with
        assert all(np.array_equal(q.center, tr["center"]) and q.bbox == tuple(float(v) for v in tr["bbox"]) for q, tr in zip(t.tracks, r.tracks))
        t.reset()
        assert t.tracks == [] and t.next_id == 1 and t.interpolate(None) == []
        dets = _dets(frames[0]["boxes"])
        t.update_with_detections(None, dets)
        assert [d.track_id for d in dets] == frames[0]["ids"].tolist()
    finally:
        t.close()


def test_hip_lightweight_tracker_with_optical_flow_on_host_and_device_frames(lib):
    hh, ww = 97, 131
    frames = _three_frames(hh, ww, 501)
    boxes = _boxes_21(hh, ww)
    runs = []
    for on_device in (False, True):
        t = HipLightweightTracker(max_tracks=32)
        try:
            fr = [torch.from_numpy(f).to("cuda") for f in frames] if on_device else frames
            dets = _dets(boxes)
            t.update_with_detections(fr[0], dets)
            assert [d.track_id for d in dets] == list(range(1, 22)) and t.info().n_points == 21
            recs = [t.interpolate(fr[1]), t.interpolate(fr[2])]
            assert t.info().last_waits == 1 and 0 < t.info().n_points < 21
            runs.append((recs, [(q.track_id, q.bbox, q.hits, q.time_since_update) for q in t.tracks]))
            with pytest.raises(RuntimeError, match="pixels"):
                t.interpolate(np.zeros((hh - 1, ww, 3), np.uint8))   # not the size of the reference frame
        finally:
            t.close()
    assert runs[0] == runs[1]
