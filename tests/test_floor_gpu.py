"""The floor map on the device: ``opd_floor_transform`` / ``_points`` / ``_classify`` and ``opd_detr_detect_frames_floor`` against the
fixture (tests/golden/floor_maps.npz, written by tools/gen_floor_golden.py) and the numpy restatement in floor_common.py.

The bound.  Decisions (flags, triangle, zone mask) must equal the fixture's on every point: the generator kept only points whose
decisions are clear.  Coordinates must lie within 4 e64 + 4 ulp(max |coordinate| of the case) of the long-double truth: e64 is the float64
restatement's own distance from it, and a fixed-order wave sum and the device's log / sqrt may each move a result by about what float64
itself does, not more.  Integer points on integer polygons make every operation of the ray cast exact: bit-identical masks."""

import ctypes as C
import faulthandler

import numpy as np
import pytest
import torch

import floor_common as F
from office_person_detection_vit_amd import HipDetrDetector, HipFloorMapper, _capi
from office_person_detection_vit_amd import floor as FL
from office_person_detection_vit_amd.frames import structured_frames
from office_person_detection_vit_amd.weights import DetrArch, ensure_weight_file

pytestmark = pytest.mark.gpu

PERSON = 1
FM = (1878, 1369, 28.1926406926406, 28.241430700447)
ZONES = [{"id": "zone_1", "polygon": [[859, 912], [1095, 912], [1095, 1350], [859, 1350]], "priority": 1},
         {"id": "zone_2", "polygon": [[1095, 912], [1331, 912], [1331, 1350], [1095, 1350]], "priority": 2},
         {"id": "zone_3", "polygon": [[1331, 912], [1567, 912], [1567, 1350], [1331, 1350]], "priority": 3}]
H = [[-0.8795888447, -2.8974379541, 417.8510123786], [-1.5459702925, -3.4570021203, 1054.0107447082], [-0.0011928509, -0.0035480452, 1.0]]


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
    return np.load(F.GOLDEN)


def _inputs(golden, name):
    boxes, pts = golden[f"{name}_boxes"], golden[f"{name}_pts"]
    return dict(boxes=boxes) if len(boxes) else dict(pts=pts)


@pytest.mark.parametrize("name", F.case_names(np.load(F.GOLDEN)))
def test_fixture_cases_on_the_device(lib, golden, name):
    model = F.case_model(golden, name)
    h = F.create(lib, model)
    try:
        rec = F.device_transform(lib, h, **_inputs(golden, name))
        info = _capi.OpdFloorModelInfo()
        _capi.check(lib.opd_floor_info(h, C.byref(info)), "opd_floor_info")
    finally:
        lib.opd_floor_destroy(h)
    assert (info.method, info.n_zones, info.n_edges) == (model["method"], len(model["zones"]), sum(len(z) for z in model["zones"]))
    assert info.n_triangles == (len(model["triangles"]) if model["method"] == F.PWA else 0)
    truth, limit = golden[f"{name}_truth_px"], F.bound(golden, name)
    d = float(np.abs(rec["px"] - truth).max())
    d64 = float(np.abs(rec["px"] - F.run(model, **_inputs(golden, name))[0]).max())
    print(f"{name}: {len(rec)} records, max |device - truth| = {d:.3e} px (bound {limit:.3e}, e64 {float(golden[f'{name}_e64']):.3e}), "
          f"max |device - float64 restatement| = {d64:.3e}")
    assert np.array_equal(rec["flags"], golden[f"{name}_truth_flags"])
    assert np.array_equal(rec["triangle"], golden[f"{name}_truth_tri"])
    assert np.array_equal(rec["zone_mask"], golden[f"{name}_truth_mask"])
    assert d <= limit
    assert np.array_equal(rec["mm"], rec["px"] * np.asarray(model["fm"][2:4]))   # one multiplication each: the same bits


def test_undistortion_round_trip(lib, golden):
    """The device's undistorted points, seen through a map that hands them back (a one-triangle piecewise affine with the identity
    matrix), re-distorted with the forward model: within the restatement's own round-trip residual + 1e-9 px of the inputs."""
    name = "pwa_distortion"
    dist, pts = golden[f"{name}_dist"], golden[f"{name}_pts"]
    ident = {"method": F.PWA, "points": np.array([[0, 0], [2000.0, 0], [0, 2000.0]]), "triangles": np.array([[0, 1, 2]], np.int32),
             "affine": np.array([[1.0, 0, 0, 0, 1, 0]]), "dist": dist, "fm": np.asarray(FM), "zones": [], "priority": np.zeros(0), "allow_overlap": False}
    h = F.create(lib, ident)
    try:
        rec = F.device_transform(lib, h, pts=pts)
    finally:
        lib.opd_floor_destroy(h)
    ux, uy = F.undistort(pts[:, 0], pts[:, 1], dist)
    print(f"undistortion: max |device - restatement| = {max(np.abs(rec['px'][:, 0] - ux).max(), np.abs(rec['px'][:, 1] - uy).max()):.3e} px")
    rx, ry = F.distort(rec["px"][:, 0], rec["px"][:, 1], dist)
    resid = max(np.abs(rx - pts[:, 0]).max(), np.abs(ry - pts[:, 1]).max())
    e_rt = float(golden[f"{name}_e_rt"])
    print(f"undistortion: round trip {resid:.3e} px, the restatement's own {e_rt:.3e} px")
    assert resid <= e_rt + 1e-9


@pytest.mark.parametrize("allow_overlap", [False, True])
def test_zone_ties_on_integer_points(lib, allow_overlap):
    """Vertices, horizontal and vertical edges and the shared edge x = 1095 of the configuration's integer polygons: every operation of
    the ray cast is exact there, so the masks are the restatement's bit for bit, `<=` / `>` asymmetries included."""
    model = FL.model_homography(H, FM, ZONES, allow_overlap=allow_overlap)
    xs = [858, 859, 860, 1094, 1095, 1096, 1330, 1331, 1332, 1566, 1567, 1568, 977, 1213]
    ys = [911, 912, 913, 1131, 1349, 1350, 1351]
    pts = np.array([(x, y) for x in xs for y in ys], np.float64)
    h = F.create(lib, model)
    try:
        got = F.device_classify(lib, h, pts)
    finally:
        lib.opd_floor_destroy(h)
    want = F.classify(model, pts[:, 0], pts[:, 1])
    assert np.array_equal(got, want), pts[got != want]
    on = dict(zip(map(tuple, pts.astype(int)), got))
    # a polygon's right and bottom edges belong to it, its left and top edges do not: the shared edge x = 1095 is zone_1's alone
    assert on[(1095, 1131)] == 1 and on[(859, 1131)] == 0 and on[(1331, 1131)] == 2 and on[(1567, 1131)] == 4
    assert on[(977, 912)] == 0 and on[(977, 1350)] == 1 and on[(859, 912)] == 0 and on[(1567, 1350)] == 4
    assert set(got.tolist()) == {0, 1, 2, 4}


@pytest.mark.parametrize("name", ["homography_config", "pwa_t_big", "tps_n65", "pwa_distortion"])
def test_rows_do_not_depend_on_the_batch(lib, golden, name):
    model = F.case_model(golden, name)
    kw = _inputs(golden, name)
    key, data = next(iter(kw.items()))
    h = F.create(lib, model)
    try:
        full = F.device_transform(lib, h, **{key: data})
        assert np.array_equal(full, F.device_transform(lib, h, **{key: data}))             # a second run
        perm = np.random.default_rng(3).permutation(len(data))
        assert np.array_equal(F.device_transform(lib, h, **{key: data[perm]}), full[perm])
        for n in (1, 3, 4, 5, 63, 64, 65):
            assert np.array_equal(F.device_transform(lib, h, **{key: data[:n]}), full[:n]), n
        for k in (0, 7, 64, len(data) - 1):                                                 # alone
            assert np.array_equal(F.device_transform(lib, h, **{key: data[k:k + 1]})[0], full[k]), k
        masks = F.device_classify(lib, h, full["px"])                                       # classify_batch on the floor points: the same zones
        assert np.array_equal(masks, full["zone_mask"])
        if key == "boxes":                                                                  # boxes read in place from device memory
            dev = torch.from_numpy(np.ascontiguousarray(data)).cuda()
            torch.cuda.synchronize()
            out = np.zeros(len(data), F.REC_DTYPE)
            _capi.check(lib.opd_floor_transform(h, C.c_void_p(dev.data_ptr()), len(data), _capi.OPD_MEM_DEVICE, out.ctypes.data), "opd_floor_transform")
            assert np.array_equal(out, full)
            assert lib.opd_floor_transform(h, data.ctypes.data, len(data), _capi.OPD_MEM_DEVICE, out.ctypes.data) == _capi.OPD_EINVAL
            assert "not device-accessible" in _capi.last_error()                            # a host pointer is refused, not read
        # nothing to do is not an error; bad arguments are
        assert lib.opd_floor_transform(h, None, 0, _capi.OPD_MEM_HOST, None) == _capi.OPD_OK
        assert lib.opd_floor_transform_points(h, None, 0, None) == _capi.OPD_OK and lib.opd_floor_classify(h, None, 0, None) == _capi.OPD_OK
        assert lib.opd_floor_transform(h, None, 1, _capi.OPD_MEM_HOST, full.ctypes.data) == _capi.OPD_EINVAL and "null input" in _capi.last_error()
        assert lib.opd_floor_transform(h, full.ctypes.data, -1, _capi.OPD_MEM_HOST, full.ctypes.data) == _capi.OPD_EINVAL
        assert lib.opd_floor_transform(h, full.ctypes.data, 1, 2, full.ctypes.data) == _capi.OPD_EINVAL and "mem_kind" in _capi.last_error()
    finally:
        lib.opd_floor_destroy(h)


def test_staging_pair_regrown_between_calls(lib, golden):
    """A handle's staging pair starts at 256 records: 8 points, then 300 (the pair is freed and allocated anew), then the 8 again.  The
    shared rows are the same bits in all three calls, and the 300 rows meet the fixture test's comparison."""
    name = "tps_n65"
    model, pts = F.case_model(golden, name), golden[f"{name}_pts"]
    assert len(pts) == 300
    h = F.create(lib, model)
    try:
        small = F.device_transform(lib, h, pts=pts[:8])
        big = F.device_transform(lib, h, pts=pts)
        again = F.device_transform(lib, h, pts=pts[:8])
    finally:
        lib.opd_floor_destroy(h)
    assert small.tobytes() == big[:8].tobytes() == again.tobytes()
    px, tri, flags, masks = F.run(model, pts=pts)
    d, limit = float(np.abs(big["px"] - px).max()), F.bound(golden, name)
    print(f"{name} across a regrow: max |device - float64 restatement| = {d:.3e} px (bound {limit:.3e})")
    assert np.array_equal(big["flags"], flags) and np.array_equal(big["triangle"], tri) and np.array_equal(big["zone_mask"], masks)
    assert d <= limit
    assert np.array_equal(big["mm"], big["px"] * np.asarray(model["fm"][2:4]))


def test_two_mappers_on_one_device(lib, golden):
    a_model, b_model = F.case_model(golden, "pwa_t_mid"), F.case_model(golden, "tps_n64")
    a_in, b_in = _inputs(golden, "pwa_t_mid"), _inputs(golden, "tps_n64")
    a = F.create(lib, a_model)
    alone = F.device_transform(lib, a, **a_in)
    b = F.create(lib, b_model)
    try:
        b_first = F.device_transform(lib, b, **b_in)
        for _ in range(3):   # used alternately: each gives what it gives alone
            assert np.array_equal(F.device_transform(lib, a, **a_in), alone)
            assert np.array_equal(F.device_transform(lib, b, **b_in), b_first)
        lib.opd_floor_destroy(a)
        a = None
        assert np.array_equal(F.device_transform(lib, b, **b_in), b_first)   # destroying one leaves the other working
        assert np.array_equal(b_first["triangle"], np.full(len(b_first), -1)) and np.array_equal(b_first["zone_mask"], golden["tps_n64_truth_mask"])
    finally:
        lib.opd_floor_destroy(b)
        if a is not None:
            lib.opd_floor_destroy(a)


def _frames(n, h, w, seed):
    return [np.ascontiguousarray(f).copy() for f in structured_frames(n, h, w, seed=seed)]


def _sig(d):
    return (d.query_index, d.bbox, d.confidence, d.camera_coords, d.floor_coords, d.floor_coords_mm, tuple(d.zone_ids))


def test_fused_call_rows_equal_the_standalone_call(lib, weight_cache):
    hw = (180, 320)
    path = ensure_weight_file(weight_cache, DetrArch(), 0, 1.0, "r50")
    det = HipDetrDetector(model_path=path, max_batch=2, max_size=(288, 512), resize=True, confidence_threshold=0.05)
    det.load_model()
    rng = np.random.default_rng(9)
    src = np.concatenate([np.array([[0, 0], [320, 0], [0, 180], [320, 180]], float), rng.uniform((10, 10), (310, 170), (20, 2))])
    dst = np.stack([5.5 * src[:, 0] + 40 + 15 * np.sin(src[:, 1] / 40.0), 7.0 * src[:, 1] + 30 + 10 * np.cos(src[:, 0] / 50.0)], 1)
    mapper = HipFloorMapper.piecewise_affine(src, dst, FM, ZONES)
    try:
        Q = det.num_queries
        pair = _frames(2, hw[0], hw[1], seed=43)
        ptrs = (C.c_void_p * 2)(*[f.ctypes.data for f in pair])
        plain, pcounts = (_capi.OpdDet * (2 * Q))(), (C.c_int32 * 2)()
        _capi.check(lib.opd_detr_detect_frames(C.c_void_p(det.model), ptrs, _capi.OPD_MEM_HOST, 2, hw[0], hw[1], 288, 512, 0.05, plain, pcounts), "detect_frames")
        labels = [r.label for b in range(2) for r in plain[b * Q:b * Q + int(pcounts[b])]]
        assert labels, "the test frames give no record at threshold 0.05: nothing to compare"
        total = 0
        for label in sorted({PERSON, max(set(labels), key=labels.count)}):
            recs, counts = (_capi.OpdDet * (2 * Q))(), (C.c_int32 * 2)()
            floor = np.frombuffer(bytearray(b"\xa5" * (2 * Q * 48)), F.REC_DTYPE)            # poisoned: untouched rows stay as they are
            poison = floor[0].copy()
            _capi.check(lib.opd_detr_detect_frames_floor(C.c_void_p(det.model), mapper._require(), ptrs, 2, hw[0], hw[1], 288, 512, 0.05, label, recs, counts,
                                                         floor.ctypes.data), "opd_detr_detect_frames_floor")
            assert list(counts) == list(pcounts) and bytes(recs) == bytes(plain)             # records and counts: what opd_detr_detect_frames gives
            written = set()
            for b in range(2):
                for r in recs[b * Q:b * Q + int(counts[b])]:
                    if r.label != label:
                        continue
                    bbox = (float(r.x1), float(r.y1), float(r.x2 - r.x1), float(r.y2 - r.y1))   # Detection.bbox as the shim derives it
                    want = mapper.transform_records([bbox])[0]
                    assert floor[b * Q + r.query_index] == want, (b, r.query_index)
                    assert want["flags"] & F.VALID
                    written.add(b * Q + r.query_index)
            total += len(written)
            rest = np.setdiff1d(np.arange(2 * Q), sorted(written))
            assert (floor[rest] == poison).all()
        assert total >= 1
        # the Python surface: the fused path, the chunked path and the ragged fall-back all equal detect + apply
        frames = _frames(3, hw[0], hw[1], seed=41)
        want = det.detect_batch(frames)
        assert all(d.floor_coords is None and d.zone_ids == [] for ds in want for d in ds)  # without a mapper nothing changes
        for ds in want:
            mapper.apply(ds)
        got = det.detect_batch(frames, floor_map=mapper)
        assert [[_sig(d) for d in ds] for ds in got] == [[_sig(d) for d in ds] for ds in want]
        assert sum(len(ds) for ds in got) >= 1 and all(d.floor_coords is not None for ds in got for d in ds)
        one = det.detect(frames[0], floor_map=mapper)
        assert [_sig(d) for d in one] == [_sig(d) for d in want[0]]
        ragged = [frames[0], _frames(1, 144, 320, seed=5)[0]]
        want_r = det.detect_batch(ragged)
        for ds in want_r:
            mapper.apply(ds)
        assert [[_sig(d) for d in ds] for ds in det.detect_batch(ragged, floor_map=mapper)] == [[_sig(d) for d in ds] for ds in want_r]
        counts_by_zone = HipFloorMapper.zone_counts([d for ds in got for d in ds])
        assert sum(counts_by_zone.values()) >= sum(len(ds) for ds in got)
        # refusals of the fused call
        recs, counts, floor = (_capi.OpdDet * (2 * Q))(), (C.c_int32 * 2)(), np.zeros(2 * Q, F.REC_DTYPE)
        fn = lib.opd_detr_detect_frames_floor
        assert fn(C.c_void_p(det.model), None, ptrs, 2, hw[0], hw[1], 288, 512, 0.05, PERSON, recs, counts, floor.ctypes.data) == _capi.OPD_EINVAL
        assert "null floor-map handle" in _capi.last_error()
        assert fn(C.c_void_p(det.model), mapper._require(), ptrs, 2, hw[0], hw[1], 288, 512, 0.05, PERSON, recs, counts, None) == _capi.OPD_EINVAL
        assert "null output buffer" in _capi.last_error()
    finally:
        mapper.close()
        det.close()
