"""GPU tests of tiled detection in one native call (-m gpu): ``tile_merge_kernel`` through ``opd_detr_merge_tiles`` on every case of
tests/tile_common.py, ``tile_resize_u8_kernel`` against the contiguous resize, ``opd_detr_detect_tiled`` /
``TiledDetector(native=True)`` end to end against the host path on the same detector, the refusals that need a handle, and that a tiled
call leaves the handle as it was.  Everything here is an equality."""

import ctypes as C
import faulthandler

import numpy as np
import pytest

import tile_common as T
from office_person_detection_vit_amd import HipDetrDetector, TiledDetector, _capi
from office_person_detection_vit_amd.detector import resize_frame
from office_person_detection_vit_amd.frames import structured_frames
from office_person_detection_vit_amd.tiling import split_tiles, tile_grid
from office_person_detection_vit_amd.weights import DetrArch, ensure_weight_file

pytestmark = pytest.mark.gpu

THRESHOLD = 0.05
CASES = T.cases()
FRAME_HW = (192, 256)
SEEDS = (5, 6, 7)   # structured frames on which the `sharp` detector's tiles give boxes that the seam merge absorbs (asserted below)


@pytest.fixture(autouse=True)
def _time_limit():
    """Every test runs under its own limit: a hang ends the process (with a traceback) instead of holding the GPU."""
    faulthandler.dump_traceback_later(300, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def lib():
    return _capi.load_library(test_hooks=True)


@pytest.fixture(scope="module")
def det(weight_cache, lib):
    d = HipDetrDetector(model_path=ensure_weight_file(weight_cache, DetrArch(), 0, 1.0, "r50"), max_batch=8, max_size=(256, 320), resize=True,
                        confidence_threshold=THRESHOLD)
    d.load_model()
    yield d
    d.close()


@pytest.fixture(scope="module")
def sharp(weight_cache, lib):
    """The same detector on the seeded weights with attention gain 2 (tests/test_workloads_gpu.py's `sharp` set).  On the gain-1 weights the
    per-tile suppression leaves ONE box per tile, on every frame seed tried, and the seam merge has nothing to absorb; on these a tile
    keeps 1 to 4 boxes and the merge absorbs about half of them, parts of one body across a seam among them."""
    d = HipDetrDetector(model_path=ensure_weight_file(weight_cache, DetrArch(), 0, 2.0, "r50"), max_batch=8, max_size=(256, 320), resize=True,
                        confidence_threshold=THRESHOLD)
    d.load_model()
    yield d
    d.close()


def _frames(n, seed, hw=FRAME_HW):
    return [np.ascontiguousarray(f).copy() for f in structured_frames(n, hw[0], hw[1], seed=seed)]


def _fields(d):
    return (d.bbox, d.confidence, d.class_id, d.class_name, d.camera_coords, d.floor_coords, d.floor_coords_mm, tuple(d.zone_ids), d.track_id,
            None if d.features is None else np.asarray(d.features).tobytes(), d.appearance_score, d.query_index)


def _same(a, b, what):
    assert len(a) == len(b), what
    for f, (x, y) in enumerate(zip(a, b)):
        assert [_fields(d) for d in x] == [_fields(d) for d in y], f"{what}: frame {f}"


# ---- 1. the merge kernel alone -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_merge_kernel_equals_the_python_rule(lib, det, case):
    rc, out, counts = T.run(lib.opd_detr_merge_tiles, case, handle=det.model)
    assert rc == _capi.OPD_OK, _capi.last_error()
    T.assert_same(case, out, counts, T.expected(case))


def test_merge_kernel_reports_a_count_above_the_stride(lib, det):
    base = next(c for c in CASES if c["name"] == "three_frames")
    case = dict(base, counts=base["counts"].copy())
    case["counts"][5] = case["stride"] + 1   # frame 1
    rc, out, counts = T.run(lib.opd_detr_merge_tiles, case, handle=det.model)
    assert rc == _capi.OPD_EINVAL and "more records than its slots" in _capi.last_error()
    want = T.expected(base)
    assert counts.tolist() == [len(want[0]), 0, len(want[2])]
    rc, out, counts = T.run(lib.opd_detr_merge_tiles, base, handle=det.model)   # the flag does not stick
    assert rc == _capi.OPD_OK
    T.assert_same(base, out, counts, want)


# ---- 2. the tile resize ------------------------------------------------------------------------------------------------------------------
RESIZE = [("2x2_down", (40, 52), tile_grid(40, 52, 2, 2, 0.125), (16, 21), 1), ("2x2_up", (40, 52), tile_grid(40, 52, 2, 2, 0.125), (33, 44), 1),
          ("1x2_quarter", (37, 64), tile_grid(37, 64, 1, 2, 0.25), (33, 44), 1), ("1x2_quarter_b", (37, 64), tile_grid(37, 64, 1, 2, 0.25), (48, 36), 1),
          ("two_frames", (40, 52), tile_grid(40, 52, 2, 2, 0.125), (33, 44), 2), ("three_frames_same", (40, 52), tile_grid(40, 52, 2, 2, 0.125), (22, 29), 3),
          ("odd_pitch_windows", (37, 63), [(1, 5, 30, 41), (3, 17, 30, 41), (7, 22, 30, 41)], (45, 60), 2)]


@pytest.mark.parametrize("name,hw,tiles,out_hw,n_frames", RESIZE, ids=[r[0] for r in RESIZE])
def test_tile_resize_equals_the_resize_of_contiguous_copies(lib, det, name, hw, tiles, out_hw, n_frames):
    """Byte for byte opd_detr_resize_u8 on contiguous copies of the windows where that entry takes the output size (it refuses edges below 32),
    and Pillow's bilinear resize itself, which that entry is held to, for every size."""
    rng = np.random.RandomState(len(name) * 131 + n_frames)
    frames = rng.randint(0, 256, size=(n_frames, hw[0], hw[1], 3)).astype(np.uint8)
    frames[:, ::5, ::3] = 255   # (extremes next to each other: rounding and clipping)
    frames[:, 1::5, 1::3] = 0
    win = np.asarray(tiles, np.int32).reshape(-1, 4)
    assert len({(int(t[2]), int(t[3])) for t in win}) == 1
    n = n_frames * len(win)
    got = np.full((n, out_hw[0], out_hw[1], 3), 7, np.uint8)
    rc = lib.opd_test_tile_resize(frames.ctypes.data_as(C.c_void_p), n_frames, hw[0], hw[1], win.ctypes.data_as(C.c_void_p), len(win), out_hw[0], out_hw[1],
                                  got.ctypes.data_as(C.c_void_p))
    assert rc == _capi.OPD_OK, _capi.last_error()
    copies = np.stack([np.ascontiguousarray(frames[f, y:y + h, x:x + w]) for f in range(n_frames) for y, x, h, w in tiles])
    pil = np.stack([resize_frame(c, out_hw[0], out_hw[1]) for c in copies])
    assert np.array_equal(got, pil), f"{name}: {int((got != pil).sum())} bytes differ from Pillow"
    if min(out_hw) >= 32:
        ref = np.zeros_like(got)
        rc = lib.opd_detr_resize_u8(C.c_void_p(det.model), copies.ctypes.data_as(C.c_void_p), n, copies.shape[1], copies.shape[2], out_hw[0], out_hw[1],
                                    ref.ctypes.data_as(C.c_void_p))
        assert rc == _capi.OPD_OK, _capi.last_error()
        assert np.array_equal(got, ref), f"{name}: {int((got != ref).sum())} bytes differ from opd_detr_resize_u8"
    if name == "three_frames_same":   # the windows' own size: the identity
        assert np.array_equal(got, copies)


# ---- 3. end to end -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def reference(sharp):
    det = sharp
    """The host path on the same detector, once: the merged lists of the three frames and the per-tile lists they were merged from."""
    frames = [_frames(1, s)[0] for s in SEEDS]
    det.device_nms = False
    want = TiledDetector(det, native=False).detect_batch(frames)
    per_tile = [det.detect_batch(split_tiles(f, 2, 2, 0.125)[0]) for f in frames]
    return frames, want, per_tile


def test_reference_lists_show_an_absorption(reference):
    frames, want, per_tile = reference
    assert all(len(w) > 0 for w in want)
    assert any(len(w) < sum(len(t) for t in p) for w, p in zip(want, per_tile)), [(len(w), [len(t) for t in p]) for w, p in zip(want, per_tile)]
    widest = max(d.bbox[2] for p in per_tile for t in p for d in t)
    assert any(d.bbox[2] > widest + 1.0 for w in want for d in w), "no kept box has grown: the seam merge itself never happened"


def test_native_equals_the_host_path_on_the_mild_weights(det):
    frames = _frames(2, 5)
    host = TiledDetector(det, native=False).detect_batch(frames)
    assert all(len(h) > 0 for h in host)
    _same(TiledDetector(det, native=True).detect_batch(frames), host, "gain-1 weights")


@pytest.mark.parametrize("device_nms", [False, True], ids=["host_nms", "device_nms"])
@pytest.mark.parametrize("n", [1, 3], ids=["one_frame", "three_frames_two_chunks"])
def test_native_equals_the_host_path(sharp, reference, n, device_nms):
    det = sharp
    frames, want, _ = reference
    det.device_nms = device_nms
    try:
        host = TiledDetector(det, native=False).detect_batch(frames[:n])
        native = TiledDetector(det, native=True).detect_batch(frames[:n])
        again = TiledDetector(det, native=True).detect_batch(frames[:n])
    finally:
        det.device_nms = False
    _same(host, want[:n], "the host path, device_nms on and off")
    _same(native, host, "native against the host path")
    _same(again, native, "native, repeated")
    assert TiledDetector(det, native=True).detect(frames[0]) is not None


def test_native_equals_the_host_path_on_a_1x2_grid(sharp, reference):
    det = sharp
    frames = reference[0]
    host = TiledDetector(det, rows=1, cols=2, native=False).detect_batch(frames[:2])
    native = TiledDetector(det, rows=1, cols=2, native=True).detect_batch(frames[:2])
    assert all(len(h) > 0 for h in host)
    _same(native, host, "1 x 2 grid")


def test_native_with_other_thresholds(sharp, reference):
    det = sharp
    frames = reference[0]
    for kw in ({"nms_threshold": 1.0}, {"nms_threshold": 0.1, "merge_threshold": 0.2}):
        _same(TiledDetector(det, native=True, **kw).detect_batch(frames[:2]), TiledDetector(det, native=False, **kw).detect_batch(frames[:2]), str(kw))


def test_kernel_table_has_the_tiled_launches(det, reference):
    frames = reference[0]
    det.set_profiling(True)
    try:
        TiledDetector(det, native=True).detect_batch(frames[:1])
        rows = (_capi.OpdKernelStat * 256)()
        n = C.c_int()
        assert det._lib.opd_detr_kernel_table(C.c_void_p(det.model), rows, 256, C.byref(n)) == _capi.OPD_OK
        names = {rows[i].name.decode(): rows[i].launches for i in range(min(n.value, 256))}
    finally:
        det.set_profiling(False)
    for k in ("tile_resize_u8_kernel", "tile_merge_kernel", "person_nms_kernel"):
        assert names.get(k) == 1, (k, names)
    assert "resize_bilinear_u8_kernel" not in names


# ---- 4. refusals that need a handle ------------------------------------------------------------------------------------------------------
def test_refusals_with_a_handle(lib, det):
    frame = _frames(1, 3, (193, 256))[0]
    mixed = tile_grid(193, 256, 2, 2, 0.125)
    assert len({(t[2], t[3]) for t in mixed}) == 2
    with pytest.raises(ValueError, match="more than one size"):
        TiledDetector(det, native=True).detect_batch([frame])
    p = _capi.OpdTileParams(struct_size=C.sizeof(_capi.OpdTileParams), person_label=1, tile_nms_threshold=0.4, merge_nms_threshold=0.4, merge_threshold=0.5,
                            edge_tolerance=0.01)
    out, counts = (_capi.OpdTileDet * (16 * 100))(), (C.c_int32 * 4)()

    def refused(text, frames, tiles, h, w, H=240, W=320):
        win = np.asarray(tiles, np.int32).reshape(-1, 4)
        ptrs = (C.c_void_p * len(frames))(*[f.ctypes.data for f in frames])
        rc = lib.opd_detr_detect_tiled(C.c_void_p(det.model), ptrs, len(frames), h, w, win.ctypes.data_as(C.c_void_p), len(win), H, W, THRESHOLD, C.byref(p), out, counts)
        assert rc == _capi.OPD_EINVAL and text in _capi.last_error(), (text, _capi.last_error())

    refused("one forward has one model size", [frame], mixed, 193, 256)
    good, grid = _frames(3, 4), tile_grid(192, 256, 2, 2, 0.125)
    refused("max_batch", good, grid, 192, 256)                                      # 3 frames x 4 tiles > 8
    refused("1024 candidates", good[:1], tile_grid(192, 256, 3, 4, 0.0), 192, 256)  # 12 tiles x 100 queries
    refused("outside the configured maximum", good[:1], grid, 192, 256, H=512, W=640)
    refused("outside the configured maximum", good[:1], grid, 192, 256, H=16, W=320)
    with pytest.raises(ValueError, match="exceed max_batch"):
        det.detect_tiled(good[:1], tile_grid(192, 256, 3, 3, 0.0))


# ---- 5. the handle afterwards ------------------------------------------------------------------------------------------------------------
def test_a_tiled_call_leaves_the_handle_as_it_was(det, reference):
    frames = reference[0]
    plain = _frames(2, 11, (180, 320))
    for device_nms in (False, True):
        det.device_nms = device_nms
        try:
            before = det.detect_batch(plain)
            TiledDetector(det, native=True).detect_batch(frames[:2])
            after = det.detect_batch(plain)
        finally:
            det.device_nms = False
        assert all(len(b) > 0 for b in before)
        _same(after, before, f"detect_batch after a tiled call, device_nms={device_nms}")
