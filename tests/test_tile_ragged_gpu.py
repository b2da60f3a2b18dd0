"""GPU tests of native tiled detection for grids whose tiles differ in size (-m gpu): ``tile_resize_ragged_u8_kernel`` alone against the canvas
the host path builds, ``opd_detr_detect_tiled_ragged`` / ``HipDetrDetector.detect_tiled_ragged`` / ``TiledDetector(native=True, mixed_sizes=True)``
end to end against ``TiledDetector(native=False)`` on the same detector, a grid of one size through the new entry against
``opd_detr_detect_tiled``, the stages against the separate calls, the kernel table, the refusal that needs a handle, and the handle afterwards.
Everything here is an equality.

Every end-to-end case keeps to frame counts at which the host path's chunks of ``max_batch`` tiles hold whole frames (n_frames x n_tiles <=
max_batch, or max_batch a multiple of n_tiles): a host chunk with part of a frame gets a canvas of its own, and nothing establishes that its
forward gives the bits of the full canvas."""

import ctypes as C
import faulthandler

import numpy as np
import pytest

import tile_stages_common as TS
from office_person_detection_vit_amd import HipDetrDetector, HipFloorMapper, HipTracker, TiledDetector, _capi
from office_person_detection_vit_amd.detector import resize_frame
from office_person_detection_vit_amd.frames import structured_frames
from office_person_detection_vit_amd.tiling import split_tiles, tile_grid
from office_person_detection_vit_amd.weights import DetrArch, ensure_weight_file

pytestmark = pytest.mark.gpu

THRESHOLD = 0.05
ODD_HW, ODD_GRID = (193, 256), tile_grid(193, 256, 2, 2, 0.125)      # 108 x 144 and 109 x 144: a side that does not divide
STRIP_HW, STRIP_GRID = (96, 384), tile_grid(96, 384, 1, 3, 0.125)    # 96 x 144 and 96 x 160: an interior tile
NINE_HW, NINE_GRID = (192, 256), tile_grid(192, 256, 3, 3, 0.125)    # 3 x 3: six window sizes (the width does not divide either)
ODD_SEEDS, STRIP_SEEDS, NINE_SEED = (5, 6, 7), (6, 4), 9   # structured frames on which the `sharp` detector's host lists are non-empty and the seam merge grows a box (asserted below)
FM = (1878, 1369, 28.1926406926406, 28.241430700447)
ZONES = [{"id": "zone_1", "polygon": [[859, 912], [1095, 912], [1095, 1350], [859, 1350]], "priority": 1},
         {"id": "zone_2", "polygon": [[1095, 912], [1331, 912], [1331, 1350], [1095, 1350]], "priority": 2},
         {"id": "zone_3", "polygon": [[1331, 912], [1567, 912], [1567, 1350], [1331, 1350]], "priority": 3}]


@pytest.fixture(autouse=True)
def _time_limit():
    """Every test runs under its own limit: a hang ends the process (with a traceback) instead of holding the GPU."""
    faulthandler.dump_traceback_later(300, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def lib():
    return _capi.load_library(test_hooks=True)


def _detector(weight_cache, max_batch=8):
    """tests/test_tile_gpu.py's `sharp` detector: the seeded weights with attention gain 2, on which the seam merge absorbs boxes."""
    d = HipDetrDetector(model_path=ensure_weight_file(weight_cache, DetrArch(), 0, 2.0, "r50"), max_batch=max_batch, max_size=(256, 320), resize=True,
                        confidence_threshold=THRESHOLD)
    d.load_model()
    return d


@pytest.fixture(scope="module")
def sharp(weight_cache, lib):
    d = _detector(weight_cache)
    yield d
    d.close()


@pytest.fixture(scope="module")
def sharp9(weight_cache, lib):
    d = _detector(weight_cache, max_batch=9)
    yield d
    d.close()


def _frames(seeds, hw):
    return [np.ascontiguousarray(structured_frames(1, hw[0], hw[1], seed=s)[0]).copy() for s in seeds]


def _host(det, rows, cols, **kw):
    return TiledDetector(det, rows=rows, cols=cols, native=False, **kw)


def _native(det, rows, cols, **kw):
    return TiledDetector(det, rows=rows, cols=cols, native=True, mixed_sizes=True, **kw)


# ---- 1. the kernel alone -----------------------------------------------------------------------------------------------------------------
THIRDS = tile_grid(37, 64, 1, 3, 0.125)   # (0, 0, 37, 24), (0, 18, 37, 27), (0, 39, 37, 25)
ODD_WINDOWS = [(1, 5, 30, 41), (3, 17, 28, 39), (7, 22, 30, 33)]
# name, frame (h, w), windows, output size of each, canvas, frames
RESIZE = [("three_sizes_in_a_larger_canvas", (37, 64), THIRDS, [(20, 30), (45, 33), (30, 52)], (48, 56), 1),   # up and down in one call; a canvas of 10.5 blocks
          ("identity_among_resized", (37, 64), THIRDS, [(37, 24), (50, 20), (18, 40)], (50, 40), 1),           # tile 0 keeps its window's size
          ("a_tile_fills_each_direction", (37, 64), THIRDS, [(40, 30), (25, 44), (33, 20)], (40, 44), 1),      # tile 0 fills the height, tile 1 the width
          ("two_frames", (37, 64), THIRDS, [(20, 30), (45, 33), (30, 52)], (48, 56), 2),
          ("odd_pitch_windows", (37, 63), ODD_WINDOWS, [(45, 60), (28, 39), (21, 50)], (45, 60), 2)]           # tile 0 fills the canvas, tile 1 is an identity


@pytest.mark.parametrize("name,hw,tiles,sizes,canvas,n_frames", RESIZE, ids=[r[0] for r in RESIZE])
def test_ragged_tile_resize_equals_the_host_canvas(lib, name, hw, tiles, sizes, canvas, n_frames):
    """Byte for byte the canvas ``_preprocess_batch`` builds from contiguous copies of the windows: zeros, and Pillow's resize of each copy in the
    top-left corner.  The output starts as 7s: a byte the kernel leaves out shows."""
    assert len(set(sizes)) == 3 and all(s[0] <= canvas[0] and s[1] <= canvas[1] for s in sizes)
    rng = np.random.RandomState(len(name) * 131 + n_frames)
    frames = rng.randint(0, 256, size=(n_frames, hw[0], hw[1], 3)).astype(np.uint8)
    frames[:, ::5, ::3] = 255   # (extremes next to each other: rounding and clipping)
    frames[:, 1::5, 1::3] = 0
    win, tile_hw = np.asarray(tiles, np.int32).reshape(-1, 4), np.asarray(sizes, np.int32).reshape(-1, 2)
    T = len(win)
    got = np.full((n_frames * T, canvas[0], canvas[1], 3), 7, np.uint8)
    rc = lib.opd_test_tile_resize_ragged(frames.ctypes.data_as(C.c_void_p), n_frames, hw[0], hw[1], win.ctypes.data_as(C.c_void_p), T, tile_hw.ctypes.data_as(C.c_void_p),
                                         canvas[0], canvas[1], got.ctypes.data_as(C.c_void_p))
    assert rc == _capi.OPD_OK, _capi.last_error()
    want = np.zeros_like(got)
    for f in range(n_frames):
        for t, ((y, x, h, w), (oh, ow)) in enumerate(zip(tiles, sizes)):
            copy = np.ascontiguousarray(frames[f, y:y + h, x:x + w])
            want[f * T + t, :oh, :ow] = resize_frame(copy, oh, ow)
            if (oh, ow) == (h, w):
                assert np.array_equal(got[f * T + t, :oh, :ow], copy), f"{name}: the identity tile {t} of frame {f}"
    assert np.array_equal(got, want), f"{name}: {int((got != want).sum())} bytes differ from the host canvas"


# ---- 2. end to end against the host path ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def reference(sharp):
    """The host path on the same detector, once: the merged lists of the 193 x 256 frames and the per-tile lists they were merged from."""
    frames = _frames(ODD_SEEDS, ODD_HW)
    sharp.device_nms = False
    want = _host(sharp, 2, 2).detect_batch(frames)
    per_tile = [sharp.detect_batch(split_tiles(f, 2, 2, 0.125)[0]) for f in frames]
    return frames, want, per_tile


def test_the_grids_are_mixed_and_the_reference_shows_an_absorption(sharp, reference):
    assert [len({(t[2], t[3]) for t in g}) for g in (ODD_GRID, STRIP_GRID, NINE_GRID)] == [2, 2, 6]
    assert len(set(sharp.tile_model_sizes(ODD_GRID))) == 2 and len(set(sharp.tile_model_sizes(STRIP_GRID))) == 2
    frames, want, per_tile = reference
    assert all(len(w) > 0 for w in want)
    assert any(len(w) < sum(len(t) for t in p) for w, p in zip(want, per_tile)), [(len(w), [len(t) for t in p]) for w, p in zip(want, per_tile)]
    widest = max(d.bbox[2] for p in per_tile for t in p for d in t)
    assert any(d.bbox[2] > widest + 1.0 for w in want for d in w), "no kept box has grown: the seam merge itself never happened"


@pytest.mark.parametrize("device_nms", [False, True], ids=["host_nms", "device_nms"])
@pytest.mark.parametrize("n", [1, 3], ids=["one_frame", "three_frames_two_chunks"])
def test_native_equals_the_host_path_on_a_side_that_does_not_divide(sharp, reference, n, device_nms):
    frames, want, _ = reference
    sharp.device_nms = device_nms
    try:
        host = _host(sharp, 2, 2).detect_batch(frames[:n])
        native = _native(sharp, 2, 2).detect_batch(frames[:n])
        again = _native(sharp, 2, 2).detect_batch(frames[:n])
        single = _native(sharp, 2, 2).detect(frames[0])
    finally:
        sharp.device_nms = False
    TS.same(host, want[:n], "the host path, device_nms on and off")
    TS.same(native, host, "native against the host path")
    TS.same(again, native, "native, repeated")
    TS.same([single], host[:1], "detect")
    TS.same(sharp.detect_tiled_ragged(frames[:n], ODD_GRID), host, "detect_tiled_ragged itself")


@pytest.mark.parametrize("device_nms", [False, True], ids=["host_nms", "device_nms"])
@pytest.mark.parametrize("n", [1, 2], ids=["one_frame", "two_frames_one_chunk"])
def test_native_equals_the_host_path_on_a_1x3_strip(sharp, n, device_nms):
    frames = _frames(STRIP_SEEDS[:n], STRIP_HW)
    sharp.device_nms = device_nms
    try:
        host = _host(sharp, 1, 3).detect_batch(frames)
        native = _native(sharp, 1, 3).detect_batch(frames)
    finally:
        sharp.device_nms = False
    assert all(len(h) > 0 for h in host)
    TS.same(native, host, "1 x 3 strip")


@pytest.mark.parametrize("device_nms", [False, True], ids=["host_nms", "device_nms"])
def test_native_equals_the_host_path_on_a_3x3_grid(sharp9, device_nms):
    frames = _frames((NINE_SEED,), NINE_HW)
    sharp9.device_nms = device_nms
    try:
        host = _host(sharp9, 3, 3).detect_batch(frames)
        native = _native(sharp9, 3, 3).detect_batch(frames)
        again = _native(sharp9, 3, 3).detect_batch(frames)
    finally:
        sharp9.device_nms = False
    assert all(len(h) > 0 for h in host)
    TS.same(native, host, "3 x 3 grid")
    TS.same(again, native, "3 x 3 grid, repeated")


def test_native_with_other_thresholds(sharp, reference):
    frames = reference[0]
    for kw in ({"nms_threshold": 1.0}, {"nms_threshold": 0.1, "merge_threshold": 0.2}):
        host = _host(sharp, 2, 2, **kw).detect_batch(frames[:2])
        assert all(len(h) > 0 for h in host)
        TS.same(_native(sharp, 2, 2, **kw).detect_batch(frames[:2]), host, str(kw))


def test_windows_of_two_sizes_with_one_model_size(sharp, reference):
    """With the longest edge at 64 both window sizes of the 193 x 256 grid land on 48 x 64: per-tile descriptors and per-tile box scaling, but no
    padding, so the batch is no ragged one and the forward replays the graph (two frames twice: the second call of a shape captures it)."""
    frames = reference[0]
    sharp.max_size = (256, 64)   # (the handle keeps its 256 x 320: only the size rule the Python side applies changes)
    try:
        assert set(sharp.tile_model_sizes(ODD_GRID)) == {(48, 64)}
        host = _host(sharp, 2, 2).detect_batch(frames[:2])
        native = [_native(sharp, 2, 2).detect_batch(frames[:2]) for _ in range(3)]
    finally:
        sharp.max_size = (256, 320)
    assert all(len(h) > 0 for h in host)
    for k, got in enumerate(native):
        TS.same(got, host, f"one model size, call {k}")


# ---- 3. a grid of one size through the new entry -------------------------------------------------------------------------------------------
def _params(det):
    return _capi.OpdTileParams(struct_size=C.sizeof(_capi.OpdTileParams), person_label=1, tile_nms_threshold=float(det.nms_threshold), merge_nms_threshold=0.4,
                               merge_threshold=0.5, edge_tolerance=0.01)


def test_a_grid_of_one_size_equals_the_uniform_entry_byte_for_byte(lib, sharp):
    frames = _frames((5, 6), (192, 256))
    grid = tile_grid(192, 256, 2, 2, 0.125)
    assert len({(t[2], t[3]) for t in grid}) == 1
    (H, W), = set(sharp.tile_model_sizes(grid))
    win, tile_hw = np.asarray(grid, np.int32).reshape(-1, 4), np.asarray([(H, W)] * 4, np.int32)
    S = 4 * sharp.num_queries
    p = _params(sharp)
    ptrs = (C.c_void_p * 2)(*[f.ctypes.data for f in frames])

    def uniform():
        out, counts = (_capi.OpdTileDet * (2 * S))(), (C.c_int32 * 2)()
        rc = lib.opd_detr_detect_tiled(C.c_void_p(sharp.model), ptrs, 2, 192, 256, win.ctypes.data_as(C.c_void_p), 4, H, W, THRESHOLD, C.byref(p), out, counts)
        assert rc == _capi.OPD_OK, _capi.last_error()
        return out, counts

    def ragged():
        out, counts = (_capi.OpdTileDet * (2 * S))(), (C.c_int32 * 2)()
        rc = lib.opd_detr_detect_tiled_ragged(C.c_void_p(sharp.model), ptrs, 2, 192, 256, win.ctypes.data_as(C.c_void_p), 4, tile_hw.ctypes.data_as(C.c_void_p), THRESHOLD,
                                              C.byref(p), None, out, counts)
        assert rc == _capi.OPD_OK, _capi.last_error()
        return out, counts

    for k, (a, b) in enumerate(((uniform(), ragged()), (ragged(), uniform()))):   # (either order: the first call of a shape runs eagerly, the later ones replay)
        (out_a, cnt_a), (out_b, cnt_b) = a, b
        assert list(cnt_a) == list(cnt_b) and all(c > 0 for c in cnt_a), (k, list(cnt_a), list(cnt_b))
        for f in range(2):
            n = cnt_a[f] * C.sizeof(_capi.OpdTileDet)
            assert C.string_at(C.addressof(out_a) + f * S * C.sizeof(_capi.OpdTileDet), n) == C.string_at(C.addressof(out_b) + f * S * C.sizeof(_capi.OpdTileDet), n), (k, f)
    TS.same(sharp.detect_tiled_ragged(frames, grid), sharp.detect_tiled(frames, grid), "the two methods on a grid of one size")


# ---- 4. the stages -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mapper(lib):
    """A piecewise-affine map over the 193 x 256 frame onto the zones' floor map (tests/test_floor_gpu.py's construction)."""
    h, w = ODD_HW
    rng = np.random.default_rng(9)
    src = np.concatenate([np.array([[0, 0], [w, 0], [0, h], [w, h]], float), rng.uniform((10, 10), (w - 10, h - 10), (20, 2))])
    dst = np.stack([5.5 * src[:, 0] + 40 + 15 * np.sin(src[:, 1] / 40.0), 7.0 * src[:, 1] + 30 + 10 * np.cos(src[:, 0] / 50.0)], 1)
    m = HipFloorMapper.piecewise_affine(src, dst, FM, ZONES, device=0)
    yield m
    m.close()


def _separate(det, frames, features=None, floor_map=None):
    """The separate calls on the same handle: detect_tiled_ragged, then extract_color_features and floor_map.apply per frame."""
    out = det.detect_tiled_ragged(frames, ODD_GRID)
    for f, dets in zip(frames, out):
        if features == "color":
            for d, row in zip(dets, det.extract_color_features(f, dets)):
                d.features = row
        if floor_map is not None:
            floor_map.apply(dets)
    return out


def _track_rows(t):
    return [bytes(r) for r in t._records()]


def test_fused_features_and_floor_equal_the_separate_calls(sharp, reference, mapper):
    frames = reference[0]
    want = _separate(sharp, frames, "color", mapper)
    assert all(len(w) > 0 and all(d.features is not None and d.floor_coords is not None for d in w) for w in want)
    TS.same(sharp.detect_tiled_ragged(frames, ODD_GRID, features="color", floor_map=mapper), want, "colour rows and floor fields, three frames in two chunks")
    TS.same(sharp.detect_tiled_ragged(frames[:1], ODD_GRID, features="color"), _separate(sharp, frames[:1], "color"), "colour rows alone")
    TS.same(sharp.detect_tiled_ragged(frames[:1], ODD_GRID, floor_map=mapper), _separate(sharp, frames[:1], None, mapper), "floor fields alone")
    td = _native(sharp, 2, 2)
    TS.same([td.detect(frames[0], floor_map=mapper)], _separate(sharp, frames[:1], None, mapper), "TiledDetector.detect(floor_map=)")
    dets, rows = td.detect_with_features(frames[0], features="color")
    TS.same([dets], _separate(sharp, frames[:1], "color"), "TiledDetector.detect_with_features")
    assert rows.tobytes() == np.stack([d.features for d in want[0]]).tobytes()


@pytest.mark.parametrize("features", ["color", None], ids=["colour_rows", "motion_only"])
def test_fused_stages_with_a_tracker_equal_the_separate_calls(sharp, reference, mapper, features):
    frames = reference[0]
    high = float(np.median([d.confidence for dets in reference[1] for d in dets]))   # both stages of the association see records
    fused, twin = (HipTracker(max_dets=512, feature_dim=256, min_hits=1, high_conf_threshold=high) for _ in range(2))
    try:
        for k, f in enumerate(frames):   # three consecutive frames: the second and third meet the tracks of the ones before
            got = sharp.detect_tiled_ragged([f], ODD_GRID, features=features, floor_map=mapper, trackers=[fused])[0]
            want = _separate(sharp, [f], features, mapper)[0]
            twin.update(want)
            assert [d.track_id for d in got] == [d.track_id for d in want], f"ids of frame {k}"
            assert any(d.track_id is not None for d in got)
            TS.same([got], [want], f"frame {k}", skip_features=True)
            assert all(d.features is None for d in got)   # (with a tracker the rows stay on the device, as in detect_and_track)
            assert _track_rows(fused) == _track_rows(twin), f"track rows after frame {k}"
            assert [(t.track_id, t.age, t.hits, t.time_since_update) for t in fused.get_tracks()] == [(t.track_id, t.age, t.hits, t.time_since_update) for t in twin.get_tracks()]
        third, twin3 = (HipTracker(max_dets=512, feature_dim=256, min_hits=1, high_conf_threshold=high) for _ in range(2))
        try:
            got = _native(sharp, 2, 2).detect_and_track(frames[0], third, features=features)
            want = twin3.update(_separate(sharp, frames[:1], features)[0])
            TS.same([got], [want], "TiledDetector.detect_and_track", skip_features=True)
            assert _track_rows(third) == _track_rows(twin3)
        finally:
            third.close()
            twin3.close()
    finally:
        fused.close()
        twin.close()


# ---- 5. the kernel table, the refusal that needs a handle ------------------------------------------------------------------------------------
def test_kernel_table_has_the_ragged_launches(sharp, reference):
    frames = reference[0]
    sharp.set_profiling(True)
    try:
        _native(sharp, 2, 2).detect_batch(frames[:1])
        rows = (_capi.OpdKernelStat * 256)()
        n = C.c_int()
        assert sharp._lib.opd_detr_kernel_table(C.c_void_p(sharp.model), rows, 256, C.byref(n)) == _capi.OPD_OK
        names = {rows[i].name.decode(): rows[i].launches for i in range(min(n.value, 256))}
    finally:
        sharp.set_profiling(False)
    for k in ("tile_resize_ragged_u8_kernel", "tile_merge_kernel", "person_nms_kernel"):
        assert names.get(k) == 1, (k, names)
    assert "tile_resize_u8_kernel" not in names and "resize_bilinear_u8_kernel" not in names


def test_a_canvas_outside_the_handle_is_refused(lib, sharp, reference):
    frame = reference[0][0]
    win = np.asarray(ODD_GRID, np.int32).reshape(-1, 4)
    p = _params(sharp)
    out, counts = (_capi.OpdTileDet * (4 * sharp.num_queries))(), (C.c_int32 * 1)()
    ptrs = (C.c_void_p * 3)(*[frame.ctypes.data] * 3)

    def refused(text, sizes, n_frames=1):
        hw = np.asarray(sizes, np.int32)
        rc = lib.opd_detr_detect_tiled_ragged(C.c_void_p(sharp.model), ptrs, n_frames, 193, 256, win.ctypes.data_as(C.c_void_p), 4, hw.ctypes.data_as(C.c_void_p), THRESHOLD,
                                              C.byref(p), None, out, counts)
        assert rc == _capi.OPD_EINVAL and text in _capi.last_error(), (text, _capi.last_error())

    refused("outside the configured maximum", [(240, 320), (240, 320), (242, 512), (242, 320)])   # the canvas is the maximum over the tiles: 242 x 512
    refused("outside the configured maximum", [(512, 100), (240, 320), (242, 320), (242, 320)])
    refused("outside the configured maximum", [(16, 320), (16, 320), (20, 320), (20, 320)])       # below 32
    refused("opd_detr_detect_tiled_ragged: 3 frames x 4 tiles", sharp.tile_model_sizes(ODD_GRID), n_frames=3)
    with pytest.raises(ValueError, match="more than one size"):   # without the keyword: today's refusal
        TiledDetector(sharp, native=True).detect_batch([frame])


# ---- 6. the handle afterwards ----------------------------------------------------------------------------------------------------------------
def test_a_mixed_call_leaves_the_handle_as_it_was(sharp, reference):
    frames = reference[0]
    plain = _frames((11, 12), (180, 320))
    even, grid = _frames((5, 6), (192, 256)), tile_grid(192, 256, 2, 2, 0.125)
    for device_nms in (False, True):
        sharp.device_nms = device_nms
        try:
            before, tiled_before = sharp.detect_batch(plain), sharp.detect_tiled(even, grid)
            mixed = _native(sharp, 2, 2).detect_batch(frames[:2])
            after, tiled_after = sharp.detect_batch(plain), sharp.detect_tiled(even, grid)
            mixed_again = _native(sharp, 2, 2).detect_batch(frames[:2])
        finally:
            sharp.device_nms = False
        assert all(len(b) > 0 for b in before) and all(len(b) > 0 for b in tiled_before)
        TS.same(after, before, f"detect_batch after a mixed call, device_nms={device_nms}")
        TS.same(tiled_after, tiled_before, f"detect_tiled on a grid of one size after a mixed call, device_nms={device_nms}")
        TS.same(mixed_again, mixed, f"a mixed call after the two, device_nms={device_nms}")
