"""CPU tests of native tiled detection for grids whose tiles differ in size (-m "not gpu"): the entry point ``opd_detr_detect_tiled_ragged`` and
the hook ``opd_test_tile_resize_ragged`` in the header, the binding and the two libraries; the entry's refusals, which all come before any
device call; ``HipDetrDetector.detect_tiled_ragged``'s argument errors and the model size it gives each tile; and ``TiledDetector``'s
``mixed_sizes`` keyword, which routes a mixed grid to that method and leaves everything else where it was."""

import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from office_person_detection_vit_amd import HipDetrDetector, TiledDetector, _capi
from office_person_detection_vit_amd.detector import model_input_size
from office_person_detection_vit_amd.tiling import tile_grid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY, HOOK = "opd_detr_detect_tiled_ragged", "opd_test_tile_resize_ragged"


@pytest.fixture(scope="module")
def lib():
    return _capi.load_library(test_hooks=True)


def test_header_binding_and_libraries_agree_on_the_new_names(lib):
    header = open(os.path.join(ROOT, "include", "opd_detr.h")).read()
    assert re.search(r"OPD_API int " + ENTRY + r"\(", header) and ENTRY in _capi.API and ENTRY not in _capi.TEST_API
    assert HOOK not in header and HOOK in _capi.TEST_API and HOOK not in _capi.API
    decl = re.search(r"OPD_API int " + ENTRY + r"\((.*?)\);", header, re.S).group(1)
    names = [a.split()[-1].lstrip("*") for a in decl.split(",")]
    assert names == ["m", "frames", "n_frames", "h", "w", "tiles_yxhw", "n_tiles", "tile_HW", "threshold", "p", "stages", "out", "counts"]
    assert len(_capi.API[ENTRY][1]) == len(names)

    def exported(path):
        out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
        return {l.split()[2] for l in out.splitlines() if len(l.split()) == 3 and l.split()[1] == "T"}

    prod, test = exported(_capi.LIB_PATH), exported(_capi.TEST_LIB_PATH)
    assert ENTRY in prod and ENTRY in test
    assert HOOK not in prod and HOOK in test


def test_arguments_are_refused_before_any_device_call(lib):
    """Without a handle: every check that does not read the handle comes first, so a null handle is the LAST thing the call reports -- for a
    mixed grid too, which is what the other tiled entries refuse and this one takes."""
    mixed = np.asarray(tile_grid(41, 52, 2, 2, 0.125), np.int32)
    assert len({(int(t[2]), int(t[3])) for t in mixed}) == 2
    sizes = np.asarray([[32, 40]] * 4, np.int32)
    p = _capi.OpdTileParams(struct_size=C.sizeof(_capi.OpdTileParams), person_label=1, tile_nms_threshold=0.4, merge_nms_threshold=0.4, merge_threshold=0.5,
                            edge_tolerance=0.01)
    frame = np.zeros((41, 52, 3), np.uint8)
    ptrs = (C.c_void_p * 1)(frame.ctypes.data)
    out, counts = (_capi.OpdTileDet * 400)(), (C.c_int32 * 1)()
    feats = np.zeros((1, 400, 256), np.float32)

    def ragged(text, frames=ptrs, tiles=mixed, n_tiles=4, h=41, w=52, hw=sizes, params=p, stages=None, o=out, c=counts):
        rc = lib.opd_detr_detect_tiled_ragged(None, frames, 1, h, w, None if tiles is None else tiles.ctypes.data_as(C.c_void_p), n_tiles,
                                              None if hw is None else hw.ctypes.data_as(C.c_void_p), 0.05, None if params is None else C.byref(params),
                                              None if stages is None else C.byref(stages), o, c)
        assert rc == _capi.OPD_EINVAL and text in _capi.last_error(), (text, _capi.last_error())
        assert ENTRY in _capi.last_error() or text == "null model handle"

    ragged("null model handle")   # (a mixed grid with good sizes: nothing but the handle is missing)
    ragged("null model handle", tiles=np.asarray(tile_grid(40, 52, 2, 2, 0.125), np.int32), h=40)   # (and a grid of one size)
    ragged("null argument", frames=None)
    ragged("null argument", o=None)
    ragged("null argument", c=None)
    ragged("null argument", tiles=None)
    ragged("null argument", params=None)
    ragged("null argument (tile_HW)", hw=None)
    ragged("struct_size", params=_capi.OpdTileParams(struct_size=8))
    ragged("n_tiles", n_tiles=0)
    outside = mixed.copy(); outside[3, 1] += 1
    ragged("lies outside the 41 x 52 frame", tiles=outside)
    negative = mixed.copy(); negative[0, 0] = -1
    ragged("lies outside", tiles=negative)
    ragged("tile_nms_threshold", params=_capi.OpdTileParams(struct_size=C.sizeof(_capi.OpdTileParams), person_label=1, tile_nms_threshold=float("nan")))
    for bad in ((0, 40), (32, 0), (-5, 40)):
        hw = sizes.copy(); hw[2] = bad
        ragged("below 1", hw=hw)
        assert "tile 2" in _capi.last_error()
    # the stages block: what opd_detr_detect_tiled_stages refuses without a handle
    ragged("opd_tile_stages.struct_size", stages=_capi.OpdTileStages(struct_size=8))
    ragged("feature_kind", stages=_capi.OpdTileStages(struct_size=C.sizeof(_capi.OpdTileStages), feature_kind=_capi.OPD_TRACK_FEAT_REID))
    ragged("features given with feature_kind", stages=_capi.OpdTileStages(struct_size=C.sizeof(_capi.OpdTileStages), feature_kind=_capi.OPD_TRACK_FEAT_NONE,
                                                                         features=feats.ctypes.data))
    ragged("floor_out is null", stages=_capi.OpdTileStages(struct_size=C.sizeof(_capi.OpdTileStages), floor=1))
    ragged("track_ids or n_featured", stages=_capi.OpdTileStages(struct_size=C.sizeof(_capi.OpdTileStages), trackers=C.addressof(ptrs)))
    ragged("null model handle", stages=_capi.OpdTileStages(struct_size=C.sizeof(_capi.OpdTileStages), feature_kind=_capi.OPD_TRACK_FEAT_COLOR,
                                                           features=feats.ctypes.data))
    # the other entries still refuse the grid this one takes
    rc = lib.opd_detr_detect_tiled(None, ptrs, 1, 41, 52, mixed.ctypes.data_as(C.c_void_p), 4, 32, 40, 0.05, C.byref(p), out, counts)
    assert rc == _capi.OPD_EINVAL and "one forward has one model size" in _capi.last_error()
    # the hook's own refusals (before any device call as well)
    canvas = np.zeros((4, 32, 40, 3), np.uint8)

    def hook(tiles=mixed, hw=sizes, H=32, W=40):
        return lib.opd_test_tile_resize_ragged(frame.ctypes.data_as(C.c_void_p), 1, 41, 52, tiles.ctypes.data_as(C.c_void_p), 4, None if hw is None else hw.ctypes.data_as(C.c_void_p),
                                               H, W, canvas.ctypes.data_as(C.c_void_p))

    assert hook(tiles=outside) == _capi.OPD_EINVAL and "outside the frame" in _capi.last_error()
    assert hook(hw=None) == _capi.OPD_EINVAL
    assert hook(H=31) == _capi.OPD_EINVAL and "outside the canvas" in _capi.last_error()
    assert hook(W=39) == _capi.OPD_EINVAL and "outside the canvas" in _capi.last_error()


def test_each_tile_gets_the_model_size_of_a_contiguous_copy():
    det = HipDetrDetector(model_path="unused", max_batch=8, max_size=(256, 320), resize=True)
    grid = tile_grid(96, 384, 1, 3, 0.125)
    assert [(t[2], t[3]) for t in grid] == [(96, 144), (96, 160), (96, 144)]
    assert det.tile_model_sizes(grid) == [(213, 320), (192, 320), (213, 320)]
    assert det.tile_model_sizes(grid) == [model_input_size(t[2], t[3], 256, 320) for t in grid]
    grid = tile_grid(193, 256, 2, 2, 0.125)
    assert [(t[2], t[3]) for t in grid] == [(108, 144), (108, 144), (109, 144), (109, 144)]
    assert det.tile_model_sizes(grid) == [model_input_size(108, 144, 256, 320)] * 2 + [model_input_size(109, 144, 256, 320)] * 2
    det.resize = False
    assert det.tile_model_sizes(grid) == [(108, 144), (108, 144), (109, 144), (109, 144)]
    # the table of the 4K grids: 2 x 3 and 3 x 3 at the 800 / 1333 rule
    big = HipDetrDetector(model_path="unused", max_batch=9, max_size=(800, 1333), resize=True)
    assert sorted(set(big.tile_model_sizes(tile_grid(2160, 3840, 2, 3, 0.125)))) == [(800, 948), (800, 1053)]
    assert sorted(set(big.tile_model_sizes(tile_grid(2160, 3840, 3, 3, 0.125)))) == [(675, 1333), (750, 1333), (800, 1280)]


def test_python_surface_and_its_refusals():
    sig = inspect.signature(HipDetrDetector.detect_tiled_ragged)
    assert [(k, v.default) for k, v in sig.parameters.items() if k != "self"] == [
        ("frames", inspect.Parameter.empty), ("tiles", inspect.Parameter.empty), ("nms_threshold", 0.4), ("merge_threshold", 0.5), ("edge_tolerance", 0.01),
        ("features", None), ("floor_map", None), ("trackers", None)]
    assert inspect.signature(TiledDetector.__init__).parameters["mixed_sizes"].default is False
    frame = np.zeros((41, 52, 3), np.uint8)
    mixed = tile_grid(41, 52, 2, 2, 0.125)
    det = HipDetrDetector(model_path="unused", max_batch=2, max_size=(256, 320))
    with pytest.raises(RuntimeError, match="Model not loaded"):
        det.detect_tiled_ragged([frame], mixed)
    det.model = 1   # (never dereferenced: every check below comes before the library call)
    try:
        with pytest.raises(ValueError, match="exceed max_batch"):
            det.detect_tiled_ragged([frame], mixed)
        det.max_batch = 8
        for bad in ([], [(0, 0, 20)], [(0, 0, 20, 20, 1)]):
            with pytest.raises(ValueError, match="non-empty list"):
                det.detect_tiled_ragged([frame], bad)
        with pytest.raises(ValueError, match="at least 1"):
            det.detect_tiled_ragged([frame], [(0, 0, 0, 20), (0, 0, 20, 20)])
        for bad in ([frame[:, ::2]], [frame.astype(np.float32)], [frame, np.zeros((41, 60, 3), np.uint8)], [frame[..., 0]]):
            with pytest.raises(ValueError, match="contiguous uint8"):
                det.detect_tiled_ragged(bad, mixed)
        with pytest.raises(ValueError, match="encoder"):
            det.detect_tiled_ragged([frame], mixed, features="encoder")
        with pytest.raises(ValueError, match="None or 'color'"):
            det.detect_tiled_ragged([frame], mixed, features="reid")
        with pytest.raises(ValueError, match="2 trackers for 1 frames"):
            det.detect_tiled_ragged([frame], mixed, trackers=[object(), object()])
        t = object()
        with pytest.raises(ValueError, match="named twice"):
            det.detect_tiled_ragged([frame, frame], mixed, trackers=[t, t])
        det.max_size, det.resize = (32, 40), False   # (windows as they are: a 20 x 52 canvas, wider than the longest edge)
        with pytest.raises(ValueError, match="exceeds the configured maximum"):
            det.detect_tiled_ragged([frame], [(0, 0, 20, 52), (21, 0, 20, 50)])
        assert det.detect_tiled_ragged([], mixed) == []
        # the other tiled methods refuse the mixed grid as they did
        for call in (det.detect_tiled, det.detect_tiled_stages):
            with pytest.raises(ValueError, match="more than one size"):
                call([frame], mixed)
    finally:
        det.model = None


class _Recorder:
    """A detector's tiled surface, recording which method a TiledDetector calls."""

    def __init__(self, ragged=True):
        self.calls = []
        if ragged:
            self.detect_tiled_ragged = lambda frames, tiles, *a, **kw: self._note("ragged", frames, tiles, kw)

    def _note(self, name, frames, tiles, kw):
        self.calls.append((name, len(tiles), {k: v for k, v in kw.items() if v is not None}))
        return [[] for _ in frames]

    def detect_tiled(self, frames, tiles, *a, **kw):
        if len({(t[2], t[3]) for t in tiles}) != 1:
            raise ValueError("tiles of more than one size: one forward has one model size")
        return self._note("tiled", frames, tiles, kw)

    def detect_tiled_stages(self, frames, tiles, *a, **kw):
        if len({(t[2], t[3]) for t in tiles}) != 1:
            raise ValueError("tiles of more than one size: one forward has one model size")
        return self._note("stages", frames, tiles, kw)


def test_tiled_detector_routes_a_mixed_grid_only_with_the_keyword():
    odd, even = np.zeros((193, 256, 3), np.uint8), np.zeros((192, 256, 3), np.uint8)
    rec = _Recorder()
    with pytest.raises(ValueError, match="more than one size"):   # today's refusal, without the keyword
        TiledDetector(rec, native=True).detect_batch([odd])
    with pytest.raises(ValueError, match="more than one size"):
        TiledDetector(rec, native=True, mixed_sizes=False).detect_with_features(odd)
    assert rec.calls == []
    td = TiledDetector(rec, native=True, mixed_sizes=True)
    floor, tracker = object(), object()
    td.detect_batch([odd, odd])
    td.detect(odd)
    td.detect(odd, floor_map=floor)
    td.detect_with_features(odd, features="color")
    td.detect_and_track(odd, tracker)
    td.detect_and_track(odd, tracker, features=None)
    assert rec.calls == [("ragged", 4, {}), ("ragged", 4, {}), ("ragged", 4, {"floor_map": floor}), ("ragged", 4, {"features": "color"}),
                         ("ragged", 4, {"features": "color", "trackers": [tracker]}), ("ragged", 4, {"trackers": [tracker]})]
    rec.calls.clear()
    td.detect_batch([even])   # a grid of one size: the calls it always took
    td.detect(even, floor_map=floor)
    td.detect_with_features(even, features="color")
    td.detect_and_track(even, tracker)
    assert [c[0] for c in rec.calls] == ["tiled", "stages", "stages", "stages"]
    rec.calls.clear()
    TiledDetector(rec, rows=3, cols=3, native=True, mixed_sizes=True).detect_batch([even])   # interior tiles: mixed at the default overlap
    assert rec.calls == [("ragged", 9, {})]
    with pytest.raises(ValueError, match="detect_tiled_ragged"):
        TiledDetector(_Recorder(ragged=False), native=True, mixed_sizes=True).detect_batch([odd])
    # mixed_sizes without native: the host path, nothing native is called
    plain = _Recorder()
    plain.detect_batch = lambda frames: [[] for _ in frames]
    assert TiledDetector(plain, mixed_sizes=True).detect_batch([odd]) == [[]] and plain.calls == []
