"""CPU tests of tiled detection in one native call (-m "not gpu"): the merge rule of csrc/opd_tile.h, run on the host by the hook
``opd_test_tile_merge_host``, against ``tiling.merge_tile_detections`` on every case of tests/tile_common.py, exactly; the two new entry
points in the header, the binding and the two libraries; the two structs; and the refusals that need no device."""

import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import tile_common as T
from office_person_detection_vit_amd import HipDetrDetector, TiledDetector, _capi
from office_person_detection_vit_amd.tiling import tile_grid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = T.cases()
NEW = ("opd_detr_detect_tiled", "opd_detr_merge_tiles")
HOOKS = ("opd_test_tile_merge_host", "opd_test_tile_resize")


@pytest.fixture(scope="module")
def lib():
    return _capi.load_library(test_hooks=True)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_host_restatement_equals_the_python_rule(lib, case):
    rc, out, counts = T.run(lib.opd_test_tile_merge_host, case)
    assert rc == _capi.OPD_OK, _capi.last_error()
    T.assert_same(case, out, counts, T.expected(case))


def test_cases_are_what_they_claim():
    """The growth chain: Python drops C only because A has grown; the random cases absorb some candidates and keep some."""
    by = {c["name"]: c for c in CASES}
    with_b, without_b = T.expected(by["growth_chain"])[0], T.expected(by["growth_chain_without_b"])[0]
    assert len(with_b) == 1 and len(without_b) == 2
    assert with_b[0][:4] == (100.0, 20.0, 150.0, 70.0) and without_b[1][:4] == (180.0, 20.0, 70.0, 70.0)
    assert T.expected(by["vertical_seam"])[0][0][:4] == (120.0, 20.0, 80.0, 70.0)
    assert T.expected(by["corner_four_tiles"])[0][0] == (120.0, 70.0, 60.0, 60.0, float(np.float32(0.9)), 1, 0, 0)
    assert T.expected(by["left_side_at_tx"])[0][0][:4] == (100.0, 10.0, 150.0, 70.0) and T.expected(by["left_side_beyond_tx"])[0][0][:4] == (100.0, 10.0, 100.0, 70.0)
    assert T.expected(by["right_side_at_tw_minus_tx"])[0][0][2] == 138.0 and T.expected(by["right_side_beyond_tw_minus_tx"])[0][0][2] == 100.0
    for c in CASES:
        if c["name"].startswith("random_") and "nms" not in c["name"]:
            for f, w in enumerate(T.expected(c)):
                n = int(np.maximum(c["counts"].reshape(c["n_frames"], -1)[f], 0).sum())
                assert 0 < len(w) < n, (c["name"], f, len(w), n)
        if c["name"].startswith("full_load"):
            assert int(c["counts"].sum()) == 4 * c["stride"]


def test_a_count_above_the_stride_empties_its_frame_and_is_reported(lib):
    case = dict(next(c for c in CASES if c["name"] == "three_frames"))
    case["counts"] = case["counts"].copy()
    case["counts"][5] = case["stride"] + 1   # frame 1
    rc, out, counts = T.run(lib.opd_test_tile_merge_host, case)
    assert rc == _capi.OPD_EINVAL and "more records than its slots" in _capi.last_error()
    want = T.expected(next(c for c in CASES if c["name"] == "three_frames"))
    assert counts.tolist() == [len(want[0]), 0, len(want[2])]


def test_header_binding_and_libraries_agree_on_the_new_names(lib):
    header = open(os.path.join(ROOT, "include", "opd_detr.h")).read()
    for name in NEW:
        assert re.search(r"OPD_API int " + name + r"\(", header) and name in _capi.API and name not in _capi.TEST_API
    for name in HOOKS:
        assert name not in header and name in _capi.TEST_API and name not in _capi.API

    def exported(path):
        out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
        return {l.split()[2] for l in out.splitlines() if len(l.split()) == 3 and l.split()[1] == "T"}

    prod, test = exported(_capi.LIB_PATH), exported(_capi.TEST_LIB_PATH)
    assert set(NEW) <= prod and set(NEW) <= test
    assert not (set(HOOKS) & prod) and set(HOOKS) <= test


def test_struct_layouts():
    assert C.sizeof(_capi.OpdTileDet) == 48 and C.sizeof(_capi.OpdTileParams) == 40
    header = open(os.path.join(ROOT, "include", "opd_detr.h")).read()
    for cname, struct in (("opd_tile_det", _capi.OpdTileDet), ("opd_tile_params", _capi.OpdTileParams)):
        body = re.search(r"typedef struct " + cname + r" \{(.*?)\} " + cname + ";", header, re.S).group(1)
        names = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
        assert names == [f[0] for f in struct._fields_], cname
    assert [(_capi.OpdTileDet.x.offset, _capi.OpdTileDet.score.offset, _capi.OpdTileDet.tile.offset)] == [(0, 32, 44)]
    assert _capi.OpdTileParams.merge_nms_threshold.offset == 16 and _capi.OpdTileParams.edge_tolerance.offset == 32


def test_arguments_are_refused_before_any_device_call(lib):
    """Without a handle: every check that does not read the handle comes first, so a null handle is the LAST thing these calls report."""
    grid = np.asarray(tile_grid(40, 52, 2, 2, 0.125), np.int32)
    p = _capi.OpdTileParams(struct_size=C.sizeof(_capi.OpdTileParams), person_label=1, tile_nms_threshold=0.4, merge_nms_threshold=0.4, merge_threshold=0.5,
                            edge_tolerance=0.01)
    frame = np.zeros((40, 52, 3), np.uint8)
    ptrs = (C.c_void_p * 1)(frame.ctypes.data)
    out, counts = (_capi.OpdTileDet * 400)(), (C.c_int32 * 1)()

    def tiled(text, frames=ptrs, tiles=grid, n_tiles=4, h=40, w=52, params=p, o=out, c=counts):
        rc = lib.opd_detr_detect_tiled(None, frames, 1, h, w, None if tiles is None else tiles.ctypes.data_as(C.c_void_p), n_tiles, 32, 40, 0.05,
                                       None if params is None else C.byref(params), o, c)
        assert rc == _capi.OPD_EINVAL and text in _capi.last_error(), (text, _capi.last_error())

    tiled("null model handle")
    tiled("null argument", frames=None)
    tiled("null argument", o=None)
    tiled("null argument", c=None)
    tiled("null argument", tiles=None)
    tiled("null argument", params=None)
    tiled("struct_size", params=_capi.OpdTileParams(struct_size=8))
    tiled("n_tiles", n_tiles=0)
    outside = grid.copy(); outside[3, 1] += 1
    tiled("lies outside the 40 x 52 frame", tiles=outside)
    negative = grid.copy(); negative[0, 0] = -1
    tiled("lies outside", tiles=negative)
    mixed = np.asarray(tile_grid(41, 52, 2, 2, 0.125), np.int32)
    tiled("more than one size", tiles=mixed, h=41)
    assert "one forward has one model size" in _capi.last_error()
    bad = _capi.OpdTileParams(struct_size=C.sizeof(_capi.OpdTileParams), person_label=1, tile_nms_threshold=float("nan"))
    tiled("tile_nms_threshold", params=bad)

    recs, tc = np.zeros((4, 10), T.DET), np.zeros(4, np.int32)

    def merge(text, tiles=grid, n_tiles=4, stride=10, n_frames=1, params=p, h=40, w=52):
        rc = lib.opd_detr_merge_tiles(None, recs.ctypes.data_as(C.c_void_p), tc.ctypes.data_as(C.c_void_p), n_frames, n_tiles, stride,
                                      None if tiles is None else tiles.ctypes.data_as(C.c_void_p), h, w, None if params is None else C.byref(params), out, counts)
        assert rc == _capi.OPD_EINVAL and text in _capi.last_error(), (text, _capi.last_error())

    merge("null model handle")
    merge("null model handle", tiles=mixed, h=41)   # (the merge takes tiles of several sizes)
    merge("null argument", tiles=None)
    merge("null argument", params=None)
    merge("struct_size", params=_capi.OpdTileParams(struct_size=48))
    merge("lies outside", tiles=outside)
    merge("1024 candidates", stride=257)
    merge("stride < 1", stride=0)
    merge("n_frames < 0", n_frames=-1)
    # the hook refuses the same
    rc = lib.opd_test_tile_merge_host(recs.ctypes.data_as(C.c_void_p), tc.ctypes.data_as(C.c_void_p), 1, 4, 257, grid.ctypes.data_as(C.c_void_p), 40, 52, C.byref(p), out, counts)
    assert rc == _capi.OPD_EINVAL


def test_python_surface_and_its_refusals():
    import inspect
    sig = inspect.signature(HipDetrDetector.detect_tiled)
    assert [(k, v.default) for k, v in sig.parameters.items() if k != "self"] == [("frames", inspect.Parameter.empty), ("tiles", inspect.Parameter.empty),
                                                                                  ("nms_threshold", 0.4), ("merge_threshold", 0.5), ("edge_tolerance", 0.01)]
    assert inspect.signature(TiledDetector.__init__).parameters["native"].default is False

    class Plain:
        def detect_batch(self, frames):
            return [[] for _ in frames]

    frame = np.zeros((40, 52, 3), np.uint8)
    assert TiledDetector(Plain()).detect_batch([frame]) == [[]]
    with pytest.raises(ValueError, match="detect_tiled"):
        TiledDetector(Plain(), native=True).detect_batch([frame])
    det = HipDetrDetector(model_path="unused", max_batch=2)
    with pytest.raises(RuntimeError, match="Model not loaded"):
        det.detect_tiled([frame], tile_grid(40, 52, 2, 2, 0.125))
    det.model = 1   # (never dereferenced: every check below comes before the library call)
    with pytest.raises(ValueError, match="exceed max_batch"):
        det.detect_tiled([frame], tile_grid(40, 52, 2, 2, 0.125))
    det.max_batch = 8
    with pytest.raises(ValueError, match="more than one size"):
        det.detect_tiled([np.zeros((41, 52, 3), np.uint8)], tile_grid(41, 52, 2, 2, 0.125))
    for bad in ([frame[:, ::2]], [frame.astype(np.float32)], [frame, np.zeros((40, 60, 3), np.uint8)], [frame[..., 0]]):
        with pytest.raises(ValueError, match="contiguous uint8"):
            det.detect_tiled(bad, tile_grid(40, 52, 2, 2, 0.125))
    assert det.detect_tiled([], tile_grid(40, 52, 2, 2, 0.125)) == []
    det.model = None
