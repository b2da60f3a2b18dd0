"""The floor map without a GPU: the numpy restatement of the kernel contract (floor_common.py) against the recorded fixture, the new
C-ABI names, every refusal of a bad configuration (made before any HIP call), the host tables the library derives, ``from_config``
parsing, and ``apply`` / ``zone_counts`` of ``HipFloorMapper`` on a stubbed library."""

import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import floor_common as F
from office_person_detection_vit_amd import HipFloorMapper, _capi
from office_person_detection_vit_amd import floor as FL
from office_person_detection_vit_amd.data_models import Detection

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FM = (1878, 1369, 28.1926406926406, 28.241430700447)
ZONES = [{"id": "zone_1", "polygon": [[859, 912], [1095, 912], [1095, 1350], [859, 1350]], "priority": 1},
         {"id": "zone_2", "polygon": [[1095, 912], [1331, 912], [1331, 1350], [1095, 1350]], "priority": 2},
         {"id": "zone_3", "polygon": [[1331, 912], [1567, 912], [1567, 1350], [1331, 1350]], "priority": 3}]
H = [[-0.8795888447, -2.8974379541, 417.8510123786], [-1.5459702925, -3.4570021203, 1054.0107447082], [-0.0011928509, -0.0035480452, 1.0]]
NEW = ["opd_floor_create", "opd_floor_destroy", "opd_floor_info", "opd_floor_transform", "opd_floor_transform_points", "opd_floor_classify",
       "opd_detr_detect_frames_floor"]


@pytest.fixture(scope="module")
def golden():
    return np.load(F.GOLDEN)


def test_fixture_reaches_the_chunk_boundaries(golden):
    names = F.case_names(golden)
    T = {n: len(golden[f"{n}_triangles"]) for n in names if int(golden[f"{n}_method"]) == F.PWA}
    assert T["pwa_n3"] == 1 and T["pwa_t_small"] < 64 < T["pwa_t_mid"] < 128 < T["pwa_t_big"] <= 512
    N = sorted(len(golden[f"{n}_points"]) for n in names if int(golden[f"{n}_method"]) == F.TPS)
    assert N == [3, 64, 65]
    Z = {len(golden[f"{n}_zone_offsets"]) - 1 for n in names}
    assert {0, 1, 64} <= Z
    verts = np.concatenate([np.diff(golden[f"{n}_zone_offsets"]) for n in names])
    assert verts.min() == 3 and verts.max() == 64
    assert any(len(golden[f"{n}_dist"]) for n in names) and list(golden["pwa_distortion_dist"][4:]) == [-0.1, 0.05, 1e-3, 1e-3, 0.0]
    for n in names:   # every case has points inside and outside of things
        flags = golden[f"{n}_truth_flags"]
        assert 0 < ((flags & F.WITHIN) != 0).sum() < len(flags), n
        if len(golden[f"{n}_zone_offsets"]) > 1:
            assert 0 < (golden[f"{n}_truth_mask"] != 0).sum() < len(flags), n
        if n in T and n != "pwa_n3":
            assert 0 < ((flags & F.EXTRAPOLATED) != 0).sum() < len(flags), n
    multi = [n for n in names if (np.array([bin(int(m)).count("1") for m in golden[f"{n}_truth_mask"]]) > 1).any()]
    assert set(multi) == {n for n in names if int(golden[f"{n}_allow_overlap"])} and multi


@pytest.mark.parametrize("name", F.case_names(np.load(F.GOLDEN)))
def test_restatement_reproduces_the_fixture(golden, name):
    model = F.case_model(golden, name)
    boxes, pts = golden[f"{name}_boxes"], golden[f"{name}_pts"]
    kw = dict(boxes=boxes) if len(boxes) else dict(pts=pts)
    px, tri, flags, masks = F.run(model, **kw)
    assert np.array_equal(tri, golden[f"{name}_truth_tri"]) and np.array_equal(flags, golden[f"{name}_truth_flags"])
    assert np.array_equal(masks, golden[f"{name}_truth_mask"])
    d = float(np.abs(px - golden[f"{name}_truth_px"]).max())
    e64 = float(golden[f"{name}_e64"])
    print(f"{name}: float64 restatement {d:.3e} from the truth, recorded e64 {e64:.3e}, device bound {F.bound(golden, name):.3e}")
    assert d <= e64 + float(np.spacing(np.abs(golden[f"{name}_truth_px"]).max()))   # (e64 was taken before the truth was rounded to float64)
    lpx, ltri, lflags, lmasks = F.run(model, dt=np.longdouble, **kw)
    assert np.array_equal(lpx.astype(np.float64), golden[f"{name}_truth_px"]) and np.array_equal(ltri, tri) and np.array_equal(lmasks, masks)
    if f"{name}_ref_px" in golden.files:   # the reference's own classes, recorded by the generator
        assert np.abs(golden[f"{name}_ref_px"] - golden[f"{name}_truth_px"]).max() <= F.bound(golden, name)
        assert np.array_equal(golden[f"{name}_ref_mask"], masks) and np.array_equal(golden[f"{name}_ref_within"], (flags & F.WITHIN) != 0)
        if model["method"] == F.PWA:
            assert np.array_equal(golden[f"{name}_ref_tri"], tri) and np.array_equal(golden[f"{name}_ref_extrapolated"], (flags & F.EXTRAPOLATED) != 0)
    if model["dist"] is not None:
        ux, uy = F.undistort(pts[:, 0], pts[:, 1], model["dist"])
        rx, ry = F.distort(ux, uy, model["dist"])
        assert max(np.abs(rx - pts[:, 0]).max(), np.abs(ry - pts[:, 1]).max()) == float(golden[f"{name}_e_rt"]) < 1e-3


def test_new_names_in_the_binding_the_header_and_the_product_library():
    header = open(os.path.join(ROOT, "include", "opd_detr.h")).read()
    for name in NEW:
        assert name in _capi.API and re.search(r"OPD_API\s+\w+\s+" + name + r"\s*\(", header), name
    assert "opd_floor_test_tables" in _capi.TEST_API and "opd_floor_test_tables" not in header
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {l.split()[2] for l in out.splitlines() if len(l.split()) == 3}
    assert set(NEW) <= exported and "opd_floor_test_tables" not in exported and "opd_launch_floor" not in exported
    assert C.sizeof(_capi.OpdFloorRec) == 48 == F.REC_DTYPE.itemsize == FL.REC_DTYPE.itemsize
    assert [f[0] for f in _capi.OpdFloorRec._fields_] == list(F.REC_DTYPE.names)
    m = re.search(r"typedef struct opd_floor_config \{(.*?)\} opd_floor_config;", header, re.S)
    fields = re.findall(r"(?:int32_t|double|const double\*|const int32_t\*)\s+([^;]+);", m.group(1))
    names = [n.split("[")[0].strip() for f in fields for n in f.split(",")]
    assert names == [f[0] for f in _capi.OpdFloorConfig._fields_]
    assert C.sizeof(_capi.OpdFloorConfig) == 8 * 4 + (9 + 2 + 4 + 5 + 6) * 8 + 7 * 8
    lib = _capi.load_library()
    assert lib.opd_floor_transform.argtypes == _capi.API["opd_floor_transform"][1]


def _refused(lib, model, text, **patch):
    cfg, keep = F.make_config(model)
    for k, v in patch.items():
        setattr(cfg, k, v)
    h = C.c_void_p()
    rc = lib.opd_floor_create(C.byref(cfg), 0, C.byref(h))
    assert rc == _capi.OPD_EINVAL and h.value is None, (patch, rc)
    assert text in _capi.last_error(), (patch, _capi.last_error())


def test_bad_configurations_are_refused_before_any_device_call(golden):
    lib = _capi.load_library()
    pwa, tps, hom = (F.case_model(golden, n) for n in ("pwa_t_small", "tps_n64", "homography_config"))
    _refused(lib, hom, "unknown method", method=7)
    sing = dict(hom, H=np.array([1.0, 2, 3, 2, 4, 6, 0, 0, 1]))
    _refused(lib, sing, "singular")
    _refused(lib, dict(hom, H=np.eye(3).reshape(9) * 1e-4), "singular")          # det = 1e-12
    _refused(lib, pwa, "at least 3 control points", n_points=2)
    _refused(lib, tps, "at least 3 control points", n_points=0)
    rng = np.random.default_rng(0)
    many = rng.uniform(0, 1000, (257, 2))
    _refused(lib, dict(tps, points=many, tps_w=np.zeros((257, 2))), "control points, the limit is 256")
    _refused(lib, dict(pwa, triangles=np.zeros((513, 3), np.int32), affine=np.zeros((513, 6))), "triangles, the limit is 512")
    _refused(lib, pwa, "at least one triangle", n_triangles=0)
    bad = pwa["triangles"].copy()
    bad[3, 1] = len(pwa["points"])
    _refused(lib, dict(pwa, triangles=bad), f"triangle 3 names point {len(pwa['points'])}")
    bad[3, 1] = -1
    _refused(lib, dict(pwa, triangles=bad), "triangle 3 names point -1")
    square = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], float)
    _refused(lib, dict(hom, zones=[square] * 65, priority=np.full(65, np.nan)), "65 zones, the limit is 64")
    _refused(lib, dict(hom, zones=[square, square[:2]], priority=np.full(2, np.nan)), "zone 1 has 2 vertices")
    _refused(lib, dict(hom, zones=[np.zeros((65, 2))], priority=np.full(1, np.nan)), "zone 0 has 65 vertices")
    _refused(lib, pwa, "null control points", points=None)
    _refused(lib, pwa, "null triangles", affine=None)
    _refused(lib, tps, "null spline weights", tps_weights=None)
    _refused(lib, dict(pwa, dist=np.array([0.0, 1250, 640, 360, -0.1, 0, 0, 0, 0])), "focal lengths")
    _refused(lib, hom, "at least 1 x 1", width_px=0)
    assert lib.opd_floor_create(None, 0, C.byref(C.c_void_p())) == _capi.OPD_EINVAL and "null configuration" in _capi.last_error()
    # arguments of the calls: a null handle is refused before anything else
    rec = np.zeros(1, F.REC_DTYPE)
    box = np.zeros((1, 4), np.float32)
    assert lib.opd_floor_transform(None, box.ctypes.data, 1, _capi.OPD_MEM_HOST, rec.ctypes.data) == _capi.OPD_EINVAL and "null handle" in _capi.last_error()
    assert lib.opd_floor_transform_points(None, rec.ctypes.data, 1, rec.ctypes.data) == _capi.OPD_EINVAL
    assert lib.opd_floor_classify(None, rec.ctypes.data, 1, rec.ctypes.data) == _capi.OPD_EINVAL
    assert lib.opd_floor_info(None, None) == _capi.OPD_EINVAL
    ptrs = (C.c_void_p * 1)(box.ctypes.data)
    assert lib.opd_detr_detect_frames_floor(None, None, ptrs, 1, 32, 32, 32, 32, 0.5, 1, None, None, None) == _capi.OPD_EINVAL
    assert "null floor-map handle" in _capi.last_error()
    lib.opd_floor_destroy(None)   # a no-op


@pytest.mark.parametrize("name", ["pwa_n3", "pwa_t_big", "tps_n3", "pwa_overlap_all"])
def test_host_tables_equal_the_restatement(golden, name):
    """What creation uploads: the triangles' inverse matrices and centroids bit for bit, the polygon edges in the reference's order, the ranks."""
    lib = _capi.load_library()
    model = F.case_model(golden, name)
    cfg, keep = F.make_config(model)
    T, Z = len(model["triangles"]) if model["method"] == F.PWA else 0, len(model["zones"])
    E = int(sum(len(z) for z in model["zones"]))
    tri, edges, ez, rank, ne = np.zeros((T, 8)), np.zeros((E, 4)), np.zeros(E, np.int32), np.zeros(Z, np.int32), C.c_int(-1)
    _capi.check(lib.opd_floor_test_tables(C.byref(cfg), tri.ctypes.data, edges.ctypes.data, ez.ctypes.data, E, rank.ctypes.data, C.byref(ne)), "opd_floor_test_tables")
    assert ne.value == E
    if T:
        assert np.array_equal(tri, F.triangle_tables(model["points"], model["triangles"]))
    want = np.concatenate([np.concatenate([z, np.roll(z, -1, axis=0)], 1) for z in model["zones"]])
    assert np.array_equal(edges, want) and np.array_equal(ez, np.repeat(np.arange(Z), [len(z) for z in model["zones"]]))
    assert np.array_equal(rank, F.zone_ranks(model["priority"], Z))
    if E:
        assert lib.opd_floor_test_tables(C.byref(cfg), None, edges.ctypes.data, None, E - 1, None, None) == _capi.OPD_EINVAL


def test_zone_ranks_follow_priority_then_order():
    assert F.zone_ranks([np.nan, 2.0, 1.0, 2.0, np.nan], 5).tolist() == [3, 1, 0, 2, 4]
    assert F.zone_ranks(None, 3).tolist() == [0, 1, 2]
    model = {"zones": [np.array([[0, 0], [10, 0], [10, 10], [0, 10]], float)] * 3, "priority": np.array([np.nan, 5.0, 5.0]), "allow_overlap": False}
    assert F.classify(model, [5.0, 20.0], [5.0, 5.0]).tolist() == [2, 0]
    assert F.classify(dict(model, allow_overlap=True), [5.0], [5.0]).tolist() == [7]


def test_model_builders_and_from_config(tmp_path):
    rng = np.random.default_rng(1)
    src = rng.uniform(0, 1000, (12, 2))
    dst = src * 1.5 + 7
    pts = tmp_path / "points.json"
    pts.write_text(json.dumps({"point_correspondences": [{"src_point": s.tolist(), "dst_point": d.tolist()} for s, d in zip(src, dst)]}))
    base = {"homography": {"matrix": H}, "zones": ZONES, "calibration": {"correspondence_file": str(pts)}}
    m = FL.model_from_config(base)                                              # no transform section: the homography, the default floor map
    assert m["method"] == F.HOMOGRAPHY and m["fm"].tolist() == list(FM) and not m["allow_overlap"] and m["dist"] is None
    assert m["zone_ids"] == ["zone_1", "zone_2", "zone_3"] and m["priority"].tolist() == [1.0, 2.0, 3.0]
    assert FL.model_from_config(dict(base, transform={"method": "kriging"}))["method"] == F.HOMOGRAPHY      # unknown: falls back
    with pytest.raises(ValueError, match="homography.matrix"):
        FL.model_from_config({"zones": ZONES})
    dist_on = {"enabled": True, "k1": -0.1, "p2": 1e-3, "center_x": 600.0}
    m = FL.model_from_config(dict(base, transform={"method": "homography", "lens_distortion": dist_on}))
    assert m["dist"] is None                                                    # distortion is ignored for the homography
    m = FL.model_from_config(dict(base, transform={"method": "piecewise_affine", "lens_distortion": dist_on}, camera_params={"focal_length": 1100.0},
                                  floormap={"image_width": 100, "image_height": 50, "image_x_mm_per_pixel": 2.0}))
    assert m["method"] == F.PWA and m["dist"].tolist() == [1100.0, 1100.0, 600.0, 360.0, -0.1, 0.0, 0.0, 1e-3, 0.0]
    assert m["fm"].tolist() == [100, 50, 2.0, 28.241430700447] and len(m["points"]) == 12 and m["affine"].shape == (len(m["triangles"]), 6)
    a = m["affine"][0]                                                          # dst = 1.5 src + 7 on every triangle
    assert np.allclose(a, [1.5, 0, 7, 0, 1.5, 7], atol=1e-9)
    for d in ({"enabled": False, "k1": -0.1}, {"enabled": True}, {"enabled": True, "k1": 1e-11}):
        assert FL.model_from_config(dict(base, transform={"method": "thin_plate_spline", "lens_distortion": d}))["dist"] is None
    m = FL.model_from_config(dict(base, transform={"method": "thin_plate_spline"}))
    assert m["method"] == F.TPS and m["tps_w"].shape == (12, 2) and np.abs(m["tps_w"]).max() < 1e-6           # an affine map has no bending part
    assert np.allclose(m["tps_affine"], [7, 1.5, 0, 7, 0, 1.5], atol=1e-6)
    with pytest.raises(ValueError, match="correspondence_file"):
        FL.model_from_config({"transform": {"method": "piecewise_affine"}})
    with pytest.raises(ValueError, match="at least 3"):
        FL.model_piecewise_affine(src[:2], dst[:2], FM, [])
    with pytest.raises(ValueError, match="singular"):
        FL.model_homography(np.zeros((3, 3)), FM, [])
    with pytest.raises(ValueError, match="duplicate zone id"):
        FL.model_homography(H, FM, [ZONES[0], ZONES[0]])
    with pytest.raises(ValueError, match="at least 3 vertices"):
        FL.model_homography(H, FM, [{"id": "a", "polygon": [[0, 0], [1, 1]]}])
    given = FL.model_piecewise_affine(src, dst, FM, [], simplices=[[0, 1, 2]])   # triangles handed in: no triangulation
    assert given["triangles"].tolist() == [[0, 1, 2]] and given["triangles"].dtype == np.int32


def test_scipy_absent_is_a_clear_error(monkeypatch):
    import builtins
    real = builtins.__import__

    def no_scipy(name, *a, **k):
        if name.startswith("scipy"):
            raise ImportError("no scipy here")
        return real(name, *a, **k)
    monkeypatch.setattr(builtins, "__import__", no_scipy)
    src = np.array([[0, 0], [10, 0], [0, 10], [10, 10]], float)
    with pytest.raises(RuntimeError, match="scipy is not installed; pass the triangles"):
        FL.model_piecewise_affine(src, src, FM, [])
    assert len(FL.model_piecewise_affine(src, src, FM, [], simplices=[[0, 1, 2], [1, 2, 3]])["triangles"]) == 2


def test_apply_and_zone_counts_on_a_stubbed_library(monkeypatch):
    calls = []

    class FakeLib:
        def opd_floor_create(self, cfg, device, out):
            calls.append(("create", cfg._obj.method, cfg._obj.n_zones, cfg._obj.allow_overlap, device))
            out._obj.value = 1
            return 0

        def opd_floor_transform(self, handle, boxes, n, kind, out):
            b = np.ctypeslib.as_array((C.c_float * (4 * n)).from_address(boxes)).reshape(n, 4)
            calls.append(("transform", n, kind, b.copy()))
            rec = np.ctypeslib.as_array((C.c_uint8 * (48 * n)).from_address(out)).view(F.REC_DTYPE)
            for i in range(n):
                rec[i]["px"] = (100.0 + i, 200.0 + i)
                rec[i]["mm"] = (1000.0 + i, 2000.0 + i)
                rec[i]["zone_mask"] = [0b101, 0, 0b010][i % 3]
                rec[i]["flags"] = F.VALID | (F.WITHIN if i % 2 == 0 else 0)
                rec[i]["triangle"] = -1
            return 0

        def opd_floor_destroy(self, handle):
            calls.append(("destroy",))

    monkeypatch.setattr(_capi, "load_library", lambda *a, **k: FakeLib())
    m = HipFloorMapper.homography(H, FM, ZONES, allow_overlap=True, device=2)
    assert calls == [("create", 0, 3, 1, 2)] and m.method == "homography" and m.zone_ids == ["zone_1", "zone_2", "zone_3"]
    dets = [Detection(bbox=(10.0, 20.0, 4.0, 6.0), confidence=0.9, class_id=1, class_name="person", camera_coords=(0.0, 0.0)),
            Detection(bbox=(1.5, 2.0, 3.0, 4.0), confidence=0.8, class_id=1, class_name="person", camera_coords=(0.0, 0.0), zone_ids=["stale"]),
            Detection(bbox=(30.5, 8.0, 3.0, 5.0), confidence=0.7, class_id=1, class_name="person", camera_coords=(0.0, 0.0))]
    assert m.apply(dets) is dets
    assert calls[-1][:3] == ("transform", 3, _capi.OPD_MEM_HOST) and calls[-1][3].dtype == np.float32
    assert calls[-1][3].tolist() == [[10.0, 20.0, 4.0, 6.0], [1.5, 2.0, 3.0, 4.0], [30.5, 8.0, 3.0, 5.0]]
    assert [d.floor_coords for d in dets] == [(100.0, 200.0), (101.0, 201.0), (102.0, 202.0)]
    assert [d.floor_coords_mm for d in dets] == [(1000.0, 2000.0), (1001.0, 2001.0), (1002.0, 2002.0)]
    assert [d.camera_coords for d in dets] == [(12.0, 26.0), (3.0, 6.0), (32.0, 13.0)]
    assert [d.zone_ids for d in dets] == [["zone_1", "zone_3"], [], ["zone_2"]]
    assert all(isinstance(v, float) for d in dets for v in d.floor_coords + d.floor_coords_mm)
    assert HipFloorMapper.zone_counts(dets) == {"zone_1": 1, "zone_3": 1, "unclassified": 1, "zone_2": 1}
    assert HipFloorMapper.zone_counts([]) == {}
    res = m.transform_batch([d.bbox for d in dets])
    assert [type(r).__name__ for r in res] == ["TransformResult"] * 3 and [r.is_within_bounds for r in res] == [True, False, True]
    assert res[1].floor_coords_px == (101.0, 201.0) and res[1].is_valid and res[1].error_reason is None
    n = len(calls)
    assert m.apply([]) == [] and m.transform_batch([]) == [] and m.classify_batch([]) == [] and len(calls) == n   # nothing to do: no call
    m.close()
    m.close()
    assert calls[-1] == ("destroy",) and calls.count(("destroy",)) == 1
    with pytest.raises(RuntimeError, match="closed"):
        m.apply(dets)
