"""The tracker without a device: the assignment solver against scipy, the restatement (track_common.py) against the ids and Kalman states the
reference's own ``Tracker`` recorded in tests/golden/track_sequences.npz (tools/gen_track_golden.py), the ``HipTracker`` surface, and the
binding against the header.

The Kalman bound is 8 x ``kalman_tol``, the value the generator MEASURED between the reference's float32 states and the float64 restatement
(x relative to max(1, |x|), P relative to max |P|): two float32 evaluations of the same recurrences that differ in summation order and
in how the 2 x 2 matrix is inverted lie a few such distances apart, not more."""

import ctypes as C
import os
import re

import numpy as np
import pytest

import track_common as TC
from office_person_detection_vit_amd import Detection, HipTracker, _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["opd_track_create", "opd_track_destroy", "opd_track_reset", "opd_track_info", "opd_track_update", "opd_track_get", "opd_assign"]


@pytest.fixture(scope="module")
def golden():
    return np.load(TC.GOLDEN)


@pytest.fixture(scope="module")
def lib():
    return _capi.load_library()


def _assign(lib, cost):
    cost = np.ascontiguousarray(cost, np.float64)
    out = np.full(cost.shape[0], -9, np.int32)
    assert lib.opd_assign(TC.ptr(cost), cost.shape[0], cost.shape[1], TC.ptr(out)) == 0, _capi.last_error()
    return out


@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (7, 1), (5, 9), (9, 5)])
def test_assign_equals_scipy_on_generic_costs(lib, shape):
    from scipy.optimize import linear_sum_assignment
    rng = np.random.default_rng(shape[0] * 100 + shape[1])
    for _ in range(50):
        cost = rng.uniform(0, 2, shape)
        rows, cols = linear_sum_assignment(cost)
        want = np.full(shape[0], -1, np.int32)
        want[rows] = cols
        np.testing.assert_array_equal(_assign(lib, cost), want)


@pytest.mark.parametrize("shape", [(1, 7), (7, 1), (5, 9), (9, 5)])
def test_assign_with_gated_entries_has_the_optimal_cost(lib, shape):
    """Entries of exactly 1.0, as the gate writes them, make several assignments optimal: only the total is compared."""
    from scipy.optimize import linear_sum_assignment
    rng = np.random.default_rng(shape[0] * 10 + shape[1])
    for _ in range(50):
        cost = rng.uniform(0, 1, shape)
        cost[rng.random(shape) < 0.5] = 1.0
        got = _assign(lib, cost)
        rows, cols = linear_sum_assignment(cost)
        used = got[got >= 0]
        assert len(used) == min(shape) == len(set(used.tolist()))
        assert cost[np.nonzero(got >= 0)[0], used].sum() == pytest.approx(cost[rows, cols].sum(), abs=1e-12)


def test_assign_degenerate_sizes_and_arguments(lib):
    out = np.full(3, -9, np.int32)
    assert lib.opd_assign(None, 3, 0, TC.ptr(out)) == 0 and out.tolist() == [-1, -1, -1]
    assert lib.opd_assign(None, 0, 4, None) == 0
    assert lib.opd_assign(None, 2, 2, TC.ptr(out)) == _capi.OPD_EINVAL and "null cost" in _capi.last_error()
    assert lib.opd_assign(None, -1, 2, TC.ptr(out)) == _capi.OPD_EINVAL


def _run(golden, name, dtype):
    params, D, frames = TC.sequence(golden, name)
    r = TC.Restatement(D, dtype, **params)
    ids = [r.update(b, f, c, ft, h) for b, f, c, ft, h, _ in frames]
    return r, ids, [fr[5].tolist() for fr in frames]


@pytest.mark.parametrize("name", TC.sequence_names(np.load(TC.GOLDEN)))
def test_restatement_reproduces_the_reference(golden, name):
    bound = 8 * float(golden["kalman_tol"])
    for dtype in (np.float64, np.float32):
        r, ids, want = _run(golden, name, dtype)
        assert ids == want, dtype
        np.testing.assert_array_equal(r.counters(), golden[f"{name}_counters"])
        x, P = r.states()
        err = TC.state_error(x, P, golden[f"{name}_x"], golden[f"{name}_P"])
        print(f"{name} {np.dtype(dtype).name}: final states {err:.3e} from the reference's (bound {bound:.3e})")
        assert err <= bound


def test_fixture_covers_the_scenarios_and_keeps_its_caps(golden):
    names = TC.sequence_names(golden)
    assert {n.split("_")[0] for n in names} == {"steady", "occlusion", "lowconf", "nofeat", "mixed", "maxage", "gate", "ring", "empty"}
    assert {int(golden[f"{n}_D"]) for n in names} == {37, 256, 512}
    assert 0 < float(golden["kalman_tol"]) < 1e-3
    for n in names:
        counts = golden[f"{n}_counts"]
        assert len(counts) <= 40 and counts.max() <= 16 and len(golden[f"{n}_counters"]) <= 12
    assert (golden["lowconf_d37_s9_ids"] == -1).any()                        # a low-confidence detection that rescued nothing
    assert (golden["empty_d37_s26_counts"] == 0).sum() >= 3
    assert golden["maxage_d37_s17_ids"].max() > len(golden["maxage_d37_s17_counters"])   # tracks died


@pytest.mark.parametrize("name", ["steady_d37_s1", "lowconf_d37_s9", "maxage_d37_s17", "gate_d37_s20", "nofeat_d37_s12", "mixed_d256_s15"])
def test_native_solver_in_the_association_gives_the_reference_ids(lib, golden, name, monkeypatch):
    """The restatement with opd_assign in the place of scipy: the sub-blocks the stages solve have one optimal assignment wherever it matters."""
    import scipy.optimize as so

    def native(cost):
        a = _assign(lib, cost)
        rows = np.nonzero(a >= 0)[0]
        return rows, a[rows]
    monkeypatch.setattr(so, "linear_sum_assignment", native)
    r, ids, want = _run(golden, name, np.float32)
    assert ids == want


def test_hip_tracker_surface(monkeypatch):
    import inspect
    sig = inspect.signature(HipTracker.__init__)
    got = {k: v.default for k, v in sig.parameters.items() if v.kind == v.POSITIONAL_OR_KEYWORD and k != "self"}
    assert got == TC.DEFAULTS and list(got) == list(TC.DEFAULTS)
    t = HipTracker()
    assert t.tracks == [] and t.next_id == 1 and t.get_tracks() == [] and t.get_confirmed_tracks() == []
    t.reset()
    with pytest.raises(ValueError, match="camera_coords"):
        t.update([Detection(bbox=(1.0, 2.0, 3.0, 4.0), confidence=0.9, class_id=1, class_name="person", camera_coords=None)])
    with pytest.raises(ValueError, match="must equal 1.0"):
        HipTracker(appearance_weight=0.5, motion_weight=0.3)
    with pytest.raises(ValueError, match="width 3"):
        HipTracker(feature_dim=8).update([Detection((1.0, 2.0, 3.0, 4.0), 0.9, 1, "person", (2.5, 6.0), features=np.zeros(3, np.float32))])
    monkeypatch.setattr(_capi, "_lib", None)
    monkeypatch.setattr(_capi, "LIB_PATH", "/nonexistent/libopd_hip.so")
    monkeypatch.setattr(_capi, "TEST_LIB_PATH", "/nonexistent/libopd_hip_test.so")
    with pytest.raises(RuntimeError, match="HIP extension not built"):
        HipTracker()


def test_binding_header_and_product_library_agree():
    import subprocess
    header = open(os.path.join(ROOT, "include", "opd_detr.h")).read()
    for name in NEW:
        assert name in _capi.API and re.search(r"OPD_API\s+\w+\s+" + name + r"\s*\(", header), name
    hooks = {"opd_track_test_matrices", "opd_track_test_state"}
    assert hooks <= set(_capi.TEST_API) and not any(h in header for h in hooks)
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {l.split()[2] for l in out.splitlines() if len(l.split()) == 3}
    assert set(NEW) <= exported and not (hooks & exported) and "opd_launch_track_commit" not in exported
    m = re.search(r"typedef struct opd_track_config \{(.*?)\} opd_track_config;", header, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = [(ty, n.strip()) for ty, names in re.findall(r"(int32_t|double)\s+([^;]+);", body) for n in names.split(",")]
    assert [n for _, n in fields] == [f[0] for f in _capi.OpdTrackConfig._fields_]
    assert [C.c_int32 if ty == "int32_t" else C.c_double for ty, _ in fields] == [f[1] for f in _capi.OpdTrackConfig._fields_]
    assert C.sizeof(_capi.OpdTrackConfig) == 6 * 4 + 5 * 8 == 64
    assert C.sizeof(_capi.OpdTrackRec) == 4 * 4 + 16 + 16 == 48
    assert C.sizeof(_capi.OpdTrackStatus) == 10 * 4
    for struct, cname in ((_capi.OpdTrackRec, "opd_track_rec"), (_capi.OpdTrackStatus, "opd_track_status")):
        m = re.search(r"typedef struct " + cname + r" \{(.*?)\} " + cname + ";", header, re.S)
        body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        names = [n.split("[")[0].strip() for _, ns in re.findall(r"(int32_t|float)\s+([^;]+);", body) for n in ns.split(",")]
        assert names == [f[0] for f in struct._fields_], cname


def test_configurations_are_refused_before_any_device_call(lib):
    def refused(text, **kw):
        cfg = _capi.OpdTrackConfig(struct_size=C.sizeof(_capi.OpdTrackConfig), **kw)
        h = C.c_void_p()
        assert lib.opd_track_create(C.byref(cfg), 0, C.byref(h)) == _capi.OPD_EINVAL and h.value is None, kw
        assert text in _capi.last_error(), (kw, _capi.last_error())
    refused("max_tracks", max_tracks=1025)
    refused("max_dets", max_dets=-1)
    refused("feature_dim", feature_dim=4096)
    refused("must equal 1.0", appearance_weight=0.5, motion_weight=0.2)
    refused("negative", max_age=-1)
    cfg = _capi.OpdTrackConfig(struct_size=8)
    h = C.c_void_p()
    assert lib.opd_track_create(C.byref(cfg), 0, C.byref(h)) == _capi.OPD_EINVAL and "struct_size" in _capi.last_error()
    assert lib.opd_track_update(None, None, None, None, None, None, 0, 0, None) == _capi.OPD_EINVAL
    assert lib.opd_track_reset(None) == _capi.OPD_EINVAL and lib.opd_track_info(None, None) == _capi.OPD_EINVAL
    lib.opd_track_destroy(None)
