"""The hybrid tracker without a device: the restatement (lwt_common.py) against what the reference's own ``LightweightTracker`` recorded in
tests/golden/lwt_sequences.npz (tools/gen_lwt_golden.py), the generator's conditions, the binding against the header, and the arguments
that are refused before the device is touched.

Exact (bit for bit): ids, counters, next ids, element types, and of the interpolate records every id, width and height and the whole box
of a track whose point was followed.  The final Kalman states lie within ``kalman_tol`` of the reference's, the value the generator
measured between the reference (BLAS products, LAPACK inverse) and the all-float64 restatement (x relative to max(1, |x|), P relative
to max |P|): the reference's own rounding (measured here: 1.06e-3 on empty_s13, at most 6.1e-6 elsewhere, against 4.34e-3).  The x and
y of a record that reports a Kalman-PREDICTED centre are a predicted position minus half the size.  The restatement evaluates in the
kernel's stated order, which no BLAS promises, so they cannot equal the reference's bit for bit; they lie within 8 x ``record_tol``,
which the generator measured on exactly these numbers between the reference and the all-float64 restatement (2.84e-5 relative to
max(1, |value|), so the bound is 0.23 px at x = 1000): two float32 evaluations of the same recurrence in different orders lie a few such
distances apart, not more."""

import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import lwt_common as LC
import track_common as TC
from office_person_detection_vit_amd import HipLightweightTracker, _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["opd_lwt_create", "opd_lwt_destroy", "opd_lwt_reset", "opd_lwt_info", "opd_lwt_update", "opd_lwt_interpolate", "opd_lwt_get"]
HOOK = "opd_test_lwt_interpolate_scripted"


@pytest.fixture(scope="module")
def golden():
    return np.load(LC.GOLDEN)


@pytest.fixture(scope="module")
def lib():
    return _capi.load_library()


@pytest.mark.parametrize("name", LC.sequence_names(np.load(LC.GOLDEN)))
def test_restatement_reproduces_the_reference(golden, name):
    params, frames = LC.sequence(golden, name)
    bound, rec_bound = float(golden["kalman_tol"]), 8 * float(golden["record_tol"])
    r = LC.Restatement(**params)
    worst = 0.0
    for f, fr in enumerate(frames):
        if fr["kind"] == "det":
            assert r.update(fr["boxes"]) == fr["ids"].tolist(), f
        else:
            assert len(fr["status"]) == len(r.pt_ids), f
            recs = r.interpolate(fr["next"], fr["status"])
            predicted = [q for q, fo in zip(recs, fr["rec_followed"]) if not fo]
            worst = max(worst, LC.records_error(predicted, fr["rec_boxes"][~fr["rec_followed"]]))
            assert LC.records_equal(recs, fr["rec_ids"], fr["rec_boxes"], fr["rec_followed"], rec_bound), f
        assert np.array_equal(r.counters(), fr["counters"]) and r.next_id == fr["next_id"], f
    x, P, is32, bbox = r.states()
    assert np.array_equal(is32, golden[f"{name}_final_is32"])
    assert np.array_equal(bbox.astype(np.float64)[:, 2:], golden[f"{name}_final_bbox"][:, 2:])
    err = TC.state_error(x, P, golden[f"{name}_final_x"], golden[f"{name}_final_P"])
    print(f"{name}: final states {err:.3e} from the reference's (bound {bound:.3e}), predicted records {worst:.3e} (bound {rec_bound:.3e})")
    assert err <= bound


def test_fixture_covers_the_classes_and_keeps_its_caps(golden):
    names = LC.sequence_names(golden)
    assert {n.split("_")[0] for n in names} == set(LC.CLASSES)
    assert int(golden["dropped"]) <= 0.1 * int(golden["drawn"]) and len(names) == int(golden["drawn"]) - int(golden["dropped"])
    assert 0 < float(golden["kalman_tol"]) < 1e-2 and 0 < float(golden["record_tol"]) < 1e-4
    lost = died = f32 = empty = 0
    for n in names:
        params, frames = LC.sequence(golden, n)
        assert len(frames) == 24 and [fr["kind"] for fr in frames] == ["det" if f % 4 == 0 else "interp" for f in range(24)]
        for fr in frames:
            if fr["kind"] == "det":
                assert np.array_equal(fr["boxes"] * 4, np.round(fr["boxes"] * 4)) and len(fr["boxes"]) <= 16   # quarter-pixel boxes
                empty += len(fr["boxes"]) == 0
            else:
                lost += int((fr["status"] == 0).sum())
                assert params["use_optical_flow"] or len(fr["status"]) == 0
        died += frames[-1]["next_id"] - 1 > len(frames[-1]["counters"])
        f32 += int(golden[f"{n}_final_is32"].sum())
    assert lost > 50 and died >= 3 and f32 >= 2 and empty >= 4
    # all points lost: every in-between frame after the first holds no point
    _, frames = LC.sequence(golden, [n for n in names if n.startswith("alllost")][0])
    assert all(len(fr["status"]) == 0 for f, fr in enumerate(frames) if fr["kind"] == "interp" and f % 4 != 1)
    # more detections than tracks, and the reverse
    counts = lambda n: [(len(fr["boxes"]), len(frames[f - 1]["counters"])) for f, fr in enumerate(frames) if fr["kind"] == "det" and f]   # noqa: E731
    _, frames = LC.sequence(golden, [n for n in names if n.startswith("moredets")][0])
    assert any(d > t for d, t in counts(0))
    _, frames = LC.sequence(golden, [n for n in names if n.startswith("moretracks")][0])
    assert any(d < t for d, t in counts(0))


def test_mixed_update_is_the_float64_update_on_a_float32_gain():
    rng = np.random.default_rng(3)
    x32 = np.array([100.25, 200.5, 1.5, -0.75], np.float32)
    P = (np.diag([100.0, 100.0, 1000.0, 1000.0]) + rng.uniform(0, 1, (4, 4))).astype(np.float32)
    z64, z32 = np.array([101.3, 199.1]), np.array([101.25, 199.0], np.float32)
    xa, Pa = LC.update(x32, P, z32)
    assert xa.dtype == np.float32 and Pa.dtype == np.float32
    xb, Pb = LC.update(x32, P, z64)
    assert xb.dtype == np.float64 and Pb.dtype == np.float32 and np.array_equal(Pa, Pb)
    K = LC.gain(P)
    assert K.dtype == np.float32
    want = x32.astype(np.float64) + (K[:, 0].astype(np.float64) * (z64[0] - float(x32[0])) + K[:, 1].astype(np.float64) * (z64[1] - float(x32[1])))
    assert np.array_equal(xb, want)
    xc, _ = LC.update(xb, P, z32)   # a float64 x stays float64 under a float32 point
    assert xc.dtype == np.float64
    xp, Pp = LC.predict(xb, P)
    assert xp.dtype == np.float64 and Pp.dtype == np.float32 and np.array_equal(Pp, TC.kalman_predict(x32, P)[1])


def test_binding_header_and_libraries_agree():
    import subprocess
    header = open(os.path.join(ROOT, "include", "opd_detr.h")).read()
    for name in NEW:
        assert name in _capi.API and re.search(r"OPD_API\s+\w+\s+" + name + r"\s*\(", header), name
    assert HOOK in _capi.TEST_API and HOOK not in header

    def exported(path):
        out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
        return {l.split()[2] for l in out.splitlines() if len(l.split()) == 3}
    prod, test = exported(_capi.LIB_PATH), exported(_capi.TEST_LIB_PATH)
    assert set(NEW) <= prod and HOOK not in prod and HOOK in test
    assert not {"opd_launch_lwt_update", "opd_launch_lwt_interp", "lwt_interp_finish"} & {n.split("(")[0] for n in prod | test}
    assert not [n for n in prod if "lwt_interp_finish" in n or "flow_enqueue" in n]
    types = {"int32_t": C.c_int32, "double": C.c_double, "float": C.c_float, "opd_flow_config": _capi.OpdFlowConfig}
    for struct, cname, size in ((_capi.OpdLwtConfig, "opd_lwt_config", 8 * 4 + 8 + 32), (_capi.OpdLwtRec, "opd_lwt_rec", 40),
                                (_capi.OpdLwtTrack, "opd_lwt_track", 6 * 4 + 10 * 8 + 64), (_capi.OpdLwtStatus, "opd_lwt_status", 10 * 4 + 8)):
        m = re.search(r"typedef struct " + cname + r" \{(.*?)\} " + cname + ";", header, re.S)
        body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        fields = []
        for ty, names in re.findall(r"(int32_t|double|float|opd_flow_config)\s+([^;]+);", body):
            for n in names.split(","):
                n = n.strip()
                dim = re.search(r"\[(\d+)\]", n)
                fields.append((n.split("[")[0], types[ty] * int(dim.group(1)) if dim else types[ty]))
        assert [f[0] for f in fields] == [f[0] for f in struct._fields_], cname
        assert all(a[1] is b[1] or (C.sizeof(a[1]) == C.sizeof(b[1]) and a[1]._type_ is b[1]._type_) for a, b in zip(fields, struct._fields_)), cname
        assert C.sizeof(struct) == size, cname
    assert "HipLightweightTracker" in __import__("office_person_detection_vit_amd").__all__


def test_arguments_are_refused_before_any_device_call(lib):
    def refused(text, **kw):
        cfg = _capi.OpdLwtConfig(struct_size=C.sizeof(_capi.OpdLwtConfig), **kw)
        h = C.c_void_p()
        assert lib.opd_lwt_create(C.byref(cfg), 0, C.byref(h)) == _capi.OPD_EINVAL and h.value is None, kw
        assert text in _capi.last_error(), (kw, _capi.last_error())
    refused("iou_threshold", iou_threshold=-0.1)
    refused("iou_threshold", iou_threshold=float("nan"))
    refused("max_tracks", max_tracks=1025)
    refused("max_dets", max_dets=1025)
    refused("max_dets", max_dets=-1)
    refused("max_age", max_age=-1)
    cfg = _capi.OpdLwtConfig(struct_size=8)
    h = C.c_void_p()
    assert lib.opd_lwt_create(C.byref(cfg), 0, C.byref(h)) == _capi.OPD_EINVAL and "struct_size" in _capi.last_error()
    n = C.c_int()
    assert lib.opd_lwt_update(None, None, 0, 0, 0, None, 0, None) == _capi.OPD_EINVAL
    assert lib.opd_lwt_interpolate(None, None, 0, 0, 0, None, 0, C.byref(n)) == _capi.OPD_EINVAL
    assert lib.opd_lwt_reset(None) == _capi.OPD_EINVAL and lib.opd_lwt_info(None, None) == _capi.OPD_EINVAL
    assert lib.opd_lwt_get(None, None, 0, C.byref(n)) == _capi.OPD_EINVAL
    lib.opd_lwt_destroy(None)


def test_class_surface_and_its_refusals(monkeypatch):
    sig = inspect.signature(HipLightweightTracker.__init__)
    got = {k: v.default for k, v in sig.parameters.items() if v.kind == v.POSITIONAL_OR_KEYWORD and k != "self"}
    assert got == LC.DEFAULTS and list(got) == list(LC.DEFAULTS)
    assert {k for k, v in sig.parameters.items() if v.kind == v.KEYWORD_ONLY} == {"device", "max_tracks"}
    for thr in (0, 0.0, -0.3, float("nan")):
        with pytest.raises(ValueError, match="iou_threshold"):
            HipLightweightTracker(iou_threshold=thr)
    t = HipLightweightTracker()
    assert t.tracks == [] and t.next_id == 1 and t.get_active_tracks() == [] and t.interpolate(None) == [] and t.info() is None
    t.reset()
    for name in ("update_with_detections", "interpolate", "reset", "get_active_tracks"):
        assert callable(getattr(t, name))
    monkeypatch.setattr(_capi, "_lib", None)
    monkeypatch.setattr(_capi, "LIB_PATH", "/nonexistent/libopd_hip.so")
    monkeypatch.setattr(_capi, "TEST_LIB_PATH", "/nonexistent/libopd_hip_test.so")
    with pytest.raises(RuntimeError, match="HIP extension not built"):
        HipLightweightTracker()
