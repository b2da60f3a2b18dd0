"""CPU-only tests of the device suppression's host side (csrc/opd_nms.h): the algorithm person_nms_kernel runs (rank by counting, one
128-bit mask per sorted position, serial scan), restated on the host by opd_test_nms_plan_host, equals opd_person_nms_batch on every
case of tests/nms_common.py; host suppression is idempotent (what sharding.assemble relies on when its records arrive suppressed);
opd_person_nms gives, byte for byte, what it gave before its IoU moved into opd_nms.h (tests/golden/nms_host.npz, recorded from that
build by tools/record_nms_golden.py); and the two new entry points are declared, prototyped and exported.  Every comparison is an
equality of bytes."""

import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import nms_common as N
from office_person_detection_vit_amd import _capi, sharding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = N.cases()
NEW_CALLS = ("opd_detr_set_nms", "opd_detr_nms_records")


@pytest.fixture(scope="module")
def lib():
    return _capi.load_library(test_hooks=True)


@pytest.fixture(scope="module")
def host_results(lib):
    """opd_person_nms_batch on every case, computed once."""
    out = {}
    for case in CASES:
        rc, dets, counts = N.run_host(lib.opd_person_nms_batch, case)
        assert rc == _capi.OPD_OK, case["name"]
        out[case["name"]] = (dets, counts)
    return out


def test_generator_covers_what_it_says(lib, host_results):
    names = {c["name"] for c in CASES}
    for stride in N.STRIDES:
        for n in N.SIZES:
            assert (f"size_n{n}_s{stride}" in names) == (n <= stride)
    assert any((c["counts"] < 0).any() and len(c["counts"]) == 3 for c in CASES)
    assert {float(c["thr"]) for c in CASES} >= {0.0, float(np.float32(0.4)), 1.0, 2.0}
    assert {c["label"] for c in CASES} >= {1, -1}
    N.assert_random_cases_mixed(lib, CASES)
    for case in CASES:
        N.assert_expectations(case, *host_results[case["name"]])
    # suppression happens somewhere and is absent somewhere; thresholds >= 1 only filter and sort
    kept = {c["name"]: int(host_results[c["name"]][1].clip(0).sum()) for c in CASES}
    assert kept["thr_1.0"] == kept["thr_2.0"] > kept["thr_0.4"] > kept["thr_0.0"] > 0
    assert kept["labels_all_s128"] > kept["labels_person_s128"]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_kernel_algorithm_on_the_host_equals_person_nms(lib, host_results, case):
    rc, dets, counts = N.run_host(lib.opd_test_nms_plan_host, case)
    assert rc == _capi.OPD_OK
    N.assert_same(case["name"], (dets, counts), host_results[case["name"]])
    # the padding slot's records, and everything of a frame the routine must not touch, are as they were
    for f in np.flatnonzero(case["counts"] < 0):
        assert dets[f].tobytes() == case["dets"][f].tobytes()


def test_plan_hook_refuses_what_the_kernel_refuses(lib):
    case = CASES[0]
    for stride in (0, 129, -1):
        bad = dict(case, stride=stride)
        assert N.run_host(lib.opd_test_nms_plan_host, bad)[0] == _capi.OPD_EINVAL
    over = dict(CASES[3], counts=np.int32([CASES[3]["stride"] + 1]))
    rc, dets, counts = N.run_host(lib.opd_test_nms_plan_host, over)
    assert rc == _capi.OPD_EINVAL and counts[0] == over["counts"][0] and dets.tobytes() == over["dets"].tobytes()


def test_host_nms_is_idempotent(lib, host_results):
    """Host suppression over already-suppressed records keeps them all, in the same order: sharding.assemble over device-suppressed
    records returns what it returns over raw ones."""
    for case in CASES:
        dets, counts = host_results[case["name"]]
        again = dict(case, dets=dets, counts=counts)
        rc, d2, c2 = N.run_host(lib.opd_person_nms_batch, again)
        assert rc == _capi.OPD_OK
        N.assert_same(case["name"] + " (second pass)", (d2, c2), (dets, counts))
    # ... and through sharding.assemble itself: raw records and suppressed records of a two-rank gather give the same detections
    case = next(c for c in CASES if c["name"] == "batch3_s100")
    dets, counts = host_results[case["name"]]
    sig = lambda frames: [[(d.bbox, d.confidence, d.query_index) for d in f] for f in frames]
    raw = sharding.assemble(case["dets"].view(np.int32).reshape(1, 3, 100, 8), case["counts"].reshape(1, 3), 2, 1, float(case["thr"]))
    sup = sharding.assemble(dets.view(np.int32).reshape(1, 3, 100, 8), counts.reshape(1, 3), 2, 1, float(case["thr"]))
    assert sig(raw) == sig(sup) and [len(f) for f in raw] == [int(c) for c in counts if c >= 0]


def test_person_nms_gives_what_it_gave_before_the_move(lib, golden_dir):
    gold = np.load(os.path.join(golden_dir, "nms_host.npz"))
    assert {k.rsplit(".", 1)[0] for k in gold.files} == {c["name"] for c in CASES}
    for case in CASES:
        name = case["name"]
        assert str(gold[name + ".digest"]) == N.input_digest(case), f"{name}: the generator no longer produces the recorded inputs"
        dets, counts = N.run_single(lib, case)
        assert np.array_equal(counts, gold[name + ".counts"]), name
        assert b"".join(N.kept_bytes(dets, counts)) == gold[name + ".kept"].tobytes(), name


def test_new_calls_are_declared_prototyped_and_exported():
    header = open(os.path.join(ROOT, "include", "opd_detr.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {l.split()[2] for l in nm.splitlines() if len(l.split()) == 3 and l.split()[1] == "T"}
    for name in NEW_CALLS:
        assert re.search(r"OPD_API int " + name + r"\(opd_detr\* m,", header), f"include/opd_detr.h does not declare {name}"
        assert name in _capi.API and name in exported
    assert "opd_test_nms_plan_host" in _capi.TEST_API and "opd_test_nms_plan_host" not in exported
    # handle checks that need no device
    lib = _capi.load_library(test_hooks=True)
    assert lib.opd_detr_set_nms(None, 1, 0.4) == _capi.OPD_EINVAL
    assert lib.opd_detr_nms_records(None, None, None, 1, 100, 1, 0.4) == _capi.OPD_EINVAL
