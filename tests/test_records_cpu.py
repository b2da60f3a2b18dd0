"""csrc/opd_records.h (where the records of a detect call lie, and how a record becomes a box and a row: one header for the host and for the six
kernels that read records) on the CPU, under AddressSanitizer + UBSan: compiled by g++ -fsanitize=address,undefined together with
tests/native/records_sanitized_driver.cpp, a stand-alone program that prints record_count, record_label, record_key and record_box64 of both record
forms, for the whole view and for every one-frame view.  What it prints is compared bit for bit with the numpy float64 expressions below."""

import os
import shutil
import subprocess

import numpy as np
import pytest

import record_view_common as RV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "office_person_detection_vit_amd", "csrc")
COUNTS = [-3, 11, 8, 3]   # below zero, above the stride, the stride itself, inside


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("records") / "records_sanitized_driver")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-I", CSRC,
           os.path.join(ROOT, "tests", "native", "records_sanitized_driver.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return exe


def _bits(v):
    return "%016x" % int(np.float64(v).view(np.uint64))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++ for the sanitizer build")
@pytest.mark.parametrize("form", ["post_process", "merged"])
def test_accessors_equal_numpy(driver, tmp_path, form):
    S = RV.S
    recs = np.concatenate([RV.dets([8, 3]), RV.dets([5, 0])] if form == "post_process" else [RV.merged([8, 3]), RV.merged([5, 0])])   # [4][S]
    path = str(tmp_path / "records.bin")
    with open(path, "wb") as fh:
        fh.write(np.asarray([0 if form == "post_process" else 1, 4, S, 0], np.int32).tobytes() + np.asarray(COUNTS, np.int32).tobytes() + recs.tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([driver, path], capture_output=True, text=True, env=env, timeout=120)
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    assert run.returncode == 0 and run.stdout.endswith("records done\n"), (run.returncode, run.stdout[-2000:], run.stderr[-2000:])

    f64 = np.float64
    want = []

    def view(tag, frames):
        """The lines of a view over `frames` (indices into recs): record idx = position in the view's own frame-major order."""
        for f, src in enumerate(frames):
            want.append(f"{tag} count {f} {min(max(COUNTS[src], 0), S)}")
        for idx in range(len(frames) * S):
            r = recs[frames[idx // S], idx % S]
            if form == "post_process":   # Detection.bbox = (x1, y1, x2 - x1, y2 - y1) in Python floats; the row is the query's
                box = (f64(r["x1"]), f64(r["y1"]), f64(r["x2"]) - f64(r["x1"]), f64(r["y2"]) - f64(r["y1"]))
                key = int(r["query_index"])
            else:                        # the four doubles as they are; the row is the position's
                box = (r["x"], r["y"], r["w"], r["h"])
                key = idx % S
            want.append(f"{tag} rec {idx} {int(r['label'])} {key} " + " ".join(_bits(v) for v in box))

    view("all", [0, 1, 2, 3])
    for f in range(4):
        view(f"frame{f}", [f])
    got = run.stdout.splitlines()[:-1]
    assert len(got) == len(want) == 2 * (4 + 4 * S)
    assert got == want, [(g, w) for g, w in zip(got, want) if g != w][:4]
    # the cases the kernels' filters and key tests are there for are among the records
    if form == "post_process":
        keys = [int(k) for k in recs["query_index"].reshape(-1)]
        assert S in keys and -1 in keys
    assert {int(v) for v in recs["label"].reshape(-1)} > {RV.LABEL}
    w32 = np.stack([recs["x2"].astype(f64) - recs["x1"].astype(f64)] if form == "post_process" else [recs["w"]]).reshape(-1)
    assert (w32.astype(np.float32).astype(f64) != w32).any(), "no width that float32 cannot hold: the float32 box would hide a second rounding"
