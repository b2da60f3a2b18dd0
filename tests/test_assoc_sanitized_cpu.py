"""csrc/opd_assoc.cpp (the assignment solver and the five-stage association of the tracker: pure C++, no HIP) under AddressSanitizer +
UBSan: compiled with g++ -fsanitize=address,undefined together with tests/native/assoc_sanitized_driver.cpp, a stand-alone program that
runs on the CPU over empty, single-row, single-column and rectangular matrices (checked against exhaustive search) and over the five
stages with every subset of tracks and detections empty in turn.  Any sanitizer report fails the test."""

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "office_person_detection_vit_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++ for the sanitizer build")
def test_association_under_address_and_ub_sanitizers(tmp_path):
    exe = str(tmp_path / "assoc_sanitized_driver")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-I", CSRC,
           os.path.join(ROOT, "tests", "native", "assoc_sanitized_driver.cpp"), os.path.join(CSRC, "opd_assoc.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    assert run.returncode == 0, (run.returncode, run.stdout[-3000:], run.stderr[-3000:])
    assert "solver cases done" in run.stdout and "failures 0" in run.stdout
    assert run.stdout.count("assoc T=") == 7 * 6 * 3
