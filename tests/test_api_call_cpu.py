"""The entry wrapper of the C-ABI (csrc/opd_device.h: api_call, lock then catch-all; csrc/opd_host.h: its lock-free form) under
AddressSanitizer + UBSan: tests/native/api_call_driver.cpp, a stand-alone program that makes no HIP call, is compiled for the host with
hipcc (opd_device.h includes the HIP runtime's header) together with csrc/opd_host.cpp and csrc/opd_loader.cpp and run on the CPU.  It
checks the code and the text of every kind of exception a body can throw, in the plain and the create flavour; nesting on one thread; a
capture's exclusive hold inside an entry point against a second thread's entry; the lock-free form against an exclusive holder.  Any
sanitizer report fails the test."""

import os
import subprocess

import pytest

from office_person_detection_vit_amd.csrc import build as native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "office_person_detection_vit_amd", "csrc")


@pytest.mark.skipif(not os.path.exists(native.hipcc_path()), reason="needs hipcc for the host build against the HIP headers")
def test_entry_wrapper_under_address_and_ub_sanitizers(tmp_path):
    exe = str(tmp_path / "api_call_driver")
    cmd = [native.hipcc_path(), "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-Wall", "-Xarch_host", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-I", CSRC, os.path.join(ROOT, "tests", "native", "api_call_driver.cpp"),
           os.path.join(CSRC, "opd_host.cpp"), os.path.join(CSRC, "opd_loader.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    assert run.returncode == 0, (run.returncode, run.stdout[-3000:], run.stderr[-3000:])
    for part in ("api_call: throwing bodies done", "api_call_unlocked: throwing bodies done", "nesting done", "capture done", "lock-free done"):
        assert part in run.stdout, run.stdout
    assert "api_call cases done, failures 0" in run.stdout
