"""Record tests/golden/nms_host.npz: what opd_person_nms of a GIVEN build of libopd_hip.so makes of every case of tests/nms_common.py.

    python tools/record_nms_golden.py --lib path/to/libopd_hip.so [--out tests/golden/nms_host.npz]

The committed file was recorded from the build of the commit before the IoU moved into csrc/opd_nms.h; tests/test_nms_cpu.py holds the
current build to it byte for byte.  Per case: `<name>.counts`, `<name>.kept` (the first counts[f] records of each frame, concatenated, as
bytes) and `<name>.digest` (sha256 of the case's inputs, so that a drift of the generator shows as such)."""

import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import nms_common as N   # noqa: E402
from office_person_detection_vit_amd import _capi   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "nms_host.npz"))
    args = ap.parse_args()
    lib = C.CDLL(args.lib)
    lib.opd_person_nms.restype = C.c_int
    lib.opd_person_nms.argtypes = [C.POINTER(_capi.OpdDet), C.c_int, C.c_int, C.c_float]
    out = {}
    for case in N.cases():
        dets, counts = N.run_single(lib, case)
        out[case["name"] + ".counts"] = counts
        out[case["name"] + ".kept"] = np.frombuffer(b"".join(N.kept_bytes(dets, counts)), np.uint8)
        out[case["name"] + ".digest"] = np.array(N.input_digest(case))
    np.savez_compressed(args.out, **out)
    print(f"{args.out}: {len(out) // 3} cases, {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
