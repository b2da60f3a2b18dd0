#!/usr/bin/env python3
"""One line per compiled kernel unit: file, f16 / bf16, sha256 of its gfx950 assembly without the `__hip_cuid_<hash>` lines (they hash the
translation unit's text, not its code).  Two revisions whose lines are equal ship the same instructions: the check of a refactor that
moves device code between files.  Compiled exactly as tools/scan_dma_waits.py compiles (csrc/build.py::device_asm: the shipped flags, the
bf16 second instantiation of every ELEM_SOURCES file); OPD_SCAN_CSRC names another revision's csrc (a worktree).
usage: isa_fingerprint.py [kernels_*.hip ...]   (default: every kernel file)"""
import hashlib, os, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.environ.get("OPD_SCAN_CSRC") or os.path.join(ROOT, "office_person_detection_vit_amd", "csrc")
sys.path.insert(0, ROOT)
from office_person_detection_vit_amd.csrc import build as B   # noqa: E402

for f in sys.argv[1:] or B.kernel_files(CSRC):
    path = f if os.path.isabs(f) else os.path.join(CSRC, f)
    for tag, asm in B.device_asm(path, CSRC).items():
        kept = "".join(l for l in asm.splitlines(keepends=True) if "__hip_cuid_" not in l)
        print(f"{os.path.basename(path)} {tag} {hashlib.sha256(kept.encode()).hexdigest()}", flush=True)
