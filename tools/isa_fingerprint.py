#!/usr/bin/env python3
"""One line per compiled kernel unit: file, f16 / bf16, sha256 of its gfx950 assembly without the `__hip_cuid_<hash>` lines (they hash the
translation unit's text, not its code).  Two revisions whose lines are equal ship the same instructions: the check of a refactor that
moves device code between files.  Compiled exactly as tools/scan_dma_waits.py compiles (csrc/build.py::device_asm: the shipped flags, the
bf16 second instantiation of every ELEM_SOURCES file); OPD_SCAN_CSRC names another revision's csrc (a worktree).
--per-kernel: one line per kernel symbol and instantiation instead (file, f16 / bf16, sha256, symbol), for a refactor that moves kernels
between FILES: the hash covers the kernel's body (its label up to its `.Lfunc_end`) and its `.amdhsa_kernel` block, with the function
index taken out of local labels and of the comments that name them (`.LBBn_m` -> `.LBB_m`: n is the kernel's position in its file) and
the blanks in front of a `;` comment collapsed (its column follows the label's width).  A `__device__` function that is not inlined lies
outside every kernel's span and is not hashed in this mode: the per-file lines cover it.
usage: isa_fingerprint.py [--per-kernel] [kernels_*.hip ...]   (default: every kernel file)"""
import hashlib, os, re, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.environ.get("OPD_SCAN_CSRC") or os.path.join(ROOT, "office_person_detection_vit_amd", "csrc")
sys.path.insert(0, ROOT)
from office_person_detection_vit_amd.csrc import build as B   # noqa: E402


def kernels(asm: str) -> dict:
    """symbol -> the text that is hashed, for every `.amdhsa_kernel` of one assembly file"""
    lines = asm.splitlines(keepends=True)
    out = {}
    for i, l in enumerate(lines):
        if not l.lstrip().startswith(".amdhsa_kernel "):
            continue
        sym = l.split()[1]
        start = next(j for j in range(i, -1, -1) if lines[j].startswith(sym + ":"))
        body_end = next(j for j in range(i, len(lines)) if lines[j].startswith(".Lfunc_end"))
        desc_end = next(j for j in range(i, len(lines)) if lines[j].lstrip().startswith(".end_amdhsa_kernel"))
        body = [x for j, x in enumerate(lines[start:body_end]) if not i <= start + j <= desc_end]   # (the block sits inside the body's span)
        text = re.sub(r"\b(L?)BB\d+_", r"\1BB_","".join(body + lines[i:desc_end + 1]))   # labels, and the loop comments that name them
        out[sym] = re.sub(r"[ \t]+;", " ;", text)                                  # (a comment's column depends on its label's width)
    return out


args = [a for a in sys.argv[1:] if a != "--per-kernel"]
per_kernel = len(args) != len(sys.argv) - 1
for f in args or B.kernel_files(CSRC):
    path = f if os.path.isabs(f) else os.path.join(CSRC, f)
    for tag, asm in B.device_asm(path, CSRC).items():
        if per_kernel:
            for sym, text in sorted(kernels(asm).items()):
                print(f"{os.path.basename(path)} {tag} {hashlib.sha256(text.encode()).hexdigest()} {sym}", flush=True)
            continue
        kept = "".join(l for l in asm.splitlines(keepends=True) if "__hip_cuid_" not in l)
        print(f"{os.path.basename(path)} {tag} {hashlib.sha256(kept.encode()).hexdigest()}", flush=True)
