"""Build the native libraries in-tree with hipcc for gfx950 (cross-compiles without a GPU):

  libopd_hip.so       the PRODUCT: exports exactly the functions of include/opd_detr.h (-fvisibility=hidden + OPD_API)
  libopd_hip_test.so  the same objects + the opd_*test*_api.o files (kernel-level hooks, bench / trace hooks, fusion switches, poison allocator): what tests/ and
                      tools/ load (`_capi.load_library(test_hooks=True)`); never loaded by the package on its own
"""

from __future__ import annotations

import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(HERE)
SOURCES = ["kernels_gemm.hip", "kernels_w8.hip", "kernels_btail.hip", "kernels_btail3.hip", "kernels_rowln.hip", "kernels_attn.hip", "kernels_misc.hip", "kernels_untyped.hip", "kernels_dec.hip", "kernels_reid.hip", "kernels_osnet.hip", "kernels_hist.hip", "kernels_flow.hip", "kernels_floor.hip", "kernels_track.hip", "kernels_lwt.hip", "kernels_crop.hip", "kernels_nms.hip", "kernels_tile.hip", "opd_loader.cpp", "opd_host.cpp", "opd_pack.cpp", "opd_model.cpp", "opd_weights.cpp", "opd_api.cpp", "opd_comm.cpp", "opd_dispatch.cpp", "opd_crop.cpp", "opd_reid.cpp", "opd_clip.cpp", "opd_osnet.cpp", "opd_color.cpp", "opd_flow.cpp", "opd_floor.cpp", "opd_assoc.cpp", "opd_track.cpp", "opd_lwt.cpp", "opd_test_api.cpp", "opd_test_bench_api.cpp", "opd_test_model_api.cpp", "opd_reid_test_api.cpp", "opd_osnet_test_api.cpp", "opd_flow_test_api.cpp", "opd_floor_test_api.cpp", "opd_track_test_api.cpp", "opd_track_streams_test_api.cpp", "opd_lwt_test_api.cpp", "opd_lwt_ingest_test_api.cpp", "opd_lwt_ingest_merged_test_api.cpp", "opd_crop_test_api.cpp", "opd_nms_test_api.cpp", "opd_tile_test_api.cpp", "opd_tile_stages_test_api.cpp", "opd_tile_reid_test_api.cpp"]
TEST_ONLY = {"opd_test_api.cpp", "opd_test_bench_api.cpp", "opd_test_model_api.cpp", "opd_reid_test_api.cpp", "opd_osnet_test_api.cpp", "opd_flow_test_api.cpp", "opd_floor_test_api.cpp", "opd_track_test_api.cpp", "opd_track_streams_test_api.cpp", "opd_lwt_test_api.cpp", "opd_lwt_ingest_test_api.cpp", "opd_lwt_ingest_merged_test_api.cpp", "opd_crop_test_api.cpp", "opd_nms_test_api.cpp", "opd_tile_test_api.cpp", "opd_tile_stages_test_api.cpp", "opd_tile_reid_test_api.cpp"}
# kernel files with 16-bit operands: ONE source, compiled for fp16 and (-DOPD_ELEM_BF16) for bf16 (opd_elem.h)
ELEM_SOURCES = ["kernels_gemm.hip", "kernels_w8.hip", "kernels_btail.hip", "kernels_btail3.hip", "kernels_rowln.hip", "kernels_attn.hip", "kernels_misc.hip"]
HEADERS = ["opd_kernels.h", "opd_elem.h", "opd_kprims.h", "opd_loader.h", "opd_host.h", "opd_pack.h", "opd_device.h", "opd_model.h", "opd_crop.h", "opd_nms.h", "opd_records.h", "opd_tile.h", "opd_reid.h", "opd_clip.h", "opd_osnet.h", "opd_flow.h", "opd_floor.h", "opd_assoc.h", "opd_track.h", "opd_lwt.h", "opd_test_util.h", "opd_track_test_rig.h", os.path.join("..", "..", "include", "opd_detr.h")]
# code-generation flags of every translation unit, and per file: the attention kernel consumes its S = K.Q^T accumulators with VALU right
# away, so its MFMAs should write VGPRs (the default AGPR form costs 56 v_accvgpr moves per key tile in a VALU-bound loop).
# tools/scan_dma_waits.py imports these: the ISA it checks must be the ISA that ships.
COMMON_FLAGS = ["-O3", "-fPIC", "-std=c++17", "--offload-arch=gfx950", "-Wall", "-Wno-unused-function", "-fvisibility=hidden"]
# the floor-map files (float64) and the tracker files (float32; the hybrid tracker's x in both) are pinned operation for operation to a numpy restatement: no fused
# multiply-adds, on the device or the host; the crop planner (float64) likewise to the host's Pillow tables, the suppression kernel
# (float32) to opd_person_nms, the seam merge of tiled detection (float64; kernel and host hook) to tiling.merge_tile_detections
EXTRA_FLAGS = {"kernels_attn.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form"], "kernels_floor.hip": ["-ffp-contract=off"], "kernels_crop.hip": ["-ffp-contract=off"], "kernels_nms.hip": ["-ffp-contract=off"],
               "opd_crop_test_api.cpp": ["-ffp-contract=off"], "opd_floor.cpp": ["-ffp-contract=off"],
               "kernels_track.hip": ["-ffp-contract=off"], "opd_track.cpp": ["-ffp-contract=off"], "kernels_lwt.hip": ["-ffp-contract=off"],
               "kernels_tile.hip": ["-ffp-contract=off"], "opd_tile_test_api.cpp": ["-ffp-contract=off"]}
BF16_FLAGS = ["-DOPD_ELEM_BF16=1"]


def hipcc_path() -> str:
    return os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def kernel_files(csrc: str = HERE) -> list:
    return sorted(f for f in os.listdir(csrc) if f.startswith("kernels_") and f.endswith(".hip"))


def device_asm(path: str, csrc: str = HERE) -> dict:
    """The gfx950 assembly of one kernel file as it ships, per instantiation ("f16", and "bf16" for an ELEM_SOURCES file): the compile
    step of tools/scan_dma_waits.py and tools/isa_fingerprint.py (`csrc`: the include directory -- another revision's sources)."""
    import tempfile
    base = os.path.basename(path)
    variants = [("f16", [])] + ([("bf16", BF16_FLAGS)] if base in ELEM_SOURCES and os.path.exists(os.path.join(csrc, "opd_elem.h")) else [])
    out = {}
    for tag, vflags in variants:
        with tempfile.NamedTemporaryFile(suffix=".s") as tmp:
            cmd = [hipcc_path()] + COMMON_FLAGS + EXTRA_FLAGS.get(base, []) + vflags + ["-S", "--cuda-device-only", "-I" + csrc, path, "-o", tmp.name]
            subprocess.check_call(cmd, stderr=subprocess.DEVNULL)
            out[tag] = open(tmp.name).read()
    return out


LIB = os.path.join(PKG, "libopd_hip.so")
TEST_LIB = os.path.join(PKG, "libopd_hip_test.so")


def _stale(target: str, deps) -> bool:
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) >= t for d in deps)


def build(verbose: bool = False, force: bool = False) -> str:
    hipcc = hipcc_path()
    objdir = os.path.join(HERE, "build")
    os.makedirs(objdir, exist_ok=True)
    hdrs = [os.path.join(HERE, h) for h in HEADERS]
    objs = []
    common, extra = COMMON_FLAGS, EXTRA_FLAGS
    jobs = []
    for src in SOURCES:
        sp = os.path.join(HERE, src)
        obj = os.path.join(objdir, os.path.splitext(src)[0] + ".o")
        objs.append(obj)
        if force or _stale(obj, [sp] + hdrs):
            jobs.append([hipcc] + common + extra.get(src, []) + (["-x", "hip"] if src.endswith(".cpp") else []) + ["-c", sp, "-o", obj])
        if src in ELEM_SOURCES:   # the bf16 instantiation of the same kernels
            obj16 = os.path.join(objdir, os.path.splitext(src)[0] + "_bf16.o")
            objs.append(obj16)
            if force or _stale(obj16, [sp] + hdrs):
                jobs.append([hipcc] + common + extra.get(src, []) + BF16_FLAGS + ["-c", sp, "-o", obj16])

    def compile_one(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True)

    if jobs:   # independent translation units: compile them side by side (bounded by MAX_JOBS, else the cores this process may use)
        from concurrent.futures import ThreadPoolExecutor
        cores = int(os.environ.get("MAX_JOBS") or 0) or len(os.sched_getaffinity(0))
        with ThreadPoolExecutor(max_workers=max(1, min(len(jobs), cores))) as pool:
            list(pool.map(compile_one, jobs))
    test_objs = {os.path.join(objdir, os.path.splitext(s)[0] + ".o") for s in TEST_ONLY}
    for lib, members in ((LIB, [o for o in objs if o not in test_objs]), (TEST_LIB, objs)):
        if force or _stale(lib, members):
            cmd = [hipcc, "-shared", "-fPIC", "--offload-arch=gfx950", "-o", lib] + members + ["-ldl"]
            if verbose:
                print(" ".join(cmd), flush=True)
            subprocess.run(cmd, check=True)
    return LIB


if __name__ == "__main__":
    print(build(verbose=True, force="--force" in sys.argv))
