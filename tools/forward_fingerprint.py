#!/usr/bin/env python3
"""Fingerprint of the forward's launch sequence and results, for refactors of csrc/opd_model.cpp: run it on the parent commit's build and on
the changed build, then compare the two JSON files -- they must be equal in every field.

    python tools/forward_fingerprint.py OUT.json

Per configuration (handle bounds, test hooks, environment switches, pixel format, batch shape) a fresh handle records
  taps      names and checksums of every launch's output, of an eager forward and of a graph replay (opd_test_set_taps)
  out       SHA-256 of logits, boxes and encoder_last_hidden_state with taps off, eager and replay
  kernels   profiling mode 1 on a detect call: the kernel table's (name, launches, flops) rows, kernel_times' launch and FLOP totals
and the benchmark shape (800 x 1333 x 8, the only one with the stage-3 frame split) its output hashes and which of the eight stage_times
entries are non-zero under profiling mode 2.  Only the seeded weights of weights.ensure_weight_file are used: the r50 architecture, and for
two routes it never takes -- the chain decoder (50 queries), the memory K/V launch behind an encoder with tails (9 decoder layers) -- the
one-block-per-stage architectures of tests/test_arch_forward_gpu.py.
"""
import ctypes as C
import hashlib
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from office_person_detection_vit_amd import _capi  # noqa: E402
from office_person_detection_vit_amd.detector import _feature_hw  # noqa: E402
from office_person_detection_vit_amd.frames import structured_frames  # noqa: E402
from office_person_detection_vit_amd.weights import DetrArch, ensure_weight_file  # noqa: E402

lib = _capi.load_library(test_hooks=True)
CACHE = os.path.join(tempfile.gettempdir(), "opd_weights")
MILD = ensure_weight_file(CACHE, DetrArch.resnet50(), 0, 1.0, "r50")
ARCHS = {"chain_q50": (1, 2, 50, 91), "kv_launch": (1, 9, 20, 91)}   # encoder layers, decoder layers, queries, labels
RAGGED_SIZES = ((256, 320), (224, 288))   # the two sizes of tests/golden/r50_mild_ragged.npz
VP = C.c_void_p


def sha(*arrays):
    return hashlib.sha256(b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)).hexdigest()


class Handle:
    def __init__(self, bounds, flags=0, env=None, arch=None):
        env = env or {}
        path = MILD
        if arch:
            e, d, q, l = ARCHS[arch]
            path = ensure_weight_file(CACHE, DetrArch(depths=(1, 1, 1, 1), encoder_layers=e, decoder_layers=d, num_queries=q, num_labels=l), 0, 1.0, "arch_" + arch)
        os.environ.update(env)
        try:
            cfg = _capi.OpdConfig(struct_size=C.sizeof(_capi.OpdConfig), max_batch=bounds[2], max_height=bounds[0], max_width=bounds[1], flags=flags)
            self.h = VP()
            _capi.check(lib.opd_detr_create(C.byref(cfg), path.encode(), 0, C.byref(self.h)), "opd_detr_create")
        finally:
            for k in env:
                del os.environ[k]
        info = _capi.OpdModelInfo()
        _capi.check(lib.opd_detr_info(self.h, C.byref(info)), "opd_detr_info")
        self.Q, self.rows, self.D = info.num_queries, info.num_classes_plus1, info.d_model

    def forward(self, pixels, fmt, B, H, W, valid=None):
        out = [np.zeros((B, self.Q, self.rows), np.float32), np.zeros((B, self.Q, 4), np.float32), np.zeros((B, _feature_hw(H) * _feature_hw(W), self.D), np.float32)]
        _capi.check(lib.opd_detr_forward_ragged(self.h, pixels.ctypes.data_as(VP), fmt, _capi.OPD_MEM_HOST, B, H, W,
                                                valid.ctypes.data_as(VP) if valid is not None else None, *[o.ctypes.data_as(VP) for o in out]), "forward")
        return sha(*out)

    def detect(self, pixels, fmt, B, H, W):
        hw = np.asarray([[H, W]] * B, np.int32)
        recs, cnts = np.zeros((B, self.Q, 8), np.int32), np.zeros(B, np.int32)
        _capi.check(lib.opd_detr_detect(self.h, pixels.ctypes.data_as(VP), fmt, _capi.OPD_MEM_HOST, B, H, W, 0.5, hw.ctypes.data_as(VP),
                                        recs.ctypes.data_as(C.POINTER(_capi.OpdDet)), cnts.ctypes.data_as(C.POINTER(C.c_int32))), "opd_detr_detect")

    def taps(self):
        sums, names = (C.c_ulonglong * 512)(), C.create_string_buffer(1 << 16)
        n = lib.opd_test_read_taps(self.h, sums, 512, names, len(names))
        return [[nm, int(sums[i])] for i, nm in enumerate(names.value.decode().split("\n")[:n])]

    def kernels(self):
        ms4, l4, f4 = (C.c_float * 4)(), (C.c_int32 * 4)(), (C.c_double * 4)()
        _capi.check(lib.opd_detr_kernel_times(self.h, ms4, l4, f4), "opd_detr_kernel_times")
        tab, n = (_capi.OpdKernelStat * 64)(), C.c_int(0)
        _capi.check(lib.opd_detr_kernel_table(self.h, tab, 64, C.byref(n)), "opd_detr_kernel_table")
        rows = sorted([tab[i].name.decode(), tab[i].launches, tab[i].flops] for i in range(n.value))   # (the table itself is ordered by time)
        return {"rows": rows, "launches": list(l4), "flops": list(f4)}

    def close(self):
        lib.opd_detr_destroy(self.h)


def fingerprint(bounds=(800, 1333, 2), flags=0, env=None, hook=None, f32=False, ragged=False, frames_n=2, arch=None):
    h = Handle(bounds, flags, env, arch)
    try:
        if hook:
            _capi.check(getattr(lib, hook[0])(h.h, hook[1]), hook[0])
        H, W = RAGGED_SIZES[0]
        frames = structured_frames(frames_n, H, W, seed=1234)
        valid = None
        if ragged:
            vh, vw = RAGGED_SIZES[1]
            valid = np.asarray(RAGGED_SIZES, np.int32)
            frames[1][vh:, :] = 0
            frames[1][:, vw:] = 0
        pixels, fmt = np.stack(frames), _capi.OPD_PIXELS_U8_BGR_HWC
        if f32:
            pixels, fmt = np.ascontiguousarray(pixels.transpose(0, 3, 1, 2)[:, ::-1].astype(np.float32) / 255.0 - 0.45), _capi.OPD_PIXELS_F32_NCHW
        args = (pixels, fmt, frames_n, H, W)
        fp = {}
        _capi.check(lib.opd_test_set_taps(h.h, 1), "opd_test_set_taps")
        h.forward(*args, valid)
        fp["taps_eager"] = h.taps()
        h.forward(*args, valid)   # capture (where the handle captures at all)
        h.forward(*args, valid)
        fp["taps_replay"] = h.taps()
        _capi.check(lib.opd_test_set_taps(h.h, 0), "opd_test_set_taps")
        fp["out"] = [h.forward(*args, valid) for _ in range(3)][::2]   # eager, replay
        if not ragged:
            _capi.check(lib.opd_detr_set_profiling(h.h, 1), "opd_detr_set_profiling")
            h.detect(*args)
            fp["kernels"] = h.kernels()
        return fp
    finally:
        h.close()


def bench_shape():
    h = Handle((800, 1333, 8))
    try:
        args = (np.stack(structured_frames(8, 800, 1333, seed=808)), _capi.OPD_PIXELS_U8_BGR_HWC, 8, 800, 1333)
        fp = {"out": [h.forward(*args) for _ in range(3)][::2]}
        _capi.check(lib.opd_detr_set_profiling(h.h, 2), "opd_detr_set_profiling")
        for _ in range(3):
            h.detect(*args)
        s8 = (C.c_float * 8)()
        _capi.check(lib.opd_detr_stage_times(h.h, s8), "opd_detr_stage_times")
        fp["stage_nonzero"] = [bool(v > 0) for v in s8]
        return fp
    finally:
        h.close()


def main(out_path):
    configs = {"fp16": {}, "bf16": {"flags": _capi.OPD_FLAG_BF16}, "small_handle": {"bounds": (256, 320, 1), "frames_n": 1}}
    for hook, values in (("opd_test_set_fuse_gemm_ln", (0,)), ("opd_test_set_fuse_btail", (0, 1, 3)), ("opd_test_set_pos_shadow", (0,)),
                         ("opd_test_set_fuse_stem_pool", (0, 1, 3))):
        for v in values:
            configs[f"{hook}({v})"] = {"hook": (hook, v)}
    for env in ({"OPD_TAIL3": "2"}, {"OPD_ENC_TAIL": "1"}, {"OPD_ENC_FRONT": "0"}, {"OPD_FUSED_ENC_FFN": "0"}, {"OPD_DEEP_FC2": "0"}, {"OPD_HEADS2": "0"},
                {"OPD_W8": "7"}, {"OPD_DUAL_OVER_TAIL": "0"}, {"OPD_SC2_TAIL": "0"}, {"OPD_TAIL_RC": "0", "OPD_Y_STRIDE2": "0"}, {"OPD_FUSED_DEC": "0"}):
        configs[" ".join(f"{k}={v}" for k, v in env.items())] = {"env": env}
    configs["OPD_TAIL3=2 multi_stream"] = {"env": {"OPD_TAIL3": "2"}, "flags": _capi.OPD_FLAG_MULTI_STREAM}
    configs["f32_pixels"] = {"f32": True}
    configs["ragged"] = {"ragged": True}
    configs["no_graph"] = {"flags": _capi.OPD_FLAG_NO_GRAPH}
    configs["chain_q50"] = {"arch": "chain_q50"}
    configs["kv_launch OPD_ENC_TAIL=1"] = {"arch": "kv_launch", "env": {"OPD_ENC_TAIL": "1"}}
    result = {}
    for name, kw in configs.items():
        result[name] = fingerprint(**kw)
        print(name, len(result[name]["taps_eager"]), "taps", flush=True)
    result["bench_shape"] = bench_shape()
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
    taps = sum(len(v.get("taps_eager", [])) + len(v.get("taps_replay", [])) for v in result.values())
    launches = sum(sum(v["kernels"]["launches"]) for v in result.values() if "kernels" in v)
    print(f"{len(result)} configurations, {taps} taps, {launches} profiled launches -> {out_path}")


if __name__ == "__main__":
    main(sys.argv[1])
