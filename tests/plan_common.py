"""plan_transformer (csrc/opd_model.cpp) through its CPU hook, for tests/test_host_cpu.py (the plans pinned without a GPU) and
tests/test_arch_forward_gpu.py (the plan against the kernel table of a profiled forward)."""

import ctypes as C
import os

import numpy as np

from office_person_detection_vit_amd import _capi

# csrc/opd_model.h: the enums of TransformerPlan / EncStep
QKV_LAUNCH, QKV_PREV_TAIL = 0, 1
OPROJ_IN_FFN, OPROJ_GEMM_LN, OPROJ_GEMM_THEN_LN = 0, 1, 2
FFN_ONE_LAUNCH, FFN_FC1_DEEP, FFN_FC1_SPLITK = 0, 1, 2
HEADS_F32, HEADS_SPLIT16 = 0, 1
# csrc/opd_test_model_api.cpp::opd_test_transformer_plan: head_out
HEAD = ("shadow", "small_enc", "enc_splits", "proj_splits", "kv_launch", "dec_fused", "dec_splits", "dec0", "dec_small_m", "dec_oproj", "heads",
        "heads_ln3", "heads_ln", "token_bound")

R50 = (6, 6, 100, 92)   # encoder layers, decoder layers, queries, classifier rows


def transformer_plan(arch, bounds, B, H, W, env=None, flags=0):
    """The plan of a d_model 256 / 8 heads / FFN 2048 model with arch = (encoder layers, decoder layers, queries, classifier rows) in a handle
    of bounds = (max_height, max_width, max_batch), for B frames of H x W, under the environment switches `env` (set for the call only: the
    hook reads them as opd_detr_create does).  Returns ({field: value}, [(qkv, oproj, ffn, splits, tail) per encoder layer])."""
    lib = _capi.load_library()
    a7 = np.asarray((256, 8, 2048) + tuple(arch), np.int32)
    head, enc = np.zeros(len(HEAD), np.int32), np.zeros((64, 5), np.int32)
    env = env or {}
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        n = lib.opd_test_transformer_plan(a7.ctypes.data, bounds[2], bounds[0], bounds[1], flags, B, H, W, head.ctypes.data, enc.ctypes.data, 64)
    finally:
        for k, v in saved.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    assert n == arch[0], lib.opd_last_error()
    return dict(zip(HEAD, (int(v) for v in head))), [tuple(int(v) for v in r) for r in enc[:n]]
