"""Times the fused bottleneck tail against the three launches it replaces, at the batch-8 800x1333 trunk shapes.
Run on the GPU box:  python tools/bench_btail.py
--res-path: instead, the residual by LDS-DMA (default) against register loads (dbg bit 16) for the stage-2 tail shapes and one 64-channel
shape, four interleaved rounds in one process.
--sc2: instead, stage 2's first block with the stride-2 shortcut inside the tail against the 3x3, the dual-source expand and the next reduce
it replaces, four interleaved rounds in one process; each figure is the minimum over the rounds."""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from office_person_detection_vit_amd import _capi  # noqa: E402

lib = _capi.load_library(test_hooks=True)
SHAPES = [  # B, H, W, C1, C3, stride
    (8, 200, 334, 64, 64, 1),     # s0b0 / s0b1 tails (-> next block's reduce)
    (8, 200, 334, 64, 128, 1),    # s0b2 tail (-> s1b0.c0)
    (8, 200, 334, 64, 0, 1),
    (8, 200, 334, 128, 128, 2),   # s1b0 tail (stride-2 3x3)
    (8, 100, 167, 128, 128, 1),   # s1b1 / s1b2 tails
    (8, 100, 167, 128, 0, 1),     # s1b3 tail
    (8, 50, 84, 256, 256, 1),     # stage-3 tails (kernels_btail3.hip)
    (8, 50, 84, 256, 0, 1),       # last stage-3 tail
    (8, 67, 120, 256, 256, 1),    # r101 at 1066x1920 (configs[3]): 22 of these
]
if "--res-path" in sys.argv:
    for s in [(8, 200, 334, 128, 128, 2), (8, 100, 167, 128, 128, 1), (8, 100, 167, 128, 0, 1), (8, 200, 334, 64, 64, 1)]:
        t = {0: [], 16: []}
        for _ in range(4):
            for dbg in (0, 16):
                us = (C.c_float * 4)()
                _capi.check(lib.opd_test_bench_btail(*s, dbg, 20, us), "bench_btail")
                t[dbg].append(us[0])
        f = lambda v: " ".join("%7.1f" % x for x in v)
        print(f"{str(s):>28s}  LDS-DMA: {f(t[0])}  registers: {f(t[16])}  min {min(t[0]):.1f} / {min(t[16]):.1f} us = {min(t[0]) / min(t[16]):.4f}", flush=True)
    sys.exit(0)
if "--sc2" in sys.argv:
    for B, H, W, C3 in [(8, 200, 334, 128), (8, 200, 334, 0)]:
        rounds = []
        for _ in range(4):
            us = (C.c_float * 4)()
            _capi.check(lib.opd_test_bench_btail_sc2(B, H, W, C3, 0, 20, us), "bench_btail_sc2")
            rounds.append(list(us))
        best = [min(r[k] for r in rounds) for k in range(4)]
        chain = best[1] + best[2] + (best[3] if C3 else 0.0)
        print(f"{str((B, H, W, 128, C3, 2)):>28s}  fused {best[0]:7.1f} us   3x3 {best[1]:6.1f} + dual expand {best[2]:6.1f}" +
              (f" + reduce {best[3]:6.1f}" if C3 else "") + f" = {chain:7.1f} us   ratio {best[0] / chain:.3f}   fused per round: " +
              " ".join("%.1f" % r[0] for r in rounds), flush=True)
    sys.exit(0)
if "--s3" in sys.argv:
    SHAPES = SHAPES[-3:]
print(f"{'shape':>28s} {'fused us':>9s} {'c1':>7s} {'c2':>7s} {'c0n':>7s} {'unfused':>8s} {'TB/s fused':>10s}")
for s in SHAPES:
    B, H, W, C1, C3, st = s
    us = (C.c_float * 4)()
    _capi.check(lib.opd_test_bench_btail(B, H, W, C1, C3, st, 0, 20, us), "bench_btail")
    OH, OW = (H - 1) // st + 1, (W - 1) // st + 1
    M = B * OH * OW
    byt = (B * H * W * C1 + M * 4 * C1 * 2 + M * C3) * 2
    print(f"{str(s):>28s} {us[0]:9.1f} {us[1]:7.1f} {us[2]:7.1f} {us[3]:7.1f} {us[1] + us[2] + us[3]:8.1f} {byt / us[0] / 1e6:10.2f}", flush=True)

if "--ablate" in sys.argv:
    print("\nablations (us): full | no 3x3 loop | no stores | no residual | no stores+residual | 3x3 only | no 3x3, no stores, no residual | residual through VGPRs")
    for s in SHAPES:
        B, H, W, C1, C3, st = s
        t = []
        for dbg in (0, 1, 2, 4, 6, 8, 7, 16):
            us = (C.c_float * 4)()
            _capi.check(lib.opd_test_bench_btail(B, H, W, C1, C3, st, dbg, 20, us), "bench_btail")
            t.append(us[0])
        print(f"{str(s):>28s} " + " ".join(f"{v:8.1f}" for v in t), flush=True)

