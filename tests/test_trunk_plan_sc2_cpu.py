"""plan_trunk (csrc/opd_model.cpp) and the first block of stage 2.  Its route stays the dual-source one (3x3, then the expand over
[a1 | block input]: PATH_DUAL / SC_EXPAND, as tests/test_host_cpu.py pins it), and by default the step carries `one_launch`: the 3x3, that
expand and the next block's reduce are issued as ONE launch of the fused tail with the stride-2 shortcut inside (kernels_btail.hip, SC2; the
same operands, K order and bits).  OPD_SC2_TAIL=0 restores the three launches.  Through opd_test_trunk_plan_one_launch, which reads the
switches as opd_detr_create does.  The choice follows the handle's configuration, never the batch at hand."""

import numpy as np
import pytest

from office_person_detection_vit_amd import _capi
from test_host_cpu import DUAL, RES_NONE, RES_SHORTCUT, RES_TRUNK, SC_EXPAND, SC_LAUNCH, SC_NONE, STORE_Y, STORE_Y_STRIDE2, TAIL, trunk_plan

R50, R101 = (3, 4, 6, 3), (3, 4, 23, 3)


def _plan(monkeypatch, depths, env, max_batch=8, B=8, H=800, W=1333, flags=0):
    """([(path, sc, res, store, C3, rev, rev_b)], [(one_launch, one_C3, one_rev)]) per block under the environment switches `env`."""
    for k in ("OPD_SC2_TAIL", "OPD_DUAL_OVER_TAIL"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    lib = _capi.load_library()
    steps, one = np.zeros((64, 7), np.int32), np.zeros((64, 3), np.int32)
    d = np.asarray(depths, np.int32)
    n = lib.opd_test_trunk_plan_one_launch(d.ctypes.data, max_batch, flags, B, H, W, 256, steps.ctypes.data, one.ctypes.data, 64)
    assert n == sum(depths), lib.opd_last_error()
    return [tuple(int(v) for v in r) for r in steps[:n]], [tuple(int(v) for v in r) for r in one[:n]]


@pytest.mark.parametrize("depths", [R50, R101], ids=["r50", "r101"])
@pytest.mark.parametrize("max_batch,B,H,W,flags", [(8, 8, 800, 1333, 0), (8, 1, 800, 1333, 0), (1, 1, 256, 320, 0), (2, 2, 256, 320, _capi.OPD_FLAG_MULTI_STREAM)],
                         ids=["benchmark", "one_frame_of_eight", "small_handle", "multi_stream"])
def test_stage2_first_block_is_one_launch_on_the_dual_source_route(monkeypatch, depths, max_batch, B, H, W, flags):
    steps, one = _plan(monkeypatch, depths, {}, max_batch, B, H, W, flags)
    i = depths[0]
    assert steps[i] == (DUAL, SC_EXPAND, RES_NONE, STORE_Y, 0, 0, 0)
    assert one[i] == (1, 128, 1)          # with the next block's reduce inside; it starts on the rows stage 1's last tail wrote last
    assert [k for k, o in enumerate(one) if o[0]] == [i]   # stages 3 / 4 keep the dual-source expand as a launch of its own
    for s in (2, 3):
        assert steps[sum(depths[:s])][:5] == (DUAL, SC_EXPAND, RES_NONE, STORE_Y, 0)
    # stage 1's last tail still hands over z and stores y at the stride-2 positions, which is where this launch reads its shortcut input
    assert steps[i - 1][:5] == (TAIL, SC_NONE, RES_TRUNK, STORE_Y_STRIDE2, 128)
    # every other step, the tile directions of the tails included, is what the default-switch hook of tests/test_host_cpu.py reports
    assert steps == trunk_plan(_capi.load_library(), depths, max_batch, flags, B, H, W)[0]


@pytest.mark.parametrize("depths", [R50, R101], ids=["r50", "r101"])
def test_switch_off_restores_the_three_launches(monkeypatch, depths):
    i = depths[0]
    on, _ = _plan(monkeypatch, depths, {})
    steps, one = _plan(monkeypatch, depths, {"OPD_SC2_TAIL": "0"})
    assert steps == on and not any(o[0] for o in one)
    # the shortcut launch + residual tail route (OPD_DUAL_OVER_TAIL=0) is another route: nothing to issue as one launch there
    steps, one = _plan(monkeypatch, depths, {"OPD_DUAL_OVER_TAIL": "0"})
    assert steps[i][:5] == (TAIL, SC_LAUNCH, RES_SHORTCUT, STORE_Y, 128) and not any(o[0] for o in one)


def test_the_choice_does_not_depend_on_the_batch(monkeypatch):
    rows = {B: (_plan(monkeypatch, R50, {}, 8, B)[0][R50[0]][:5], _plan(monkeypatch, R50, {}, 8, B)[1][R50[0]]) for B in (1, 2, 5, 8)}
    assert len(set(rows.values())) == 1


def test_one_block_stage2_keeps_the_next_stage_reduce_as_a_launch(monkeypatch):
    """depths[1] == 1: the next block belongs to stage 3 (reduce 512 -> 256), which this kernel does not fuse: the C3 = 0 form."""
    steps, one = _plan(monkeypatch, (3, 1, 6, 3), {})
    assert steps[3][:5] == (DUAL, SC_EXPAND, RES_NONE, STORE_Y, 0) and one[3][:2] == (1, 0)
