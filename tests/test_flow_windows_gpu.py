"""Lucas-Kanade on the device at every window edge and pyramid depth ``opd_flow_create`` accepts (3, 5 .. 21; one to eight levels), on
frames smaller than the window, with max_iter 1 and 5 and with two eigenvalue thresholds: ``opd_flow_*`` with each case's config
against tests/golden/flow_windows.npz, the float64 restatement of flow_common.py on the cases of flow_common.WINDOW_CASES (pinned by
test_flow_cpu.py, which also shows that the bounds below catch a kernel that kept the constant of the default window in one place).

Bounds, as in test_flow_gpu.py.  Every fixture point takes each decision at a recorded margin, so status is compared on every point.
At fixed work (a negative epsilon: the step-length stop is off) positions lie within 4 * d_f32 of the float64 restatement, d_f32 being
that case's largest |float32 restatement - float64 restatement| from the fixture (at most 2.5e-4 px by the generator's rule, so the
bound is at most 1e-3 px).  At the case's own criteria (epsilon = 0.01) within 2 * epsilon = 0.02 px.  Gray and pyramid are exact."""

import faulthandler

import numpy as np
import pytest
import torch

import flow_common as F
from office_person_detection_vit_amd import _capi
from office_person_detection_vit_amd.frames import noise_frame

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _time_limit():
    """Every test runs under its own limit: a hang ends the process (with a traceback) instead of holding the GPU."""
    faulthandler.dump_traceback_later(120, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def lib():
    return _capi.load_library(test_hooks=True)


@pytest.fixture(scope="module")
def windows():
    return F.load_windows()[0]


_PAIRS = {}


def _pair(name):
    """The case's two frames, built once (cases that share a seed and a config share the pair)."""
    h, w, seed, win, _, shift, more = F.WINDOW_CASES[name]
    key = (h, w, seed, win, F.window_top(name), shift, more.get("dim", False), more.get("grid", False))
    if key not in _PAIRS:
        _PAIRS[key] = F.window_pair(name)
    return _PAIRS[key]


class Flow:
    """A handle that is destroyed with the block."""

    def __init__(self, lib, h, w, max_points=64, **cfg):
        self.lib, self.h = lib, F.flow_create(lib, h, w, max_points, **cfg)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.lib.opd_flow_destroy(self.h)

    def pair(self, f0, f1, pts):
        F.flow_set_reference(self.lib, self.h, f0)
        return F.flow_track(self.lib, self.h, f1, pts)


def _check_fixed_work(name, g, got, st, note=""):
    bound = 4.0 * g["d_f32"]
    d = np.abs(got.astype(np.float64) - g["next_fixed"]).max(axis=1)
    print(f"{name}{note}: max |device - float64| = {d.max():.3e} (point {int(d.argmax())}), bound 4 * d_f32 = {bound:.3e}; "
          f"found {int(st.sum())} of {len(st)}")
    assert np.array_equal(st, g["status_fixed"])
    assert d.max() <= bound


@pytest.mark.parametrize("name", list(F.WINDOW_CASES))
def test_lk_parity_at_fixed_work(lib, windows, name):
    h, w = F.WINDOW_CASES[name][:2]
    g = windows[name]
    with Flow(lib, h, w, epsilon=-1.0, **F.window_handle_config(name)) as fl:
        got, st = fl.pair(*_pair(name), g["pts"])
        levels = len(F.flow_levels(lib, fl.h))
    assert levels == F.window_top(name) + 1                  # (the win = 13 boundary: three levels; the eight-level case: eight)
    _check_fixed_work(name, g, got, st)
    if h < F.WINDOW_CASES[name][3] and w < F.WINDOW_CASES[name][3]:
        assert levels == 1 and not st.any()                  # a frame smaller than the window: one level, every point lost


@pytest.mark.parametrize("name", list(F.WINDOW_CASES))
def test_lk_parity_at_the_case_criteria(lib, windows, name):
    h, w = F.WINDOW_CASES[name][:2]
    g = windows[name]
    with Flow(lib, h, w, epsilon=0.01, **F.window_handle_config(name)) as fl:
        got, st = fl.pair(*_pair(name), g["pts"])
    d = np.abs(got.astype(np.float64) - g["next_default"]).max(axis=1)
    print(f"{name}: epsilon 0.01, max |device - float64| = {d.max():.3e}, bound 0.02; found {int(st.sum())} of {len(st)}")
    assert np.array_equal(st, g["status_default"])
    assert d.max() <= 0.02


def test_the_two_thresholds_differ_on_the_device(lib, windows):
    hi, lo = "w9_eig1e-2", "w9_eig1e-6"
    st = {}
    for name in (hi, lo):
        h, w = F.WINDOW_CASES[name][:2]
        with Flow(lib, h, w, **F.window_handle_config(name)) as fl:
            st[name] = fl.pair(*_pair(name), windows[name]["pts"])[1]
    differ = st[hi] != st[lo]
    assert np.array_equal(differ, windows[hi]["status_default"] != windows[lo]["status_default"]) and differ.sum() >= 4
    assert (st[lo][differ] == 1).all()                       # found at 1e-6, lost at 1e-2


def test_one_handle_plans_its_levels_per_frame(lib, windows):
    """A handle created for 240 x 320 with win = 7 (top level 5 there) first on the 97 x 131 pair (top level 3), then on its own size."""
    small, large = "w7_97x131_l3", "w7_240x320_l7"
    assert F.WINDOW_CASES[small][3] == F.WINDOW_CASES[large][3] == 7 and F.window_top(small) == 3 and F.window_top(large) == 5
    # max_level 7 on the small frame ends at the same top level as the case's own max_level 3: level 4 would be 7 x 9
    assert F.top_level(97, 131, 7, 7) == 3
    with Flow(lib, 240, 320, epsilon=-1.0, **F.window_handle_config(large)) as fl:
        for name in (small, large, small):
            got, st = fl.pair(*_pair(name), windows[name]["pts"])
            assert len(F.flow_levels(lib, fl.h)) == F.window_top(name) + 1
            _check_fixed_work(name, windows[name], got, st, " in the 240x320 handle")


# ---- pyramids down to a few pixels -------------------------------------------------------------------------------------------------
SWEEP = [(h, w) for h in (9, 10) for w in range(4, 41)] + [(1, 1), (1, 7), (2, 3), (3, 2), (4, 4), (5, 9), (7, 16), (13, 17)]


def _same_levels(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for l, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and np.array_equal(g, w), (what, l, g.shape, w.shape, int((g != w).sum()) if g.shape == w.shape else None)


def test_small_pyramids_are_bit_exact(lib):
    """win = 3, max_level = 7: every residue of the row width against the four-pixel groups of the kernels, levels down to 4 x 5 (level
    l + 1 exists while it is wider and taller than 3), in one handle sized for the largest frame of the sweep."""
    depths = set()
    with Flow(lib, 13, 40, win=3, max_level=7) as fl:
        for h, w in SWEEP:
            frame = noise_frame(h, w, seed=100 * h + w)
            want = F.pyramid(frame, 3, 7)
            F.flow_set_reference(lib, fl.h, frame)
            _same_levels(F.flow_levels(lib, fl.h), want, (h, w))
            depths.add(len(want))
    assert depths == {1, 2, 3}


@pytest.mark.parametrize("hw,levels", [((13, 17), 3), ((520, 650), 8)])
def test_deep_pyramid_and_odd_device_address(lib, hw, levels):
    frame = noise_frame(hw[0], hw[1], seed=hw[0])
    want = F.pyramid(frame, 3, 7)
    assert len(want) == levels
    with Flow(lib, *hw, win=3, max_level=7) as fl:
        if hw == (520, 650):                                   # (13 x 17 from the host is part of the sweep above)
            F.flow_set_reference(lib, fl.h, frame)
            _same_levels(F.flow_levels(lib, fl.h), want, hw)
        # at an odd device address (byte loads instead of dwords): the same levels
        odd = torch.zeros(frame.size + 1, dtype=torch.uint8, device="cuda")
        odd[1:] = torch.from_numpy(frame).cuda().reshape(-1)
        torch.cuda.synchronize()
        F.flow_set_reference(lib, fl.h, (odd.data_ptr() + 1, hw[0], hw[1]), mem_kind=_capi.OPD_MEM_DEVICE)
        _same_levels(F.flow_levels(lib, fl.h), want, (hw, "odd address"))
