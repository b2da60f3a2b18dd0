"""Shared by the optical-flow tests (test_flow_cpu.py, test_flow_gpu.py, test_flow_windows_gpu.py), tools/gen_flow_golden.py,
tools/gen_flow_windows_golden.py and tools/bench_flow.py: a numpy
restatement of the pyramidal Lucas-Kanade contract of csrc/kernels_flow.hip (float64, or float32 with ``dtype=np.float32``), seeded
frame builders, the fixture's cases and the ctypes calls of the ``opd_flow_*`` entry points.

The contract is OpenCV's ``calcOpticalFlowPyrLK`` with the window interpolation and sums in floating point instead of 14-bit fixed
point; gray conversion and pyramid are integer and exact.  All points of a call are advanced together here (arrays [N][win][win]);
no point's arithmetic reads another point's."""

from __future__ import annotations

import ctypes as C
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "flow.npz")
FLT_EPSILON = float(np.finfo(np.float32).eps)
DEFAULTS = dict(win=21, max_level=3, max_iter=30, epsilon=0.01, min_eig=1e-4)
SHIFTS = ((0.3, -0.45), (3.7, -2.2), (12.4, 9.1))     # analytic displacements (dx, dy) in pixels; the last is 1.5 px at the top level
SHIFT_HW = (240, 320)
SHIFT_SEED = 77


# ---- the restatement --------------------------------------------------------------------------------------------------------------
def reflect101(i, n):
    """Index i of an n-long axis under reflect-101 (-1 -> 1, n -> n - 2), for any distance outside (period 2n - 2)."""
    i = np.asarray(i, np.int64)
    if n == 1:
        return np.zeros_like(i)
    p = 2 * n - 2
    i = np.mod(i, p)
    return np.where(i >= n, p - i, i)


def gray_u8(bgr):
    b, g, r = (bgr[..., k].astype(np.int64) for k in range(3))
    return ((1868 * b + 9617 * g + 4899 * r + 8192) >> 14).astype(np.uint8)


def pyr_down(src):
    h, w = src.shape
    oh, ow = (h + 1) // 2, (w + 1) // 2
    k = (1, 4, 6, 4, 1)
    s = src.astype(np.int64)
    rows = sum(k[i + 2] * s[reflect101(2 * np.arange(oh) + i, h)] for i in range(-2, 3))
    out = sum(k[j + 2] * rows[:, reflect101(2 * np.arange(ow) + j, w)] for j in range(-2, 3))
    return ((out + 128) >> 8).astype(np.uint8)


def top_level(h, w, win, max_level):
    """The effective top level: the largest l <= max_level with every level 1 .. l wider and taller than win."""
    L = 0
    for _ in range(max_level):
        h, w = (h + 1) // 2, (w + 1) // 2
        if h <= win or w <= win:
            break
        L += 1
    return L


def pyramid(bgr, win=21, max_level=3):
    levels = [gray_u8(np.asarray(bgr))]
    for _ in range(top_level(levels[0].shape[0], levels[0].shape[1], win, max_level)):
        levels.append(pyr_down(levels[-1]))
    return levels


def scharr(img):
    h, w = img.shape
    s = img.astype(np.int64)
    ym, yp = reflect101(np.arange(h) - 1, h), reflect101(np.arange(h) + 1, h)
    xm, xp = reflect101(np.arange(w) - 1, w), reflect101(np.arange(w) + 1, w)
    sx = 3 * (s[ym][:, xp] - s[ym][:, xm]) + 10 * (s[:, xp] - s[:, xm]) + 3 * (s[yp][:, xp] - s[yp][:, xm])
    sy = 3 * (s[yp][:, xm] - s[ym][:, xm]) + 10 * (s[yp] - s[ym]) + 3 * (s[yp][:, xp] - s[ym][:, xp])
    return sx, sy


def _padded(img, pad, reflect):
    h, w = img.shape
    if reflect:
        return img[reflect101(np.arange(-pad, h + pad), h)][:, reflect101(np.arange(-pad, w + pad), w)]
    out = np.zeros((h + 2 * pad, w + 2 * pad), img.dtype)
    out[pad:pad + h, pad:pad + w] = img
    return out


def _sample(padded, pad, top_left, win, T):
    """Bilinear samples [N][win][win] of a padded level at top_left + (x, y), x, y = 0 .. win - 1."""
    f = np.floor(top_left)
    ix, iy = f[:, 0].astype(np.int64) + pad, f[:, 1].astype(np.int64) + pad
    a, b = (top_left[:, 0] - f[:, 0]).astype(T)[:, None, None], (top_left[:, 1] - f[:, 1]).astype(T)[:, None, None]
    k = np.arange(win + 1)
    patch = padded[(iy[:, None] + k)[:, :, None], (ix[:, None] + k)[:, None, :]].astype(T)
    one = T(1)
    return ((one - a) * (one - b) * patch[:, :-1, :-1] + a * (one - b) * patch[:, :-1, 1:] + (one - a) * b * patch[:, 1:, :-1]
            + a * b * patch[:, 1:, 1:])


def _out_of_range(top_left, w, h, win):
    f = np.floor(top_left)
    return (f[:, 0] < -win) | (f[:, 0] >= w) | (f[:, 1] < -win) | (f[:, 1] >= h)


def _border_margin(top_left, w, h, win):
    """Distance of a window corner from the nearest limit of the range test (the test is floor(v) < -win or floor(v) >= size)."""
    x, y = top_left[:, 0].astype(np.float64), top_left[:, 1].astype(np.float64)
    return np.minimum(np.minimum(np.abs(x + win), np.abs(x - w)), np.minimum(np.abs(y + win), np.abs(y - h)))


# What a kernel that kept the default window's constant in one place would compute (``defect`` of lk_pyramids; test_flow_cpu.py shows
# that the fixture's bounds catch each of them): the last window sample or the partial last round of the lane map k = lane + 64 t left out
# of the sums, 21 in the range tests, 10 as the half-window offset, 2 * 441 as the eigenvalue's normalisation.
DEFECTS = ("last_sample", "partial_round", "range_21", "half_10", "eig_441")


def lk_pyramids(prev_levels, next_levels, pts, win=21, max_iter=30, epsilon=0.01, min_eig=1e-4, dtype=np.float64, diag=None, defect=None):
    """Pyramidal LK on two gray pyramids.  Returns (next_xy [N][2] of ``dtype``, status [N] uint8).  ``diag`` (a dict) receives per
    point the margins of every decision taken: 'border' (pixels of the level), 'eig' (factor between minEig or D and its threshold,
    >= 1 in either direction), 'stop' (distance of max |delta + delta_prev| from 0.01) and 'converged' (no level ran out of
    iterations).  ``defect`` (one of DEFECTS; off by default, and then nothing here differs) makes the one deliberate mistake named."""
    assert defect is None or defect in DEFECTS, defect
    T = dtype
    pts = np.asarray(pts, np.float32).reshape(-1, 2)
    N = len(pts)
    half = T(10 if defect == "half_10" else (win - 1) // 2)
    status = np.ones(N, np.uint8)
    centre = np.zeros((N, 2), T)
    m_border, m_eig, m_stop = np.full(N, np.inf), np.full(N, np.inf), np.full(N, np.inf)
    converged = np.ones(N, bool)
    rwin = 21 if defect == "range_21" else win                 # the window edge as the range tests see it
    eig_norm = 2 * 441 if defect == "eig_441" else 2 * win * win
    live_samples = None                                        # [win][win] 0 / 1: the window samples that enter the sums (None: all)
    if defect in ("last_sample", "partial_round"):
        first_out = win * win - 1 if defect == "last_sample" else 64 * (win * win // 64)
        live_samples = (np.arange(win * win) < first_out).astype(T).reshape(win, win)
    pad = rwin + 2
    L = len(prev_levels) - 1
    for l in range(L, -1, -1):
        I, J = prev_levels[l], next_levels[l]
        h, w = I.shape
        sx, sy = scharr(I)
        Ip, Jp, Sxp, Syp = _padded(I, pad, True), _padded(J, pad, True), _padded(sx, pad, False), _padded(sy, pad, False)
        q = pts.astype(T) * T(1.0 / (1 << l)) - half
        centre = q + half if l == L else centre * T(2)
        m_border = np.minimum(m_border, _border_margin(q, w, h, win))
        out = _out_of_range(q, w, h, rwin)
        if l == 0:
            status[out] = 0
        idx = np.flatnonzero(~out)
        if len(idx) == 0:
            continue
        Iw, Sx, Sy = (_sample(P, pad, q[idx], win, T) for P in (Ip, Sxp, Syp))
        if live_samples is not None:
            Sx, Sy = Sx * live_samples, Sy * live_samples      # every sum below carries a factor Sx or Sy
        scale = T(1.0 / (1 << 20))
        A11, A12, A22 = ((Sx * Sx).sum((1, 2)) * scale, (Sx * Sy).sum((1, 2)) * scale, (Sy * Sy).sum((1, 2)) * scale)
        D = A11 * A22 - A12 * A12
        eig = (A22 + A11 - np.sqrt((A11 - A22) * (A11 - A22) + T(4) * A12 * A12)) / T(eig_norm)
        with np.errstate(divide="ignore"):
            for v, thr in ((eig, min_eig), (D, FLT_EPSILON)):
                r = np.abs(v.astype(np.float64)) / thr
                m_eig[idx] = np.minimum(m_eig[idx], np.where(v.astype(np.float64) <= 0, np.inf, np.maximum(r, 1.0 / r)))
        bad = (eig < T(min_eig)) | (D < T(FLT_EPSILON))
        if l == 0:
            status[idx[bad]] = 0
        idx, Iw, Sx, Sy, A11, A12, A22, D = (v[~bad] for v in (idx, Iw, Sx, Sy, A11, A12, A22, D))
        n = centre[idx] - half
        prev_delta = np.zeros_like(n)
        live = np.ones(len(idx), bool)
        for j in range(max_iter):
            k = np.flatnonzero(live)
            if len(k) == 0:
                break
            m_border[idx[k]] = np.minimum(m_border[idx[k]], _border_margin(n[k], w, h, win))
            out = _out_of_range(n[k], w, h, rwin)
            if l == 0:
                status[idx[k[out]]] = 0
            live[k[out]] = False
            k = k[~out]
            if len(k) == 0:
                break
            diff = _sample(Jp, pad, n[k], win, T) - Iw[k]
            b1, b2 = T(32) * (diff * Sx[k]).sum((1, 2)) * scale, T(32) * (diff * Sy[k]).sum((1, 2)) * scale
            delta = np.stack([(A12[k] * b2 - A22[k] * b1) / D[k], (A12[k] * b1 - A11[k] * b2) / D[k]], 1).astype(T)
            n[k] += delta
            small = (delta * delta).sum(1) <= T(epsilon) * T(epsilon)
            swing = np.abs(delta + prev_delta[k]).max(1)
            if j > 0:
                m_stop[idx[k[~small]]] = np.minimum(m_stop[idx[k[~small]]], np.abs(swing[~small].astype(np.float64) - 0.01))
            back = ~small & (j > 0) & (swing < T(0.01))
            n[k[back]] -= delta[back] * T(0.5)
            prev_delta[k] = delta
            live[k[small | back]] = False
        converged[idx[live]] = False
        centre[idx] = n + half
    if diag is not None:
        diag.update(border=m_border, eig=m_eig, stop=m_stop, converged=converged)
    return centre, status


def lk_restatement(prev_bgr, next_bgr, pts, win=21, max_level=3, max_iter=30, epsilon=0.01, min_eig=1e-4, dtype=np.float64, diag=None,
                   defect=None):
    return lk_pyramids(pyramid(prev_bgr, win, max_level), pyramid(next_bgr, win, max_level), pts, win, max_iter, epsilon, min_eig,
                       dtype, diag, defect)


# ---- frames -----------------------------------------------------------------------------------------------------------------------
FLAT_BGR = (60, 140, 200)


def flat_rect(h, w):
    """(y0, y1, x0, x1) of the flat rectangle painted into the structured pair: larger than a window plus the largest refinement."""
    rh, rw = min(64, h // 2), min(64, w // 2)
    y0, x0 = h // 8, w // 8
    return y0, y0 + rh, x0, x0 + rw


def structured_pair(h, w, seed, shift=(2, 1)):
    """A structured frame, and the same scene moved by the integer ``shift`` (dx, dy) (edge pixels repeated) with a little seeded noise;
    the flat rectangle stays where it is in both."""
    from office_person_detection_vit_amd.frames import structured_frame
    f0 = structured_frame(h, w, seed)
    dx, dy = shift
    ys, xs = np.clip(np.arange(h) - dy, 0, h - 1), np.clip(np.arange(w) - dx, 0, w - 1)
    rng = np.random.default_rng(seed + 1)
    f1 = np.clip(f0[ys][:, xs].astype(np.int16) + rng.integers(-2, 3, f0.shape), 0, 255).astype(np.uint8)
    y0, y1, x0, x1 = flat_rect(h, w)
    f0 = f0.copy()
    f0[y0:y1, x0:x1] = FLAT_BGR
    f1[y0:y1, x0:x1] = FLAT_BGR
    return np.ascontiguousarray(f0), np.ascontiguousarray(f1)


def analytic_frame(h, w, seed, dx=0.0, dy=0.0, waves=12):
    """A texture of ``waves`` low-frequency sinusoids per channel, evaluated at (x - dx, y - dy) and quantised to uint8: the frame
    with (dx, dy) is the frame without, displaced by exactly that."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    x, y = x - dx, y - dy
    out = np.empty((h, w, 3), np.uint8)
    for c in range(3):
        period = rng.uniform(16.0, 96.0, waves)
        theta = rng.uniform(0.0, 2.0 * np.pi, waves)
        phase = rng.uniform(0.0, 2.0 * np.pi, waves)
        amp = rng.uniform(0.5, 1.0, waves)
        amp *= 110.0 / amp.sum()
        v = 127.5 + sum(amp[k] * np.sin(2.0 * np.pi / period[k] * (np.cos(theta[k]) * x + np.sin(theta[k]) * y) + phase[k])
                        for k in range(waves))
        out[..., c] = np.clip(np.rint(v), 0, 255).astype(np.uint8)
    return out


def analytic_pair(shift, hw=SHIFT_HW, seed=SHIFT_SEED):
    return analytic_frame(hw[0], hw[1], seed), analytic_frame(hw[0], hw[1], seed, shift[0], shift[1])


def shift_points(hw=SHIFT_HW, margin=48, step=32):
    """A grid of points far enough inside that the window stays in the frame under the largest shift."""
    ys, xs = np.mgrid[margin:hw[0] - margin + 1:step, margin:hw[1] - margin + 1:step]
    return np.stack([xs.ravel() + 0.25, ys.ravel() + 0.5], 1).astype(np.float32)


# the fixture's LK cases on structured pairs: name -> (h, w, seed, number of points)
LK_CASES = {"97x131": (97, 131, 501, 100), "720x1280": (720, 1280, 502, 100)}


def special_points(h, w):
    """name -> (x, y): the lost-point cases of the structured pair (the generator moves them along y until every decision is clear)."""
    y0, y1, x0, x1 = flat_rect(h, w)
    return {"flat": ((x0 + x1) / 2.0, (y0 + y1) / 2.0), "outside": (-60.0, h * 0.6)}


# ---- every window and pyramid depth (tests/golden/flow_windows.npz, tools/gen_flow_windows_golden.py) ----------------------------
GOLDEN_WINDOWS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "flow_windows.npz")
TEXTURE_AMPLITUDE = 300.0   # sum of the sinusoids' amplitudes per channel: about 43 gray levels rms with 24 of them, so a sample clips at 3 sigma
DIM_FACTOR = 0.03      # amplitude of the texture inside the dim region of a case that asks for one (see textured_pair)


def textured_frame(h, w, seed, win, top, dx=0.0, dy=0.0, waves=24):
    """analytic_frame with texture at every scale a pyramid of ``top`` + 1 levels and a ``win`` window look at: ``waves`` sinusoids per
    channel with periods log-uniform between max(4, 0.75 win) and 4.5 win 2^top.  (A single fine scale aliases in the coarse levels; a
    single coarse one leaves a small window without gradient.)"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    x, y = x - dx, y - dy
    out = np.empty((h, w, 3), np.uint8)
    lo, hi = max(4.0, 0.75 * win), 4.5 * win * (1 << top)
    for c in range(3):
        period = np.exp(rng.uniform(np.log(lo), np.log(hi), waves))
        theta = rng.uniform(0.0, 2.0 * np.pi, waves)
        phase = rng.uniform(0.0, 2.0 * np.pi, waves)
        amp = rng.uniform(0.5, 1.0, waves)
        amp *= TEXTURE_AMPLITUDE / amp.sum()
        v = 127.5 + sum(amp[k] * np.sin(2.0 * np.pi / period[k] * (np.cos(theta[k]) * x + np.sin(theta[k]) * y) + phase[k])
                        for k in range(waves))
        out[..., c] = np.clip(np.rint(v), 0, 255).astype(np.uint8)
    return out


def window_rect(h, w, win):
    """(y0, y1, x0, x1) of the flat rectangle of a textured pair, win + 8 on each side (a window anywhere within 4 px of its centre sees
    no gradient), or None where the frame is not at least twice that in both directions."""
    side = win + 8
    if h < 2 * side or w < 2 * side:
        return None
    y0, x0 = h // 8, w // 8
    return y0, y0 + side, x0, x0 + side


def dim_rect(h, w):
    """(y0, y1, x0, x1) of the dim region: the lower right quarter."""
    return h // 2, h, w // 2, w


def grid_frame(h, w, seed, dx=0.0, dy=0.0):
    """The strongest smooth texture uint8 holds at a window's scale: 127.5 + 110 sin(2 pi x / Px) sin(2 pi y / Py), periods seeded in
    10 .. 13 px (a little more than a 9 x 9 window), the same in the three channels.  Its gradient has about 29 gray levels per pixel rms in either direction, which puts
    the smaller eigenvalue (about g^2 / 2048) near 0.4: well above a threshold of 1e-2."""
    rng = np.random.default_rng(seed)
    px, py = rng.uniform(10.0, 13.0, 2)
    fx, fy = rng.uniform(0.0, 2.0 * np.pi, 2)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    v = 127.5 + 110.0 * np.sin(2.0 * np.pi / px * (x - dx) + fx) * np.sin(2.0 * np.pi / py * (y - dy) + fy)
    return np.repeat(np.clip(np.rint(v), 0, 255).astype(np.uint8)[..., None], 3, axis=2)


def textured_pair(h, w, seed, win, top, shift, dim=False, grid=False):
    """A textured frame and the same texture evaluated at the sub-pixel ``shift`` (dx, dy); the flat rectangle (window_rect) is painted
    into both where it fits.  ``grid``: grid_frame in place of textured_frame.  ``dim``: inside dim_rect both frames keep only
    DIM_FACTOR of the texture's amplitude around mid-gray, so that the smaller eigenvalue there (which goes with the amplitude squared,
    so it is about 1e-3 of the grid's) lies between two thresholds a factor 10^4 apart."""
    if grid:
        frames = [grid_frame(h, w, seed), grid_frame(h, w, seed, shift[0], shift[1])]
    else:
        frames = [textured_frame(h, w, seed, win, top), textured_frame(h, w, seed, win, top, shift[0], shift[1])]
    for f in frames:
        if dim:
            y0, y1, x0, x1 = dim_rect(h, w)
            f[y0:y1, x0:x1] = np.rint(127.5 + DIM_FACTOR * (f[y0:y1, x0:x1].astype(np.float64) - 127.5)).astype(np.uint8)
        rect = window_rect(h, w, win)
        if rect:
            f[rect[0]:rect[1], rect[2]:rect[3]] = FLAT_BGR
    return np.ascontiguousarray(frames[0]), np.ascontiguousarray(frames[1])


def _window_cases():
    """name -> (h, w, seed, win, max_level, shift, further config).  Further config: max_iter, min_eig (the restatement's names), grid
    (grid_frame in place of the multi-scale texture), dim (a dim region in the pair), same_points_as (the case whose points this one
    shares, so that statuses can be compared point by point) and random (False: the generator draws candidates around the frame, from
    -win - 3 to size + 3, and every one of them is lost)."""
    cases = {}
    for win in range(3, 22, 2):
        # every window on a small frame at max_level 3 (97x131: top 3 up to win 11, else top 2; at 13 the third level is 13 x 17 and only
        # the "<=" of the rule ends the pyramid) and at max_level 7 on 240x320 (top 6, 5, 5, 4, 4, 4, 3, 3, 3, 3)
        # (shifts go with the window; half a window and two pixels upwards, so that a window that starts with its upper half outside
        # the level leaves through the top limit of the range test with every test a pixel clear)
        # (seeds: 1000 + win and 2000 + win, plus 100 until the generator finds every special point of the case)
        cases[f"w{win}_97x131_l3"] = (97, 131, {15: 1115}.get(win, 1000 + win), win, 3, (round(0.1 * win, 2), -(0.5 * win + 2.0)), {})
        cases[f"w{win}_240x320_l7"] = (240, 320, {3: 2203}.get(win, 2000 + win), win, 7, (round(0.4 * win, 2), -(0.5 * win + 2.0)), {})
    cases["w5_643x709_l7"] = (643, 709, 3005, 5, 7, (2.85, -4.5), {})                   # eight levels: level 7 is 6 x 6
    cases["w21_22x30_l3"] = (22, 30, 3021, 21, 3, (0.6, -0.4), {})                       # one level by frame size: level 1 would be 11 x 15
    cases["w5_3x40_l3"] = (3, 40, 3105, 5, 3, (-4.5, -0.2), {})                           # ... 2 x 20
    cases["w3_1x1_l3"] = (1, 1, 3203, 3, 3, (0.0, 0.0), dict(random=False))             # frames smaller than the window
    cases["w7_2x5_l3"] = (2, 5, 3207, 7, 3, (0.3, -0.2), dict(random=False))
    cases["w21_6x8_l3"] = (6, 8, 3221, 21, 3, (0.6, -0.4), dict(random=False))
    cases["w9_iter1"] = (97, 131, 3301, 9, 3, (0.9, -6.5), dict(max_iter=1))
    cases["w9_iter5"] = (97, 131, 3301, 9, 3, (0.9, -6.5), dict(max_iter=5))
    # two thresholds on the same points.  A threshold of 1e-2 with a margin of 10 asks for an eigenvalue of 0.1, which the multi-scale
    # texture does not reach: a full-contrast grid and two levels (its period is gone from level 2 on), and a shift that stays below
    # half a period; the dim region holds the points that are found at 1e-6 and lost at 1e-2
    cases["w9_eig1e-2"] = (97, 131, 3401, 9, 1, (0.9, -3.5), dict(min_eig=1e-2, dim=True, grid=True))
    cases["w9_eig1e-6"] = (97, 131, 3401, 9, 1, (0.9, -3.5), dict(min_eig=1e-6, dim=True, grid=True, same_points_as="w9_eig1e-2"))
    return cases


WINDOW_CASES = _window_cases()
BOUNDARY_CASE = "w13_97x131_l3"      # three levels, because level 3 (13 x 17) is no larger than the window
EIGHT_LEVEL_CASE = "w5_643x709_l7"


def window_top(name):
    h, w, _, win, max_level = WINDOW_CASES[name][:5]
    return top_level(h, w, win, max_level)


def window_pair(name):
    h, w, seed, win, _, shift, more = WINDOW_CASES[name]
    return textured_pair(h, w, seed, win, window_top(name), shift, dim=more.get("dim", False), grid=more.get("grid", False))


def window_params(name):
    """The restatement's keyword arguments of a case (epsilon left to the caller)."""
    _, _, _, win, max_level, _, more = WINDOW_CASES[name]
    return dict(win=win, max_level=max_level, max_iter=more.get("max_iter", 30), min_eig=more.get("min_eig", 1e-4))


def window_handle_config(name):
    """The same as fields of opd_flow_config."""
    p = window_params(name)
    return dict(win=p["win"], max_level=p["max_level"], max_iter=p["max_iter"], min_eig_threshold=p["min_eig"])


def load_windows():
    """name -> dict(pts, kind, next_fixed, status_fixed, next_default, status_default, d_f32, drawn) of the windows fixture, and its
    margins (eigenvalue factor, range-test pixels, swing, |float32 - float64| limit, range-test pixels of the small windows' specials)."""
    z = np.load(GOLDEN_WINDOWS)
    off = z["offsets"]
    cases = {}
    for i, name in enumerate(z["names"].tolist()):
        cases[name] = {key: z[key][off[i]:off[i + 1]] for key in ("pts", "kind", "next_fixed", "status_fixed", "next_default", "status_default")}
        cases[name].update(d_f32=float(z["d_f32"][i]), drawn=tuple(int(v) for v in z["drawn"][i]))
    return cases, z["margins"]


def outside_xs(win):
    """The x coordinates (quarter pixels, nearest the frame first) a case's 'outside' point may take.  For win < 21 the window corner
    floor(x - (win - 1) / 2) is at least one pixel below -win, so the point is lost at this window, while floor(x - 10) >= -21: it would
    be in range were the window 21.  For win = 21: more than a window and a refinement outside."""
    if win == 21:
        return [-40.0 - 0.25 * k for k in range(0, 81)]
    first = -(win + 3) / 2.0
    return [first - 0.25 * k for k in range(0, int((first + 11.0) * 4) + 1)]


# ---- ctypes -----------------------------------------------------------------------------------------------------------------------
def flow_create(lib, max_h, max_w, max_points=128, device=0, **cfg):
    """A handle; ``cfg``: win, max_level, max_iter, epsilon, min_eig_threshold (zeros / absent: the defaults)."""
    from office_person_detection_vit_amd import _capi
    c = _capi.OpdFlowConfig(max_h=max_h, max_w=max_w, max_points=max_points, **cfg)
    handle = C.c_void_p()
    _capi.check(lib.opd_flow_create(C.byref(c), device, C.byref(handle)), "opd_flow_create")
    return handle


def _frame_args(frame, mem_kind):
    if mem_kind == 0:
        assert frame.dtype == np.uint8 and frame.flags.c_contiguous
        return C.c_void_p(frame.ctypes.data), frame.shape[0], frame.shape[1]
    ptr, h, w = frame
    return C.c_void_p(int(ptr)), h, w


def flow_set_reference(lib, handle, frame, mem_kind=0):
    from office_person_detection_vit_amd import _capi
    ptr, h, w = _frame_args(frame, mem_kind)
    _capi.check(lib.opd_flow_set_reference(handle, ptr, mem_kind, h, w), "opd_flow_set_reference")


def flow_track(lib, handle, frame, pts, mem_kind=0):
    """(next_xy [n][2] float32, status [n] uint8) of ``opd_flow_track``; ``frame``: a host array, or (device pointer, h, w)."""
    from office_person_detection_vit_amd import _capi
    ptr, h, w = _frame_args(frame, mem_kind)
    pts = np.ascontiguousarray(np.asarray(pts, np.float32).reshape(-1, 2))
    out = np.full((len(pts), 2), np.nan, np.float32)
    st = np.full(len(pts), 255, np.uint8)
    _capi.check(lib.opd_flow_track(handle, ptr, mem_kind, h, w, pts.ctypes.data_as(C.c_void_p), len(pts), out.ctypes.data_as(C.c_void_p),
                                   st.ctypes.data_as(C.c_void_p)), "opd_flow_track")
    return out, st


def flow_levels(lib, handle, which=0):
    """The gray pyramid of the handle's reference (``which`` = 0) or of the frame it replaced (1), read back through the test hook."""
    from office_person_detection_vit_amd import _capi
    h, w, n = C.c_int(), C.c_int(), C.c_int()
    _capi.check(lib.opd_flow_test_level(handle, which, 0, None, C.byref(h), C.byref(w), C.byref(n)), "opd_flow_test_level")
    levels = []
    for l in range(n.value):
        _capi.check(lib.opd_flow_test_level(handle, which, l, None, C.byref(h), C.byref(w), C.byref(n)), "opd_flow_test_level")
        out = np.zeros((h.value, w.value), np.uint8)
        _capi.check(lib.opd_flow_test_level(handle, which, l, out.ctypes.data_as(C.c_void_p), C.byref(h), C.byref(w), C.byref(n)),
                    "opd_flow_test_level")
        levels.append(out)
    return levels
