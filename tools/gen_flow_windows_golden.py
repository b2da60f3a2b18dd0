"""Write tests/golden/flow_windows.npz: optical-flow points for every window edge (3, 5 .. 21), pyramids of one to eight levels, frames
smaller than the window, max_iter 1 and 5 and two eigenvalue thresholds (flow_common.WINDOW_CASES), and what the float64 restatement
(tests/flow_common.py) gives for them.  Frames are not stored: the tests rebuild them from the seeds (flow_common.window_pair).

Per case: the points, the restatement's next_xy and status with epsilon = 0 ("fixed work") and with epsilon = 0.01, d_f32 = the largest
distance between the float32 and the float64 restatement over those points at epsilon = 0, which point is which (0: drawn, 1: in the
flat rectangle, 2: outside the frame) and how many candidates were drawn and were clear.

Candidates come from a seeded stream, at most 4000 per case, uniformly over the frame plus 4 px (cases with ``random=False``: from
-win - 3 to size + 3).  One is kept only when every decision the algorithm takes for it is clear of its threshold in the float64 runs,
by the margins of tools/gen_flow_golden.py: smaller eigenvalue and determinant >= 10 x or <= 0.1 x their thresholds, every range test
>= 1 pixel from its limit, the swing test >= 1e-4 from 0.01 (fixed work) and no level out of iterations (except in the max_iter cases,
where the iteration count is the stop); and, new here, only when its own |float32 - float64| at epsilon = 0 is at most 2.5e-4 px and
its float32 status is the float64 one (small windows meet ill-conditioned systems that the margins do not see; 2.5e-4 is 2.5 times the
largest distance measured over the well-conditioned points of all cases, so 4 * d_f32 <= 1e-3 px).  All of this is decided by the
restatement alone.  Cases that share their points (``same_points_as``) keep a candidate when it is clear in each of them.

Kept per case: the first 24 candidates found in every run, the first 8 lost in every run, for cases that share points also the first 8
whose status differs between the cases (at least 4 are required: the thresholds 1e-2 and 1e-6 differ on points of the dim region, whose
texture has 0.03 of the grid's amplitude and so about 1e-3 of its eigenvalue), filled up to 32 with further found ones; for the frames
smaller than the window the first 32 clear ones (all lost).  Then up to three special points, all lost and clear:

  flat     within 3 px of the centre of the flat rectangle (the window stays inside it), where the frame has one;
  outside  the first of flow_common.outside_xs(win) x rows around 0.6 h: for win < 21 lost at this window by the range test on the
           starting corner, but in range were the window 21;
  exit     (win < 21, cases with found points) a point whose window starts in range near the top or left limit and leaves through it
           while it is refined, and which the float32 restatement with 21 in its range tests does not lose, or leaves more than 1e-3 px
           away.  This is the point that shows a 21 in the range tests: the test on the starting corner cannot, because a window it
           refuses lies wholly outside the level, where the derivatives are zero, so the determinant test refuses it too.  The shifts
           of the cases (half a window and two pixels upwards) are what lets such a window leave with every test clear.

The range-test margin of 1 px holds at every level, and a point near the limit meets the limit of every level at another place:
corner x / 2^l - (win - 1) / 2 against -win.  With c = (win + 1) / 2, an outside point needs x <= -c - m at level 0 (margin m) and
at every level l >= 1 either x / 2^l <= -c - m or x / 2^l >= -c + m.  At win = 3 (c = 2) and m = 1, level 1 then asks for x <= -6 and
level 2 for x <= -12 or x >= -4: nothing in [-11, -3] once there are three levels.  The position p that refinement carries an exit point to is bound the same
way: p <= -c - m at level 0 and p >= 2 (-c + m) at level 1, an interval that is empty at win = 3 and a single value at win = 5 for
m = 1.  So the outside point at win = 3 and the exit point at win <= 5, and only they, are held to m = 0.5 px; the outside point at
win = 3 has integer coordinates, for which x / 2^l - 1 is exact in float32 and the test cannot come out differently there.  Half a pixel
is still 2000 times the 2.5e-4 px that a kept point's float32 run may differ by.

The script asserts every quota and margin on what it writes and fails rather than writing a thinner case.  The archive is written
with fixed time stamps, so running it again gives the same bytes.

    python tools/gen_flow_windows_golden.py
"""

from __future__ import annotations

import io
import os
import sys
import zipfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import flow_common as F  # noqa: E402

EIG_MARGIN, BORDER_MARGIN, STOP_MARGIN, F32_LIMIT = 10.0, 1.0, 1e-4, 2.5e-4
SMALL_WINDOW_BORDER = 0.5      # range-test margin of the outside point at win = 3 and of the exit point at win <= 5 (see above)


def special_border(kind, win):
    """The range-test margin (pixels) a point of that kind is held to."""
    small = (kind == 2) & (win == 3) | (kind == 3) & (win <= 5)
    return np.where(small, SMALL_WINDOW_BORDER, BORDER_MARGIN)
MAX_DRAWN, CHUNK = 4000, 500
N_FOUND, N_LOST, N_MIXED, N_MIN_MIXED, N_POINTS = 24, 8, 8, 4, 32


class Case:
    def __init__(self, name):
        self.name = name
        self.h, self.w, self.seed, self.win, self.max_level, self.shift, self.more = F.WINDOW_CASES[name]
        self.params = F.window_params(name)
        f0, f1 = F.window_pair(name)
        self.pyr = F.pyramid(f0, self.win, self.max_level), F.pyramid(f1, self.win, self.max_level)
        assert len(self.pyr[0]) == F.window_top(name) + 1

    def lk(self, pts, epsilon, **kw):
        p = self.params
        return F.lk_pyramids(self.pyr[0], self.pyr[1], pts, p["win"], p["max_iter"], epsilon, p["min_eig"], **kw)

    def run(self, pts, border=BORDER_MARGIN):
        """next / status at epsilon = 0 and 0.01, which points are clear, the per-point |float32 - float64| at epsilon = 0."""
        d0, d1 = {}, {}
        n0, s0 = self.lk(pts, 0.0, diag=d0)
        n1, s1 = self.lk(pts, 0.01, diag=d1)
        n32, s32 = self.lk(pts, 0.0, dtype=np.float32)
        d32 = np.abs(n32.astype(np.float64) - n0).max(axis=1)
        ok = np.ones(len(pts), bool)
        for d, fixed in ((d0, True), (d1, False)):
            ok &= (d["eig"] >= EIG_MARGIN) & (d["border"] >= border)
            if "max_iter" not in self.more:
                ok &= d["converged"]
            if fixed:
                ok &= d["stop"] >= STOP_MARGIN
        ok &= (d32 <= F32_LIMIT) & (s32 == s0) & (s0 == s1)
        return n0, s0, n1, s1, ok, d32


def run_group(group, pts, border=BORDER_MARGIN):
    """Clear in every case of the group; the status (at either epsilon: they are equal on clear points) per case."""
    runs = [c.run(pts, border) for c in group]
    ok = np.logical_and.reduce([r[4] for r in runs])
    return ok, np.stack([r[1] for r in runs], 1)


def draw(group):
    c = group[0]
    rng = np.random.default_rng(c.seed)
    lo, past = (-c.win - 3.0, 3.0) if c.more.get("random") is False else (-4.0, 4.0)
    picked = {"found": [], "lost": [], "mixed": []}
    drawn = kept = 0
    everything_lost = c.more.get("random") is False
    while drawn < MAX_DRAWN:
        cand = np.stack([rng.uniform(lo, c.w + past, CHUNK), rng.uniform(lo, c.h + past, CHUNK)], 1).astype(np.float32)
        drawn += CHUNK
        ok, st = run_group(group, cand)
        kept += int(ok.sum())
        for i in np.flatnonzero(ok):
            key = "found" if st[i].all() else ("mixed" if st[i].any() else "lost")
            picked[key].append(cand[i])
        if everything_lost:
            if len(picked["lost"]) >= N_POINTS:
                break
        elif len(picked["found"]) >= N_POINTS and (len(group) == 1 or len(picked["mixed"]) >= N_MIXED):
            break
    if everything_lost:
        assert not picked["found"] and not picked["mixed"] and len(picked["lost"]) >= N_POINTS, (c.name, {k: len(v) for k, v in picked.items()})
        pts = picked["lost"][:N_POINTS]
    else:
        assert len(picked["found"]) >= N_FOUND, (c.name, "found", len(picked["found"]), "of", drawn)
        lost = picked["lost"][:N_LOST]
        mixed = picked["mixed"][:N_MIXED] if len(group) > 1 else []
        assert len(group) == 1 or len(mixed) >= N_MIN_MIXED, (c.name, "status differs on", len(mixed))
        n_found = max(N_FOUND, N_POINTS - len(lost) - len(mixed))
        pts = picked["found"][:n_found] + mixed + lost
    return np.array(pts, np.float32), kept, drawn


def flat_point(group):
    c = group[0]
    rect = F.window_rect(c.h, c.w, c.win)
    if rect is None:
        return None
    x, y = (rect[2] + rect[3]) / 2.0, (rect[0] + rect[1]) / 2.0
    offsets = sorted(((dx * 0.5, dy * 0.5) for dx in range(-6, 7) for dy in range(-6, 7)), key=lambda o: (abs(o[0]) + abs(o[1]), o))
    cand = np.array([(x + dx, y + dy) for dx, dy in offsets], np.float32)    # within 3 px of the centre: the window stays inside
    ok, st = run_group(group, cand)
    good = np.flatnonzero(ok & ~st.any(axis=1))
    if len(good):
        return cand[good[0]]
    raise AssertionError(f"{c.name}: no clear flat point")


def outside_point(group):
    c = group[0]
    border = float(special_border(2, c.win))
    xs = [x for x in F.outside_xs(c.win) if c.win != 3 or x == int(x)]
    rows = sorted(range(c.h), key=lambda y: abs(y - int(0.6 * c.h)))
    cand = np.array([(x, y + dy) for y in rows for dy in ((0.0,) if c.win == 3 else (0.5, 0.25, 0.75, 0.0)) for x in xs], np.float32)[:4000]
    ok, st = run_group(group, cand, border)
    good = ok & ~st.any(axis=1)
    assert good.any(), f"{c.name}: no clear outside point"
    return cand[np.flatnonzero(good)[0]]


def exit_point(group):
    """A point whose window starts in range and leaves through the top or left limit (floor < -win) while it is refined, where the
    float32 restatement with 21 in its range tests goes on instead: it finds the point, or leaves it more than 1e-3 px away.  (The
    range test on the starting corner cannot show that mistake: a window it refuses lies wholly outside the level, where the
    derivatives are zero, and the determinant test refuses it as well.)"""
    c = group[0]
    if c.win == 21 or c.more.get("random") is False:
        return None
    half = (c.win - 1) // 2
    near = [half - c.win + 1.25 + 0.25 * k for k in range(2 * c.win + 4)]   # corners from 1.25 px to half a window inside the limit
    target = min(20000.0, 600000.0 / (c.win * c.win))                        # candidates along the top and the left limit: more where windows are small
    step = max(0.125, (c.w + c.h) * len(near) / target)
    cand = [(x, y) for y in near for x in np.arange(2.0, c.w - 2.0, step)] + [(x, y) for x in near for y in np.arange(2.0, c.h - 2.0, step)]
    cand = np.array(cand, np.float32)
    ok, st = run_group(group, cand, float(special_border(3, c.win)))
    good = ok & ~st.any(axis=1)
    for k in group:
        n0, s0 = k.lk(cand, 0.0)
        nd, sd = k.lk(cand, 0.0, dtype=np.float32, defect="range_21")
        good &= (sd != s0) | (np.abs(nd.astype(np.float64) - n0).max(axis=1) > 1e-3)
    assert good.any(), f"{c.name}: no clear exit point among {len(cand)}, {int(ok.sum())} clear, {int((ok & ~st.any(axis=1)).sum())} of them lost"
    return cand[np.flatnonzero(good)[0]]


def write_npz(path, arrays):
    """np.savez_compressed with fixed time stamps: the same arrays give the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    groups = {}
    for name, case in F.WINDOW_CASES.items():
        groups.setdefault(case[6].get("same_points_as", name), []).append(name)
    per_case = {}
    for names in groups.values():
        group = [Case(n) for n in names]
        pts, kept, drawn = draw(group)
        kind = [0] * len(pts)
        for k, special in ((1, flat_point(group)), (2, outside_point(group)), (3, exit_point(group))):
            if special is not None:
                pts = np.concatenate([pts, special[None]])
                kind.append(k)
        kind = np.array(kind, np.uint8)
        for case in group:
            n0, s0, n1, s1, ok, d32 = case.run(pts, special_border(kind, case.win))
            assert ok.all(), (case.name, np.flatnonzero(~ok))
            assert not s0[kind != 0].any()
            found = int(s0.sum())
            assert found >= N_FOUND or case.more.get("random") is False and found == 0, (case.name, found)
            d_f32 = float(d32.max())
            per_case[case.name] = dict(pts=pts, kind=kind, next_fixed=n0, status_fixed=s0, next_default=n1, status_default=s1, d_f32=d_f32,
                                       drawn=(kept, drawn))
            print(f"{case.name}: levels {len(case.pyr[0])}, kept {kept} / {drawn} drawn, {len(pts)} points, found {found}, d_f32 = {d_f32:.3e}, "
                  f"specials {pts[kind != 0].tolist()}")
        if len(group) > 1:
            differs = int((per_case[names[0]]["status_fixed"] != per_case[names[1]]["status_fixed"]).sum())
            assert differs >= N_MIN_MIXED
            print(f"{names[0]} / {names[1]}: status differs on {differs} points")
    # one array per quantity, the cases one behind the other in the table's order (an archive member per case and quantity would be
    # mostly headers); flow_common.load_windows cuts them apart again
    names = list(F.WINDOW_CASES)
    out = {"margins": np.array([EIG_MARGIN, BORDER_MARGIN, STOP_MARGIN, F32_LIMIT, SMALL_WINDOW_BORDER]), "names": np.array(names),
           "offsets": np.cumsum([0] + [len(per_case[n]["pts"]) for n in names]).astype(np.int32),
           "d_f32": np.array([per_case[n]["d_f32"] for n in names]), "drawn": np.array([per_case[n]["drawn"] for n in names], np.int32)}
    for key in ("pts", "kind", "next_fixed", "status_fixed", "next_default", "status_default"):
        out[key] = np.concatenate([per_case[n][key] for n in names])
    write_npz(F.GOLDEN_WINDOWS, out)
    print("wrote", F.GOLDEN_WINDOWS, os.path.getsize(F.GOLDEN_WINDOWS), "bytes")


if __name__ == "__main__":
    main()
