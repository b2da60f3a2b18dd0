"""Write tests/golden/flow.npz: the points of the optical-flow tests and what the float64 restatement (tests/flow_common.py) gives for
them.  Frames are not stored: the tests rebuild them from the seeds in flow_common.

Per structured pair (flow_common.LK_CASES): 100 points, the two lost-point cases (flat, outside), the restatement's next_xy and
status with epsilon = 0 ("fixed work": only the swing test stops a level) and with the default criteria, and d_f32 = the largest
distance between the restatement in float32 and in float64 over those points at epsilon = 0.  For the analytic pairs: the points,
next_xy / status per shift and e_ref = the restatement's largest error against the true displacement; and points 3 px from the edges
of the first analytic pair that are found.

Points are drawn from a seeded stream and kept only when every decision the algorithm takes for them is clear of its threshold in the
float64 run, so that a float32 implementation takes the same decisions: smaller eigenvalue and determinant >= 10 x or <= 0.1 x their
thresholds, every range test >= 1 pixel from its limit, the swing test >= 1e-4 from 0.01, and no level out of iterations.  The script
asserts these margins on what it writes.

    python tools/gen_flow_golden.py
"""

from __future__ import annotations

import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import flow_common as F  # noqa: E402

EIG_MARGIN, BORDER_MARGIN, STOP_MARGIN = 10.0, 1.0, 1e-4


def clear(diag, fixed_work):
    ok = (diag["eig"] >= EIG_MARGIN) & (diag["border"] >= BORDER_MARGIN) & diag["converged"]
    return ok & (diag["stop"] >= STOP_MARGIN) if fixed_work else ok


def run_both(f0, f1, pts):
    """The restatement at epsilon = 0 and at the default criteria; which points are clear in both."""
    d0, d1 = {}, {}
    n0, s0 = F.lk_restatement(f0, f1, pts, epsilon=0.0, diag=d0)
    n1, s1 = F.lk_restatement(f0, f1, pts, diag=d1)
    return n0, s0, n1, s1, clear(d0, True) & clear(d1, False)


def main():
    out = {"margins": np.array([EIG_MARGIN, BORDER_MARGIN, STOP_MARGIN]), "numpy_version": np.array(np.__version__)}
    for name, (h, w, seed, n) in F.LK_CASES.items():
        f0, f1 = F.structured_pair(h, w, seed)
        rng = np.random.default_rng(seed)
        cand = np.stack([rng.uniform(-4, w + 4, 8 * n), rng.uniform(-4, h + 4, 8 * n)], 1).astype(np.float32)
        keep = np.flatnonzero(run_both(f0, f1, cand)[4])[:n]
        assert len(keep) == n, (name, len(keep))
        pts = cand[keep]
        # the status cases: the named positions, moved along y (nearest first) until every decision is clear
        special = []
        for key, (x, y) in F.special_points(h, w).items():
            for dy in sorted(range(-(h // 3), h // 3), key=abs):
                p = np.array([[x, y + dy]], np.float32)
                _, s0, _, s1, ok = run_both(f0, f1, p)
                if ok[0] and s0[0] == s1[0] == 0:
                    break
            else:
                raise AssertionError(f"{name}: no clear '{key}' point")
            special.append(p[0])
        allp = np.concatenate([pts, np.array(special, np.float32)])
        n0, s0, n1, s1, ok = run_both(f0, f1, allp)
        assert ok.all()
        n32, s32 = F.lk_restatement(f0, f1, allp, epsilon=0.0, dtype=np.float32)
        assert np.array_equal(s32, s0)
        d_f32 = float(np.abs(n32.astype(np.float64) - n0).max())
        out.update({f"{name}_pts": allp, f"{name}_next_fixed": n0, f"{name}_status_fixed": s0, f"{name}_next_default": n1,
                    f"{name}_status_default": s1, f"{name}_d_f32": np.float64(d_f32)})
        print(f"{name}: {len(allp)} points, found {int(s0.sum())} / {int(s1.sum())}, d_f32 = {d_f32:.3e}, specials {np.array(special).tolist()} -> {s0[n:].tolist()}")
    # points 3 px from each edge of the analytic pair with the smallest shift (the structured frames are flat along their edges): the first
    # one per edge that is found with every decision clear
    a, b = F.analytic_pair(F.SHIFTS[0])
    H, W = F.SHIFT_HW
    border = []
    for edge in ([(3.0, y) for y in range(30, H - 30, 5)], [(W - 4.0, y) for y in range(30, H - 30, 5)],
                 [(x, 3.0) for x in range(30, W - 30, 5)], [(x, H - 4.0) for x in range(30, W - 30, 5)]):
        p = np.array(edge, np.float32)
        _, s0, _, s1, ok = run_both(a, b, p)
        good = np.flatnonzero(ok & (s0 == 1) & (s1 == 1))
        if len(good):
            border.append(p[good[0]])
    assert len(border) >= 2, border
    border = np.array(border, np.float32)
    n0, s0, n1, s1, ok = run_both(a, b, border)
    out.update(border_pts=border, border_next=n1, border_status=s1)
    print(f"border: {border.tolist()} -> {n1.round(3).tolist()}")
    cand = F.shift_points()
    ok = np.ones(len(cand), bool)
    for shift in F.SHIFTS:
        a, b = F.analytic_pair(shift)
        n0, s0, n1, s1, c = run_both(a, b, cand)
        ok &= c & (s0 == 1) & (s1 == 1)
    pts = cand[ok]
    assert len(pts) >= 16, len(pts)
    out["shift_pts"] = pts
    for k, shift in enumerate(F.SHIFTS):
        a, b = F.analytic_pair(shift)
        n0, s0, n1, s1, c = run_both(a, b, pts)
        assert c.all() and s1.all()
        e_ref = float(np.abs(n1 - pts - np.array(shift)).max())
        out.update({f"shift{k}_next": n1, f"shift{k}_status": s1, f"shift{k}_e_ref": np.float64(e_ref)})
        print(f"shift {shift}: {len(pts)} points, e_ref = {e_ref:.4f} px")
    np.savez_compressed(F.GOLDEN, **out)
    print("wrote", F.GOLDEN, os.path.getsize(F.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
