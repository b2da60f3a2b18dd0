"""The ingest launch of the fused detect-and-track call (``track_ingest_kernel``, csrc/kernels_track.hip) restated in numpy: one frame's
kept records -> the staging image the tracker's two launches read.  The values are the float32 numbers the Python path hands to
``opd_track_update`` today: ``detector.py::_postprocess_batch`` takes differences and sums of the record's float32 corners as Python
floats (float64), ``HipTracker.update`` stores them into float32 arrays (one rounding each)."""

import numpy as np

DET = np.dtype([("x1", "<f4"), ("y1", "<f4"), ("x2", "<f4"), ("y2", "<f4"), ("score", "<f4"), ("label", "<i4"), ("query_index", "<i4"), ("frame", "<i4")])
ROWS_NONE, ROWS_BY_QUERY, ROWS_BY_SLOT = 0, 1, 2


def pack(records):
    """(boxes xywh [n][4], foot [n][2]) float32 of `records` (a DET array)."""
    x1, y1 = records["x1"].astype(np.float64), records["y1"].astype(np.float64)
    bw, bh = records["x2"].astype(np.float64) - x1, records["y2"].astype(np.float64) - y1
    boxes = np.stack([records["x1"], records["y1"], bw.astype(np.float32), bh.astype(np.float32)], axis=1).astype(np.float32).reshape(-1, 4)
    foot = np.stack([(x1 + bw / 2).astype(np.float32), (y1 + bh).astype(np.float32)], axis=1).reshape(-1, 2)
    return boxes, foot


def ingest(records, n, Q, D, frame, rows_kind, rows, slot_map, n_person, slots, boxes, foot, has, feat):
    """What the launch does to the four staging arrays (in place; they arrive holding the caller's sentinels) and the count it
    publishes.  `records`: DET [Q]; `rows`: [..][D]; `slot_map`: [slots] of which min(n_person, slots) are filled."""
    n = max(0, min(int(n), Q))
    b, f = pack(records[:n])
    boxes[:n], foot[:n] = b, f
    for i in range(n):
        q = int(records["query_index"][i])
        src = None
        if 0 <= q < Q:
            if rows_kind == ROWS_BY_QUERY:
                src = rows[frame * Q + q]
            elif rows_kind == ROWS_BY_SLOT:
                filled = min(int(n_person), slots)
                hit = np.nonzero(np.asarray(slot_map[:filled]) == frame * Q + q)[0]
                if len(hit):
                    src = rows[int(hit[-1])]
        has[i] = 0 if src is None else 1
        if src is not None:
            feat[i] = src
    return n


def hard_records():
    """Records whose corners need all 24 mantissa bits, whose widths are not float32 numbers, and with negative x1."""
    f = np.float32
    rows = [
        (f(16777215.0) / f(8192.0), f(16777213.0) / f(16384.0), f(16777211.0) / f(4096.0), f(16777209.0) / f(8192.0)),   # 24 significant bits each
        (f(0.1), f(0.3), f(1000.3), f(700.7)),                     # x2 - x1 is not a float32 number
        (f(1.0) / f(3.0), f(2.0) / f(3.0), f(1279.0) + f(1.0) / f(3.0), f(719.9)),
        (f(-3.7), f(-0.2), f(55.55), f(120.1)),                    # negative x1 and y1
        (f(-1e-3), f(5.0), f(1e-3), f(5.0) + f(2.0 ** -20)),       # a tiny box across zero
        (f(10.0), f(20.0), f(10.0), f(20.0)),                      # empty
        (f(1e6) + f(0.0625), f(3.0), f(1e6) + f(7.4375), f(4.0)),
    ]
    rng = np.random.default_rng(11)
    for _ in range(57):
        x1, y1 = f(rng.uniform(-50, 1200)), f(rng.uniform(-50, 700))
        rows.append((x1, y1, f(x1 + f(rng.uniform(0, 400))) * f(1.0000001), f(y1 + f(rng.uniform(0, 400)))))
    recs = np.zeros(len(rows), DET)
    for i, (x1, y1, x2, y2) in enumerate(rows):
        recs[i] = (x1, y1, x2, y2, f(0.9) - f(0.01) * f(i), 1, len(rows) - 1 - i, 0)
    return recs
