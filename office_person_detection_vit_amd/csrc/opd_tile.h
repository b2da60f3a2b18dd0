// opd_tile.h — the seam merge of tiled detection (tiling.merge_tile_detections), written once for the host (opd_tile_test_api.cpp:
// opd_test_tile_merge_host) and for the device (kernels_tile.hip::tile_merge_kernel): float64, operation for operation what the Python
// rule evaluates, so that a frame's merged list is Python's, double for double.  No multiply-add may be fused (iw * ih, aa + ab - inter
// would round once instead of twice): the pragma in every function here, -ffp-contract=off for the two files besides.
//
//   opd_tile_frame_box   rule 1: the frame box of a tile-local record            opd_tile_iou_iomin  tiling._iou_iomin
//   opd_tile_cut         rule 2: is a box side cut by an INTERIOR tile edge      opd_tile_absorb     rule 4: one (candidate, kept box) step
//   opd_tile_out         rule 6: a kept box as an output record
//   opd_tile_merge_frame rules 1 to 7 for ONE frame: gather, stable descending order by counting (opd_nms_before), greedy walk, output.
//                        `Walk` is the one part host and device do differently: the search of the kept list for the first box that
//                        absorbs a candidate (TileWalkSerial here; the kernel's wave-wide one in kernels_tile.hip).
#pragma once
#include <stdint.h>

#include "opd_nms.h"

enum { OPD_TILE_MAX_CAND = 1024 };   // candidates of one frame (n_tiles x stride)

// a and b as Python's min(a, b) / max(a, b) return them: the first argument unless the second is strictly smaller / larger
OPD_NMS_HD inline double opd_tile_min(double a, double b) { return b < a ? b : a; }
OPD_NMS_HD inline double opd_tile_max(double a, double b) { return b > a ? b : a; }

// Rule 1.  xywh as HipDetrDetector._postprocess_batch hands it to Python (the subtractions in double), then shifted by the tile origin
OPD_NMS_HD inline void opd_tile_frame_box(const opd_det& r, int y0, int x0, double* box) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double x = (double)r.x1, y = (double)r.y1, w = (double)r.x2 - (double)r.x1, h = (double)r.y2 - (double)r.y1;
    box[0] = x + (double)x0;
    box[1] = y + (double)y0;
    box[2] = (x + (double)x0) + w;
    box[3] = (y + (double)y0) + h;
}

// Rule 2.  tiling.py: cut = (x0 > 0 and x <= tx) or (x0 + tw < W and x + w >= tw - tx) or the same in y
OPD_NMS_HD inline bool opd_tile_cut(const opd_det& r, int y0, int x0, int th, int tw, int frame_h, int frame_w, double edge_tolerance) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double x = (double)r.x1, y = (double)r.y1, w = (double)r.x2 - (double)r.x1, h = (double)r.y2 - (double)r.y1;
    const double ty = edge_tolerance * (double)th, tx = edge_tolerance * (double)tw;
    return (x0 > 0 && x <= tx) || ((long long)x0 + tw < frame_w && x + w >= (double)tw - tx) ||
           (y0 > 0 && y <= ty) || ((long long)y0 + th < frame_h && y + h >= (double)th - ty);
}

// tiling._iou_iomin(a, b)
OPD_NMS_HD inline void opd_tile_iou_iomin(const double* a, const double* b, double* iou, double* iomin) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double iw = opd_tile_min(a[2], b[2]) - opd_tile_max(a[0], b[0]);
    const double ih = opd_tile_min(a[3], b[3]) - opd_tile_max(a[1], b[1]);
    if (iw <= 0 || ih <= 0) { *iou = 0.0; *iomin = 0.0; return; }
    const double inter = iw * ih;
    const double aa = opd_tile_max(0.0, a[2] - a[0]) * opd_tile_max(0.0, a[3] - a[1]);
    const double ab = opd_tile_max(0.0, b[2] - b[0]) * opd_tile_max(0.0, b[3] - b[1]);
    const double uni = aa + ab - inter, small = opd_tile_min(aa, ab);
    *iou = uni > 0 ? inter / uni : 0.0;
    *iomin = small > 0 ? inter / small : 0.0;
}

// Rule 4, one step: does kept box `k` absorb candidate `c`?  0: no.  OPD_TILE_MERGE: the two parts of one body (the merge test comes
// first, the parts' IoU may be high too).  OPD_TILE_DROP: plain IoU suppression.
enum { OPD_TILE_MERGE = 1, OPD_TILE_DROP = 2 };
OPD_NMS_HD inline int opd_tile_absorb(const double* c, int c_tile, bool c_cut, const double* k, int k_tile, bool k_cut, double merge_nms_threshold,
                                      double merge_threshold) {
    double iou, iomin;
    opd_tile_iou_iomin(c, k, &iou, &iomin);
    if (c_tile != k_tile && (c_cut || k_cut) && iomin > merge_threshold) return OPD_TILE_MERGE;
    return iou > merge_nms_threshold ? OPD_TILE_DROP : 0;
}
// ... and what a merge makes of the kept box: the union (min / max with the kept box first, as Python writes it)
OPD_NMS_HD inline void opd_tile_union(double* k, const double* c) {
    k[0] = opd_tile_min(k[0], c[0]);
    k[1] = opd_tile_min(k[1], c[1]);
    k[2] = opd_tile_max(k[2], c[2]);
    k[3] = opd_tile_max(k[3], c[3]);
}

// Rule 6.  `r`: the record of the candidate that OPENED the kept slot, `tile` its tile
OPD_NMS_HD inline opd_tile_det opd_tile_out(const double* box, const opd_det& r, int tile) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    opd_tile_det o;
    o.x = box[0]; o.y = box[1]; o.w = box[2] - box[0]; o.h = box[3] - box[1];
    o.score = r.score; o.label = r.label; o.query_index = r.query_index; o.tile = tile;
    return o;
}

namespace opd {

// What one frame's merge reads: device pointers for the kernel, host pointers for the hook
struct TileMergeParams {
    const opd_det* recs;          // [n_frames * n_tiles][stride], tile-local pixels, per tile already filtered and suppressed
    const int32_t* tile_counts;   // [n_frames * n_tiles]; < 0: taken as 0; > stride: the frame yields count 0 and *flag is raised
    const int32_t* tiles_yxhw;    // [n_tiles][4] = (y0, x0, th, tw)
    opd_tile_det* out;            // [n_frames][n_tiles * stride]
    int32_t* counts;              // [n_frames]
    int32_t* flag;                // one word, set to 1 for a count above the stride (never cleared here)
    int n_frames, n_tiles, stride, frame_h, frame_w;
    double merge_nms_threshold, merge_threshold, edge_tolerance;
};

// The working set of one frame: the candidates in sorted order, over which the kept list grows IN PLACE -- kept slot k is written while
// candidate i >= k is being decided, when slots <= i have all been read.  (The kernel keeps it in LDS, the hook on the stack.)
struct TileWork {
    float uscore[OPD_TILE_MAX_CAND];     // gather order (tile, record): what the ranks are counted on
    int32_t usrc[OPD_TILE_MAX_CAND];     // tile * stride + record of gather position c
    int32_t order[OPD_TILE_MAX_CAND];    // sorted position -> gather position (zeroed first: in range whatever NaN scores do to the ranks)
    double box[OPD_TILE_MAX_CAND][4];    // sorted candidates, then kept boxes
    int32_t src[OPD_TILE_MAX_CAND];      // tile * stride + record
    int32_t cut[OPD_TILE_MAX_CAND];
};

// The serial search: the first kept box, in kept order, that absorbs the candidate (-1: none), and how (*how)
struct TileWalkSerial {
    OPD_NMS_HD int first(const TileWork& w, int nk, const double* c, int c_tile, bool c_cut, int stride, double nms, double mrg, int* how) const {
        for (int k = 0; k < nk; ++k)
            if ((*how = opd_tile_absorb(c, c_tile, c_cut, w.box[k], w.src[k] / stride, w.cut[k] != 0, nms, mrg))) return k;
        return -1;
    }
    OPD_NMS_HD void sync() const {}
    OPD_NMS_HD int lane() const { return 0; }
    OPD_NMS_HD int lanes() const { return 1; }
};

// Rules 1 to 7 for frame `f`.  Every lane of `walk` (one on the host, a wave on the device) runs this with the same arguments; loops
// over candidates are strided by walk.lanes(), walk.sync() separates a phase's writes to `w` from the next phase's reads, and the
// greedy walk itself is uniform: walk.first() gives every lane the same answer.
template <typename Walk>
OPD_NMS_HD inline void opd_tile_merge_frame(const TileMergeParams& p, int f, TileWork& w, const Walk& walk) {
    const int lane = walk.lane(), lanes = walk.lanes(), T = p.n_tiles, S = p.stride;
    const opd_det* recs = p.recs + (size_t)f * T * S;
    const int32_t* tc = p.tile_counts + (size_t)f * T;
    opd_tile_det* out = p.out + (size_t)f * T * S;
    // rule 7, and the gather (tile, record) order
    int n = 0;
    bool over = false;
    for (int t = 0; t < T; ++t) {
        const int cnt = tc[t];
        if (cnt > S) { over = true; break; }
        for (int i = lane; i < cnt; i += lanes) {
            w.uscore[n + i] = recs[(size_t)t * S + i].score;
            w.usrc[n + i] = t * S + i;
        }
        if (cnt > 0) n += cnt;   // n <= T * S <= OPD_TILE_MAX_CAND (the launcher's check)
    }
    if (over) {
        if (lane == 0) { *p.flag = 1; p.counts[f] = 0; }
        return;
    }
    for (int i = lane; i < n; i += lanes) w.order[i] = 0;
    walk.sync();
    // rule 3: rank by counting = the position in Python's stable sort on -score
    for (int i = lane; i < n; i += lanes) {
        const float si = w.uscore[i];
        int rank = 0;
        for (int j = 0; j < n; ++j) rank += opd_nms_before(w.uscore[j], j, si, i);
        w.order[rank] = i;   // rank <= n - 1
    }
    walk.sync();
    // rules 1 and 2 at the sorted positions
    for (int r = lane; r < n; r += lanes) {
        const int s = w.usrc[w.order[r]], t = s / S;
        const int32_t* g = p.tiles_yxhw + 4 * t;
        opd_tile_frame_box(recs[s], g[0], g[1], w.box[r]);
        w.cut[r] = opd_tile_cut(recs[s], g[0], g[1], g[2], g[3], p.frame_h, p.frame_w, p.edge_tolerance);
        w.src[r] = s;
    }
    walk.sync();
    // rules 4 and 5
    int nk = 0;
    const bool absorbing = p.merge_nms_threshold < 1.0;
    for (int i = 0; i < n; ++i) {
        const double c[4] = {w.box[i][0], w.box[i][1], w.box[i][2], w.box[i][3]};
        const int c_src = w.src[i];
        const bool c_cut = w.cut[i] != 0;
        int how = 0;
        const int k = absorbing ? walk.first(w, nk, c, c_src / S, c_cut, S, p.merge_nms_threshold, p.merge_threshold, &how) : -1;
        walk.sync();   // (slot nk may be slot i: every lane has read it)
        if (lane == 0) {
            if (k < 0) {
                for (int q = 0; q < 4; ++q) w.box[nk][q] = c[q];
                w.src[nk] = c_src;
                w.cut[nk] = c_cut;
            } else if (how == OPD_TILE_MERGE) {
                opd_tile_union(w.box[k], c);
                w.cut[k] = w.cut[k] && c_cut;   // a part that was not cut completes the body
            }
        }
        if (k < 0) ++nk;
        walk.sync();
    }
    // rule 6
    for (int k = lane; k < nk; k += lanes) out[k] = opd_tile_out(w.box[k], recs[w.src[k]], w.src[k] / S);
    if (lane == 0) p.counts[f] = nk;
}

#if defined(__HIP__) || defined(__HIPCC__)
// kernels_tile.hip.  One workgroup (one wave) per frame; hipErrorInvalidValue for n_tiles * stride outside [1, OPD_TILE_MAX_CAND]
hipError_t opd_launch_tile_merge(const TileMergeParams& p, hipStream_t stream);
// Pillow-exact bilinear resize (resize_bilinear_u8_kernel's arithmetic and tables) of windows of larger frames: batch index b = frame * n_tiles + tile
// reads the th x tw window at (y0, x0)[tile] of frame b / n_tiles ([n_frames][frame_h][frame_w][3]) and writes out[b][oh][ow][3].  The caller has
// checked that every window lies inside the frame.
struct TileResizeParams {
    const uint8_t* frames;
    uint8_t* out;
    const int32_t* tiles_yxhw;   // device, [n_tiles][4]; every tile th x tw
    int n_frames, n_tiles, frame_h, frame_w, th, tw, oh, ow;
    const int32_t *bounds_h, *coeff_h, *bounds_v, *coeff_v;
    int ksize_h, ksize_v;
};
hipError_t opd_launch_tile_resize_u8(const TileResizeParams& p, hipStream_t stream);
// The same for tiles that differ in size: batch image b = frame * n_tiles + tile has the descriptor desc[tile] (device memory, 64 bytes: it travels
// as 16 int32 words) and writes out[b][H][W][3], the canvas of a ragged batch: the resize of its window to oh x ow in the top-left corner, 0 elsewhere.
// The caller has checked that every window lies inside the frame, that 1 <= oh <= H and 1 <= ow <= W, and that the tables are opd_resize_coeffs(tw, ow)
// and opd_resize_coeffs(th, oh).
struct TileRaggedDesc {
    int32_t y0, x0, th, tw, oh, ow, ksize_h, ksize_v;
    const int32_t *bounds_h, *coeff_h, *bounds_v, *coeff_v;   // device
};
static_assert(sizeof(TileRaggedDesc) == 64, "TileRaggedDesc is uploaded as 16 int32 words");
struct TileRaggedParams {
    const uint8_t* frames;
    uint8_t* out;
    const TileRaggedDesc* desc;   // device, [n_tiles]
    int n_frames, n_tiles, frame_h, frame_w, H, W;
};
hipError_t opd_launch_tile_resize_ragged_u8(const TileRaggedParams& p, hipStream_t stream);
#endif

}  // namespace opd
