// kernels_track.hip — the launches of one `Tracker.update` (src/tracking/tracker.py, track.py, kalman_filter.py, similarity.py of the
// reference).  All state is float32 as the reference's numpy arrays are; the file is built with -ffp-contract=off, so every expression
// below is evaluated operation by operation in the order written (tests/track_common.py restates the same order in numpy).
//
//   track_predict_cost_kernel  one workgroup of 256 threads (four waves) per live track.
//       Kalman predict, dt = 1 (thread 0).  F = [[1 0 1 0] [0 1 0 1] [0 0 1 0] [0 0 0 1]] has two non-zeros per row at most, so
//         x <- (x0 + x2, x1 + x3, x2, x3);  A = F P: A[0][j] = P[0][j] + P[2][j], A[1][j] = P[1][j] + P[3][j], rows 2 and 3 copied;
//         B = A F^T: B[i][0] = A[i][0] + A[i][2], B[i][1] = A[i][1] + A[i][3], columns 2 and 3 copied;  P <- B + Q for all 16 entries,
//         Q = q * [[1/4 0 1/2 0] [0 1/4 0 1/2] [1/2 0 1 0] [0 1/2 0 1]] with q = float32(0.1).  (A sum of products of which two are
//         non-zero is the same number in any order: this equals a full float32 matrix product bit for bit.)
//       Smoothed feature.  Thread i owns elements i, i + 256, ...: e = ring[oldest]; e = 0.9f * f + 0.1f * e for every younger entry f.
//         The sum of squares: every thread adds its own elements in ascending order, a wave adds its 64 partial sums by an xor
//         butterfly (all lanes end with the same bits), the four wave sums go through LDS and are added as ((w0 + w1) + w2) + w3.
//         norm = sqrtf(sum); e / norm when norm > 1e-6f.  Nothing here depends on T, N or the slot.
//       Cost rows.  IoU distance and the gate per detection by one thread each (double on the float32 boxes, the arithmetic of
//         similarity_matrix_kernel; the gate in float32: sqrtf(dx * dx + dy * dy) > max_dist).  The dot product with a detection's
//         feature by one wave: lane l adds elements l, l + 64, ... in ascending order, then the butterfly; which wave takes which
//         detection changes no bit.  app = float32(1.0 - double(clip(dot, -1, 1))), comb as `_compute_cost_matrix` in double.
//   track_commit_kernel        one workgroup per matched or new track: Kalman (thread 0), feature ring (all threads).
//   track_ingest_kernel        the fused detect-and-track call only: one wave per record slot of a frame turns the kept records, where the
//       suppression kernel left them, into the staging image the two launches above read (boxes xywh, foot points, flags, feature rows) and
//       leaves the kept count on the device for the predict launch.  Plain loads and stores: no LDS-DMA, no counted waits.
//   track_assoc_kernel         sequence calls only: one wave does between the two launches what the host does in a per-frame call (the five
//       association stages with the host's solver, ids and counters, new slots, deletions) on a track table that stays on the device for the
//       call.  The predict and commit launches then take their row count, slots and list from that table (`hdr` set), under a grid that is an
//       upper bound.  Plain loads and stores here too.
//   track_*_multi_kernel       streams calls only: the four above for C trackers in one launch each.  blockIdx.y is the camera; its parameter block comes
//       out of a descriptor array in device memory; the arithmetic is the body of the one-tracker kernel, called on that block.
#include <hip/hip_runtime.h>

#include "opd_kprims.h"
#include "opd_track.h"

namespace {

__device__ void kalman_predict(float* x, float* P) {
    const float q = 0.1f;
    x[0] = x[0] + x[2];
    x[1] = x[1] + x[3];
    float A[16], B[16];
    for (int j = 0; j < 4; ++j) {
        A[j] = P[j] + P[8 + j];
        A[4 + j] = P[4 + j] + P[12 + j];
        A[8 + j] = P[8 + j];
        A[12 + j] = P[12 + j];
    }
    for (int i = 0; i < 4; ++i) {
        B[4 * i] = A[4 * i] + A[4 * i + 2];
        B[4 * i + 1] = A[4 * i + 1] + A[4 * i + 3];
        B[4 * i + 2] = A[4 * i + 2];
        B[4 * i + 3] = A[4 * i + 3];
    }
    const float q4 = 0.25f * q, q2 = 0.5f * q;
    const float Q[16] = {q4, 0.f, q2, 0.f, 0.f, q4, 0.f, q2, q2, 0.f, q, 0.f, 0.f, q2, 0.f, q};
    for (int k = 0; k < 16; ++k) P[k] = B[k] + Q[k];
}

// Measurement z = (z0, z1), H = [I 0], R = I.  S = P[0:2][0:2] + I.  Its inverse in closed form, in this order: det = s00 * s11 - s01 * s10;
// i00 = s11 / det, i01 = (-s01) / det, i10 = (-s10) / det, i11 = s00 / det.  K = P[:, 0:2] S^-1: K[i][c] = P[i][0] * i0c + P[i][1] * i1c.
// x <- x + (K[i][0] * y0 + K[i][1] * y1).  M = I - K H (M[i][j] = (i == j) - K[i][j] for j < 2, (i == j) - 0 beyond);
// P <- M P: ((M[i][0] * P[0][j] + M[i][1] * P[1][j]) + M[i][2] * P[2][j]) + M[i][3] * P[3][j].
__device__ void kalman_update(float* x, float* P, float z0, float z1) {
    const float y0 = z0 - x[0], y1 = z1 - x[1];
    const float s00 = P[0] + 1.0f, s01 = P[1], s10 = P[4], s11 = P[5] + 1.0f;
    const float det = s00 * s11 - s01 * s10;
    const float i00 = s11 / det, i01 = (-s01) / det, i10 = (-s10) / det, i11 = s00 / det;
    float K[8], M[16], N[16];
    for (int i = 0; i < 4; ++i) {
        K[2 * i] = P[4 * i] * i00 + P[4 * i + 1] * i10;
        K[2 * i + 1] = P[4 * i] * i01 + P[4 * i + 1] * i11;
    }
    for (int i = 0; i < 4; ++i) x[i] = x[i] + (K[2 * i] * y0 + K[2 * i + 1] * y1);
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) M[4 * i + j] = (i == j ? 1.0f : 0.0f) - (j < 2 ? K[2 * i + j] : 0.0f);
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j)
            N[4 * i + j] = ((M[4 * i] * P[j] + M[4 * i + 1] * P[4 + j]) + M[4 * i + 2] * P[8 + j]) + M[4 * i + 3] * P[12 + j];
    for (int k = 0; k < 16; ++k) P[k] = N[k];
}

// The bodies of the four launches take their parameters by reference: the one-tracker kernels below hand them their by-value argument, the camera-batched
// ones (track_*_multi_kernel, at the end of the file) the block of blockIdx.y's camera out of a descriptor array.  blockIdx.x means the same in both.
__device__ __forceinline__ void track_predict_cost_body(const TrackPredictParams& p) {
    __shared__ float sm[TRACK_MAX_DIM];          // the smoothed feature
    __shared__ double iou_d[TRACK_MAX_DETS];     // IoU distance per detection, before rounding
    __shared__ uint8_t gated[TRACK_MAX_DETS];
    __shared__ float wsum[TRACK_THREADS / 64];
    __shared__ float pos[2];
    const int t = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (p.hdr && (p.hdr[TRACK_HDR_STOPPED] != 0 || t >= p.hdr[TRACK_HDR_T])) return;   // (sequence call: the grid is an upper bound; the whole workgroup leaves)
    const int slot = p.hdr ? p.tab[TRACK_ENTRY_INTS * t] : p.slots[t], D = p.D;
    const int N = p.n_dev ? *p.n_dev : p.d.n;   // (the fused call: the count is the ingest launch's, at most Q <= TRACK_MAX_DETS)
    if (tid == 0) {
        float x[4], P[16];
        for (int k = 0; k < 4; ++k) x[k] = p.s.x[4 * slot + k];
        for (int k = 0; k < 16; ++k) P[k] = p.s.P[16 * slot + k];
        kalman_predict(x, P);
        for (int k = 0; k < 4; ++k) p.s.x[4 * slot + k] = x[k];
        for (int k = 0; k < 16; ++k) p.s.P[16 * slot + k] = P[k];
        pos[0] = x[0];
        pos[1] = x[1];
    }
    const int len = p.s.ring_meta[2 * slot], head = p.s.ring_meta[2 * slot + 1];
    const float* ring = p.s.ring + (size_t)slot * TRACK_RING * D;
    float ss = 0.f;
    if (len > 0) {
        for (int d = tid; d < D; d += TRACK_THREADS) {
            float e = ring[(size_t)head * D + d];
            for (int k = 1; k < len; ++k) {
                const float f = ring[(size_t)((head + k) % TRACK_RING) * D + d];
                e = 0.9f * f + 0.1f * e;
            }
            sm[d] = e;
            ss = ss + e * e;
        }
    }
    ss = wave_sum(ss);
    if (lane == 0) wsum[wave] = ss;
    __syncthreads();   // sm, wsum and pos are complete
    if (len > 0) {
        const float norm = sqrtf(((wsum[0] + wsum[1]) + wsum[2]) + wsum[3]);
        for (int d = tid; d < D; d += TRACK_THREADS) {
            float e = sm[d];
            if (norm > 1e-6f) e = e / norm;
            sm[d] = e;   // (each element is read and written by its own thread)
            p.s.smooth[(size_t)slot * D + d] = e;
        }
    }
    const float px = pos[0], py = pos[1];
    const double bx = p.s.box[4 * slot], by = p.s.box[4 * slot + 1], bw = p.s.box[4 * slot + 2], bh = p.s.box[4 * slot + 3];
    for (int j = tid; j < N; j += TRACK_THREADS) {
        const double x2 = p.d.boxes[4 * j], y2 = p.d.boxes[4 * j + 1], w2 = p.d.boxes[4 * j + 2], h2 = p.d.boxes[4 * j + 3];
        const double ix0 = bx > x2 ? bx : x2, iy0 = by > y2 ? by : y2;
        const double ix1 = (bx + bw) < (x2 + w2) ? (bx + bw) : (x2 + w2), iy1 = (by + bh) < (y2 + h2) ? (by + bh) : (y2 + h2);
        double iou = 0.0;
        if (ix1 > ix0 && iy1 > iy0) {
            const double inter = (ix1 - ix0) * (iy1 - iy0);
            const double uni = bw * bh + w2 * h2 - inter;
            if (uni > 0.0) {
                iou = inter / uni;
                iou = iou < 0.0 ? 0.0 : (iou > 1.0 ? 1.0 : iou);
            }
        }
        const double dist = 1.0 - iou;
        iou_d[j] = dist;
        p.iou[(size_t)t * N + j] = (float)dist;
        const float dx = px - p.d.foot[2 * j], dy = py - p.d.foot[2 * j + 1];
        gated[j] = p.max_dist > 0.f && sqrtf(dx * dx + dy * dy) > p.max_dist;
    }
    __syncthreads();   // the normalised sm, iou_d and gated are complete
    for (int j = wave; j < N; j += TRACK_THREADS / 64) {   // (wave-uniform: no divergence around the butterfly)
        const bool both = len > 0 && p.d.feat != nullptr && p.d.has[j] != 0;
        float dot = 0.f;
        if (both) {
            const float* f = p.d.feat + (size_t)j * D;
            for (int d = lane; d < D; d += 64) dot = dot + sm[d] * f[d];
            dot = wave_sum(dot);
            dot = dot < -1.f ? -1.f : (dot > 1.f ? 1.f : dot);
        }
        if (lane == 0) {
            const double app = 1.0 - (double)dot;
            const double aw = both ? p.aw : 0.0, total = aw + p.mw;
            double c = 0.0;
            if (both) c += aw * app;
            c += p.mw * iou_d[j];
            p.app[(size_t)t * N + j] = both ? (float)app : 1.0f;
            p.comb[(size_t)t * N + j] = (gated[j] || total == 0.0) ? 1.0f : (float)(c / total);
        }
    }
}

__global__ __launch_bounds__(TRACK_THREADS) void track_predict_cost_kernel(const TrackPredictParams p) { track_predict_cost_body(p); }

__device__ __forceinline__ void track_commit_body(const TrackCommitParams& p) {
    const int tid = threadIdx.x, D = p.D;
    if (p.hdr && (p.hdr[TRACK_HDR_STOPPED] != 0 || (int)blockIdx.x >= p.hdr[TRACK_HDR_M])) return;   // (sequence call: the grid is an upper bound)
    const int32_t* op = p.ops + 4 * blockIdx.x;
    const int slot = op[0], det = op[1], kind = op[2], missing = op[3];
    const int len = kind == TRACK_OP_NEW ? 0 : p.s.ring_meta[2 * slot], head = kind == TRACK_OP_NEW ? 0 : p.s.ring_meta[2 * slot + 1];
    __syncthreads();   // every thread holds the ring's old extent before thread 0 writes the new one
    const bool has = p.d.feat != nullptr && p.d.has[det] != 0;
    if (tid == 0) {
        const float z0 = p.d.foot[2 * det], z1 = p.d.foot[2 * det + 1];
        float x[4], P[16];
        if (kind == TRACK_OP_NEW) {
            x[0] = z0; x[1] = z1; x[2] = 0.f; x[3] = 0.f;
            for (int k = 0; k < 16; ++k) P[k] = 0.f;
            P[0] = 100.f; P[5] = 100.f; P[10] = 1000.f; P[15] = 1000.f;
        } else {
            for (int k = 0; k < 4; ++k) x[k] = p.s.x[4 * slot + k];
            for (int k = 0; k < 16; ++k) P[k] = p.s.P[16 * slot + k];
            if (missing >= 3) {   // observation-centric re-update: (predict, update) on the points between the last observation and this one
                const float l0 = p.s.last[2 * slot], l1 = p.s.last[2 * slot + 1];
                for (int i = 1; i <= missing; ++i) {
                    const float w = (float)((double)i / (double)(missing + 1));
                    kalman_predict(x, P);
                    kalman_update(x, P, l0 + w * (z0 - l0), l1 + w * (z1 - l1));
                }
            }
            kalman_update(x, P, z0, z1);
        }
        for (int k = 0; k < 4; ++k) p.s.x[4 * slot + k] = x[k];
        for (int k = 0; k < 16; ++k) p.s.P[16 * slot + k] = P[k];
        p.s.last[2 * slot] = z0;
        p.s.last[2 * slot + 1] = z1;
        for (int k = 0; k < 4; ++k) p.s.box[4 * slot + k] = p.d.boxes[4 * det + k];
        int nlen = len, nhead = head;
        if (has) {
            if (len < TRACK_RING) nlen = len + 1;
            else nhead = (head + 1) % TRACK_RING;
        }
        p.s.ring_meta[2 * slot] = nlen;
        p.s.ring_meta[2 * slot + 1] = nhead;
    }
    if (has) {   // a full ring: the new entry takes the oldest one's place
        const int at = len < TRACK_RING ? (head + len) % TRACK_RING : head;
        float* dst = p.s.ring + ((size_t)slot * TRACK_RING + at) * D;
        const float* src = p.d.feat + (size_t)det * D;
        for (int d = tid; d < D; d += TRACK_THREADS) dst[d] = src[d];
    }
}

__global__ __launch_bounds__(TRACK_THREADS) void track_commit_kernel(const TrackCommitParams p) { track_commit_body(p); }

// A feature row into the staging image: 64 lanes x 16 bytes = a 256-float row in one load each where both sides are 16-byte aligned
__device__ __forceinline__ void ingest_row(const float* src, float* dst, int D, int lane) {
    if ((D & 3) == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
        const float4* s4 = reinterpret_cast<const float4*>(src);
        float4* d4 = reinterpret_cast<float4*>(dst);
        for (int d = lane; d < D / 4; d += TRACK_INGEST_THREADS) d4[d] = s4[d];
    } else {
        for (int d = lane; d < D; d += TRACK_INGEST_THREADS) dst[d] = src[d];
    }
}

// One workgroup of one wave per record slot of a frame (p.view: that frame alone).  A record is 32 bytes (a merged one 48) and a row at most 8 KB: the launch is bound by its
// latency, not by bandwidth, so the geometry is many small workgroups that each finish in one round trip instead of few large ones that loop.  No LDS,
// no barrier: the slot search ends in a wave-wide maximum.
__device__ __forceinline__ void track_ingest_body(const TrackIngestParams& p) {
    const int i = blockIdx.x, lane = threadIdx.x, D = p.D, Q = p.view.stride;
    if (p.hdr && p.hdr[TRACK_HDR_STOPPED] != 0) return;
    const int n = opd::record_count(p.view, 0);
    if (i == 0 && lane == 0) *p.n_out = n;
    if (i >= n) return;   // (the whole workgroup)
    const int key = opd::record_key(p.view, i);
    const bool named = (unsigned)key < (unsigned)Q;
    const float* src = nullptr;
    if (p.rows_kind == TRACK_ROWS_BY_KEY) {
        if (named) src = p.rows + ((size_t)p.frame * Q + key) * D;
    } else if (p.rows_kind == TRACK_ROWS_BY_SLOT) {   // the slot whose entry names this record; a record without one enters with has = 0
        int filled = *p.n_person;
        filled = filled < p.slots ? filled : p.slots;
        const int want = p.frame * Q + key;
        int k = -1;
        if (named)
            for (int s = lane; s < filled; s += TRACK_INGEST_THREADS)
                if (p.slot_map[s] == want) k = s;   // (a key names one record of a frame at most)
        for (int o = 32; o > 0; o >>= 1) {
            const int other = __shfl_xor(k, o);
            k = other > k ? other : k;
        }
        if (k >= 0) src = p.rows + (size_t)k * D;
    }
    if (lane == 0) {
        // the values HipTracker.update hands to opd_track_update: the float32 box, and the foot point as camera_coords holds it, in float64 from the
        // UNROUNDED box and rounded where update stores it (not the foot point of the rounded box)
        double box[4];
        opd::record_box64(p.view, i, box);
        for (int k = 0; k < 4; ++k) p.boxes[4 * i + k] = (float)box[k];
        p.foot[2 * i] = (float)(box[0] + box[2] / 2);
        p.foot[2 * i + 1] = (float)(box[1] + box[3]);
        p.has[i] = src != nullptr;
    }
    if (src != nullptr) ingest_row(src, p.feat + (size_t)i * D, D, lane);
}

__global__ __launch_bounds__(TRACK_INGEST_THREADS) void track_ingest_kernel(const TrackIngestParams p) { track_ingest_body(p); }

// ---- the association on the device (sequence calls) -------------------------------------------------------------------------------------------
// opd_assoc.cpp by ONE wave, pair for pair: the same five stages over the same sub-blocks with the same comparisons, and a solver that takes the
// columns in the host's order.  The host's scan of the remaining columns (solve_wide) picks, among the positions k of remaining[] whose `shortest`
// is the minimum, the LARGEST k with an unassigned column when there is one and the SMALLEST k otherwise (a later position replaces an equal one
// only when its column is unassigned).  Here every lane keeps (minimum, largest unassigned position, smallest position) over the columns it owns and
// DPP reductions combine them.  The block a stage solves is copied to LDS first when it fits (TRACK_ASSOC_CACHE_FLOATS), since every step reads one
// row of it and a global load would be the longest link of that step's chain.  Duals and `shortest` are double and every expression is written as
// the host writes it, so with contraction off equal inputs give the same pick at every step, ties included.  A barrier of a one-wave workgroup is
// no instruction, only the fence that orders one lane's LDS / global writes before another lane's reads.
enum { NONE16 = 0xFFFF };
struct AssocLds {
    double u[TRACK_MAX_DETS], shortest[TRACK_MAX_DETS];
    uint16_t row_of[TRACK_MAX_DETS], path[TRACK_MAX_DETS], col_of[TRACK_MAX_DETS];
    uint8_t in_sr[TRACK_MAX_DETS], taken[TRACK_MAX_DETS];
    uint16_t high[TRACK_MAX_DETS], low[TRACK_MAX_DETS], tracks[TRACK_MAX_TRACKS], tentative[TRACK_MAX_TRACKS];
};
static_assert(TRACK_MAX_DETS == TRACK_MAX_TRACKS && TRACK_MAX_DETS < NONE16, "the per-row and per-column arrays share one size, indices fit 16 bits");

__device__ inline int lanes_below(unsigned long long mask, int lane) { return __popcll(mask & ((1ull << lane) - 1ull)); }

// list[count ..] <- the values of the lanes with `pred`, in lane order; returns the new count
__device__ inline int wave_append(uint16_t* list, int count, int value, bool pred, int lane) {
    const unsigned long long m = __ballot(pred);
    if (pred) list[count + lanes_below(m, lane)] = (uint16_t)value;
    return count + __popcll(m);
}

// Entry (i, j) of the solver's matrix: the sub-block tr x dl of `m`, transposed when it is tall, a value that is not finite counted as 1e9 (assign_rect).
// `cache` (nullable): the block as the solver sees it, [nr][nc] in LDS.
__device__ inline float assoc_entry(const float* m, int N, const uint16_t* tr, const uint16_t* dl, bool tall, int i, int j) {
    return tall ? m[(size_t)tr[j] * N + dl[i]] : m[(size_t)tr[i] * N + dl[j]];
}
__device__ inline double assoc_cost(const float* cache, int nc, const float* m, int N, const uint16_t* tr, const uint16_t* dl, bool tall, int i, int j) {
    const double v = (double)(cache ? cache[i * nc + j] : assoc_entry(m, N, tr, dl, tall, i, j));
    return isfinite(v) ? v : 1e9;
}

// The minimum of a double over the wave's 64 lanes, the same bits in every lane: four DPP steps inside each row of 16 lanes (the neighbour, the other
// pair, the other quad, the other half), then the four rows by readlane.  (Every lane is active where this is called.)
template <int CTRL>
__device__ inline double dpp_f64(double x) {
    int lo = __double2loint(x), hi = __double2hiint(x);
    lo = __builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xF, 0xF, false);
    hi = __builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xF, 0xF, false);
    return __hiloint2double(hi, lo);
}
__device__ inline double readlane_f64(double x, int lane) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), lane), __builtin_amdgcn_readlane(__double2loint(x), lane));
}
__device__ inline double wave_min_f64(double x) {
    double o = dpp_f64<0xB1>(x);   // quad_perm [1, 0, 3, 2]
    x = o < x ? o : x;
    o = dpp_f64<0x4E>(x);          // quad_perm [2, 3, 0, 1]
    x = o < x ? o : x;
    o = dpp_f64<0x141>(x);         // row_half_mirror
    x = o < x ? o : x;
    o = dpp_f64<0x140>(x);         // row_mirror
    x = o < x ? o : x;
    double r = readlane_f64(x, 0);
    for (int row = 16; row < 64; row += 16) {
        o = readlane_f64(x, row);
        r = o < r ? o : r;
    }
    return r;
}

// The largest / smallest int over the wave's 64 lanes, in every lane (the steps of wave_min_f64)
template <int CTRL>
__device__ inline int dpp_i32(int x) { return __builtin_amdgcn_update_dpp(x, x, CTRL, 0xF, 0xF, false); }
__device__ inline int wave_max_i32(int x) {
    int o = dpp_i32<0xB1>(x);
    x = o > x ? o : x;
    o = dpp_i32<0x4E>(x);
    x = o > x ? o : x;
    o = dpp_i32<0x141>(x);
    x = o > x ? o : x;
    o = dpp_i32<0x140>(x);
    x = o > x ? o : x;
    int r = __builtin_amdgcn_readlane(x, 0);
    for (int row = 16; row < 64; row += 16) {
        o = __builtin_amdgcn_readlane(x, row);
        r = o > r ? o : r;
    }
    return r;
}
__device__ inline int wave_min_i32(int x) { return ~wave_max_i32(~x); }   // (~ reverses the order of signed ints)

// solve_wide: nr <= nc; L.col_of [nr] and L.row_of [nc] out.  Lane l OWNS columns l, l + 64, ...: their `shortest`, dual, row, path entry and their
// POSITION in the host's remaining[] (-1 once taken out) live in its registers, so a step of the search is one LDS round trip (the row of the cost
// block and its dual) and register work; the swap-remove moves a position, not a column.  LDS sees the per-column state once per row, for the dual
// update of the rows and lane 0's walk along the path.
// ASSOC_QMAX: the columns a lane owns at most; a block of up to 64, 128 or 256 columns runs the instantiation that carries no more (assoc_solve).
template <int ASSOC_QMAX>
__device__ void assoc_solve_q(AssocLds& L, float* cache, const float* m, int N, const uint16_t* tr, const uint16_t* dl, bool tall, int nr, int nc, int lane) {
    const double INF = __builtin_huge_val();
    const int qn = (nc + 63) >> 6;
    if (nr * nc > TRACK_ASSOC_CACHE_FLOATS) cache = nullptr;   // (a block that does not fit is read from the global matrix at every step)
    if (cache)
        for (int e = lane; e < nr * nc; e += 64) cache[e] = assoc_entry(m, N, tr, dl, tall, e / nc, e % nc);
    for (int k = lane; k < nr; k += 64) { L.u[k] = 0.0; L.col_of[k] = NONE16; }
    for (int k = lane; k < nc; k += 64) L.row_of[k] = NONE16;
    double sh[ASSOC_QMAX], vv[ASSOC_QMAX];
    int ro[ASSOC_QMAX], pos[ASSOC_QMAX], pa[ASSOC_QMAX];
#pragma unroll
    for (int q = 0; q < ASSOC_QMAX; ++q) { vv[q] = 0.0; ro[q] = -1; sh[q] = INF; pa[q] = NONE16; pos[q] = -1; }
    for (int cur = 0; cur < nr; ++cur) {
#pragma unroll
        for (int q = 0; q < ASSOC_QMAX; ++q) {
            const int j = lane + 64 * q;
            sh[q] = INF; pa[q] = NONE16;
            pos[q] = j < nc ? nc - 1 - j : -1;   // remaining[k] = nc - 1 - k
        }
        for (int k = lane; k < nr; k += 64) L.in_sr[k] = 0;
        __syncthreads();
        int n_rem = nc, i = cur, sink = -1;
        double min_val = 0.0;
        while (sink < 0) {
            if (lane == 0) L.in_sr[i] = 1;
            const double ui = L.u[i];
            double best = INF;
            int k_un = -1, k_first = 0x7fffffff;
#pragma unroll
            for (int q = 0; q < ASSOC_QMAX; ++q) {
                if (q < qn && pos[q] >= 0) {
                    const double r = min_val + assoc_cost(cache, nc, m, N, tr, dl, tall, i, lane + 64 * q) - ui - vv[q];
                    if (r < sh[q]) { sh[q] = r; pa[q] = i; }
                    const double s = sh[q];
                    const int k = pos[q];
                    const bool un = ro[q] < 0;
                    if (s < best) { best = s; k_first = k; k_un = un ? k : -1; }
                    else if (s == best) {
                        k_first = k < k_first ? k : k_first;
                        if (un && k > k_un) k_un = k;
                    }
                }
            }
            // the host's pick among the positions that attain the minimum: the largest whose column is unassigned, else the smallest
            const double lowest = wave_min_f64(best);
            const bool cand = best == lowest;
            int index = wave_max_i32(cand ? k_un : -1);
            if (index < 0) index = wave_min_i32(cand ? k_first : 0x7fffffff);
            if (index >= n_rem) return;   // (cannot happen with finite costs; every lane holds the same index)
            min_val = lowest;
            --n_rem;
            int mine_j = -1, mine_r = -1;
#pragma unroll
            for (int q = 0; q < ASSOC_QMAX; ++q) {
                if (q < qn) {
                    if (pos[q] == index) { mine_j = lane + 64 * q; mine_r = ro[q]; pos[q] = -1; }   // taken out ...
                    else if (pos[q] == n_rem) pos[q] = index;                                        // ... and the last one takes its place
                }
            }
            const int owner = __ffsll(__ballot(mine_j >= 0)) - 1;   // (one lane)
            const int j = __builtin_amdgcn_readlane(mine_j, owner), r = __builtin_amdgcn_readlane(mine_r, owner);
            if (r < 0) sink = j;
            else i = r;
        }
#pragma unroll
        for (int q = 0; q < ASSOC_QMAX; ++q) {
            const int j = lane + 64 * q;
            if (j < nc) { L.shortest[j] = sh[q]; L.path[j] = (uint16_t)pa[q]; }
        }
        __syncthreads();
        for (int r = lane; r < nr; r += 64)
            if (L.in_sr[r] && r != cur) L.u[r] += min_val - L.shortest[L.col_of[r]];
        if (lane == 0) L.u[cur] += min_val;
#pragma unroll
        for (int q = 0; q < ASSOC_QMAX; ++q)
            if (lane + 64 * q < nc && pos[q] < 0) vv[q] -= min_val - sh[q];   // (the columns taken out: the host's in_sc)
        __syncthreads();
        if (lane == 0) {   // augment along the path back to the new row
            int j = sink;
            for (int step = 0; step < nr; ++step) {   // (a path visits a row once: at most nr steps)
                const int r = L.path[j];
                L.row_of[j] = (uint16_t)r;
                const int was = L.col_of[r];
                L.col_of[r] = (uint16_t)j;
                j = was;
                if (r == cur) break;
            }
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < ASSOC_QMAX; ++q) {
            const int j = lane + 64 * q;
            if (j < nc) { const int r = L.row_of[j]; ro[q] = r == NONE16 ? -1 : r; }
        }
    }
}

__device__ void assoc_solve(AssocLds& L, float* cache, const float* m, int N, const uint16_t* tr, const uint16_t* dl, bool tall, int nr, int nc, int lane) {
    if (nc <= 64) assoc_solve_q<1>(L, cache, m, N, tr, dl, tall, nr, nc, lane);
    else if (nc <= 128) assoc_solve_q<2>(L, cache, m, N, tr, dl, tall, nr, nc, lane);
    else if (nc <= 256) assoc_solve_q<4>(L, cache, m, N, tr, dl, tall, nr, nc, lane);
    else assoc_solve_q<TRACK_MAX_DETS / 64>(L, cache, m, N, tr, dl, tall, nr, nc, lane);
}

// One stage (`stage` of opd_assoc.cpp): rows tr x columns dl of `m`.  Kept pairs go to ops[4 * M ..] as (track row, detection) in the order of the
// rows; tr becomes the rows left over, dl loses the matched detections when remove_dets.  The test reads the RAW matrix entry, as the host does.
__device__ void assoc_stage(AssocLds& L, float* cache, const float* m, int N, uint16_t* tr, int& n_tr, uint16_t* dl, int& n_dl, double thr, bool inclusive, bool remove_dets,
                            int32_t* ops, int& M, int lane) {
    if (n_tr == 0 || n_dl == 0) return;
    const bool tall = n_tr > n_dl;
    assoc_solve(L, cache, m, N, tr, dl, tall, tall ? n_dl : n_tr, tall ? n_tr : n_dl, lane);
    for (int k = lane; k < n_dl; k += 64) L.taken[k] = 0;
    __syncthreads();
    int n_left = 0;
    for (int base = 0; base < n_tr; base += 64) {
        const int i = base + lane;
        bool ok = false;
        int trk = 0, det = 0;
        if (i < n_tr) {
            trk = tr[i];
            const int j = tall ? L.row_of[i] : L.col_of[i];
            if (j != NONE16) {
                det = dl[j];
                const double v = (double)m[(size_t)trk * N + det];
                ok = inclusive ? v <= thr : v < thr;
                if (ok) L.taken[j] = 1;
            }
        }
        __syncthreads();   // the chunk is in registers before its places are written over
        const unsigned long long mk = __ballot(ok);
        if (ok) {
            const int at = M + lanes_below(mk, lane);
            ops[4 * at] = trk;
            ops[4 * at + 1] = det;
        }
        M += __popcll(mk);
        n_left = wave_append(tr, n_left, trk, i < n_tr && !ok, lane);
        __syncthreads();
    }
    n_tr = n_left;
    if (!remove_dets) return;
    int n_rest = 0;
    for (int base = 0; base < n_dl; base += 64) {
        const int j = base + lane;
        const bool rest = j < n_dl && !L.taken[j];
        const int det = j < n_dl ? dl[j] : 0;
        __syncthreads();
        n_rest = wave_append(dl, n_rest, det, rest, lane);
        __syncthreads();
    }
    n_dl = n_rest;
}

// `cache`: the kernel's dynamic LDS, [TRACK_ASSOC_CACHE_FLOATS]: the block a stage solves, when it fits
__device__ __forceinline__ void track_assoc_body(const TrackAssocParams& p, float* cache) {
    __shared__ AssocLds L;
    const int lane = threadIdx.x, S = p.S, E = TRACK_ENTRY_INTS;
    if (p.hdr[TRACK_HDR_STOPPED] != 0) return;
    int T = p.hdr[TRACK_HDR_T], N = p.n_dev ? *p.n_dev : p.n, n_free = p.hdr[TRACK_HDR_N_FREE], next_id = p.hdr[TRACK_HDR_NEXT_ID];
    T = T < 0 ? 0 : (T > S ? S : T);   // (a table the host wrote: the clamps keep every index below inside its array whatever it holds)
    N = N < 0 ? 0 : (N > TRACK_MAX_DETS ? TRACK_MAX_DETS : N);
    n_free = n_free < 0 ? 0 : (n_free > S - T ? S - T : n_free);
    for (int t = lane; t < T; t += 64) p.tab[E * t + 4] += 1;   // `Track.predict`
    for (int j = lane; j < N; j += 64) p.ids[j] = -1;
    int n_high = 0, n_low = 0, n_trk = 0, n_tent = 0, M = 0;
    for (int base = 0; base < N; base += 64) {
        const int j = base + lane;
        const bool hi = j < N && (double)p.conf[(size_t)j * p.conf_stride] >= p.high_conf;
        n_high = wave_append(L.high, n_high, j, hi, lane);
        n_low = wave_append(L.low, n_low, j, j < N && !hi, lane);
    }
    for (int base = 0; base < T; base += 64) {
        const int t = base + lane;
        const bool confirmed = t < T && p.tab[E * t + 3] >= p.min_hits;
        n_trk = wave_append(L.tracks, n_trk, t, confirmed, lane);
        n_tent = wave_append(L.tentative, n_tent, t, t < T && !confirmed, lane);
    }
    __syncthreads();
    if (T > 0 && N > 0) {
        // the five stages of associate(), one after the other (a loop, so that the solver is compiled once): 0 appearance only, <= 0.3; 1 appearance + IoU
        // behind the distance gate; 2 IoU only; 3 the low-confidence rescue (those detections are never removed, nor start tracks); 4 the tentative
        // tracks on what is left of the high-confidence detections
        for (int st = 0; st < 5; ++st) {
            const float* m = st == 0 ? p.app : (st == 1 || st == 4) ? p.comb : p.iou;
            uint16_t* tr = st == 4 ? L.tentative : L.tracks;
            uint16_t* dl = st == 3 ? L.low : L.high;
            int n_tr = st == 4 ? n_tent : n_trk, n_dl = st == 3 ? n_low : n_high;
            const double thr = st == 0 ? 0.3 : st == 2 ? 1.0 - 0.4 : 1.0 - 0.5;
            assoc_stage(L, cache, m, N, tr, n_tr, dl, n_dl, thr, st == 0, st != 3, p.ops, M, lane);
            if (st == 4) n_tent = n_tr;
            else n_trk = n_tr;
            if (st == 3) n_low = n_dl;
            else n_high = n_dl;
        }
    }
    if (p.unmatched) {   // (test hook) associate()'s unmatched_tracks: every row in order when there is no detection, else confirmed rows, then tentative ones
        if (lane == 0) p.unmatched[0] = N > 0 ? n_trk + n_tent : T;
        for (int k = lane; k < (N > 0 ? n_trk : T); k += 64) p.unmatched[1 + k] = N > 0 ? L.tracks[k] : k;
        for (int k = lane; k < (N > 0 ? n_tent : 0); k += 64) p.unmatched[1 + n_trk + k] = L.tentative[k];
    }
    int n_new = n_high;   // the high-confidence detections no stage matched, ascending: they start tracks
    if (n_new > n_free) {   // out of slots: matches and new tracks are dropped, the frame counts as one without detections, the call ends here
        if (lane == 0) { p.hdr[TRACK_HDR_STOPPED] = 1; p.hdr[TRACK_HDR_STOP_T] = T; p.hdr[TRACK_HDR_STOP_NEW] = n_new; }
        M = 0;
        n_new = 0;
    }
    __syncthreads();   // the pairs in ops and the aged counters are complete
    for (int k = lane; k < M; k += 64) {   // (a row is matched once at most: every lane has its own entry)
        int32_t* e = p.tab + E * p.ops[4 * k];
        const int det = p.ops[4 * k + 1];
        p.ops[4 * k] = e[0]; p.ops[4 * k + 2] = TRACK_OP_MATCHED; p.ops[4 * k + 3] = e[4];
        e[2] += 1; e[3] += 1; e[4] = 0;
        p.ids[det] = e[1];
    }
    for (int r = lane; r < n_new; r += 64) {
        const int det = L.high[r], slot = p.free_slots[n_free - 1 - r], id = next_id + r;
        int32_t* e = p.tab + E * (T + r);
        e[0] = slot; e[1] = id; e[2] = 1; e[3] = 1; e[4] = 0;
        int32_t* op = p.ops + 4 * (M + r);
        op[0] = slot; op[1] = det; op[2] = TRACK_OP_NEW; op[3] = 0;
        p.ids[det] = id;
    }
    M += n_new; T += n_new; n_free -= n_new; next_id += n_new;
    __syncthreads();
    // the tracks that went max_age frames without a match leave, in order; their slots go back on the stack
    int keep = 0;
    for (int base = 0; base < T; base += 64) {
        const int t = base + lane;
        int32_t e[TRACK_ENTRY_INTS] = {0, 0, 0, 0, 0};
        if (t < T)
            for (int k = 0; k < E; ++k) e[k] = p.tab[E * t + k];
        __syncthreads();   // the chunk is in registers before its places are written over
        const bool stay = t < T && e[4] < p.max_age, go = t < T && !stay;
        const unsigned long long ms = __ballot(stay), mg = __ballot(go);
        if (stay)
            for (int k = 0; k < E; ++k) p.tab[E * (keep + lanes_below(ms, lane)) + k] = e[k];
        if (go) p.free_slots[n_free + lanes_below(mg, lane)] = e[0];
        keep += __popcll(ms);
        n_free += __popcll(mg);
        __syncthreads();
    }
    if (lane == 0) {
        p.hdr[TRACK_HDR_T] = keep; p.hdr[TRACK_HDR_NEXT_ID] = next_id; p.hdr[TRACK_HDR_N_FREE] = n_free; p.hdr[TRACK_HDR_M] = M;
        p.hdr[TRACK_HDR_FRAMES_DONE] = p.frame + 1;
    }
}

__global__ __launch_bounds__(TRACK_ASSOC_THREADS) void track_assoc_kernel(const TrackAssocParams p) {
    extern __shared__ float cache[];
    track_assoc_body(p, cache);
}

// ---- several cameras in one launch (opd_track_update_streams, opd_detr_detect_streams_track) ---------------------------------------
// blockIdx.y is the camera, blockIdx.x what it is above, under a grid that covers the largest bound among the cameras of the step.  The workgroup copies
// its camera's block out of descs [gridDim.y] (a uniform load: it lands in scalar registers as a kernel argument does) and runs the body above on it.
// It leaves at once where the camera has nothing to do in this launch (`hdr` null: no frame at this step, or a bound of zero), where it lies beyond the
// camera's own bound, and, inside the body, where the camera's TRACK_HDR_STOPPED is set.  Cameras share no memory: each block names its own tracker's
// table, staging image and slot state.
__global__ __launch_bounds__(TRACK_THREADS) void track_predict_cost_multi_kernel(const TrackPredictParams* __restrict__ descs) {
    const TrackPredictParams p = descs[blockIdx.y];
    if (!p.hdr || (int)blockIdx.x >= p.T) return;
    track_predict_cost_body(p);
}

__global__ __launch_bounds__(TRACK_THREADS) void track_commit_multi_kernel(const TrackCommitParams* __restrict__ descs) {
    const TrackCommitParams p = descs[blockIdx.y];
    if (!p.hdr || (int)blockIdx.x >= p.M) return;
    track_commit_body(p);
}

__global__ __launch_bounds__(TRACK_INGEST_THREADS) void track_ingest_multi_kernel(const TrackIngestParams* __restrict__ descs) {
    const TrackIngestParams p = descs[blockIdx.y];
    if (!p.hdr || (int)blockIdx.x >= p.view.stride) return;
    track_ingest_body(p);
}

__global__ __launch_bounds__(TRACK_ASSOC_THREADS) void track_assoc_multi_kernel(const TrackAssocParams* __restrict__ descs) {
    extern __shared__ float cache[];
    const TrackAssocParams p = descs[blockIdx.y];
    if (!p.hdr) return;
    track_assoc_body(p, cache);
}

}  // namespace

// What a launcher refuses, per parameter block: the one-tracker launchers and the camera-batched ones (on the host's copy of every block) share it
static bool assoc_params_ok(const TrackAssocParams& p) {
    if (p.S < 1 || p.S > TRACK_MAX_TRACKS || p.n < 0 || p.n > TRACK_MAX_DETS || p.conf_stride < 1 || p.frame < 0) return false;
    return p.hdr && p.tab && p.free_slots && p.app && p.iou && p.comb && p.ops && p.ids && (p.conf || (!p.n_dev && p.n == 0));
}
static bool ingest_params_ok(const TrackIngestParams& p) {
    const int Q = p.view.stride;
    if (Q < 1 || Q > TRACK_MAX_DETS || p.D < 1 || p.D > TRACK_MAX_DIM || p.frame < 0 || p.slots < 0) return false;
    if (p.rows_kind != TRACK_ROWS_NONE && p.rows_kind != TRACK_ROWS_BY_KEY && p.rows_kind != TRACK_ROWS_BY_SLOT) return false;
    if (!p.view.records == !p.view.merged || !p.view.counts || !p.boxes || !p.foot || !p.has || !p.n_out) return false;
    if (p.rows_kind != TRACK_ROWS_NONE && (!p.rows || !p.feat)) return false;
    return p.rows_kind != TRACK_ROWS_BY_SLOT || (p.slot_map && p.n_person);
}
static bool predict_params_ok(const TrackPredictParams& p) {
    if (p.T <= 0 || p.T > TRACK_MAX_TRACKS || p.d.n < 0 || p.d.n > TRACK_MAX_DETS || p.D < 1 || p.D > TRACK_MAX_DIM) return false;
    return p.hdr ? p.tab != nullptr : p.slots != nullptr;
}
static bool commit_params_ok(const TrackCommitParams& p) { return p.M > 0 && p.M <= TRACK_MAX_TRACKS && p.D >= 1 && p.D <= TRACK_MAX_DIM && p.ops; }

hipError_t opd_launch_track_assoc(const TrackAssocParams& p, hipStream_t stream) {
    if (!assoc_params_ok(p)) return hipErrorInvalidValue;
    OPD_SET_MAX_LDS_ONCE(track_assoc_kernel, TRACK_ASSOC_CACHE_FLOATS * 4);
    OPD_LAUNCH(track_assoc_kernel, dim3(1), dim3(TRACK_ASSOC_THREADS), TRACK_ASSOC_CACHE_FLOATS * 4, stream, p);
    return hipGetLastError();
}

hipError_t opd_launch_track_ingest(const TrackIngestParams& p, hipStream_t stream) {
    if (!ingest_params_ok(p)) return hipErrorInvalidValue;
    OPD_LAUNCH(track_ingest_kernel, dim3(p.view.stride), dim3(TRACK_INGEST_THREADS), 0, stream, p);
    return hipGetLastError();
}

hipError_t opd_launch_track_predict_cost(const TrackPredictParams& p, hipStream_t stream) {
    if (!predict_params_ok(p)) return hipErrorInvalidValue;
    OPD_LAUNCH(track_predict_cost_kernel, dim3(p.T), dim3(TRACK_THREADS), 0, stream, p);
    return hipGetLastError();
}

hipError_t opd_launch_track_commit(const TrackCommitParams& p, hipStream_t stream) {
    if (!commit_params_ok(p)) return hipErrorInvalidValue;
    OPD_LAUNCH(track_commit_kernel, dim3(p.M), dim3(TRACK_THREADS), 0, stream, p);
    return hipGetLastError();
}

// The camera-batched launches.  `host`: the C blocks of the step as the host built them, `dev` the same bytes on the device.  A block with a null `hdr`
// is a camera without work in this launch; every other block passes the one-tracker launcher's checks.  grid.x: the largest bound among them.
// *launched (nullable): whether a launch was made (none where no camera has work).
template <typename P, typename Ok, typename Bound>
static hipError_t multi_grid(const P* host, const P* dev, int C, Ok ok, Bound bound, int* grid_x) {
    *grid_x = 0;
    if (!host || !dev || C < 1 || C > TRACK_MAX_CAMERAS) return hipErrorInvalidValue;
    for (int c = 0; c < C; ++c) {
        if (!host[c].hdr) continue;
        if (!ok(host[c])) return hipErrorInvalidValue;
        *grid_x = bound(host[c]) > *grid_x ? bound(host[c]) : *grid_x;
    }
    return hipSuccess;
}

hipError_t opd_launch_track_assoc_multi(const TrackAssocParams* host, const TrackAssocParams* dev, int C, hipStream_t stream, int* launched) {
    int gx = 0;
    const hipError_t e = multi_grid(host, dev, C, assoc_params_ok, [](const TrackAssocParams&) { return 1; }, &gx);
    if (launched) *launched = e == hipSuccess && gx > 0;
    if (e != hipSuccess || gx == 0) return e;
    OPD_SET_MAX_LDS_ONCE(track_assoc_multi_kernel, TRACK_ASSOC_CACHE_FLOATS * 4);
    OPD_LAUNCH(track_assoc_multi_kernel, dim3(1, C), dim3(TRACK_ASSOC_THREADS), TRACK_ASSOC_CACHE_FLOATS * 4, stream, dev);
    return hipGetLastError();
}

hipError_t opd_launch_track_ingest_multi(const TrackIngestParams* host, const TrackIngestParams* dev, int C, hipStream_t stream, int* launched) {
    int gx = 0;
    const hipError_t e = multi_grid(host, dev, C, ingest_params_ok, [](const TrackIngestParams& p) { return (int)p.view.stride; }, &gx);
    if (launched) *launched = e == hipSuccess && gx > 0;
    if (e != hipSuccess || gx == 0) return e;
    OPD_LAUNCH(track_ingest_multi_kernel, dim3(gx, C), dim3(TRACK_INGEST_THREADS), 0, stream, dev);
    return hipGetLastError();
}

hipError_t opd_launch_track_predict_cost_multi(const TrackPredictParams* host, const TrackPredictParams* dev, int C, hipStream_t stream, int* launched) {
    int gx = 0;
    const hipError_t e = multi_grid(host, dev, C, predict_params_ok, [](const TrackPredictParams& p) { return (int)p.T; }, &gx);
    if (launched) *launched = e == hipSuccess && gx > 0;
    if (e != hipSuccess || gx == 0) return e;
    OPD_LAUNCH(track_predict_cost_multi_kernel, dim3(gx, C), dim3(TRACK_THREADS), 0, stream, dev);
    return hipGetLastError();
}

hipError_t opd_launch_track_commit_multi(const TrackCommitParams* host, const TrackCommitParams* dev, int C, hipStream_t stream, int* launched) {
    int gx = 0;
    const hipError_t e = multi_grid(host, dev, C, commit_params_ok, [](const TrackCommitParams& p) { return (int)p.M; }, &gx);
    if (launched) *launched = e == hipSuccess && gx > 0;
    if (e != hipSuccess || gx == 0) return e;
    OPD_LAUNCH(track_commit_multi_kernel, dim3(gx, C), dim3(TRACK_THREADS), 0, stream, dev);
    return hipGetLastError();
}
