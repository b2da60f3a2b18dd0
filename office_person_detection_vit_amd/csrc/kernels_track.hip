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

__global__ __launch_bounds__(TRACK_THREADS) void track_predict_cost_kernel(const TrackPredictParams p) {
    __shared__ float sm[TRACK_MAX_DIM];          // the smoothed feature
    __shared__ double iou_d[TRACK_MAX_DETS];     // IoU distance per detection, before rounding
    __shared__ uint8_t gated[TRACK_MAX_DETS];
    __shared__ float wsum[TRACK_THREADS / 64];
    __shared__ float pos[2];
    const int t = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int slot = p.slots[t], D = p.D, N = p.n_dev ? *p.n_dev : p.d.n;   // (the fused call: the count is the ingest launch's, at most Q <= TRACK_MAX_DETS)
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

__global__ __launch_bounds__(TRACK_THREADS) void track_commit_kernel(const TrackCommitParams p) {
    const int tid = threadIdx.x, D = p.D;
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

// One workgroup of one wave per record slot of a frame.  A record is 32 bytes and a row at most 8 KB: the launch is bound by its latency, not by
// bandwidth, so the geometry is many small workgroups that each finish in one round trip (64 lanes x 16 bytes = a 256-float row in one load each)
// instead of few large ones that loop.  No LDS, no barrier: the slot search ends in a wave-wide maximum.
__global__ __launch_bounds__(TRACK_INGEST_THREADS) void track_ingest_kernel(const TrackIngestParams p) {
    const int i = blockIdx.x, lane = threadIdx.x, D = p.D;
    int n = *p.count;
    n = n < 0 ? 0 : (n > p.Q ? p.Q : n);
    if (i == 0 && lane == 0) *p.n_out = n;
    if (i >= n) return;   // (the whole workgroup)
    const opd_det r = p.records[i];
    const float* src = nullptr;
    if (p.rows_kind == TRACK_ROWS_BY_QUERY) {
        if ((unsigned)r.query_index < (unsigned)p.Q) src = p.rows + ((size_t)p.frame * p.Q + r.query_index) * D;
    } else if (p.rows_kind == TRACK_ROWS_BY_SLOT) {
        int filled = *p.n_person;
        filled = filled < p.slots ? filled : p.slots;
        const int want = p.frame * p.Q + r.query_index;
        int k = -1;
        if ((unsigned)r.query_index < (unsigned)p.Q)
            for (int s = lane; s < filled; s += TRACK_INGEST_THREADS)
                if (p.slot_map[s] == want) k = s;   // (a query index names one record of a frame at most)
        for (int o = 32; o > 0; o >>= 1) {
            const int other = __shfl_xor(k, o);
            k = other > k ? other : k;
        }
        if (k >= 0) src = p.rows + (size_t)k * D;
    }
    if (lane == 0) {
        // the values detector.py::_postprocess_batch and HipTracker.update hand to opd_track_update: differences and sums in double, rounded once
        const double bw = (double)r.x2 - (double)r.x1, bh = (double)r.y2 - (double)r.y1;
        p.boxes[4 * i] = r.x1;
        p.boxes[4 * i + 1] = r.y1;
        p.boxes[4 * i + 2] = (float)bw;
        p.boxes[4 * i + 3] = (float)bh;
        p.foot[2 * i] = (float)((double)r.x1 + bw / 2);
        p.foot[2 * i + 1] = (float)((double)r.y1 + bh);
        p.has[i] = src != nullptr;
    }
    if (src == nullptr) return;
    float* dst = p.feat + (size_t)i * D;
    if ((D & 3) == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
        const float4* s4 = reinterpret_cast<const float4*>(src);
        float4* d4 = reinterpret_cast<float4*>(dst);
        for (int d = lane; d < D / 4; d += TRACK_INGEST_THREADS) d4[d] = s4[d];
    } else {
        for (int d = lane; d < D; d += TRACK_INGEST_THREADS) dst[d] = src[d];
    }
}

}  // namespace

hipError_t opd_launch_track_ingest(const TrackIngestParams& p, hipStream_t stream) {
    if (p.Q < 1 || p.Q > TRACK_MAX_DETS || p.D < 1 || p.D > TRACK_MAX_DIM || p.frame < 0 || p.slots < 0) return hipErrorInvalidValue;
    if (p.rows_kind != TRACK_ROWS_NONE && p.rows_kind != TRACK_ROWS_BY_QUERY && p.rows_kind != TRACK_ROWS_BY_SLOT) return hipErrorInvalidValue;
    if (!p.records || !p.count || !p.boxes || !p.foot || !p.has || !p.n_out) return hipErrorInvalidValue;
    if (p.rows_kind != TRACK_ROWS_NONE && (!p.rows || !p.feat)) return hipErrorInvalidValue;
    if (p.rows_kind == TRACK_ROWS_BY_SLOT && (!p.slot_map || !p.n_person)) return hipErrorInvalidValue;
    OPD_LAUNCH(track_ingest_kernel, dim3(p.Q), dim3(TRACK_INGEST_THREADS), 0, stream, p);
    return hipGetLastError();
}

hipError_t opd_launch_track_predict_cost(const TrackPredictParams& p, hipStream_t stream) {
    if (p.T <= 0 || p.T > TRACK_MAX_TRACKS || p.d.n < 0 || p.d.n > TRACK_MAX_DETS || p.D < 1 || p.D > TRACK_MAX_DIM) return hipErrorInvalidValue;
    OPD_LAUNCH(track_predict_cost_kernel, dim3(p.T), dim3(TRACK_THREADS), 0, stream, p);
    return hipGetLastError();
}

hipError_t opd_launch_track_commit(const TrackCommitParams& p, hipStream_t stream) {
    if (p.M <= 0 || p.M > TRACK_MAX_TRACKS || p.D < 1 || p.D > TRACK_MAX_DIM) return hipErrorInvalidValue;
    OPD_LAUNCH(track_commit_kernel, dim3(p.M), dim3(TRACK_THREADS), 0, stream, p);
    return hipGetLastError();
}
