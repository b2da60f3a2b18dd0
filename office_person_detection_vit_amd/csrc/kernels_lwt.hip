// kernels_lwt.hip — the two launches of the reference's hybrid tracker (`LightweightTracker`, src/tracking/lightweight_tracker.py:211-455,
// with its `LightweightTrack` and the bookkeeping of `OpticalFlowTracker`).  Built with -ffp-contract=off: every expression is evaluated
// operation by operation in the order written, and tests/lwt_common.py restates the same order in numpy.
//
// The Kalman formulas and their order are those of kernels_track.hip.  What differs is the element type of x.  The reference's P, S and K
// are float32 arrays always; its x starts as float32, and `KalmanFilter.update` with the float64 centre of a detection-frame match makes it
// float64 for good (y = z - H x is float64, so K @ y and x + K @ y are).  An update with one of LK's float32 points leaves a float32 x
// float32.  So a track carries x as double plus a flag "x still holds float32 values and is computed on in float32".
//
//   lwt_update_kernel   `update_with_detections`: ONE workgroup of 256 threads (the greedy match is sequential; the launch is bound by
//       latency, not throughput).  (a) IoU matrix in double on the float32 boxes, one wave per row, with each row's maximum and its
//       lowest column cached in LDS.  (b) Greedy match: the maximum over the cached row maxima, ties to the lowest row-major index
//       (numpy's argmax), stop below the threshold; the matched row and column leave, and only rows whose cached column was taken are
//       scanned again.  The match reads boxes only, which the predict does not change, so it runs first and (c) an update whose new
//       tracks would not fit ends here having written nothing.  (d) Prefix sums: the position of every surviving track, the rank of
//       every unmatched detection.  (e) One thread per track: predict, counters, the matched detection's update, written to its
//       position in the OTHER bank; one thread per unmatched detection: a new track.  (f) ids, flow points, head.
//   lwt_interp_kernel   `interpolate`: one workgroup, one thread per track.  A track whose id has a followed point moves its box there and
//       is updated with the point; any other track is predicted.  Then the point list is compacted to the followed points in order.
//   lwt_ingest_kernel   the fused detect calls only (opd_detr_detect_frames_hybrid, opd_detr_detect_tiled_hybrid and their sequence forms): one
//       wave turns the kept records of a frame, read through the call's RecordView where the suppression kernel or (a tiled call) the seam
//       merge left them, into the float32 [n][4] xywh image `np.array([d.bbox for d in dets], np.float32)` is -- corners as they
//       are, width and height as differences in double rounded once (track_ingest_kernel's box rule) -- and leaves the kept count on the
//       device, where lwt_update_kernel (LwtUpdateParams::count) reads it.
#include <hip/hip_runtime.h>

#include "opd_kprims.h"
#include "opd_lwt.h"

namespace {

struct Kf {
    double x[4];
    float P[16];
    int f32;
};

__device__ void kf_load(Kf& k, const LwtBank& b, int i) {
    for (int j = 0; j < 4; ++j) k.x[j] = b.x[4 * i + j];
    for (int j = 0; j < 16; ++j) k.P[j] = b.P[16 * i + j];
    k.f32 = b.meta[LWT_META * i + LWT_F32];
}

__device__ void kf_store(const Kf& k, const LwtBank& b, int i) {
    for (int j = 0; j < 4; ++j) b.x[4 * i + j] = k.x[j];
    for (int j = 0; j < 16; ++j) b.P[16 * i + j] = k.P[j];
    b.meta[LWT_META * i + LWT_F32] = k.f32;
}

// F = [[1 0 1 0] [0 1 0 1] [0 0 1 0] [0 0 0 1]], P <- (F P) F^T + Q: kernels_track.hip's kalman_predict, x in its own element type
__device__ void kf_predict(Kf& k) {
    if (k.f32) {
        const float a = (float)k.x[0] + (float)k.x[2], b = (float)k.x[1] + (float)k.x[3];
        k.x[0] = a;
        k.x[1] = b;
    } else {
        k.x[0] = k.x[0] + k.x[2];
        k.x[1] = k.x[1] + k.x[3];
    }
    const float q = 0.1f;
    float* P = k.P;
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
    for (int j = 0; j < 16; ++j) P[j] = B[j] + Q[j];
}

// kernels_track.hip's kalman_update.  S, its inverse, K and P <- (I - K H) P in float32; y = z - H x and x <- x + K y in float32 when both x
// and z are float32, else in double on the float32 K (numpy promotes K for `K @ y`), after which x is float64 for good.
__device__ void kf_update(Kf& k, double z0, double z1, bool z_f32) {
    float* P = k.P;
    const float s00 = P[0] + 1.0f, s01 = P[1], s10 = P[4], s11 = P[5] + 1.0f;
    const float det = s00 * s11 - s01 * s10;
    const float i00 = s11 / det, i01 = (-s01) / det, i10 = (-s10) / det, i11 = s00 / det;
    float K[8], M[16], N[16];
    for (int i = 0; i < 4; ++i) {
        K[2 * i] = P[4 * i] * i00 + P[4 * i + 1] * i10;
        K[2 * i + 1] = P[4 * i] * i01 + P[4 * i + 1] * i11;
    }
    if (k.f32 && z_f32) {
        const float y0 = (float)z0 - (float)k.x[0], y1 = (float)z1 - (float)k.x[1];
        for (int i = 0; i < 4; ++i) {
            const float v = (float)k.x[i] + (K[2 * i] * y0 + K[2 * i + 1] * y1);
            k.x[i] = v;
        }
    } else {
        const double y0 = z0 - k.x[0], y1 = z1 - k.x[1];
        for (int i = 0; i < 4; ++i) k.x[i] = k.x[i] + ((double)K[2 * i] * y0 + (double)K[2 * i + 1] * y1);
        k.f32 = 0;
    }
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) M[4 * i + j] = (i == j ? 1.0f : 0.0f) - (j < 2 ? K[2 * i + j] : 0.0f);
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j)
            N[4 * i + j] = ((M[4 * i] * P[j] + M[4 * i + 1] * P[4 + j]) + M[4 * i + 2] * P[8 + j]) + M[4 * i + 3] * P[12 + j];
    for (int j = 0; j < 16; ++j) P[j] = N[j];
}

// `_compute_iou` in double on float32 boxes, Python's max / min spelled out (the second argument wins only when strictly beyond the first)
__device__ double iou_xywh(const float* a, const float* b) {
    const double x1 = a[0], y1 = a[1], w1 = a[2], h1 = a[3], x2 = b[0], y2 = b[1], w2 = b[2], h2 = b[3];
    const double xi1 = x2 > x1 ? x2 : x1, yi1 = y2 > y1 ? y2 : y1;
    const double r1 = x1 + w1, r2 = x2 + w2, b1 = y1 + h1, b2 = y2 + h2;
    const double xi2 = r2 < r1 ? r2 : r1, yi2 = b2 < b1 ? b2 : b1;
    const double dw = xi2 - xi1, dh = yi2 - yi1;
    const double iw = dw > 0.0 ? dw : 0.0, ih = dh > 0.0 ? dh : 0.0;
    const double inter = iw * ih;
    const double uni = (w1 * h1 + w2 * h2) - inter;
    if (uni <= 0.0) return 0.0;
    return inter / uni;
}

// (value, index) maxima: the larger value, among equal values the lower index -- numpy's argmax over a row-major matrix
struct Best {
    double v;
    int i;
};
__device__ __forceinline__ bool beats(double v, int i, const Best& b) { return v > b.v || (v == b.v && i < b.i); }
__device__ __forceinline__ Best wave_best(Best b) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(b.v, o);
        const int oi = __shfl_xor(b.i, o);
        if (beats(ov, oi, b)) { b.v = ov; b.i = oi; }
    }
    return b;   // all 64 lanes hold the same pair
}

// a[0, n) (LDS, n <= 4 * LWT_THREADS) <- its exclusive prefix sums; returns the total.  Thread i owns a[4 i .. 4 i + 3].
__device__ int block_exclusive_scan(int* a, int n, int* wtot) {
    static_assert(LWT_THREADS == 256 && 4 * LWT_THREADS >= LWT_MAX_TRACKS && 4 * LWT_THREADS >= LWT_MAX_DETS, "four waves, four elements per thread");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    __syncthreads();   // a is complete; wtot is free
    int v[4], s = 0;
    for (int k = 0; k < 4; ++k) {
        const int idx = 4 * tid + k;
        v[k] = idx < n ? a[idx] : 0;
        s += v[k];
    }
    int inc = s;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(inc, o);
        if (lane >= o) inc += u;
    }
    if (lane == 63) wtot[wave] = inc;
    __syncthreads();
    int base = inc - s;
    for (int w = 0; w < wave; ++w) base += wtot[w];
    const int total = ((wtot[0] + wtot[1]) + wtot[2]) + wtot[3];
    for (int k = 0; k < 4; ++k) {
        const int idx = 4 * tid + k;
        if (idx < n) a[idx] = base;
        base += v[k];
    }
    __syncthreads();
    return total;
}

// the row's maximum over the columns still free, and its lowest column (a taken column counts as the zero the reference writes there)
__device__ __forceinline__ Best row_best(const double* row, int N, const int* det_row, int lane) {
    Best b{0.0, 0};
    for (int d = lane; d < N; d += 64) {
        if (det_row[d] >= 0) continue;
        const double v = row[d];
        if (v > b.v) { b.v = v; b.i = d; }
    }
    return wave_best(b);
}

__global__ __launch_bounds__(LWT_THREADS) void lwt_update_kernel(const LwtUpdateParams p) {
    __shared__ double rowmax[LWT_MAX_TRACKS];
    __shared__ int rowarg[LWT_MAX_TRACKS];
    __shared__ int row_det[LWT_MAX_TRACKS];   // the detection a track was matched to, -1: none
    __shared__ int det_row[LWT_MAX_DETS];     // the track a detection was matched to, -1: none
    __shared__ int keep[LWT_MAX_TRACKS];      // 1: the track survives this call; then its position in the other bank
    __shared__ int fresh[LWT_MAX_DETS];       // 1: the detection starts a track; then its rank among those
    __shared__ double wv[LWT_THREADS / 64];
    __shared__ int wi[LWT_THREADS / 64];
    __shared__ int wtot[LWT_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (p.stop && *p.stop) return;   // (every thread, before the first barrier: a frame of the sequence call before this one was refused)
    int N = p.N;
    if (p.count) {   // the detection count lives on the device (the fused detect call); p.N is the bound the buffers were sized for
        const int n = __builtin_amdgcn_readfirstlane(*p.count);   // (a scalar, like p.N: every loop bound below stays wave-uniform)
        N = n < 0 ? 0 : (n > N ? N : n);
    }
    int T = p.head[LWT_HEAD_TRACKS];
    T = T < 0 ? 0 : (T > p.max_tracks ? p.max_tracks : T);
    const int next_id = p.head[LWT_HEAD_NEXT_ID], old_points = p.head[LWT_HEAD_POINTS];
    for (int r = tid; r < T; r += LWT_THREADS) row_det[r] = -1;
    for (int d = tid; d < N; d += LWT_THREADS) det_row[d] = -1;
    // ---- (a) the IoU matrix, one wave per row
    for (int r = wave; r < T; r += LWT_THREADS / 64) {   // (wave-uniform: no divergence around the butterfly)
        Best b{0.0, 0};
        for (int d = lane; d < N; d += 64) {
            const double v = iou_xywh(p.src.bbox + 4 * r, p.dets + 4 * d);
            p.iou[(size_t)r * N + d] = v;
            if (v > b.v) { b.v = v; b.i = d; }
        }
        b = wave_best(b);
        if (lane == 0) { rowmax[r] = b.v; rowarg[r] = b.i; }
    }
    __syncthreads();
    // ---- (b) greedy matching
    int matched = 0;
    const int most = T < N ? T : N;
    while (matched < most) {
        Best b{-1.0, 0x7fffffff};
        for (int r = tid; r < T; r += LWT_THREADS)
            if (row_det[r] < 0 && beats(rowmax[r], r * N + rowarg[r], b)) { b.v = rowmax[r]; b.i = r * N + rowarg[r]; }
        b = wave_best(b);
        if (lane == 0) { wv[wave] = b.v; wi[wave] = b.i; }
        __syncthreads();
        b = Best{wv[0], wi[0]};
        for (int w = 1; w < LWT_THREADS / 64; ++w)
            if (beats(wv[w], wi[w], b)) { b.v = wv[w]; b.i = wi[w]; }
        if (b.v < p.thr) break;   // (the same pair in every thread)
        const int t = b.i / N, d = b.i - t * N;
        if (tid == 0) { row_det[t] = d; det_row[d] = t; }
        __syncthreads();   // the match is visible; wv and wi have been read
        for (int r = wave; r < T; r += LWT_THREADS / 64) {
            if (row_det[r] >= 0 || rowarg[r] != d) continue;
            const Best c = row_best(p.iou + (size_t)r * N, N, det_row, lane);
            if (lane == 0) { rowmax[r] = c.v; rowarg[r] = c.i; }
        }
        ++matched;
        __syncthreads();
    }
    // ---- (c) room for the new tracks?  Nothing has been written so far.
    const int n_new = N - matched;
    if (T + n_new > p.max_tracks) {
        if (tid == 0) {
            p.result[LWT_HEAD_TRACKS] = T;
            p.result[LWT_HEAD_NEXT_ID] = next_id;
            p.result[LWT_HEAD_POINTS] = old_points;
            p.result[LWT_HEAD_ERROR] = 1;
            if (p.stop) *p.stop = 1;   // sticky: every launch the sequence call has enqueued behind this one leaves at once
        }
        return;
    }
    // ---- (d) who stays and where
    for (int r = tid; r < T; r += LWT_THREADS)
        keep[r] = row_det[r] >= 0 || p.src.meta[LWT_META * r + LWT_TSU] + 1 <= p.max_age;
    for (int d = tid; d < N; d += LWT_THREADS) fresh[d] = det_row[d] < 0;
    const int kept = block_exclusive_scan(keep, T, wtot);
    block_exclusive_scan(fresh, N, wtot);
    // ---- (e) the tracks
    for (int r = tid; r < T; r += LWT_THREADS) {
        const int32_t* m = p.src.meta + LWT_META * r;
        const int d = row_det[r];
        if (d < 0 && m[LWT_TSU] + 1 > p.max_age) continue;
        const int q = keep[r];
        Kf k;
        kf_load(k, p.src, r);
        kf_predict(k);
        int32_t* o = p.dst.meta + LWT_META * q;
        o[LWT_ID] = m[LWT_ID];
        o[LWT_AGE] = m[LWT_AGE] + 1;
        if (d >= 0) {
            const float* box = p.dets + 4 * d;
            const double cx = (double)box[0] + (double)box[2] / 2.0, cy = (double)box[1] + (double)box[3] / 2.0;
            kf_update(k, cx, cy, false);
            for (int j = 0; j < 4; ++j) p.dst.bbox[4 * q + j] = box[j];
            p.dst.center[2 * q] = cx;
            p.dst.center[2 * q + 1] = cy;
            o[LWT_HITS] = m[LWT_HITS] + 1;
            o[LWT_TSU] = 0;
        } else {
            for (int j = 0; j < 4; ++j) p.dst.bbox[4 * q + j] = p.src.bbox[4 * r + j];
            p.dst.center[2 * q] = p.src.center[2 * r];
            p.dst.center[2 * q + 1] = p.src.center[2 * r + 1];
            o[LWT_HITS] = m[LWT_HITS];
            o[LWT_TSU] = m[LWT_TSU] + 1;
        }
        kf_store(k, p.dst, q);
    }
    // ---- (e) new tracks, (f) ids and flow points, in detection order
    for (int d = tid; d < N; d += LWT_THREADS) {
        const float* box = p.dets + 4 * d;
        const double cx = (double)box[0] + (double)box[2] / 2.0, cy = (double)box[1] + (double)box[3] / 2.0;
        int id, q;
        if (det_row[d] >= 0) {
            id = p.src.meta[LWT_META * det_row[d] + LWT_ID];
            q = keep[det_row[d]];
        } else {
            id = next_id + fresh[d];
            q = kept + fresh[d];
            Kf k;
            k.x[0] = (float)cx; k.x[1] = (float)cy; k.x[2] = 0.0; k.x[3] = 0.0;
            for (int j = 0; j < 16; ++j) k.P[j] = 0.f;
            k.P[0] = 100.f; k.P[5] = 100.f; k.P[10] = 1000.f; k.P[15] = 1000.f;
            k.f32 = 1;
            int32_t* o = p.dst.meta + LWT_META * q;
            o[LWT_ID] = id; o[LWT_AGE] = 0; o[LWT_HITS] = 1; o[LWT_TSU] = 0;
            for (int j = 0; j < 4; ++j) p.dst.bbox[4 * q + j] = box[j];
            p.dst.center[2 * q] = cx;
            p.dst.center[2 * q + 1] = cy;
            kf_store(k, p.dst, q);
        }
        p.result[LWT_HEAD + d] = id;
        if (p.use_flow) {
            p.pts.xy[2 * d] = (float)cx;
            p.pts.xy[2 * d + 1] = (float)cy;
            p.pts.id[d] = id;
            p.pts.pos[d] = q;
        }
    }
    if (tid == 0) {   // (every thread read the head before the first barrier)
        const int head[LWT_HEAD] = {kept + n_new, next_id + n_new, p.use_flow ? N : 0, 0};
        for (int j = 0; j < LWT_HEAD; ++j) { p.head[j] = head[j]; p.result[j] = head[j]; }
    }
}

__global__ __launch_bounds__(LWT_THREADS) void lwt_interp_kernel(const LwtInterpParams p) {
    __shared__ int pt_of[LWT_MAX_TRACKS];   // the followed point of a track, -1: none
    __shared__ int flag[LWT_MAX_DETS];
    __shared__ int wtot[LWT_THREADS / 64];
    const int tid = threadIdx.x;
    if (p.stop && *p.stop) return;
    int T = p.head[LWT_HEAD_TRACKS], np = p.next ? p.head[LWT_HEAD_POINTS] : 0;
    T = T < 0 ? 0 : (T > LWT_MAX_TRACKS ? LWT_MAX_TRACKS : T);
    np = np < 0 ? 0 : (np > LWT_MAX_DETS ? LWT_MAX_DETS : np);
    const int next_id = p.head[LWT_HEAD_NEXT_ID];
    for (int r = tid; r < T; r += LWT_THREADS) pt_of[r] = -1;
    __syncthreads();
    for (int j = tid; j < np; j += LWT_THREADS) {
        const int pos = p.pts.pos[j];
        if (p.status[j] == 1 && (unsigned)pos < (unsigned)T && p.s.meta[LWT_META * pos + LWT_ID] == p.pts.id[j]) pt_of[pos] = j;
    }
    __syncthreads();
    for (int r = tid; r < T; r += LWT_THREADS) {
        int32_t* m = p.s.meta + LWT_META * r;
        const int j = pt_of[r];
        const float w = p.s.bbox[4 * r + 2], h = p.s.bbox[4 * r + 3];
        const double hw = (double)w / 2.0, hh = (double)h / 2.0;
        Kf k;
        kf_load(k, p.s, r);
        LwtRec rec;
        rec.id = m[LWT_ID];
        rec.reserved = 0;
        rec.bbox[2] = w;
        rec.bbox[3] = h;
        if (j >= 0) {
            const float cx = p.next[2 * j], cy = p.next[2 * j + 1];
            const float bx = cx - (float)hw, by = cy - (float)hh;   // a float32 scalar minus a Python float: float32
            kf_update(k, cx, cy, true);
            p.s.bbox[4 * r] = bx;
            p.s.bbox[4 * r + 1] = by;
            p.s.center[2 * r] = cx;
            p.s.center[2 * r + 1] = cy;
            m[LWT_HITS] = m[LWT_HITS] + 1;
            m[LWT_TSU] = 0;
            rec.bbox[0] = bx;
            rec.bbox[1] = by;
        } else {
            kf_predict(k);
            m[LWT_AGE] = m[LWT_AGE] + 1;
            m[LWT_TSU] = m[LWT_TSU] + 1;
            if (k.f32) {
                const float bx = (float)k.x[0] - (float)hw, by = (float)k.x[1] - (float)hh;
                rec.bbox[0] = bx;
                rec.bbox[1] = by;
            } else {
                rec.bbox[0] = k.x[0] - hw;
                rec.bbox[1] = k.x[1] - hh;
            }
        }
        kf_store(k, p.s, r);
        p.recs[r] = rec;
    }
    // ---- the followed points stay, in order.  Thread i moves points 4 i .. 4 i + 3: read before the scan's barriers, written after them.
    float nx[4], ny[4];
    int id[4], pos[4], st[4];
    for (int k = 0; k < 4; ++k) {
        const int j = 4 * tid + k;
        st[k] = j < np && p.status[j] == 1;
        if (st[k]) { nx[k] = p.next[2 * j]; ny[k] = p.next[2 * j + 1]; id[k] = p.pts.id[j]; pos[k] = p.pts.pos[j]; }
        if (j < np) flag[j] = st[k];
    }
    const int left = block_exclusive_scan(flag, np, wtot);
    for (int k = 0; k < 4; ++k) {
        const int j = 4 * tid + k;
        if (!st[k]) continue;
        const int q = flag[j];
        p.pts.xy[2 * q] = nx[k];
        p.pts.xy[2 * q + 1] = ny[k];
        p.pts.id[q] = id[k];
        p.pts.pos[q] = pos[k];
    }
    if (tid == 0) {
        const int head[LWT_HEAD] = {T, next_id, left, 0};
        for (int j = 0; j < LWT_HEAD; ++j) { p.head[j] = head[j]; p.result[j] = head[j]; }
    }
}

__global__ __launch_bounds__(64) void lwt_ingest_kernel(const LwtIngestParams p) {
    if (p.stop && *p.stop) return;
    const int n = opd::record_count(p.view, 0);   // (clamped to the stride, whatever lies there)
    if (threadIdx.x == 0) *p.n_out = n;
    for (int i = threadIdx.x; i < n; i += 64) {
        double box[4];
        opd::record_box64(p.view, i, box);
        for (int k = 0; k < 4; ++k) p.boxes[4 * i + k] = (float)box[k];
    }
}

}  // namespace

hipError_t opd_launch_lwt_ingest(const LwtIngestParams& p, hipStream_t stream) {
    const opd::RecordView& v = p.view;
    if (v.stride < 1 || v.stride > LWT_MAX_DETS || (v.records != nullptr) == (v.merged != nullptr) || !v.counts || !p.boxes || !p.n_out) return hipErrorInvalidValue;
    OPD_LAUNCH(lwt_ingest_kernel, dim3(1), dim3(64), 0, stream, p);
    return hipGetLastError();
}

hipError_t opd_launch_lwt_update(const LwtUpdateParams& p, hipStream_t stream) {
    if (p.N < 0 || p.N > LWT_MAX_DETS || p.max_tracks < 1 || p.max_tracks > LWT_MAX_TRACKS) return hipErrorInvalidValue;
    OPD_LAUNCH(lwt_update_kernel, dim3(1), dim3(LWT_THREADS), 0, stream, p);
    return hipGetLastError();
}

hipError_t opd_launch_lwt_interp(const LwtInterpParams& p, hipStream_t stream) {
    OPD_LAUNCH(lwt_interp_kernel, dim3(1), dim3(LWT_THREADS), 0, stream, p);
    return hipGetLastError();
}
