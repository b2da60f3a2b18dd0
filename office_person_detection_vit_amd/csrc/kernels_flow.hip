// kernels_flow.hip — pyramidal Lucas-Kanade flow of sparse points between two BGR uint8 frames (`OpticalFlowTracker.track`,
// src/tracking/lightweight_tracker.py:141-202: cv2.cvtColor + cv2.calcOpticalFlowPyrLK).  The arithmetic is OpenCV's with the window
// interpolation and the sums in float32 instead of 14-bit fixed point ("Optical flow"); gray and pyramid are exact integers.
//
//   flow_gray_kernel     256 threads = 64 groups of 4 pixels x 4 rows.  g = (1868 B + 9617 G + 4899 R + 8192) >> 14.  Four pixels are
//                        three dwords when the row's bytes start on a dword (always, for an aligned frame whose width is a multiple of
//                        4) and twelve byte loads otherwise; one dword store into the pitched level 0.
//   flow_pyrdown_kernel  256 threads = 64 groups of 4 output pixels x 4 output rows.  (sum k_i k_j src + 128) >> 8 with k = 1 4 6 4 1
//                        and reflect-101 indices.  Four outputs read columns 8t - 2 .. 8t + 8 of five rows: four dwords per row where
//                        they lie inside the row, reflected byte loads at the left and right edge; one dword store.
//   flow_lk_kernel       one wave per point, all levels in one launch.  Per level the wave stages the (win + 3)^2 reference pixels around
//                        the window in LDS (reflect-101), derives Scharr x / y at the (win + 1)^2 integer positions (zero outside the
//                        level), and every lane keeps the bilinear I, Sx, Sy of its <= 7 window samples in registers.  An iteration
//                        reads the new frame's level through the cache (4 bytes per sample), and adds the two mismatch sums over the
//                        wave by an xor butterfly: every lane holds the same bits, so all decisions are wave-uniform, and a point's
//                        result depends on nothing but its own coordinates and the two pyramids.  With FlowParams::count the launch
//                        is sized for an upper bound and the device-resident count decides which waves have a point.
//   All three take a nullable `stop` word (a sequence call's: set by a refused frame, it makes every launch behind it leave at once).
#include <float.h>
#include <hip/hip_runtime.h>

#include "opd_flow.h"
#include "opd_kprims.h"

namespace {

// index i of an n-long axis under reflect-101, any distance outside
__device__ __forceinline__ int reflect101(int i, int n) {
    if ((unsigned)i < (unsigned)n) return i;
    if (n == 1) return 0;
    const int p = 2 * n - 2;
    i %= p;
    if (i < 0) i += p;
    return i >= n ? p - i : i;
}

__device__ __forceinline__ unsigned gray_of(unsigned b, unsigned g, unsigned r) { return (1868u * b + 9617u * g + 4899u * r + 8192u) >> 14; }

// `stop` (nullable, here and in the two kernels below): a device word that a sequence call raises when a frame of its is refused; the
// launches of the frames behind it, already enqueued, find it set and leave at once, before any barrier and any store.
__global__ __launch_bounds__(256) void flow_gray_kernel(const uint8_t* __restrict__ bgr, uint8_t* __restrict__ gray, int h, int w, int pitch,
                                                        const int32_t* __restrict__ stop) {
    if (stop && *stop) return;
    const int x = 4 * (int)(blockIdx.x * 64 + threadIdx.x), y = blockIdx.y * 4 + threadIdx.y;
    if (x >= w || y >= h) return;
    const uint8_t* src = bgr + ((size_t)y * w + x) * 3;
    unsigned out;
    if (x + 4 <= w && (reinterpret_cast<uintptr_t>(src) & 3) == 0) {
        const unsigned* s = reinterpret_cast<const unsigned*>(src);
        const unsigned d0 = s[0], d1 = s[1], d2 = s[2];   // B0 G0 R0 B1 | G1 R1 B2 G2 | R2 B3 G3 R3
        out = gray_of(d0 & 255u, (d0 >> 8) & 255u, (d0 >> 16) & 255u) | gray_of(d0 >> 24, d1 & 255u, (d1 >> 8) & 255u) << 8 |
              gray_of((d1 >> 16) & 255u, d1 >> 24, d2 & 255u) << 16 | gray_of((d2 >> 8) & 255u, (d2 >> 16) & 255u, d2 >> 24) << 24;
    } else {
        out = 0u;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (x + k < w) out |= gray_of(src[3 * k], src[3 * k + 1], src[3 * k + 2]) << (8 * k);
    }
    *reinterpret_cast<unsigned*>(gray + (size_t)y * pitch + x) = out;   // (x + 3 < pitch: the pitch is a multiple of 16)
}

__global__ __launch_bounds__(256) void flow_pyrdown_kernel(const uint8_t* __restrict__ src, int sh, int sw, int spitch, uint8_t* __restrict__ dst,
                                                           int oh, int ow, int dpitch, const int32_t* __restrict__ stop) {
    if (stop && *stop) return;
    const int t = blockIdx.x * 64 + threadIdx.x, oy = blockIdx.y * 4 + threadIdx.y;
    if (4 * t >= ow || oy >= oh) return;
    const int c0 = 8 * t - 2;                       // first source column of the group; it needs c0 .. c0 + 10
    const bool inside = c0 - 2 >= 0 && c0 + 14 <= sw;   // the four dwords at c0 - 2 hold columns of the row only
    unsigned acc[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const uint8_t* row = src + (size_t)reflect101(2 * oy + i - 2, sh) * spitch;
        unsigned v[11];
        if (inside) {
            const unsigned* s = reinterpret_cast<const unsigned*>(row + c0 - 2);   // (spitch and c0 - 2 are multiples of 4)
            const unsigned d[4] = {s[0], s[1], s[2], s[3]};
#pragma unroll
            for (int j = 0; j < 11; ++j) v[j] = (d[(j + 2) >> 2] >> (8 * ((j + 2) & 3))) & 255u;
        } else {
#pragma unroll
            for (int j = 0; j < 11; ++j) v[j] = row[reflect101(c0 + j, sw)];
        }
        const unsigned ki = i == 0 || i == 4 ? 1u : (i == 2 ? 6u : 4u);
#pragma unroll
        for (int o = 0; o < 4; ++o) acc[o] += ki * (v[2 * o] + 4u * v[2 * o + 1] + 6u * v[2 * o + 2] + 4u * v[2 * o + 3] + v[2 * o + 4]);
    }
    unsigned out = 0u;
#pragma unroll
    for (int o = 0; o < 4; ++o) out |= ((acc[o] + 128u) >> 8) << (8 * o);   // (columns >= ow of the last group: scratch behind the row)
    *reinterpret_cast<unsigned*>(dst + (size_t)oy * dpitch + 4 * t) = out;
}

enum { PATCH_LD = OPD_FLOW_MAX_WIN + 4, DERIV_LD = OPD_FLOW_MAX_WIN + 2, SAMPLES = (OPD_FLOW_MAX_WIN * OPD_FLOW_MAX_WIN + 63) / 64 };

__global__ __launch_bounds__(64) void flow_lk_kernel(const FlowParams p) {
    __shared__ float patch[(OPD_FLOW_MAX_WIN + 3) * PATCH_LD];   // reference pixels, rows / columns floor(q) - 1 .. floor(q) + win + 1
    __shared__ float dxs[(OPD_FLOW_MAX_WIN + 1) * DERIV_LD];     // Scharr x at floor(q) .. floor(q) + win
    __shared__ float dys[(OPD_FLOW_MAX_WIN + 1) * DERIV_LD];
    const int pt = blockIdx.x, lane = threadIdx.x;
    if (p.stop && *p.stop) return;
    if (p.count && pt >= *p.count) return;   // (the whole wave, before the first barrier: the launch was sized for a bound)
    const int win = p.win, nwin = win * win;
    const float half = (float)((win - 1) / 2), fwin = (float)win;
    const float px = p.pts[2 * pt], py = p.pts[2 * pt + 1];
    float cx = 0.f, cy = 0.f;   // the guess: window centre in the current level
    int status = 1;
    for (int l = p.top; l >= 0; --l) {
        const FlowLevel lv = p.lv[l];
        const float scale = 1.f / (float)(1 << l), fw = (float)lv.w, fh = (float)lv.h;
        const float qx = px * scale - half, qy = py * scale - half;
        if (l == p.top) { cx = qx + half; cy = qy + half; }
        else { cx *= 2.f; cy *= 2.f; }
        const float fqx = floorf(qx), fqy = floorf(qy);
        if (!(fqx >= -fwin && fqx < fw && fqy >= -fwin && fqy < fh)) {   // (also a NaN coordinate)
            if (l == 0) status = 0;
            continue;
        }
        const int iqx = (int)fqx, iqy = (int)fqy;
        __syncthreads();   // the previous level's LDS reads are done
        const int pw = win + 3;
        for (int k = lane; k < pw * pw; k += 64) {
            const int r = k / pw, c = k - r * pw;
            patch[r * PATCH_LD + c] = (float)lv.ref[(size_t)reflect101(iqy - 1 + r, lv.h) * lv.pitch + reflect101(iqx - 1 + c, lv.w)];
        }
        __syncthreads();
        const int dw = win + 1;
        for (int k = lane; k < dw * dw; k += 64) {
            const int r = k / dw, c = k - r * dw;
            const float* P = patch + (r + 1) * PATCH_LD + (c + 1);
            const bool in = (unsigned)(iqx + c) < (unsigned)lv.w && (unsigned)(iqy + r) < (unsigned)lv.h;
            const float sx = 3.f * (P[-PATCH_LD + 1] - P[-PATCH_LD - 1]) + 10.f * (P[1] - P[-1]) + 3.f * (P[PATCH_LD + 1] - P[PATCH_LD - 1]);
            const float sy = 3.f * (P[PATCH_LD - 1] - P[-PATCH_LD - 1]) + 10.f * (P[PATCH_LD] - P[-PATCH_LD]) + 3.f * (P[PATCH_LD + 1] - P[-PATCH_LD + 1]);
            dxs[r * DERIV_LD + c] = in ? sx : 0.f;   // (small integers: exact)
            dys[r * DERIV_LD + c] = in ? sy : 0.f;
        }
        __syncthreads();
        float Iw[SAMPLES], Sx[SAMPLES], Sy[SAMPLES];
        float a11 = 0.f, a12 = 0.f, a22 = 0.f;
        {
            const float a = qx - fqx, b = qy - fqy;
            const float w00 = (1.f - a) * (1.f - b), w01 = a * (1.f - b), w10 = (1.f - a) * b, w11 = a * b;
#pragma unroll
            for (int t = 0; t < SAMPLES; ++t) {
                const int k = lane + 64 * t;
                Iw[t] = Sx[t] = Sy[t] = 0.f;
                if (k < nwin) {
                    const int r = k / win, c = k - r * win;
                    const float* P = patch + (r + 1) * PATCH_LD + (c + 1);
                    const float* X = dxs + r * DERIV_LD + c;
                    const float* Y = dys + r * DERIV_LD + c;
                    Iw[t] = w00 * P[0] + w01 * P[1] + w10 * P[PATCH_LD] + w11 * P[PATCH_LD + 1];
                    Sx[t] = w00 * X[0] + w01 * X[1] + w10 * X[DERIV_LD] + w11 * X[DERIV_LD + 1];
                    Sy[t] = w00 * Y[0] + w01 * Y[1] + w10 * Y[DERIV_LD] + w11 * Y[DERIV_LD + 1];
                    a11 += Sx[t] * Sx[t];
                    a12 += Sx[t] * Sy[t];
                    a22 += Sy[t] * Sy[t];
                }
            }
        }
        const float flt_scale = 1.f / (float)(1 << 20);
        const float A11 = wave_sum(a11) * flt_scale, A12 = wave_sum(a12) * flt_scale, A22 = wave_sum(a22) * flt_scale;
        const float D = A11 * A22 - A12 * A12;
        const float min_eig = (A22 + A11 - sqrtf((A11 - A22) * (A11 - A22) + 4.f * A12 * A12)) / (float)(2 * nwin);
        if (min_eig < p.min_eig || D < FLT_EPSILON) {
            if (l == 0) status = 0;
            continue;
        }
        float nx = cx - half, ny = cy - half, pdx = 0.f, pdy = 0.f;
        for (int j = 0; j < p.max_iter; ++j) {
            const float fx = floorf(nx), fy = floorf(ny);
            if (!(fx >= -fwin && fx < fw && fy >= -fwin && fy < fh)) {
                if (l == 0) status = 0;
                break;
            }
            const int ix = (int)fx, iy = (int)fy;
            const float a = nx - fx, b = ny - fy;
            const float w00 = (1.f - a) * (1.f - b), w01 = a * (1.f - b), w10 = (1.f - a) * b, w11 = a * b;
            float b1 = 0.f, b2 = 0.f;
#pragma unroll
            for (int t = 0; t < SAMPLES; ++t) {
                const int k = lane + 64 * t;
                if (k < nwin) {
                    const int r = k / win, c = k - r * win;
                    const uint8_t* r0 = lv.cur + (size_t)reflect101(iy + r, lv.h) * lv.pitch;
                    const uint8_t* r1 = lv.cur + (size_t)reflect101(iy + r + 1, lv.h) * lv.pitch;
                    const int x0 = reflect101(ix + c, lv.w), x1 = reflect101(ix + c + 1, lv.w);
                    const float diff = (w00 * (float)r0[x0] + w01 * (float)r0[x1] + w10 * (float)r1[x0] + w11 * (float)r1[x1]) - Iw[t];
                    b1 += diff * Sx[t];
                    b2 += diff * Sy[t];
                }
            }
            b1 = wave_sum(b1) * (32.f * flt_scale);
            b2 = wave_sum(b2) * (32.f * flt_scale);
            const float dx = (A12 * b2 - A22 * b1) / D, dy = (A12 * b1 - A11 * b2) / D;
            nx += dx;
            ny += dy;
            if (dx * dx + dy * dy <= p.eps2) break;
            if (j > 0 && fabsf(dx + pdx) < 0.01f && fabsf(dy + pdy) < 0.01f) {
                nx -= dx * 0.5f;
                ny -= dy * 0.5f;
                break;
            }
            pdx = dx;
            pdy = dy;
        }
        cx = nx + half;
        cy = ny + half;
    }
    if (lane == 0) {
        p.next[2 * pt] = cx;
        p.next[2 * pt + 1] = cy;
        p.status[pt] = (uint8_t)status;
    }
}

}  // namespace

hipError_t opd_launch_flow_gray(const uint8_t* bgr, uint8_t* gray, int h, int w, int pitch, hipStream_t stream, const int32_t* stop) {
    OPD_LAUNCH(flow_gray_kernel, dim3(((w + 3) / 4 + 63) / 64, (h + 3) / 4), dim3(64, 4), 0, stream, bgr, gray, h, w, pitch, stop);
    return hipGetLastError();
}

hipError_t opd_launch_flow_pyrdown(const uint8_t* src, int sh, int sw, int spitch, uint8_t* dst, int dpitch, hipStream_t stream, const int32_t* stop) {
    const int oh = (sh + 1) / 2, ow = (sw + 1) / 2;
    OPD_LAUNCH(flow_pyrdown_kernel, dim3(((ow + 3) / 4 + 63) / 64, (oh + 3) / 4), dim3(64, 4), 0, stream, src, sh, sw, spitch, dst, oh, ow, dpitch, stop);
    return hipGetLastError();
}

hipError_t opd_launch_flow_lk(const FlowParams& p, hipStream_t stream) {
    if (p.n <= 0) return hipSuccess;
    OPD_LAUNCH(flow_lk_kernel, dim3(p.n), dim3(64), 0, stream, p);
    return hipGetLastError();
}
