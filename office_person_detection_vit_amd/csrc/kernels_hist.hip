// kernels_hist.hip — colour-histogram appearance features (FeatureExtractor.extract_batch, src/tracking/feature_extractor.py:90-137) of
// crops read in place from BGR uint8 frames (opd_kernels.h: ColorParams).
//
//   color_hist_kernel    grid (crops, spans) x 256 threads.  A workgroup takes one span of a crop's rows.  A row is a byte stream that
//                        starts at any address (3 * x1 into a frame row), so it is cut into 12-byte groups on the 4-byte grid below the
//                        row start: a lane reads one group as three aligned dwords (four pixels when the group is full), and the first
//                        and last group of a row mask their bytes outside the row.  A dword is loaded only when it holds at least one
//                        byte of the row, so nothing outside the pages of the row is touched.  Groups of all rows of the span are dealt
//                        to the lanes in one flat index: a 40-pixel-wide crop keeps the lanes as busy as a 1920-pixel one.
//                        Each wave counts into its own LDS histogram [3][64] with LDS atomics; sum v and sum v^2 per channel stay in
//                        registers (64-bit) and are added across the wave by shuffles.  The workgroup then adds its non-zero bins and
//                        its six sums to the crop's accumulator with integer atomics: the result is the same for any grid.
//   color_finish_kernel  one wave per crop: counts -> fp32, mean = S / n and std = sqrt(n * Q - S^2) / n in fp64 (exact integers under
//                        the root: 0 for a uniform crop, as numpy gives), the 198 entries rounded to fp32 as the reference does, norm in
//                        fp64, one division and rounding per entry, zeros behind entry 197.
#include <hip/hip_runtime.h>

#include "../../include/opd_detr.h"
#include "opd_kprims.h"

namespace {

typedef unsigned long long u64;

// The crop with index `idx`: false = nothing to do for it (no record of the class in that slot, or a descriptor with row < 0)
__device__ __forceinline__ bool load_crop(const ColorParams& p, int idx, ColorCrop* c) {
    if (p.crops) {
        *c = p.crops[idx];
        return c->row >= 0;
    }
    const int b = idx / p.view.stride, i = idx - b * p.view.stride;
    if (i >= opd::record_count(p.view, b)) return false;
    if (!p.any_label && opd::record_label(p.view, idx) != p.label) return false;
    double box[4];   // the box as it travels to opd_color_features: float32
    opd::record_box64(p.view, idx, box);
    int x1, y1, x2, y2;
    const bool ok = opd_color_rect((double)(float)box[0], (double)(float)box[1], (double)(float)box[2], (double)(float)box[3], p.fh, p.fw, &x1, &y1, &x2, &y2);
    c->row = b * p.view.stride + opd::record_key(p.view, idx);
    c->pitch = 3 * p.fw;
    c->w = ok ? x2 - x1 : 0;
    c->h = ok ? y2 - y1 : 0;
    c->src = ok ? p.frames + ((size_t)b * p.fh * p.fw + (size_t)y1 * p.fw + x1) * 3 : p.frames;
    return true;
}

// the sum that belongs to channel `ch` when slot s (byte position mod 3 inside a group) carries channel (s - rot) mod 3
__device__ __forceinline__ unsigned pick(const unsigned (&s)[3], int ch, int rot) {
    const int slot = ch + rot >= 3 ? ch + rot - 3 : ch + rot;
    return slot == 0 ? s[0] : (slot == 1 ? s[1] : s[2]);
}

__global__ __launch_bounds__(256) void color_hist_kernel(const ColorParams p) {
    __shared__ unsigned hist[4][192];
    ColorCrop c;
    if (!load_crop(p, blockIdx.x, &c)) return;   // (uniform over the workgroup)
    if (c.w <= 0 || c.h <= 0) return;            // dummy crop: the finish kernel knows its counts
    const int rps = (c.h + (int)gridDim.y - 1) / (int)gridDim.y;
    const int r0 = (int)blockIdx.y * rps, r1 = min(c.h, r0 + rps);
    if (r0 >= r1) return;
    const int t = threadIdx.x;
    for (int k = t; k < 4 * 192; k += 256) (&hist[0][0])[k] = 0u;
    __syncthreads();
    unsigned* const wh = hist[t >> 6];
    const int rowb = 3 * c.w;
    const int gpr = (rowb + 3 + 11) / 12;   // groups that can hold bytes of a row starting up to 3 bytes into its first dword
    const int items = (r1 - r0) * gpr;
    u64 S[3] = {0, 0, 0}, Q[3] = {0, 0, 0};
    for (int it = t; it < items; it += 256) {
        const int r = it / gpr, g = it - r * gpr;
        const uint8_t* rowp = c.src + (size_t)(r0 + r) * c.pitch;
        const int k = (int)(reinterpret_cast<uintptr_t>(rowp) & 3);
        const int lo = max(12 * g, k) - 12 * g, hi = min(12 * g + 12, k + rowb) - 12 * g;   // the row's bytes inside this group
        if (lo >= hi) continue;
        const unsigned* ap = reinterpret_cast<const unsigned*>(rowp - k) + 3 * g;
        const int rot = k == 3 ? 0 : k;          // byte j of a group carries channel (j - k) mod 3
        unsigned* hb[3];                          // histogram of the channel in slot 0, 1, 2
#pragma unroll
        for (int s = 0; s < 3; ++s) hb[s] = wh + 64 * (s - rot < 0 ? s - rot + 3 : s - rot);
        unsigned s1[3] = {0, 0, 0}, s2[3] = {0, 0, 0};
        if (lo == 0 && hi == 12) {
            const unsigned d[3] = {ap[0], ap[1], ap[2]};
#pragma unroll
            for (int j = 0; j < 12; ++j) {
                const unsigned v = (d[j >> 2] >> (8 * (j & 3))) & 255u;
                atomicAdd(hb[j % 3] + (v >> 2), 1u);
                s1[j % 3] += v;
                s2[j % 3] += v * v;
            }
        } else {
            unsigned d[3];
#pragma unroll
            for (int q = 0; q < 3; ++q) d[q] = (4 * q < hi && 4 * q + 4 > lo) ? ap[q] : 0u;   // only dwords that hold a byte of the row
#pragma unroll
            for (int j = 0; j < 12; ++j) {
                if (j < lo || j >= hi) continue;
                const unsigned v = (d[j >> 2] >> (8 * (j & 3))) & 255u;
                atomicAdd(hb[j % 3] + (v >> 2), 1u);
                s1[j % 3] += v;
                s2[j % 3] += v * v;
            }
        }
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            S[ch] += pick(s1, ch, rot);
            Q[ch] += pick(s2, ch, rot);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            S[ch] += __shfl_xor(S[ch], o);
            Q[ch] += __shfl_xor(Q[ch], o);
        }
    unsigned* acc = p.acc + (size_t)blockIdx.x * OPD_COLOR_ACC_WORDS;
    u64* acc64 = reinterpret_cast<u64*>(acc + 192);
    if ((t & 63) == 0) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            atomicAdd(acc64 + ch, S[ch]);
            atomicAdd(acc64 + 3 + ch, Q[ch]);
        }
    }
    __syncthreads();
    if (t < 192) {
        const unsigned n = hist[0][t] + hist[1][t] + hist[2][t] + hist[3][t];
        if (n) atomicAdd(acc + t, n);
    }
}

__global__ __launch_bounds__(64) void color_finish_kernel(const ColorParams p) {
    ColorCrop c;
    if (!load_crop(p, blockIdx.x, &c)) return;
    const unsigned* acc = p.acc + (size_t)blockIdx.x * OPD_COLOR_ACC_WORDS;
    const u64* acc64 = reinterpret_cast<const u64*>(acc + 192);
    const int l = threadIdx.x;
    const bool dummy = c.w <= 0 || c.h <= 0;   // np.zeros((64, 32, 3)): 2048 pixels in bin 0 of every channel, mean = std = 0
    const u64 n = dummy ? 2048ull : (u64)c.w * (u64)c.h;
    float v[4];
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = (float)(dummy ? (l == 0 ? 2048u : 0u) : acc[l + 64 * k]);
    v[3] = 0.f;
    if (l < 6 && !dummy) {
        const u64 s = acc64[l >> 1], q = acc64[3 + (l >> 1)];
        const double stat = (l & 1) ? sqrt((double)(n * q - s * s)) / (double)n : (double)s / (double)n;
        v[3] = (float)stat;
    }
    double ss = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) ss += (double)v[k] * (double)v[k];
    const double den = sqrt(wave_sum(ss)) + 1e-8;
    float* out = p.out + (size_t)c.row * OPD_COLOR_DIM;
#pragma unroll
    for (int k = 0; k < 4; ++k) out[l + 64 * k] = (float)((double)v[k] / den);   // (entries 198 .. 255: 0 / den)
}

}  // namespace

hipError_t opd_launch_color_features(const ColorParams& p, int spans, hipStream_t stream) {
    if (p.n <= 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(p.acc, 0, (size_t)p.n * OPD_COLOR_ACC_WORDS * 4, stream);
    if (e != hipSuccess) return e;
    OPD_LAUNCH(color_hist_kernel, dim3(p.n, spans < 1 ? 1 : spans), dim3(256), 0, stream, p);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    OPD_LAUNCH(color_finish_kernel, dim3(p.n), dim3(64), 0, stream, p);
    return hipGetLastError();
}
