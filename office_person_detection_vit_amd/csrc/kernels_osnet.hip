// kernels_osnet.hip — the OSNet tower of the Re-ID path (opd_osnet.cpp), gfx950, fp16 activations and operands, fp32 accumulation, NHWC.
//
//   osnet_preprocess_kernel   crop + BGR->RGB + Pillow-exact bilinear resize to 256 x 128 + ToTensor / Normalize table -> [256][128][4]
//   osnet_stem_kernel         7x7 stride-2 convolution 3 -> C0 (<= 64) with folded BN and ReLU, direct, weights in LDS
//   osnet_maxpool_kernel      3x3 stride-2 max-pool, padding 1
//   osnet_gemm_kernel<EPI>    every 1x1 convolution: grouped, optional second K segment, epilogue none / bias+ReLU / bias+identity+ReLU
//   osnet_dwconv_kernel       depthwise 3x3 (padding 1) with folded BN and ReLU over a channel range
//   osnet_gate_kernel         the shared ChannelGate of an OSBlock for its four streams: pooled means -> fc1 -> ReLU -> fc2 -> sigmoid
//   osnet_combine_kernel      x2 = sum over streams of gate * stream, in stream order
//   osnet_avgpool2_kernel     2x2 average pool of a transition
//   osnet_head_kernel         global average pool -> fc (BN1d folded) -> ReLU -> L2 normalisation, fp32
//
// Every reduction (gate pools, global pool, L2 norm, GEMM K loop) runs in an order fixed by the shapes alone: no float atomics and no
// split depending on the crop count, so a crop's features do not depend on the other crops of the call.
//
// MFMA operand layout (as in kernels_reid.hip): v_mfma_f32_16x16x32_f16(A, B): lane (g = lane >> 4, li = lane & 15) feeds
// A[li][k0 + 8g .. 8g + 7] and B[li][k0 + 8g .. 8g + 7] and receives D[4g + r][li], r = 0 .. 3, D[i][j] = sum_k A[i][k] B[j][k].
#include <hip/hip_runtime.h>
#include <math.h>

#include "opd_osnet.h"
#include "opd_kprims.h"

namespace {

// ---- pre-processing ---------------------------------------------------------------------------------------------------------------------
// grid (256 output rows, crops), block 128 (output columns): one output pixel per thread (opd_crop.h), stored through the normalisation
// table as four halves.
__global__ __launch_bounds__(128) void osnet_preprocess_kernel(const opd::ReidCrop* __restrict__ crops, const unsigned char* __restrict__ base,
                                                               const _Float16* __restrict__ lut, _Float16* __restrict__ img) {
    const opd::ReidCrop c = crops[blockIdx.y];
    const int yo = blockIdx.x, xo = threadIdx.x;
    const opd::CropRgb rgb = opd::crop_resample_pixel(c, base, xo, yo, opd::OSNET_W, opd::OSNET_H);
    half4 o;
    o[0] = lut[rgb.c[0]];
    o[1] = lut[256 + rgb.c[1]];
    o[2] = lut[512 + rgb.c[2]];
    o[3] = (_Float16)0.f;
    *reinterpret_cast<half4*>(img + (((size_t)blockIdx.y * opd::OSNET_H + yo) * opd::OSNET_W + xo) * 4) = o;
}

// ---- stem -----------------------------------------------------------------------------------------------------------------------------
// One thread per output pixel of [128][64], all 64 (padded) output channels in registers; weights [147][64] fp32 in LDS, read as broadcasts.
constexpr int STEM_OH = opd::OSNET_H / 2, STEM_OW = opd::OSNET_W / 2;

__global__ __launch_bounds__(256) void osnet_stem_kernel(const _Float16* __restrict__ img, const _Float16* __restrict__ w,
                                                         const float* __restrict__ bias, _Float16* __restrict__ out, int C0) {
    __shared__ float4v ws[147 * 16];
    for (int i = threadIdx.x; i < 147 * 16; i += 256) {
        const half4 h = *reinterpret_cast<const half4*>(w + 4 * i);
        ws[i] = float4v{(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
    }
    __syncthreads();
    const int p = blockIdx.x * 256 + threadIdx.x;   // < STEM_OH * STEM_OW (grid is exact)
    const int oy = p / STEM_OW, ox = p % STEM_OW;
    const _Float16* src = img + (size_t)blockIdx.y * opd::OSNET_H * opd::OSNET_W * 4;
    float4v acc[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = float4v{0.f, 0.f, 0.f, 0.f};
    for (int ky = 0; ky < 7; ++ky) {
        const int iy = 2 * oy - 3 + ky;
        if (iy < 0 || iy >= opd::OSNET_H) continue;
        for (int kx = 0; kx < 7; ++kx) {
            const int ix = 2 * ox - 3 + kx;
            if (ix < 0 || ix >= opd::OSNET_W) continue;
            const half4 v = *reinterpret_cast<const half4*>(src + ((size_t)iy * opd::OSNET_W + ix) * 4);
            const float4v* wt = ws + (ky * 7 + kx) * 3 * 16;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float x = (float)v[c];
#pragma unroll
                for (int j = 0; j < 16; ++j) acc[j] += x * wt[c * 16 + j];
            }
        }
    }
    _Float16* o = out + ((size_t)blockIdx.y * STEM_OH * STEM_OW + p) * C0;
#pragma unroll
    for (int j = 0; j < 16; ++j)
        if (4 * j < C0) {
            half4 h;
#pragma unroll
            for (int r = 0; r < 4; ++r) h[r] = (_Float16)fmaxf(acc[j][r] + bias[4 * j + r], 0.f);
            *reinterpret_cast<half4*>(o + 4 * j) = h;
        }
}

// ---- max-pool 3x3 stride 2 padding 1: [nb][H][W][C] -> [nb][H/2][W/2][C], one thread per (output pixel, 8 channels) ---------------------
__global__ __launch_bounds__(256) void osnet_maxpool_kernel(const _Float16* __restrict__ in, _Float16* __restrict__ out, int H, int W, int C,
                                                            int total) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int c8 = C / 8, OH = H / 2, OW = W / 2;
    const int cq = t % c8, pix = t / c8;
    const int ox = pix % OW, oy = (pix / OW) % OH, n = pix / (OW * OH);
    half8 m;
#pragma unroll
    for (int r = 0; r < 8; ++r) m[r] = (_Float16)-INFINITY;
    for (int ky = 0; ky < 3; ++ky) {
        const int iy = 2 * oy - 1 + ky;
        if (iy < 0 || iy >= H) continue;
        for (int kx = 0; kx < 3; ++kx) {
            const int ix = 2 * ox - 1 + kx;
            if (ix < 0 || ix >= W) continue;
            const half8 v = *reinterpret_cast<const half8*>(in + (((size_t)n * H + iy) * W + ix) * C + 8 * cq);
#pragma unroll
            for (int r = 0; r < 8; ++r) m[r] = v[r] > m[r] ? v[r] : m[r];
        }
    }
    *reinterpret_cast<half8*>(out + (size_t)pix * C + 8 * cq) = m;
}

// ---- 1x1 convolutions ------------------------------------------------------------------------------------------------------------------
// out[m][n] = epi(sum_k A[m][k] W[n][k]) with A = [a1 | a2] (two K segments, each a multiple of 8), group z = blockIdx.z shifting the A and
// output columns and the W / bias rows.  Workgroup tile 128 (M) x 32 (N): wave w owns rows 32w .. 32w + 31; fragments are read straight
// from global memory (L1 / L2 serve the reuse), K in steps of 32.
__device__ __forceinline__ half8 frag(const _Float16* row, int k, int K) {
    if (k < K) return *reinterpret_cast<const half8*>(row + k);
    half8 z;
#pragma unroll
    for (int r = 0; r < 8; ++r) z[r] = (_Float16)0.f;
    return z;
}

template <int EPI>
__global__ __launch_bounds__(256) void osnet_gemm_kernel(const opd::OsnetGemm p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane >> 4, li = lane & 15;
    const int z = blockIdx.z;
    const int m0 = blockIdx.x * 128 + wave * 32, n0 = blockIdx.y * 32;
    const int ldw = p.k1 + p.k2;
    const _Float16* W = static_cast<const _Float16*>(p.w) + (size_t)z * p.N * ldw;
    const bool j1 = n0 + 16 < p.N;   // the second 16-column tile exists (N is a multiple of 16)
    const _Float16* wr0 = W + (size_t)(n0 + li) * ldw;
    const _Float16* wr1 = W + (size_t)(j1 ? n0 + 16 + li : n0 + li) * ldw;
    const int r0 = min(m0 + li, p.M - 1), r1 = min(m0 + 16 + li, p.M - 1);   // rows beyond M: a valid row, not stored
    float4v acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = float4v{0.f, 0.f, 0.f, 0.f};
    {
        const _Float16* A = static_cast<const _Float16*>(p.a1) + (size_t)z * p.a_gcol;
        const _Float16* x0 = A + (size_t)r0 * p.lda1;
        const _Float16* x1 = A + (size_t)r1 * p.lda1;
        for (int k0 = 0; k0 < p.k1; k0 += 32) {
            const int k = k0 + 8 * g;
            const half8 a0 = frag(wr0, k, p.k1), a1 = frag(wr1, k, p.k1);
            const half8 b0 = frag(x0, k, p.k1), b1 = frag(x1, k, p.k1);
            acc[0][0] = mfma16(a0, b0, acc[0][0]);
            acc[0][1] = mfma16(a1, b0, acc[0][1]);
            acc[1][0] = mfma16(a0, b1, acc[1][0]);
            acc[1][1] = mfma16(a1, b1, acc[1][1]);
        }
    }
    if (p.k2 > 0) {
        const _Float16* A = static_cast<const _Float16*>(p.a2);
        const _Float16* x0 = A + (size_t)r0 * p.lda2;
        const _Float16* x1 = A + (size_t)r1 * p.lda2;
        for (int k0 = 0; k0 < p.k2; k0 += 32) {
            const int k = k0 + 8 * g;
            const half8 a0 = frag(wr0 + p.k1, k, p.k2), a1 = frag(wr1 + p.k1, k, p.k2);
            const half8 b0 = frag(x0, k, p.k2), b1 = frag(x1, k, p.k2);
            acc[0][0] = mfma16(a0, b0, acc[0][0]);
            acc[0][1] = mfma16(a1, b0, acc[0][1]);
            acc[1][0] = mfma16(a0, b1, acc[1][0]);
            acc[1][1] = mfma16(a1, b1, acc[1][1]);
        }
    }
    // lane holds out[m0 + 16i + li][n0 + 16j + 4g + r]
    _Float16* O = static_cast<_Float16*>(p.out) + (size_t)z * p.o_gcol;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int m = m0 + 16 * i + li;
        if (m >= p.M) continue;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (j == 1 && !j1) continue;
            const int n = n0 + 16 * j + 4 * g;
            float4v v = acc[i][j];
            if (EPI != OSNET_EPI_NONE) v += *reinterpret_cast<const float4v*>(p.bias + (size_t)z * p.N + n);
            if (EPI == OSNET_EPI_RESID_RELU) {
                const half4 id = *reinterpret_cast<const half4*>(static_cast<const _Float16*>(p.res) + (size_t)m * p.ldr + n);
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] += (float)id[r];
            }
            half4 h;
#pragma unroll
            for (int r = 0; r < 4; ++r) h[r] = (_Float16)(EPI == OSNET_EPI_NONE ? v[r] : fmaxf(v[r], 0.f));
            *reinterpret_cast<half4*>(O + (size_t)m * p.ldo + n) = h;
        }
    }
}

// ---- depthwise 3x3 + folded BN + ReLU over channels [c0, c0 + nc) of [nb][H][W][ld]; weights [9][ldw] and bias [ldw] indexed by channel,
// one thread per (pixel, 4 channels), taps in row-major order --------------------------------------------------------------------------
__global__ __launch_bounds__(256) void osnet_dwconv_kernel(const _Float16* __restrict__ in, _Float16* __restrict__ out, const float* __restrict__ w,
                                                           const float* __restrict__ bias, int H, int W, int ld, int c0, int nc, int ldw, int total) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int c4 = nc / 4;
    const int c = c0 + 4 * (t % c4), pix = t / c4;
    const int x = pix % W, y = (pix / W) % H, n = pix / (W * H);
    float4v acc = *reinterpret_cast<const float4v*>(bias + c);
    float4v s = float4v{0.f, 0.f, 0.f, 0.f};
    for (int ky = 0; ky < 3; ++ky) {
        const int iy = y - 1 + ky;
        if (iy < 0 || iy >= H) continue;
        for (int kx = 0; kx < 3; ++kx) {
            const int ix = x - 1 + kx;
            if (ix < 0 || ix >= W) continue;
            const half4 v = *reinterpret_cast<const half4*>(in + (((size_t)n * H + iy) * W + ix) * ld + c);
            const float4v wt = *reinterpret_cast<const float4v*>(w + (ky * 3 + kx) * ldw + c);
#pragma unroll
            for (int r = 0; r < 4; ++r) s[r] += (float)v[r] * wt[r];
        }
    }
    acc += s;
    half4 h;
#pragma unroll
    for (int r = 0; r < 4; ++r) h[r] = (_Float16)fmaxf(acc[r], 0.f);
    *reinterpret_cast<half4*>(out + (size_t)pix * ld + c) = h;
}

// ---- ChannelGate of the four streams: grid (crops, 4 streams), block 256.  Streams lie side by side in t [nb * HW][4 mid].  The pooled
// sum of a channel is split over `parts` fixed row ranges, each summed in row order, and the parts are added in order. --------------------
__global__ __launch_bounds__(256) void osnet_gate_kernel(const _Float16* __restrict__ t, const float* __restrict__ w1, const float* __restrict__ b1,
                                                         const float* __restrict__ w2, const float* __restrict__ b2, float* __restrict__ gates,
                                                         int HW, int mid, int hid) {
    __shared__ float part[256];
    __shared__ float pooled[256];
    __shared__ float hidden[64];
    const int n = blockIdx.x, s = blockIdx.y, tid = threadIdx.x;
    const int parts = 256 / mid;
    const int c = tid % mid, q = tid / mid;
    const int ld = 4 * mid;
    if (q < parts) {
        const int rows = (HW + parts - 1) / parts;
        const int p0 = q * rows, p1 = min(HW, p0 + rows);
        const _Float16* src = t + (size_t)n * HW * ld + s * mid + c;
        float acc = 0.f;
        for (int p = p0; p < p1; ++p) acc += (float)src[(size_t)p * ld];
        part[q * mid + c] = acc;
    }
    __syncthreads();
    if (tid < mid) {
        float acc = 0.f;
        for (int j = 0; j < parts; ++j) acc += part[j * mid + tid];
        pooled[tid] = acc / (float)HW;
    }
    __syncthreads();
    if (tid < hid) {
        float acc = b1[tid];
        for (int k = 0; k < mid; ++k) acc += w1[tid * mid + k] * pooled[k];
        hidden[tid] = fmaxf(acc, 0.f);
    }
    __syncthreads();
    if (tid < mid) {
        float acc = b2[tid];
        for (int k = 0; k < hid; ++k) acc += w2[tid * hid + k] * hidden[k];
        gates[((size_t)n * 4 + s) * mid + tid] = 1.0f / (1.0f + expf(-acc));
    }
}

// ---- x2[m][c] = sum_s gates[crop][s][c] * t[m][s mid + c], streams in order; one thread per (pixel, 4 channels) --------------------------
__global__ __launch_bounds__(256) void osnet_combine_kernel(const _Float16* __restrict__ t, const float* __restrict__ gates, _Float16* __restrict__ x2,
                                                            int HW, int mid, int total) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c4 = mid / 4;
    const int c = 4 * (i % c4), m = i / c4, n = m / HW;
    const _Float16* row = t + (size_t)m * 4 * mid + c;
    const float* gr = gates + (size_t)n * 4 * mid + c;
    float4v acc = float4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const half4 v = *reinterpret_cast<const half4*>(row + s * mid);
        const float4v gv = *reinterpret_cast<const float4v*>(gr + s * mid);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] += gv[r] * (float)v[r];
    }
    half4 h;
#pragma unroll
    for (int r = 0; r < 4; ++r) h[r] = (_Float16)acc[r];
    *reinterpret_cast<half4*>(x2 + (size_t)m * mid + c) = h;
}

// ---- 2x2 average pool: [nb][H][W][C] -> [nb][H/2][W/2][C], one thread per (output pixel, 4 channels) ------------------------------------
__global__ __launch_bounds__(256) void osnet_avgpool2_kernel(const _Float16* __restrict__ in, _Float16* __restrict__ out, int H, int W, int C,
                                                             int total) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int c4 = C / 4, OH = H / 2, OW = W / 2;
    const int c = 4 * (t % c4), pix = t / c4;
    const int ox = pix % OW, oy = (pix / OW) % OH, n = pix / (OW * OH);
    const _Float16* p00 = in + (((size_t)n * H + 2 * oy) * W + 2 * ox) * C + c;
    const half4 a = *reinterpret_cast<const half4*>(p00), b = *reinterpret_cast<const half4*>(p00 + C);
    const half4 d = *reinterpret_cast<const half4*>(p00 + (size_t)W * C), e = *reinterpret_cast<const half4*>(p00 + (size_t)W * C + C);
    half4 h;
#pragma unroll
    for (int r = 0; r < 4; ++r) h[r] = (_Float16)((((float)a[r] + (float)b[r]) + (float)d[r] + (float)e[r]) * 0.25f);
    *reinterpret_cast<half4*>(out + (size_t)pix * C + c) = h;
}

// ---- head: one workgroup of 512 threads per crop.  Channel c's mean over the HW rows (row order), fc with BN1d folded (wt [C][512],
// k order), ReLU, then the L2 norm by a fixed tree over the 512 outputs. ---------------------------------------------------------------
__global__ __launch_bounds__(512) void osnet_head_kernel(const _Float16* __restrict__ x, const float* __restrict__ wt, const float* __restrict__ b,
                                                         float* __restrict__ feat, int HW, int C) {
    __shared__ float pooled[512];
    __shared__ float sq[512];
    const int n = blockIdx.x, e = threadIdx.x;
    if (e < C) {
        const _Float16* src = x + (size_t)n * HW * C + e;
        float acc = 0.f;
        for (int p = 0; p < HW; ++p) acc += (float)src[(size_t)p * C];
        pooled[e] = acc / (float)HW;
    }
    __syncthreads();
    float y = b[e];
    for (int k = 0; k < C; ++k) y += wt[(size_t)k * 512 + e] * pooled[k];
    y = fmaxf(y, 0.f);
    sq[e] = y * y;
    __syncthreads();
    for (int o = 256; o >= 1; o >>= 1) {
        if (e < o) sq[e] += sq[e + o];
        __syncthreads();
    }
    feat[(size_t)n * 512 + e] = y / sqrtf(sq[0]);
}

}  // namespace

namespace {
int blocks_for(int total) { return (total + 255) / 256; }
}  // namespace

hipError_t opd_launch_osnet_preprocess(const opd::ReidCrop* crops, const unsigned char* base, const f16_t* lut, f16_t* img, int ncrops,
                                       hipStream_t stream) {
    if (ncrops <= 0) return hipErrorInvalidValue;
    OPD_LAUNCH(osnet_preprocess_kernel, dim3(opd::OSNET_H, ncrops), dim3(opd::OSNET_W), 0, stream, crops, base,
               reinterpret_cast<const _Float16*>(lut), reinterpret_cast<_Float16*>(img));
    return hipGetLastError();
}

hipError_t opd_launch_osnet_stem(const f16_t* img, const f16_t* w, const float* bias, f16_t* out, int ncrops, int C0, hipStream_t stream) {
    if (ncrops <= 0 || C0 <= 0 || C0 > 64 || C0 % 8) return hipErrorInvalidValue;
    OPD_LAUNCH(osnet_stem_kernel, dim3(STEM_OH * STEM_OW / 256, ncrops), dim3(256), 0, stream, reinterpret_cast<const _Float16*>(img),
               reinterpret_cast<const _Float16*>(w), bias, reinterpret_cast<_Float16*>(out), C0);
    return hipGetLastError();
}

hipError_t opd_launch_osnet_maxpool(const f16_t* in, f16_t* out, int ncrops, int H, int W, int C, hipStream_t stream) {
    if (ncrops <= 0 || H % 2 || W % 2 || C % 8 || C <= 0) return hipErrorInvalidValue;
    const int total = ncrops * (H / 2) * (W / 2) * (C / 8);
    OPD_LAUNCH(osnet_maxpool_kernel, dim3(blocks_for(total)), dim3(256), 0, stream, reinterpret_cast<const _Float16*>(in),
               reinterpret_cast<_Float16*>(out), H, W, C, total);
    return hipGetLastError();
}

hipError_t opd_launch_osnet_gemm(int epi, const opd::OsnetGemm& p, int groups, hipStream_t stream) {
    if (p.M <= 0 || p.N <= 0 || p.N % 16 || p.k1 <= 0 || p.k1 % 8 || p.k2 < 0 || p.k2 % 8 || groups < 1 || !p.a1 || !p.w || !p.out) return hipErrorInvalidValue;
    if (p.lda1 % 8 || p.ldo % 4 || p.a_gcol % 8 || p.o_gcol % 4 || (p.k2 && (!p.a2 || p.lda2 % 8))) return hipErrorInvalidValue;
    if ((epi != OSNET_EPI_NONE && !p.bias) || (epi == OSNET_EPI_RESID_RELU && (!p.res || p.ldr % 4))) return hipErrorInvalidValue;
    const dim3 grid((p.M + 127) / 128, (p.N + 31) / 32, groups);
    switch (epi) {
        case OSNET_EPI_NONE: OPD_LAUNCH(osnet_gemm_kernel<OSNET_EPI_NONE>, grid, dim3(256), 0, stream, p); break;
        case OSNET_EPI_RELU: OPD_LAUNCH(osnet_gemm_kernel<OSNET_EPI_RELU>, grid, dim3(256), 0, stream, p); break;
        case OSNET_EPI_RESID_RELU: OPD_LAUNCH(osnet_gemm_kernel<OSNET_EPI_RESID_RELU>, grid, dim3(256), 0, stream, p); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t opd_launch_osnet_dwconv(const f16_t* in, f16_t* out, const float* w, const float* bias, int ncrops, int H, int W, int ld, int c0, int nc,
                                   int ldw, hipStream_t stream) {
    if (ncrops <= 0 || nc <= 0 || nc % 4 || c0 % 4 || ld % 4 || ldw % 4 || c0 + nc > ld || c0 + nc > ldw) return hipErrorInvalidValue;
    const int total = ncrops * H * W * (nc / 4);
    OPD_LAUNCH(osnet_dwconv_kernel, dim3(blocks_for(total)), dim3(256), 0, stream, reinterpret_cast<const _Float16*>(in),
               reinterpret_cast<_Float16*>(out), w, bias, H, W, ld, c0, nc, ldw, total);
    return hipGetLastError();
}

hipError_t opd_launch_osnet_gate(const f16_t* t, const float* w1, const float* b1, const float* w2, const float* b2, float* gates, int ncrops, int HW,
                                 int mid, int hid, hipStream_t stream) {
    if (ncrops <= 0 || HW <= 0 || mid <= 0 || mid > 256 || hid <= 0 || hid > 64) return hipErrorInvalidValue;
    OPD_LAUNCH(osnet_gate_kernel, dim3(ncrops, 4), dim3(256), 0, stream, reinterpret_cast<const _Float16*>(t), w1, b1, w2, b2, gates, HW, mid, hid);
    return hipGetLastError();
}

hipError_t opd_launch_osnet_combine(const f16_t* t, const float* gates, f16_t* x2, int ncrops, int HW, int mid, hipStream_t stream) {
    if (ncrops <= 0 || HW <= 0 || mid <= 0 || mid % 4) return hipErrorInvalidValue;
    const int total = ncrops * HW * (mid / 4);
    OPD_LAUNCH(osnet_combine_kernel, dim3(blocks_for(total)), dim3(256), 0, stream, reinterpret_cast<const _Float16*>(t), gates,
               reinterpret_cast<_Float16*>(x2), HW, mid, total);
    return hipGetLastError();
}

hipError_t opd_launch_osnet_avgpool2(const f16_t* in, f16_t* out, int ncrops, int H, int W, int C, hipStream_t stream) {
    if (ncrops <= 0 || H % 2 || W % 2 || C % 4 || C <= 0) return hipErrorInvalidValue;
    const int total = ncrops * (H / 2) * (W / 2) * (C / 4);
    OPD_LAUNCH(osnet_avgpool2_kernel, dim3(blocks_for(total)), dim3(256), 0, stream, reinterpret_cast<const _Float16*>(in),
               reinterpret_cast<_Float16*>(out), H, W, C, total);
    return hipGetLastError();
}

hipError_t opd_launch_osnet_head(const f16_t* x, const float* wt, const float* b, float* feat, int ncrops, int HW, int C, hipStream_t stream) {
    if (ncrops <= 0 || HW <= 0 || C <= 0 || C > 512) return hipErrorInvalidValue;
    OPD_LAUNCH(osnet_head_kernel, dim3(ncrops), dim3(512), 0, stream, reinterpret_cast<const _Float16*>(x), wt, b, feat, HW, C);
    return hipGetLastError();
}
