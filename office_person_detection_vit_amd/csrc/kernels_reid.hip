// kernels_reid.hip — the CLIP ViT image tower of the Re-ID path (opd_clip.cpp), gfx950, fp16 operands with fp32 accumulation.
//
//   reid_preprocess_kernel   crop + BGR->RGB + Pillow-exact bicubic resize (centre 224 x 224 window only) + /255 + mean/std -> patch rows
//   reid_gemm_kernel<EPI>    every linear layer: 64 x 64 output tile per workgroup, K in steps of 64 through LDS, v_mfma_f32_16x16x32_f16
//   reid_layernorm_kernel    LayerNorm over the hidden size, fp32 statistics, one wave per row
//   reid_attention_kernel    softmax(q k^T) v of one (crop, head): T <= 64 tokens, head_dim 64, scores on chip
//   reid_l2norm_kernel       feature rows / their L2 norm
//
// No kernel splits a reduction across workgroups and none depends on the launch's row count for its arithmetic, so a crop's features
// are bit-identical whatever else is in the batch.
//
// MFMA operand layout (as in kernels_gemm.hip): v_mfma_f32_16x16x32_f16(A, B): lane (g = lane >> 4, li = lane & 15) feeds
// A[li][k0 + 8g .. 8g + 7] and B[li][k0 + 8g .. 8g + 7] (both operands row-major in k) and receives D[4g + r][li], r = 0 .. 3,
// D[i][j] = sum_k A[i][k] B[j][k].
#include <hip/hip_runtime.h>
#include <math.h>

#include "opd_clip.h"
#include "opd_kprims.h"

namespace {

// ---- pre-processing -------------------------------------------------------------------------------------------------------------------
// grid (224 output rows, crops), block 224 (output columns): one output pixel of the centre window per thread (opd_crop.h), stored into
// its patch row through the normalisation table.
__global__ __launch_bounds__(224) void reid_preprocess_kernel(const opd::ReidCrop* __restrict__ crops, const unsigned char* __restrict__ base,
                                                              const f16_t* __restrict__ lut, f16_t* __restrict__ patches, int P, int T) {
    const opd::ReidCrop c = crops[blockIdx.y];
    const int KP = 3 * P * P;
    const int gw = opd::REID_IMG / P;
    f16_t* dst = patches + (size_t)blockIdx.y * T * KP;
    const int yo = blockIdx.x, xo = threadIdx.x;
    if (yo == 0)
        for (int i = xo; i < KP; i += blockDim.x) dst[i] = 0;   // row 0: the class token's slot (its value comes through the bias table)
    const opd::CropRgb rgb = opd::crop_resample_pixel(c, base, xo, yo, opd::REID_IMG, opd::REID_IMG);
    const int p = (yo / P) * gw + xo / P;
    f16_t* o = dst + (size_t)(1 + p) * KP + ((yo % P) * P + xo % P) * 3;
#pragma unroll
    for (int ch3 = 0; ch3 < 3; ++ch3) o[ch3] = lut[ch3 * 256 + rgb.c[ch3]];
}

// ---- linear layers ----------------------------------------------------------------------------------------------------------------------
constexpr int GP = 72;   // LDS pitch (halves) of a [64][64] operand tile: 144-byte rows, fragment reads 4 banks apart

template <int EPI>
__global__ __launch_bounds__(256) void reid_gemm_kernel(const _Float16* __restrict__ X, const _Float16* __restrict__ W, const float* __restrict__ bias,
                                                        int period, void* __restrict__ out, int M, int N, int K) {
    __shared__ _Float16 Xs[64 * GP];
    __shared__ _Float16 Ws[64 * GP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, li = lane & 15;
    const int wm = wave >> 1, wn = wave & 1;
    const int m0 = blockIdx.x * 64, n0 = blockIdx.y * 64;
    // each thread moves two 16-byte chunks of each operand per K step: rows tid / 8 and tid / 8 + 32, columns (tid % 8) * 8
    const int lr = tid >> 3, lc = (tid & 7) * 8;
    const _Float16* xr0 = X + (size_t)min(m0 + lr, M - 1) * K + lc;        // rows beyond M: a valid row, its results are not stored
    const _Float16* xr1 = X + (size_t)min(m0 + lr + 32, M - 1) * K + lc;
    const _Float16* wr0 = W + (size_t)(n0 + lr) * K + lc;
    const _Float16* wr1 = W + (size_t)(n0 + lr + 32) * K + lc;
    half8 px0 = *reinterpret_cast<const half8*>(xr0), px1 = *reinterpret_cast<const half8*>(xr1);
    half8 pw0 = *reinterpret_cast<const half8*>(wr0), pw1 = *reinterpret_cast<const half8*>(wr1);
    float4v acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = float4v{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < K; k0 += 64) {
        __syncthreads();
        *reinterpret_cast<half8*>(Xs + lr * GP + lc) = px0;
        *reinterpret_cast<half8*>(Xs + (lr + 32) * GP + lc) = px1;
        *reinterpret_cast<half8*>(Ws + lr * GP + lc) = pw0;
        *reinterpret_cast<half8*>(Ws + (lr + 32) * GP + lc) = pw1;
        __syncthreads();
        if (k0 + 64 < K) {   // next step's operands travel while this step's MFMAs run
            px0 = *reinterpret_cast<const half8*>(xr0 + k0 + 64);
            px1 = *reinterpret_cast<const half8*>(xr1 + k0 + 64);
            pw0 = *reinterpret_cast<const half8*>(wr0 + k0 + 64);
            pw1 = *reinterpret_cast<const half8*>(wr1 + k0 + 64);
        }
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            half8 a[2], b[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) a[j] = *reinterpret_cast<const half8*>(Ws + (wn * 32 + j * 16 + li) * GP + ks * 32 + g * 8);
#pragma unroll
            for (int i = 0; i < 2; ++i) b[i] = *reinterpret_cast<const half8*>(Xs + (wm * 32 + i * 16 + li) * GP + ks * 32 + g * 8);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = mfma16(a[j], b[i], acc[i][j]);
        }
    }
    // lane holds out[m0 + wm*32 + i*16 + li][n0 + wn*32 + j*16 + 4g + r]
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int m = m0 + wm * 32 + i * 16 + li;
        if (m >= M) continue;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int n = n0 + wn * 32 + j * 16 + 4 * g;
            float4v v = acc[i][j];
            if (EPI == REID_EPI_F32_PBIAS) {
                if (bias) v += *reinterpret_cast<const float4v*>(bias + (size_t)(m % period) * N + n);
                *reinterpret_cast<float4v*>(static_cast<float*>(out) + (size_t)m * N + n) = v;
            } else {
                v += *reinterpret_cast<const float4v*>(bias + n);
                if (EPI == REID_EPI_F32_RESID) {
                    float4v* o = reinterpret_cast<float4v*>(static_cast<float*>(out) + (size_t)m * N + n);
                    *o = *o + v;
                } else {
                    half4 h;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float x = v[r];
                        if (EPI == REID_EPI_F16_QGELU) x = x * (1.0f / (1.0f + expf(-1.702f * x)));   // quick_gelu in fp32, rounded once
                        h[r] = (_Float16)x;
                    }
                    *reinterpret_cast<half4*>(static_cast<_Float16*>(out) + (size_t)m * N + n) = h;
                }
            }
        }
    }
}

// ---- LayerNorm ----------------------------------------------------------------------------------------------------------------------------
// 4 rows per 256-thread workgroup, lane holds columns j * 128 + 2 lane + {0, 1}; mean, then the mean of squared deviations (torch's order).
__global__ __launch_bounds__(256) void reid_layernorm_kernel(const float* __restrict__ x, int row_stride, const float* __restrict__ gam,
                                                             const float* __restrict__ bet, float* y32, _Float16* __restrict__ y16, int rows, int H) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (r >= rows) return;
    const int nj = H >> 7;
    const float* xr = x + (size_t)r * row_stride * H;
    float v[16];
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j)
        if (j < nj) {
            const float2 t = *reinterpret_cast<const float2*>(xr + j * 128 + 2 * lane);
            v[2 * j] = t.x; v[2 * j + 1] = t.y;
            s += t.x + t.y;
        }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
    const float mean = s / (float)H;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j)
        if (j < nj) {
            const float d0 = v[2 * j] - mean, d1 = v[2 * j + 1] - mean;
            q += d0 * d0 + d1 * d1;
        }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) q += __shfl_xor(q, o);
    const float rstd = 1.0f / sqrtf(q / (float)H + 1e-5f);
#pragma unroll
    for (int j = 0; j < 8; ++j)
        if (j < nj) {
            const int c = j * 128 + 2 * lane;
            const float o0 = (v[2 * j] - mean) * rstd * gam[c] + bet[c];
            const float o1 = (v[2 * j + 1] - mean) * rstd * gam[c + 1] + bet[c + 1];
            y16[(size_t)r * H + c] = (_Float16)o0;
            y16[(size_t)r * H + c + 1] = (_Float16)o1;
            if (y32) *reinterpret_cast<float2*>(y32 + (size_t)r * row_stride * H + c) = make_float2(o0, o1);
        }
}

// ---- attention --------------------------------------------------------------------------------------------------------------------------
// One wave per (head, crop).  Q, K (token rows) and V^T land in LDS zero-padded to 64 tokens; S^T = K Q^T by MFMA, stored as S[query][key]
// fp32; one lane per query row does the fp32 softmax and writes P fp16; O^T = V^T P^T by MFMA.
constexpr int AP = 72;    // LDS pitch (halves) of the [64][64] fp16 tiles
constexpr int SP = 68;    // LDS pitch (floats) of S

__global__ __launch_bounds__(64) void reid_attention_kernel(const _Float16* __restrict__ qkv, _Float16* __restrict__ out, int T, int H) {
    __shared__ _Float16 Qs[64 * AP], Ks[64 * AP], Vt[64 * AP], Ps[64 * AP];
    __shared__ float S[64 * SP];
    const int h = blockIdx.x, crop = blockIdx.y;
    const int lane = threadIdx.x, g = lane >> 4, li = lane & 15;
    const size_t row0 = (size_t)crop * T;
    const int ld = 3 * H;
    for (int c = lane; c < 64 * 8; c += 64) {
        const int t = c >> 3, d0 = (c & 7) * 8;
        half8 q, k, v;
        if (t < T) {
            const _Float16* src = qkv + (row0 + t) * ld + h * 64 + d0;
            q = *reinterpret_cast<const half8*>(src);
            k = *reinterpret_cast<const half8*>(src + H);
            v = *reinterpret_cast<const half8*>(src + 2 * H);
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) q[j] = k[j] = v[j] = (_Float16)0.f;
        }
        *reinterpret_cast<half8*>(Qs + t * AP + d0) = q;
        *reinterpret_cast<half8*>(Ks + t * AP + d0) = k;
#pragma unroll
        for (int j = 0; j < 8; ++j) Vt[(d0 + j) * AP + t] = v[j];
    }
    __syncthreads();
    // S^T tile (kt, qt): D[key 16kt + 4g + r][query 16qt + li]
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int qt = 0; qt < 4; ++qt) {
            float4v s = float4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const half8 a = *reinterpret_cast<const half8*>(Ks + (kt * 16 + li) * AP + ks * 32 + g * 8);
                const half8 b = *reinterpret_cast<const half8*>(Qs + (qt * 16 + li) * AP + ks * 32 + g * 8);
                s = mfma16(a, b, s);
            }
            *reinterpret_cast<float4v*>(S + (qt * 16 + li) * SP + kt * 16 + 4 * g) = s;
        }
    __syncthreads();
    {
        const int q = lane;
        float* srow = S + q * SP;
        _Float16* prow = Ps + q * AP;
        if (q < T) {
            float mx = -INFINITY;
            for (int k = 0; k < T; ++k) mx = fmaxf(mx, srow[k]);
            float sum = 0.f;
            for (int k = 0; k < T; ++k) {
                const float e = expf(srow[k] - mx);
                srow[k] = e;
                sum += e;
            }
            const float inv = 1.0f / sum;
            for (int k = 0; k < 64; ++k) prow[k] = k < T ? (_Float16)(srow[k] * inv) : (_Float16)0.f;
        } else {
            for (int k = 0; k < 64; ++k) prow[k] = (_Float16)0.f;
        }
    }
    __syncthreads();
    // O^T tile (dt, qt): D[d 16dt + 4g + r][query 16qt + li]
#pragma unroll
    for (int qt = 0; qt < 4; ++qt) {
        const int q = qt * 16 + li;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
            float4v o = float4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const half8 a = *reinterpret_cast<const half8*>(Vt + (dt * 16 + li) * AP + ks * 32 + g * 8);
                const half8 b = *reinterpret_cast<const half8*>(Ps + q * AP + ks * 32 + g * 8);
                o = mfma16(a, b, o);
            }
            if (q < T) {
                half4 hv;
#pragma unroll
                for (int r = 0; r < 4; ++r) hv[r] = (_Float16)o[r];
                *reinterpret_cast<half4*>(out + (row0 + q) * H + h * 64 + dt * 16 + 4 * g) = hv;
            }
        }
    }
}

// ---- L2 normalisation --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void reid_l2norm_kernel(float* __restrict__ y, int E) {
    float* row = y + (size_t)blockIdx.x * E;
    float s = 0.f;
    for (int c = threadIdx.x; c < E; c += 64) s += row[c] * row[c];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
    const float inv = 1.0f / sqrtf(s);
    for (int c = threadIdx.x; c < E; c += 64) row[c] *= inv;
}

}  // namespace

hipError_t opd_launch_reid_gemm(int epi, const f16_t* X, const f16_t* W, const float* bias, int period, void* out, int M, int N, int K,
                                hipStream_t stream) {
    if (M <= 0 || N <= 0 || K <= 0 || N % 64 || K % 64 || (epi == REID_EPI_F32_PBIAS && bias && period <= 0)) return hipErrorInvalidValue;
    if (epi != REID_EPI_F32_PBIAS && !bias) return hipErrorInvalidValue;
    const dim3 grid((M + 63) / 64, N / 64);
    const _Float16* x = reinterpret_cast<const _Float16*>(X);
    const _Float16* w = reinterpret_cast<const _Float16*>(W);
    switch (epi) {
        case REID_EPI_F16_BIAS: OPD_LAUNCH(reid_gemm_kernel<REID_EPI_F16_BIAS>, grid, dim3(256), 0, stream, x, w, bias, period, out, M, N, K); break;
        case REID_EPI_F32_RESID: OPD_LAUNCH(reid_gemm_kernel<REID_EPI_F32_RESID>, grid, dim3(256), 0, stream, x, w, bias, period, out, M, N, K); break;
        case REID_EPI_F16_QGELU: OPD_LAUNCH(reid_gemm_kernel<REID_EPI_F16_QGELU>, grid, dim3(256), 0, stream, x, w, bias, period, out, M, N, K); break;
        case REID_EPI_F32_PBIAS: OPD_LAUNCH(reid_gemm_kernel<REID_EPI_F32_PBIAS>, grid, dim3(256), 0, stream, x, w, bias, period, out, M, N, K); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t opd_launch_reid_layernorm(const float* x, int row_stride, const float* g, const float* b, float* y32, f16_t* y16, int rows, int H,
                                     hipStream_t stream) {
    if (rows <= 0 || H % 128 || H > 1024 || row_stride < 1) return hipErrorInvalidValue;
    OPD_LAUNCH(reid_layernorm_kernel, dim3((rows + 3) / 4), dim3(256), 0, stream, x, row_stride, g, b, y32, reinterpret_cast<_Float16*>(y16), rows, H);
    return hipGetLastError();
}

hipError_t opd_launch_reid_attention(const f16_t* qkv, f16_t* out, int crops, int T, int H, hipStream_t stream) {
    if (crops <= 0 || T < 1 || T > 64 || H % 64) return hipErrorInvalidValue;
    OPD_LAUNCH(reid_attention_kernel, dim3(H / 64, crops), dim3(64), 0, stream, reinterpret_cast<const _Float16*>(qkv),
               reinterpret_cast<_Float16*>(out), T, H);
    return hipGetLastError();
}

hipError_t opd_launch_reid_l2norm(float* y, int rows, int E, hipStream_t stream) {
    if (rows <= 0 || E <= 0) return hipErrorInvalidValue;
    OPD_LAUNCH(reid_l2norm_kernel, dim3(rows), dim3(64), 0, stream, y, E);
    return hipGetLastError();
}

hipError_t opd_launch_reid_preprocess(const opd::ReidCrop* crops, const unsigned char* base, const f16_t* lut, f16_t* patches, int ncrops,
                                      int P, int T, hipStream_t stream) {
    if (ncrops <= 0 || P <= 0 || opd::REID_IMG % P) return hipErrorInvalidValue;
    OPD_LAUNCH(reid_preprocess_kernel, dim3(opd::REID_IMG, ncrops), dim3(opd::REID_IMG), 0, stream, crops, base, lut, patches, P, T);
    return hipGetLastError();
}
