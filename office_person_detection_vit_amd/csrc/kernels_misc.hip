// kernels_misc.hip — HBM-bound element-wise / small kernels of the DETR detect path that read or write 16-bit operands (gfx950; the small
// kernels without one -- resize, heads, post-process, ROI features -- are kernels_untyped.hip).
//
//   preprocess   SURVEY.md §8 a1: BGR->RGB, x*(1/255), (x-mean)/std   (HF:models/detr/image_processing_detr.py:639-668)
//   maxpool      a3: MaxPool2d(k3,s2,p1)                              (HF:models/resnet/modeling_resnet.py:84)
//   layernorm    a9/a12: nn.LayerNorm(256), eps 1e-5                  (HF:models/detr/modeling_detr.py:606,629-639)
#include <hip/hip_runtime.h>
#include <math.h>
#include <vector>
#include "opd_kprims.h"

namespace {

// ImageNet statistics, RGB order (HF:utils/constants.py IMAGENET_DEFAULT_MEAN/STD)
__constant__ float c_mean[3] = {0.485f, 0.456f, 0.406f};
__constant__ float c_std[3] = {0.229f, 0.224f, 0.225f};

// One thread per OUTPUT pixel of the zero-bordered NHWC4 image [B][Hp][Wp][4] (image at offset (3,3)): 3 bytes in (BGR),
// 8 bytes out (RGB0 fp16).  Same op order as the oracle: (float(u8) * (1/255) - mean) / std.  The border is the stem
// convolution's zero padding, materialised so that the stem's LDS-DMA needs no per-tap bounds logic.
// valid_hw (nullable): [B][2] = (h, w) of each frame inside the H x W canvas; pixels outside are written as zeros, which
// is what HF's pad-after-normalise produces for a ragged batch (HF:models/detr/image_processing_detr.py:639-668).
__global__ void preprocess_u8_kernel(const uint8_t* __restrict__ in, f16_t* __restrict__ out, int B, int H, int W, int Hp, int Wp,
                                     const int32_t* __restrict__ valid_hw) {
#pragma clang fp contract(off)  // keep mul / sub / div separately rounded, like the reference's tensor ops
    // one thread = 4 consecutive pixels of a padded row: 12 source bytes, two 16-byte stores (one pixel per thread moved
    // 1.7 TB/s: 35 us at batch 8; the arithmetic per pixel is unchanged)
    const int groups = (Wp + 3) >> 2;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)B * Hp * groups) return;
    const int xg = (int)(i % groups);
    const size_t t = i / groups;
    const int yp = (int)(t % Hp);
    const int b = (int)(t / Hp);
    const int y = yp - 3;
    const int vh = valid_hw ? valid_hw[2 * b] : H, vw = valid_hw ? valid_hw[2 * b + 1] : W;
    const bool row_ok = (unsigned)y < (unsigned)vh;
    const uint8_t* srow = in + ((size_t)b * H + (row_ok ? y : 0)) * W * 3;
    f16_t* orow = out + (((size_t)b * Hp + yp) * Wp) * 4;
    const float k = 1.0f / 255.0f;
    half4 o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int xp = xg * 4 + j, x = xp - 3;
        o[j][0] = o[j][1] = o[j][2] = o[j][3] = (elem_t)0.f;
        if (row_ok && (unsigned)x < (unsigned)vw) {
            const uint8_t* s = srow + (size_t)x * 3;
            const float bl = (float)s[0], g = (float)s[1], r = (float)s[2];
            o[j][0] = (elem_t)((r * k - c_mean[0]) / c_std[0]);
            o[j][1] = (elem_t)((g * k - c_mean[1]) / c_std[1]);
            o[j][2] = (elem_t)((bl * k - c_mean[2]) / c_std[2]);
        }
    }
    if (xg * 4 + 3 < Wp && (Wp & 1) == 0) {   // rows are 8 Wp bytes long: the 32-byte groups are 16-byte aligned when Wp is even ...
        half8 a, c;
#pragma unroll
        for (int q = 0; q < 4; ++q) { a[q] = o[0][q]; a[4 + q] = o[1][q]; c[q] = o[2][q]; c[4 + q] = o[3][q]; }
        *reinterpret_cast<half8*>(orow + (size_t)xg * 16) = a;
        *reinterpret_cast<half8*>(orow + (size_t)xg * 16 + 8) = c;
    } else {                                    // ... otherwise (and for the last partial group) pixel by pixel
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (xg * 4 + j < Wp) *reinterpret_cast<half4*>(orow + (size_t)(xg * 4 + j) * 4) = o[j];
    }
}

__global__ void preprocess_f32_kernel(const float* __restrict__ pv, f16_t* __restrict__ out, int B, int H, int W, int Hp, int Wp,
                                      const int32_t* __restrict__ valid_hw) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)B * Hp * Wp) return;
    const int xp = (int)(i % Wp);
    const size_t t = i / Wp;
    const int yp = (int)(t % Hp);
    const int b = (int)(t / Hp);
    const int y = yp - 3, x = xp - 3;
    half4 o;
    o[0] = o[1] = o[2] = o[3] = (elem_t)0.f;
    const int vh = valid_hw ? valid_hw[2 * b] : H, vw = valid_hw ? valid_hw[2 * b + 1] : W;
    if ((unsigned)y < (unsigned)vh && (unsigned)x < (unsigned)vw) {
        const size_t HW = (size_t)H * W;
        const float* s = pv + (size_t)b * 3 * HW + (size_t)y * W + x;
        o[0] = (elem_t)s[0];
        o[1] = (elem_t)s[HW];
        o[2] = (elem_t)s[2 * HW];
    }
    *reinterpret_cast<half4*>(out + i * 4) = o;
}

// One thread per (output pixel, 8-channel group); 9 x 16-byte loads, 1 x 16-byte store.
__global__ void maxpool_kernel(const f16_t* __restrict__ x, f16_t* __restrict__ out, int B, int H, int W, int C, int OH,
                               int OW) {
    const int cg = C >> 3;
    const size_t total = (size_t)B * OH * OW * cg;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int c8 = (int)(i % cg);
    size_t r = i / cg;
    const int ow = (int)(r % OW);
    r /= OW;
    const int oh = (int)(r % OH);
    const int b = (int)(r / OH);
    half8 m;
#pragma unroll
    for (int j = 0; j < 8; ++j) m[j] = (elem_t)(-65504.f);
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
        const int ih = oh * 2 - 1 + kh;
        if ((unsigned)ih >= (unsigned)H) continue;
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
            const int iw = ow * 2 - 1 + kw;
            if ((unsigned)iw >= (unsigned)W) continue;
            const half8 v = *reinterpret_cast<const half8*>(x + (((size_t)b * H + ih) * W + iw) * C + c8 * 8);
#pragma unroll
            for (int j = 0; j < 8; ++j) m[j] = v[j] > m[j] ? v[j] : m[j];
        }
    }
    *reinterpret_cast<half8*>(out + (((size_t)b * OH + oh) * OW + ow) * C + c8 * 8) = m;
}

// One wave per row of 256: lane holds 4 consecutive elements; two-pass (mean, then centred variance) in fp32.
__global__ __launch_bounds__(256) void layernorm256_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, float* __restrict__ y,
                                                           f16_t* __restrict__ y16, int rows) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    const float4v v = *reinterpret_cast<const float4v*>(x + (size_t)row * 256 + lane * 4);
    const float mean = wave_sum(v[0] + v[1] + v[2] + v[3]) * (1.0f / 256.0f);
    const float d0 = v[0] - mean, d1 = v[1] - mean, d2 = v[2] - mean, d3 = v[3] - mean;
    const float var = wave_sum(d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3) * (1.0f / 256.0f);
    const float rstd = 1.0f / sqrtf(var + 1e-5f);
    const float4v g = *reinterpret_cast<const float4v*>(gamma + lane * 4);
    const float4v bb = *reinterpret_cast<const float4v*>(beta + lane * 4);
    float4v o;
    o[0] = d0 * rstd * g[0] + bb[0];
    o[1] = d1 * rstd * g[1] + bb[1];
    o[2] = d2 * rstd * g[2] + bb[2];
    o[3] = d3 * rstd * g[3] + bb[3];
    if (y) *reinterpret_cast<float4v*>(y + (size_t)row * 256 + lane * 4) = o;
    if (y16) {
        half4 h;
        h[0] = (elem_t)o[0]; h[1] = (elem_t)o[1]; h[2] = (elem_t)o[2]; h[3] = (elem_t)o[3];
        *reinterpret_cast<half4*>(y16 + (size_t)row * 256 + lane * 4) = h;
    }
}

// y[row][:] = c[:] for every row (fp32 and an fp16 copy): the decoder's state after the self-attention block of layer 0, which does
// not depend on the input (opd_weights.cpp::build_weights, "dec0").
__global__ __launch_bounds__(256) void broadcast_rows256_kernel(const float* __restrict__ c, float* __restrict__ y, f16_t* __restrict__ y16, int rows) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    const float4v v = *reinterpret_cast<const float4v*>(c + lane * 4);
    *reinterpret_cast<float4v*>(y + (size_t)row * 256 + lane * 4) = v;
    half4 h;
    h[0] = (elem_t)v[0]; h[1] = (elem_t)v[1]; h[2] = (elem_t)v[2]; h[3] = (elem_t)v[3];
    *reinterpret_cast<half4*>(y16 + (size_t)row * 256 + lane * 4) = h;
}

// Split-K reduction + residual + LayerNorm: one wave per row of 256, slabs summed in slice order (deterministic).
__global__ __launch_bounds__(256) void reduce_ln256_kernel(const float* __restrict__ partials, int nsplit, size_t slab_stride,
                                                           const float* __restrict__ residual, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, float* __restrict__ y,
                                                           f16_t* __restrict__ y16, int rows, const float* __restrict__ pos,
                                                           const float* const* __restrict__ pos_ptrs, int period, f16_t* __restrict__ yp16) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    const size_t o = (size_t)row * 256 + lane * 4;
    float4v v = *reinterpret_cast<const float4v*>(partials + o);
    for (int z = 1; z < nsplit; ++z) v += *reinterpret_cast<const float4v*>(partials + z * slab_stride + o);
    if (residual) v += *reinterpret_cast<const float4v*>(residual + o);
    float4v out = v;
    if (gamma) {
        const float mean = wave_sum(v[0] + v[1] + v[2] + v[3]) * (1.0f / 256.0f);
        const float d0 = v[0] - mean, d1 = v[1] - mean, d2 = v[2] - mean, d3 = v[3] - mean;
        const float var = wave_sum(d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3) * (1.0f / 256.0f);
        const float rstd = 1.0f / sqrtf(var + 1e-5f);
        const float4v g = *reinterpret_cast<const float4v*>(gamma + lane * 4);
        const float4v bb = *reinterpret_cast<const float4v*>(beta + lane * 4);
        out[0] = d0 * rstd * g[0] + bb[0];
        out[1] = d1 * rstd * g[1] + bb[1];
        out[2] = d2 * rstd * g[2] + bb[2];
        out[3] = d3 * rstd * g[3] + bb[3];
    }
    if (y) *reinterpret_cast<float4v*>(y + o) = out;
    if (y16) {
        half4 h;
        h[0] = (elem_t)out[0]; h[1] = (elem_t)out[1]; h[2] = (elem_t)out[2]; h[3] = (elem_t)out[3];
        *reinterpret_cast<half4*>(y16 + o) = h;
    }
    if (yp16) {   // second fp16 shadow: the row PLUS its position embedding (what the q / k projections read); pos [period][256] per frame
        const int fr = row / period, pr = row - fr * period;
        const float* prow = (pos_ptrs ? pos_ptrs[fr] : pos) + (size_t)pr * 256 + lane * 4;
        const float4v pe = *reinterpret_cast<const float4v*>(prow);
        half4 h;
        h[0] = (elem_t)(out[0] + pe[0]); h[1] = (elem_t)(out[1] + pe[1]); h[2] = (elem_t)(out[2] + pe[2]); h[3] = (elem_t)(out[3] + pe[3]);
        *reinterpret_cast<half4*>(yp16 + o) = h;
    }
}

__global__ void cast_f16_kernel(const float* __restrict__ x, f16_t* __restrict__ y, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) reinterpret_cast<elem_t*>(y)[i] = (elem_t)x[i];
}

// Cross-attention map (get_attention_map): mean over heads and over the selected queries of softmax(q . k^T * scale) for ONE frame and
// ONE decoder layer, fp32 arithmetic on the fp16 q / k the forward left on the device.  Pass 1: one wave per (selected query, head) row
// -> row maximum and sum of exponentials.  Pass 2: one thread per key sums the normalised weights over the rows in a fixed order.
__global__ __launch_bounds__(256) void attn_map_rowstat_kernel(const f16_t* __restrict__ q, int ldq, const f16_t* __restrict__ k, int ldk,
                                                               const int32_t* __restrict__ sel, int nsel, int heads, int Lk, float scale,
                                                               const int32_t* __restrict__ key_valid2, int key_row, float2* __restrict__ stat) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);   // row = selected query x head
    if (row >= nsel * heads) return;
    const int lane = threadIdx.x & 63, h = row % heads, qi = sel[row / heads];
    float qv[32];
#pragma unroll
    for (int d = 0; d < 32; ++d) qv[d] = (float)reinterpret_cast<const elem_t*>(q)[(size_t)qi * ldq + h * 32 + d];
    const int vr = key_valid2 ? key_valid2[0] : 0x7fffffff, vc = key_valid2 ? key_valid2[1] : 0x7fffffff;
    float mx = -INFINITY;
    for (int key = lane; key < Lk; key += 64) {
        const int kr = key / key_row, kc = key - kr * key_row;
        if (kr >= vr || kc >= vc) continue;
        float s = 0.f;
#pragma unroll
        for (int d = 0; d < 32; ++d) s = fmaf(qv[d], (float)reinterpret_cast<const elem_t*>(k)[(size_t)key * ldk + h * 32 + d], s);
        mx = fmaxf(mx, s * scale);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    float sum = 0.f;
    for (int key = lane; key < Lk; key += 64) {
        const int kr = key / key_row, kc = key - kr * key_row;
        if (kr >= vr || kc >= vc) continue;
        float s = 0.f;
#pragma unroll
        for (int d = 0; d < 32; ++d) s = fmaf(qv[d], (float)reinterpret_cast<const elem_t*>(k)[(size_t)key * ldk + h * 32 + d], s);
        sum += expf(s * scale - mx);
    }
    sum = wave_sum(sum);
    if (lane == 0) stat[row] = make_float2(mx, sum);
}
__global__ __launch_bounds__(256) void attn_map_mean_kernel(const f16_t* __restrict__ q, int ldq, const f16_t* __restrict__ k, int ldk,
                                                            const int32_t* __restrict__ sel, int nsel, int heads, int Lk, float scale,
                                                            const int32_t* __restrict__ key_valid2, int key_row, const float2* __restrict__ stat,
                                                            float* __restrict__ out) {
    const int key = blockIdx.x * 256 + threadIdx.x;
    if (key >= Lk) return;
    const int vr = key_valid2 ? key_valid2[0] : 0x7fffffff, vc = key_valid2 ? key_valid2[1] : 0x7fffffff;
    const int kr = key / key_row, kc = key - kr * key_row;
    float acc = 0.f;
    if (kr < vr && kc < vc) {
        for (int row = 0; row < nsel * heads; ++row) {
            const int h = row % heads, qi = sel[row / heads];
            float s = 0.f;
#pragma unroll
            for (int d = 0; d < 32; ++d)
                s = fmaf((float)reinterpret_cast<const elem_t*>(q)[(size_t)qi * ldq + h * 32 + d],
                         (float)reinterpret_cast<const elem_t*>(k)[(size_t)key * ldk + h * 32 + d], s);
            const float2 st = stat[row];
            acc += expf(s * scale - st.x) / st.y;
        }
    }
    out[key] = acc / (float)(nsel * heads);
}

}  // namespace

hipError_t OPD_SYM(opd_launch_attention_map)(const f16_t* q, int ldq, const f16_t* k, int ldk, const int32_t* sel, int nsel, int heads, int Lk, float scale,
                                    const int32_t* key_valid2, int key_row, void* stat, float* out, hipStream_t stream) {
    if (nsel <= 0 || heads <= 0 || Lk <= 0 || key_row <= 0) return hipErrorInvalidValue;
    OPD_LAUNCH(attn_map_rowstat_kernel, dim3((nsel * heads + 3) / 4), dim3(256), 0, stream, q, ldq, k, ldk, sel, nsel, heads, Lk, scale,
                       key_valid2, key_row, reinterpret_cast<float2*>(stat));
    OPD_LAUNCH(attn_map_mean_kernel, dim3((Lk + 255) / 256), dim3(256), 0, stream, q, ldq, k, ldk, sel, nsel, heads, Lk, scale, key_valid2,
                       key_row, reinterpret_cast<const float2*>(stat), out);
    return hipGetLastError();
}

hipError_t OPD_SYM(opd_launch_preprocess_u8)(const uint8_t* frames, f16_t* out, int B, int H, int W, int Hp, int Wp, const int32_t* valid_hw,
                                    hipStream_t stream) {
    if (Hp < H + 6 || Wp < W + 6) return hipErrorInvalidValue;
    const size_t ngroups = (size_t)B * Hp * ((Wp + 3) / 4);
    OPD_LAUNCH(preprocess_u8_kernel, dim3(blocks_for(ngroups, 256)), dim3(256), 0, stream, frames, out, B, H, W, Hp, Wp, valid_hw);
    return hipGetLastError();
}

hipError_t OPD_SYM(opd_launch_preprocess_f32)(const float* pv, f16_t* out, int B, int H, int W, int Hp, int Wp, const int32_t* valid_hw,
                                     hipStream_t stream) {
    if (Hp < H + 6 || Wp < W + 6) return hipErrorInvalidValue;
    const size_t npix = (size_t)B * Hp * Wp;
    OPD_LAUNCH(preprocess_f32_kernel, dim3(blocks_for(npix, 256)), dim3(256), 0, stream, pv, out, B, H, W, Hp, Wp, valid_hw);
    return hipGetLastError();
}

hipError_t OPD_SYM(opd_launch_maxpool)(const f16_t* x, f16_t* out, int B, int H, int W, int C, int OH, int OW,
                              hipStream_t stream) {
    if (C % 8 != 0) return hipErrorInvalidValue;
    const size_t total = (size_t)B * OH * OW * (C / 8);
    OPD_LAUNCH(maxpool_kernel, dim3(blocks_for(total, 256)), dim3(256), 0, stream, x, out, B, H, W, C, OH, OW);
    return hipGetLastError();
}

hipError_t OPD_SYM(opd_launch_layernorm)(const float* x, const float* gamma, const float* beta, float* y, f16_t* y16, int rows,
                                hipStream_t stream) {
    if (rows <= 0) return hipErrorInvalidValue;
    OPD_LAUNCH(layernorm256_kernel, dim3((rows + 3) / 4), dim3(256), 0, stream, x, gamma, beta, y, y16, rows);
    return hipGetLastError();
}

hipError_t OPD_SYM(opd_launch_broadcast_rows)(const float* c, float* y, f16_t* y16, int rows, hipStream_t stream) {
    if (rows <= 0 || !c || !y || !y16) return hipErrorInvalidValue;
    OPD_LAUNCH(broadcast_rows256_kernel, dim3((rows + 3) / 4), dim3(256), 0, stream, c, y, y16, rows);
    return hipGetLastError();
}

hipError_t OPD_SYM(opd_launch_reduce_ln)(const float* partials, int nsplit, size_t slab_stride, const float* residual,
                                const float* gamma, const float* beta, float* y, f16_t* y16, int rows, hipStream_t stream) {
    return OPD_SYM(opd_launch_reduce_ln_pos)(partials, nsplit, slab_stride, residual, gamma, beta, y, y16, rows, nullptr, nullptr, 0, nullptr, stream);
}

// ... plus a second fp16 output yp16 = fp16(y + pos[frame][row % period]) (pos: one table, or pos_ptrs: one table per frame)
hipError_t OPD_SYM(opd_launch_reduce_ln_pos)(const float* partials, int nsplit, size_t slab_stride, const float* residual, const float* gamma,
                                    const float* beta, float* y, f16_t* y16, int rows, const float* pos, const float* const* pos_ptrs,
                                    int period, f16_t* yp16, hipStream_t stream) {
    if (rows <= 0 || nsplit < 1 || (yp16 && (period <= 0 || (!pos && !pos_ptrs)))) return hipErrorInvalidValue;
    OPD_LAUNCH(reduce_ln256_kernel, dim3((rows + 3) / 4), dim3(256), 0, stream, partials, nsplit, slab_stride, residual,
                       gamma, beta, y, y16, rows, pos, pos_ptrs, period, yp16);
    return hipGetLastError();
}

// Split-K reduction of a convolution: fp32 slabs summed in slice order (deterministic; slab 0 carries the bias), ReLU, one rounding to the
// 16-bit operand type.  8 elements per thread (two 16-byte loads per slab, one 16-byte store).
static __global__ __launch_bounds__(256) void reduce_act16_kernel(const float* __restrict__ partials, int nsplit, size_t slab_stride, f16_t* __restrict__ out,
                                                           size_t n8, int relu) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n8) return;
    const size_t o = i * 8;
    float4v a = *reinterpret_cast<const float4v*>(partials + o), b = *reinterpret_cast<const float4v*>(partials + o + 4);
    for (int z = 1; z < nsplit; ++z) {
        a += *reinterpret_cast<const float4v*>(partials + z * slab_stride + o);
        b += *reinterpret_cast<const float4v*>(partials + z * slab_stride + o + 4);
    }
    half8 h;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        h[r] = (elem_t)(relu && a[r] < 0.f ? 0.f : a[r]);
        h[4 + r] = (elem_t)(relu && b[r] < 0.f ? 0.f : b[r]);
    }
    *reinterpret_cast<half8*>(reinterpret_cast<elem_t*>(out) + o) = h;
}

hipError_t OPD_SYM(opd_launch_reduce_act16)(const float* partials, int nsplit, size_t slab_stride, f16_t* out, size_t n, int relu, hipStream_t stream) {
    if (nsplit < 1 || n == 0 || (n % 8) != 0 || (slab_stride % 4) != 0) return hipErrorInvalidValue;
    OPD_LAUNCH(reduce_act16_kernel, dim3((unsigned)((n / 8 + 255) / 256)), dim3(256), 0, stream, partials, nsplit, slab_stride, out, n / 8, relu);
    return hipGetLastError();
}

hipError_t OPD_SYM(opd_launch_cast_f16)(const float* x, f16_t* y, size_t n, hipStream_t stream) {
    OPD_LAUNCH(cast_f16_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, stream, x, y, n);
    return hipGetLastError();
}
