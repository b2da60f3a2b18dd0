// kernels_untyped.hip — the small kernels of the DETR detect path WITHOUT a 16-bit operand (gfx950): uint8, int32, fp32 and fp64 only, so the
// file is compiled once (it is not in csrc/build.py's ELEM_SOURCES; the typed small kernels are kernels_misc.hip).
//
//   resize       SURVEY.md §8 a1: Pillow's two-pass 8-bit bilinear resampler (HF:models/detr/image_processing_detr.py:424-436)
//   gemm_f32     plan-build-time fp32 GEMM (position-embedding folds)
//   heads        a13: class_labels_classifier + DetrMLPPredictionHead + sigmoid (HF:...modeling_detr.py:1284-1300,1410-1411)
//   postprocess  a14: HF post_process_object_detection               (HF:models/detr/image_processing_detr.py:805-856)
//   roi_features a17: FeatureExtractor.extract_roi_features           (src/tracking/feature_extractor.py:39-88)
//   checksum     diagnostic tap (opd_test_set_taps)
//   similarity   tracker cost matrix (src/tracking/similarity.py:42-220)
#include <hip/hip_runtime.h>
#include <math.h>
#include "opd_kprims.h"

namespace {

// Bilinear resize of uint8 HxWx3 frames, bit-exact with Pillow's two-pass 8-bit resampler, which is what HF's image
// processor runs on the host (HF:models/detr/image_processing_detr.py:424-436 -> PIL Image.resize(BILINEAR);
// Pillow src/libImaging/Resample.c: ImagingResampleHorizontal_8bpc / ImagingResampleVertical_8bpc).  Both passes use
// 22-bit fixed-point coefficients (tables built on the host by opd_resize_coeffs with Pillow's formulas) and each pass
// rounds to uint8: out = clip8((2^21 + sum_k pixel_k * coeff_k) >> 22).  One thread per output pixel computes the few
// horizontally resampled source rows it needs (rounded, like the intermediate image) and combines them vertically.
__global__ void resize_bilinear_u8_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int B, int h, int w, int oh,
                                          int ow, const int32_t* __restrict__ bh, const int32_t* __restrict__ kh, int ksh,
                                          const int32_t* __restrict__ bv, const int32_t* __restrict__ kv, int ksv) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)B * oh * ow) return;
    const int xo = (int)(i % ow);
    const size_t t = i / ow;
    const int yo = (int)(t % oh);
    const int b = (int)(t / oh);
    const int xmin = bh[2 * xo], xcnt = bh[2 * xo + 1];
    const int ymin = bv[2 * yo], ycnt = bv[2 * yo + 1];
    const int32_t* ckh = kh + (size_t)xo * ksh;
    const int32_t* ckv = kv + (size_t)yo * ksv;
    const int half = 1 << 21;
    int a0 = half, a1 = half, a2 = half;
    for (int j = 0; j < ycnt; ++j) {
        const uint8_t* row = in + (((size_t)b * h + ymin + j) * w + xmin) * 3;
        int s0 = half, s1 = half, s2 = half;
        for (int k = 0; k < xcnt; ++k) {
            const int c = ckh[k];
            s0 += (int)row[3 * k] * c;
            s1 += (int)row[3 * k + 1] * c;
            s2 += (int)row[3 * k + 2] * c;
        }
        s0 >>= 22; s1 >>= 22; s2 >>= 22;   // arithmetic shift, then clip8
        s0 = s0 < 0 ? 0 : (s0 > 255 ? 255 : s0);
        s1 = s1 < 0 ? 0 : (s1 > 255 ? 255 : s1);
        s2 = s2 < 0 ? 0 : (s2 > 255 ? 255 : s2);
        const int c = ckv[j];
        a0 += s0 * c; a1 += s1 * c; a2 += s2 * c;
    }
    a0 >>= 22; a1 >>= 22; a2 >>= 22;
    uint8_t* o = out + i * 3;
    o[0] = (uint8_t)(a0 < 0 ? 0 : (a0 > 255 ? 255 : a0));
    o[1] = (uint8_t)(a1 < 0 ? 0 : (a1 > 255 ? 255 : a1));
    o[2] = (uint8_t)(a2 < 0 ? 0 : (a2 > 255 ? 255 : a2));
}

// Plan-build-time fp32 GEMM (pos-embedding folds): one thread per output, K-loop in order; not on the hot path.
__global__ void gemm_f32_kernel(const float* __restrict__ A, const float* __restrict__ Wt, const float* __restrict__ bias,
                                float* __restrict__ C, int M, int N, int K, int ldc) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    const int m = blockIdx.y;
    if (n >= N || m >= M) return;
    const float* a = A + (size_t)m * K;
    const float* w = Wt + (size_t)n * K;
    float acc = 0.f;
    for (int k = 0; k < K; ++k) acc = fmaf(a[k], w[k], acc);
    C[(size_t)m * ldc + n] = acc + (bias ? bias[n] : 0.f);
}

// Heads (HF:models/detr/modeling_detr.py:1284-1300, 1317-1322, 1410-1411): class logits and the box MLP + sigmoid for the decoder
// states, fp32 throughout — on the matrix pipe: v_mfma_f32_16x16x4_f32 is an exact fp32 fma chain (k-ordered, one rounding per
// product) at the fp32 vector rate, without the vector pipe's loads-per-FMA problem.  One 512-thread workgroup per 16 decoder rows
// (the MFMA's 16 columns); a wave owns 16-channel output tiles (weights = A operand straight from L2: [in][out] storage gives
// lane (k, n) a coalesced read; rows = B operand from LDS) and chains the 64 MFMAs of a tile's K = 256 on one accumulator, two tiles
// interleaved per wave.  The decoder's final LayerNorm (two-pass fp32, as kernels_misc.hip::layernorm256_kernel) runs on the rows first when
// ln_gamma is given.  Batch 8 (800 rows, 50 workgroups): 30 us, against 35 us for the VALU form of rounds 1-2 (4 rows per
// 1024-thread block, every weight loaded once per 4 rows); what remains is six L2 round trips for the weights.
constexpr int HEAD_ROWS = 16;
constexpr int HEAD_LD = 260;   // fp32 words per LDS row (256 + 4: rows 8 apart do not share a bank)

__global__ __launch_bounds__(512) void heads_kernel(HeadParams p) {
    __shared__ float h[HEAD_ROWS][HEAD_LD];
    __shared__ float t1[HEAD_ROWS][HEAD_LD];
    __shared__ float part[8][64];
    const int row0 = blockIdx.x * HEAD_ROWS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    {   // rows -> LDS: 32 threads per row, 8 consecutive columns each; optional LayerNorm by the same 32 threads
        const int r = tid >> 5, c0 = (tid & 31) * 8;
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = row0 + r < p.rows ? p.hs[(size_t)(row0 + r) * 256 + c0 + j] : 0.f;
        auto ln_rows = [&](const float* __restrict__ gamma, const float* __restrict__ beta) {   // two-pass fp32 LayerNorm by the row's 32 threads
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j) s += v[j];
#pragma unroll
            for (int o = 16; o > 0; o >>= 1) s += __shfl_xor(s, o);
            const float mean = s * (1.0f / 256.0f);
            float q = 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j) { v[j] -= mean; q += v[j] * v[j]; }
#pragma unroll
            for (int o = 16; o > 0; o >>= 1) q += __shfl_xor(q, o);
            const float rstd = 1.0f / sqrtf(q * (1.0f / 256.0f) + 1e-5f);
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = v[j] * rstd * gamma[c0 + j] + beta[c0 + j];
        };
        if (p.partials) {   // fused decoder: the last layer's FFN arrives as partial sums (kernels_dec.hip::dec_ffn_kernel): + b2, summed in order, LN3
            const size_t rc = (size_t)(row0 + r < p.rows ? row0 + r : p.rows - 1) * 256 + c0;
            float4v pa[16], pb[16];
#pragma unroll
            for (int sp = 0; sp < 16; ++sp) {   // every slab requested before the first one is needed (a dependent load costs ~1 us)
                const float* ps = p.partials + (size_t)(sp < p.nsplit ? sp : p.nsplit - 1) * p.rows * 256 + rc;
                pa[sp] = *reinterpret_cast<const float4v*>(ps);
                pb[sp] = *reinterpret_cast<const float4v*>(ps + 4);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] += p.ffn_b2[c0 + j];
#pragma unroll
            for (int sp = 0; sp < 16; ++sp)
                if (sp < p.nsplit) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) { v[j] += pa[sp][j]; v[4 + j] += pb[sp][j]; }
                }
            if (row0 + r >= p.rows) {
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = 0.f;
            }
            ln_rows(p.ln3_gamma, p.ln3_beta);
        }
        if (p.ln_gamma) ln_rows(p.ln_gamma, p.ln_beta);
#pragma unroll
        for (int j = 0; j < 8; ++j) h[r][c0 + j] = v[j];
    }
    __syncthreads();
    // out[m][n] = act(sum_k in[m][k] * wt[k][n] + bias[n]) for the workgroup's 16 rows m: D[row = channel][col = m] per 16-channel
    // tile; lane (kq = lane >> 4, i = lane & 15) feeds A[i][kq] = wt[k0 + kq][n0 + i] and B[kq][i] = in[i][k0 + kq], and receives
    // channels n0 + 4 kq + r of row i.
    const int kq = lane >> 4, li = lane & 15;
    auto layer = [&](const float (*in)[HEAD_LD], const float* __restrict__ wt, const int N, const int ntiles, auto&& emit) {
        for (int nt = wave; nt < ntiles; nt += 16) {   // this wave's tiles nt and nt + 8, interleaved (two accumulator chains)
            const int nA = nt * 16 + li, nB = (nt + 8) * 16 + li;
            const bool okA = nA < N, okB = nt + 8 < ntiles && nB < N;
            float4v accA = {0.f, 0.f, 0.f, 0.f}, accB = {0.f, 0.f, 0.f, 0.f};
            // 2 x 32 weight operands (half the reduction of the tile pair) are requested before their first MFMA: the kernel is a
            // latency chain (every weight comes from L2, ~1 us away), so two round trips per tile pair instead of sixteen (46 us)
#pragma unroll 1
            for (int half = 0; half < 2; ++half) {
                float a[32], b2[32];
#pragma unroll
                for (int u = 0; u < 32; ++u) {
                    const int k = (half * 32 + u) * 4 + kq;
                    a[u] = okA ? wt[(size_t)k * N + nA] : 0.f;
                    b2[u] = okB ? wt[(size_t)k * N + nB] : 0.f;
                }
#pragma unroll
                for (int u = 0; u < 32; ++u) {
                    const float x = in[li][(half * 32 + u) * 4 + kq];
                    accA = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], x, accA, 0, 0, 0);
                    accB = __builtin_amdgcn_mfma_f32_16x16x4f32(b2[u], x, accB, 0, 0, 0);
                }
            }
            emit(nt * 16 + kq * 4, accA);
            if (nt + 8 < ntiles) emit((nt + 8) * 16 + kq * 4, accB);
        }
    };
    // class logits: lane holds channels n .. n + 3 of row li
    layer(h, p.wc, p.ncls, (p.ncls + 15) / 16, [&](const int n, const float4v acc) {
        if (row0 + li < p.rows)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (n + r < p.ncls) p.logits[(size_t)(row0 + li) * p.ncls + n + r] = acc[r] + p.bc[n + r];
    });
    // box MLP: 256 -> 256 -> 256 -> 4, ReLU between, sigmoid at the end
    layer(h, p.w1, 256, 16, [&](const int n, const float4v acc) {
#pragma unroll
        for (int r = 0; r < 4; ++r) { const float v = acc[r] + p.b1[n + r]; t1[li][n + r] = v > 0.f ? v : 0.f; }
    });
    __syncthreads();   // t1 complete; every wave is done reading h
    layer(t1, p.w2, 256, 16, [&](const int n, const float4v acc) {
#pragma unroll
        for (int r = 0; r < 4; ++r) { const float v = acc[r] + p.b2[n + r]; h[li][n + r] = v > 0.f ? v : 0.f; }   // h is free: second hidden layer
    });
    __syncthreads();
    {   // last layer: 64 outputs (row = lane >> 2, coordinate = lane & 3), the reduction split over the 8 waves (32 k each), summed in order
        const int r = lane >> 2, c = lane & 3;
        float a = 0.f;
#pragma unroll 8
        for (int kk = 0; kk < 32; ++kk) a = fmaf(h[r][wave * 32 + kk], p.w3[(wave * 32 + kk) * 4 + c], a);
        part[wave][lane] = a;
    }
    __syncthreads();
    if (tid < 64) {
        const int r = tid >> 2, c = tid & 3;
        float a = part[0][tid];
#pragma unroll
        for (int w = 1; w < 8; ++w) a += part[w][tid];
        if (row0 + r < p.rows) p.boxes[(size_t)(row0 + r) * 4 + c] = 1.0f / (1.0f + expf(-(a + p.b3[c])));
    }
}

struct DetRec {
    float x1, y1, x2, y2, score;
    int32_t label, query_index, frame;
};

// One block (1024 threads = 16 waves) per frame.  Phase 1: wave w takes queries w, w+16, ... (at most 8); it issues the
// loads of ALL its queries first (one L2 round trip instead of one per query), then its lanes stride the classes with
// wave-level max / sum / first-argmax reductions.  Phase 2: one thread per query converts the box and compacts the kept
// queries in query order via a block prefix sum.  (One thread per query with serial class loops: 24 us.)
__global__ __launch_bounds__(1024) void postprocess_kernel(PostParams p) {
    __shared__ int flags[128];
    __shared__ float s_score[128];
    __shared__ int s_label[128];
    const int b = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    {
        float v0[8], v1[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int qq = wave + i * 16;
            const float* lg = p.logits + ((size_t)b * p.Q + (qq < p.Q ? qq : 0)) * p.ncls;
            v0[i] = lane < p.ncls ? lg[lane] : -INFINITY;
            v1[i] = lane + 64 < p.ncls ? lg[lane + 64] : -INFINITY;
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int qq = wave + i * 16;
            float mx = fmaxf(v0[i], v1[i]);
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
            const float e0 = lane < p.ncls ? expf(v0[i] - mx) : 0.f;
            const float e1 = lane + 64 < p.ncls ? expf(v1[i] - mx) : 0.f;
            float sum = e0 + e1, best = -1.f;
            int bl = 0x7fffffff;
            if (lane < p.ncls - 1) { best = e0; bl = lane; }
            if (lane + 64 < p.ncls - 1 && e1 > best) { best = e1; bl = lane + 64; }   // ascending class order: first maximum
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                sum += __shfl_xor(sum, o);
                const float ob = __shfl_xor(best, o);
                const int ol = __shfl_xor(bl, o);
                if (ob > best || (ob == best && ol < bl)) { best = ob; bl = ol; }   // ties -> lowest class index
            }
            if (lane == 0 && qq < p.Q) { s_score[qq] = best / sum; s_label[qq] = bl; }
        }
    }
    __syncthreads();
    const int q = threadIdx.x;
    float score = 0.f, x1 = 0.f, y1 = 0.f, x2 = 0.f, y2 = 0.f;
    int label = 0, keep = 0;
    if (q < p.Q) {
        score = s_score[q];
        label = s_label[q];
        const float* bx = p.boxes + ((size_t)b * p.Q + q) * 4;
        const float h = (float)p.orig_hw[b * 2], w = (float)p.orig_hw[b * 2 + 1];
        x1 = (bx[0] - 0.5f * bx[2]) * w;
        y1 = (bx[1] - 0.5f * bx[3]) * h;
        x2 = (bx[0] + 0.5f * bx[2]) * w;
        y2 = (bx[1] + 0.5f * bx[3]) * h;
        keep = score > p.threshold ? 1 : 0;
    }
    if (q < 128) flags[q] = keep;
    __syncthreads();
    if (q >= 128) return;
    int pos = 0;
    for (int i = 0; i < q; ++i) pos += flags[i];
    if (keep) {
        DetRec* rec = reinterpret_cast<DetRec*>(p.records) + (size_t)b * p.Q + pos;
        rec->x1 = x1; rec->y1 = y1; rec->x2 = x2; rec->y2 = y2; rec->score = score;
        rec->label = label; rec->query_index = q; rec->frame = b;
    }
    if (q == 127) p.counts[b] = pos + keep;
}

// One block per ROI: mean over the ROI window of the [h][w][256] map, then L2 normalise.  1024 threads = 16 groups of 64 lanes; a lane owns 4
// channels (one 16-byte load per position), group g takes the window positions g, g + 16, ... in row-major order, and the 16 partial sums of
// a channel are added in group order: a fixed summation order whatever the window.  (The first form -- 256 threads, one channel each, a serial
// loop over the whole window -- took ~90 us for a large box: up to 1050 dependent-latency iterations on one CU.)
__device__ __forceinline__ void roi_pool_l2(const float* __restrict__ enc, float* __restrict__ out_row, const int x0, const int y0, const int x1,
                                            const int y1, const int w, float (&part)[16][256], float (&red)[4]) {
    const int t = threadIdx.x, g = t >> 6, l = t & 63;
    const int bw = x1 - x0, n = (y1 - y0) * bw;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int p = g; p < n; p += 16) {
        const int dy = p / bw, dx = p - dy * bw;
        const float4 v = *reinterpret_cast<const float4*>(enc + ((size_t)(y0 + dy) * w + (x0 + dx)) * 256 + 4 * l);
        acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
    *reinterpret_cast<float4*>(&part[g][4 * l]) = acc;
    __syncthreads();
    if (t < 256) {
        float sum = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) sum += part[k][t];
        const float mean = sum / (float)n;
        const float ss = wave_sum(mean * mean);
        if ((t & 63) == 0) red[t >> 6] = ss;
        part[0][t] = mean;   // (row 0 has been read by this thread only)
    }
    __syncthreads();
    if (t < 256) {
        const float norm = sqrtf(red[0] + red[1] + red[2] + red[3]);
        out_row[t] = part[0][t] / (norm + 1e-8f);
    }
}
__global__ __launch_bounds__(1024) void roi_features_kernel(const float* __restrict__ enc, const int32_t* __restrict__ rois,
                                                            float* __restrict__ out, int h, int w) {
    __shared__ float part[16][256];
    __shared__ float red[4];
    const int r = blockIdx.x;
    roi_pool_l2(enc, out + (size_t)r * 256, rois[r * 4], rois[r * 4 + 1], rois[r * 4 + 2], rois[r * 4 + 3], w, part, red);
}
// The same for the RECORDS the post-process kernel left on the device (opd_detr_detect_frames_features): block (i, b) takes record i of frame
// b; a record of class `label` gets its feature in row `query_index` of out[b] (other rows are not written).  Box -> map window as
// opd_detr_roi_features computes it on the host from the (x, y, w, h) float32 box of a `Detection` (feature_extractor.py:68-78): the width is
// the float32 difference, the scaling runs in double, the casts truncate.
__global__ __launch_bounds__(1024) void roi_features_rec_kernel(const float* __restrict__ enc, const DetRec* __restrict__ recs,
                                                               const int32_t* __restrict__ counts, const int32_t* __restrict__ orig_hw, int label,
                                                               float* __restrict__ out, int Q, int h, int w) {
    __shared__ float part[16][256];
    __shared__ float red[4];
    const int i = blockIdx.x, b = blockIdx.y;
    if (i >= counts[b]) return;
    const DetRec r = recs[(size_t)b * Q + i];
    if (r.label != label) return;
    const double oh = (double)orig_hw[2 * b], ow = (double)orig_hw[2 * b + 1];
    const double x = (double)r.x1, y = (double)r.y1, bw = (double)(r.x2 - r.x1), bh = (double)(r.y2 - r.y1);
    int x0 = (int)((x / ow) * w), y0 = (int)((y / oh) * h);
    int x1 = (int)(((x + bw) / ow) * w), y1 = (int)(((y + bh) / oh) * h);
    x0 = max(0, min(x0, w - 1)); y0 = max(0, min(y0, h - 1));
    x1 = max(x0 + 1, min(x1, w)); y1 = max(y0 + 1, min(y1, h));
    roi_pool_l2(enc + (size_t)b * h * w * 256, out + ((size_t)b * Q + r.query_index) * 256, x0, y0, x1, y1, w, part, red);
}

}  // namespace

hipError_t opd_launch_resize_u8(const uint8_t* in, uint8_t* out, int B, int h, int w, int oh, int ow, const int32_t* bounds_h,
                                const int32_t* coeff_h, int ksize_h, const int32_t* bounds_v, const int32_t* coeff_v, int ksize_v,
                                hipStream_t stream) {
    if (B <= 0 || h <= 0 || w <= 0 || oh <= 0 || ow <= 0) return hipErrorInvalidValue;
    const size_t npix = (size_t)B * oh * ow;
    OPD_LAUNCH(resize_bilinear_u8_kernel, dim3(blocks_for(npix, 256)), dim3(256), 0, stream, in, out, B, h, w, oh, ow, bounds_h,
                       coeff_h, ksize_h, bounds_v, coeff_v, ksize_v);
    return hipGetLastError();
}

// Diagnostic tap (opd_test_set_taps): position-weighted 64-bit sum of a buffer's 32-bit words, one partial per block.
static __global__ void checksum_kernel(const uint32_t* __restrict__ buf, size_t nwords, unsigned long long* __restrict__ slots) {
    __shared__ unsigned long long part[256];
    unsigned long long acc = 0ull;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nwords; i += (size_t)gridDim.x * blockDim.x)
        acc += (unsigned long long)buf[i] * (unsigned long long)((i * 2654435761ull + 1ull) | 1ull);
    part[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) slots[blockIdx.x] = part[0];
}

hipError_t opd_launch_checksum(const void* buf, size_t bytes, unsigned long long* slots, hipStream_t stream) {
    OPD_LAUNCH(checksum_kernel, dim3(OPD_TAP_BLOCKS), dim3(256), 0, stream, reinterpret_cast<const uint32_t*>(buf), bytes / 4, slots);
    return hipGetLastError();
}

hipError_t opd_launch_gemm_f32(const float* A, const float* Wt, const float* bias, float* C, int M, int N, int K, int ldc,
                               hipStream_t stream) {
    OPD_LAUNCH(gemm_f32_kernel, dim3((N + 63) / 64, M), dim3(64), 0, stream, A, Wt, bias, C, M, N, K, ldc);
    return hipGetLastError();
}

hipError_t opd_launch_heads(const HeadParams& p, hipStream_t stream) {
    if (p.ncls > 256 || p.rows <= 0) return hipErrorInvalidValue;
    if (p.partials && (p.nsplit < 1 || p.nsplit > 16 || !p.ffn_b2 || !p.ln3_gamma || !p.ln3_beta)) return hipErrorInvalidValue;
    OPD_LAUNCH(heads_kernel, dim3((p.rows + HEAD_ROWS - 1) / HEAD_ROWS), dim3(512), 0, stream, p);
    return hipGetLastError();
}

hipError_t opd_launch_postprocess(const PostParams& p, hipStream_t stream) {
    if (p.Q > 128 || p.ncls > 128 || p.B <= 0) return hipErrorInvalidValue;
    OPD_LAUNCH(postprocess_kernel, dim3(p.B), dim3(1024), 0, stream, p);
    return hipGetLastError();
}

// Tracker cost matrix (src/tracking/similarity.py:42-220): one thread per (track i, detection j).
//   cos = clip(dot_fp32(f1[i], f2[j]), -1, 1)  if both carry features        (appearance term, weight aw)
//   iou of the xywh boxes, 0 when the intersection is empty or the union is not positive, clipped to [0, 1]   (weight mw)
//   similarity = clip((aw*cos + mw*iou) / (weights used), 0, 1) in double like the reference's Python floats, stored as fp32;
//   as_distance: 1 - similarity (computed on the fp32 value, like `1.0 - similarity_matrix`).
__global__ void similarity_matrix_kernel(const float* __restrict__ f1, const float* __restrict__ b1, const uint8_t* __restrict__ has1,
                                         int n1, const float* __restrict__ f2, const float* __restrict__ b2,
                                         const uint8_t* __restrict__ has2, int n2, int D, double aw, double mw, int as_distance,
                                         float* __restrict__ out) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n1 * n2) return;
    const int i = idx / n2, j = idx - i * n2;
    double score = 0.0, total = 0.0;
    if (f1 && f2 && (!has1 || has1[i]) && (!has2 || has2[j])) {
        const float* a = f1 + (size_t)i * D;
        const float* c = f2 + (size_t)j * D;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        int k = 0;
        for (; k + 4 <= D; k += 4) {
            acc[0] = fmaf(a[k], c[k], acc[0]); acc[1] = fmaf(a[k + 1], c[k + 1], acc[1]);
            acc[2] = fmaf(a[k + 2], c[k + 2], acc[2]); acc[3] = fmaf(a[k + 3], c[k + 3], acc[3]);
        }
        for (; k < D; ++k) acc[0] = fmaf(a[k], c[k], acc[0]);
        float dot = (acc[0] + acc[1]) + (acc[2] + acc[3]);
        dot = dot < -1.f ? -1.f : (dot > 1.f ? 1.f : dot);
        score += aw * (double)dot;
        total += aw;
    }
    {
        const double x1 = b1[4 * i], y1 = b1[4 * i + 1], w1 = b1[4 * i + 2], h1 = b1[4 * i + 3];
        const double x2 = b2[4 * j], y2 = b2[4 * j + 1], w2 = b2[4 * j + 2], h2 = b2[4 * j + 3];
        const double ix0 = x1 > x2 ? x1 : x2, iy0 = y1 > y2 ? y1 : y2;
        const double ix1 = (x1 + w1) < (x2 + w2) ? (x1 + w1) : (x2 + w2), iy1 = (y1 + h1) < (y2 + h2) ? (y1 + h1) : (y2 + h2);
        double iou = 0.0;
        if (ix1 > ix0 && iy1 > iy0) {
            const double inter = (ix1 - ix0) * (iy1 - iy0);
            const double uni = w1 * h1 + w2 * h2 - inter;
            if (uni > 0.0) {
                iou = inter / uni;
                iou = iou < 0.0 ? 0.0 : (iou > 1.0 ? 1.0 : iou);
            }
        }
        score += mw * iou;
        total += mw;
    }
    double sim = total > 0.0 ? score / total : 0.0;
    sim = sim < 0.0 ? 0.0 : (sim > 1.0 ? 1.0 : sim);
    const float simf = (float)sim;
    out[idx] = as_distance ? 1.0f - simf : simf;
}

hipError_t opd_launch_similarity_matrix(const float* f1, const float* b1, const uint8_t* has1, int n1, const float* f2, const float* b2,
                                        const uint8_t* has2, int n2, int D, double aw, double mw, int as_distance, float* out,
                                        hipStream_t stream) {
    if (n1 <= 0 || n2 <= 0 || D <= 0 || !b1 || !b2 || !out) return hipErrorInvalidValue;
    OPD_LAUNCH(similarity_matrix_kernel, dim3((n1 * n2 + 127) / 128), dim3(128), 0, stream, f1, b1, has1, n1, f2, b2, has2, n2, D, aw,
                       mw, as_distance, out);
    return hipGetLastError();
}

hipError_t opd_launch_roi_features(const float* enc, const int32_t* rois, float* out, int n, int h, int w,
                                   hipStream_t stream) {
    if (n <= 0) return hipErrorInvalidValue;
    OPD_LAUNCH(roi_features_kernel, dim3(n), dim3(1024), 0, stream, enc, rois, out, h, w);
    return hipGetLastError();
}
hipError_t opd_launch_roi_features_records(const float* enc, const void* records, const int32_t* counts, const int32_t* orig_hw, int label,
                                           float* out, int B, int Q, int h, int w, hipStream_t stream) {
    if (B <= 0 || Q <= 0 || h <= 0 || w <= 0 || !enc || !records || !counts || !orig_hw || !out) return hipErrorInvalidValue;
    OPD_LAUNCH(roi_features_rec_kernel, dim3(Q, B), dim3(1024), 0, stream, enc, reinterpret_cast<const DetRec*>(records), counts, orig_hw, label, out, Q, h, w);
    return hipGetLastError();
}
