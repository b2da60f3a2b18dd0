// opd_kprims.h — the device-side primitives the kernel files share ("kernel primitives"): vector types, the swizzled LDS tile row, tile
// order, 16-bit packing, waits and fences, the spelling of LDS-DMA requests, tile-row coordinates of the convolutions, wave reductions.
// Included by every kernels_*.hip; the host-side handle layer is opd_device.h, the launchers' declarations are opd_kernels.h.
// Everything here is __forceinline__ and lives in an anonymous namespace: a kernel file compiles to what it would with the text in place.
#pragma once
#include <hip/hip_runtime.h>
#include "opd_elem.h"
#include "opd_kernels.h"

// ---- vector types (elem_t: fp16, or bf16 in the second instantiation of an ELEM_SOURCES file; _Float16 everywhere else) ----------------
typedef elem_t half8 __attribute__((ext_vector_type(8)));
typedef elem_t half4 __attribute__((ext_vector_type(4)));
typedef float float4v __attribute__((ext_vector_type(4)));
typedef float float2v __attribute__((ext_vector_type(2)));
typedef unsigned int uint2v __attribute__((ext_vector_type(2)));
typedef unsigned int uint4v __attribute__((ext_vector_type(4)));

namespace {

// ---- LDS tile row: 64 halfs = 128 bytes, 16-byte chunks XOR-swizzled by the row so that ds_read_b128 fragment reads are conflict free ----
constexpr int ROW_BYTES = 128;
__device__ __forceinline__ int swz(int row, int chunk) { return row * ROW_BYTES + ((chunk ^ (row & 7)) << 4); }

// ---- tile order and division ------------------------------------------------------------------------------------------------------------
// XCD-aware block -> tile map (cdna_hip_programming.md T1, bijective form).  Workgroups are dealt round-robin over the 8
// XCDs (blocks b and b+8 share an XCD and its private 4 MiB L2), so hand each XCD a CONTIGUOUS range of logical tile
// ids: the n-tiles of one m-tile (which re-read the same activation rows) then run on one XCD, back to back, and the
// rows are fetched from HBM / Infinity Cache once instead of once per n-tile.  Speed only, never correctness.
__device__ __forceinline__ int xcd_logical_block(int bid, int nblocks) {
    const int q = nblocks >> 3, r = nblocks & 7;
    const int x = bid & 7, k = bid >> 3;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + k;
}
// the same ranges, each walked in descending order (BtailParams::rev)
__device__ __forceinline__ int xcd_logical_block_rev(int bid, int nblocks) {
    const int q = nblocks >> 3, r = nblocks & 7;
    const int x = bid & 7, k = bid >> 3;
    return (x < r ? x * (q + 1) + q - k : r * (q + 1) + (x - r) * q + q - 1 - k);
}
// m / d by the host-computed reciprocal (opd_make_fastdiv: a runtime division is ~40 VALU instructions)
__device__ __forceinline__ int fdiv(const int m, const FastDiv& f) {   // m >= 0
    return f.one ? m : (int)(__umulhi((unsigned)m, f.mul) >> f.shift);
}

// ---- 16-bit packing -------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned pack2h(float a, float b) {
    typedef elem_t half2v __attribute__((ext_vector_type(2)));
    half2v h;
    h[0] = (elem_t)a;
    h[1] = (elem_t)b;
    unsigned u;
    __builtin_memcpy(&u, &h, 4);
    return u;
}
__device__ __forceinline__ void unpack2h(unsigned u, float& a, float& b) {
    typedef elem_t half2v __attribute__((ext_vector_type(2)));
    half2v h;
    __builtin_memcpy(&h, &u, 4);
    a = (float)h[0];
    b = (float)h[1];
}
__device__ __forceinline__ half8 as_half8(unsigned a, unsigned b, unsigned c, unsigned d) {
    uint4v u = {a, b, c, d};
    half8 h;
    __builtin_memcpy(&h, &u, 16);
    return h;
}

// ---- waits and fences -------------------------------------------------------------------------------------------------------------------
// THE COUNTED-WAIT RULE.  `s_waitcnt vmcnt(N)` proves that an LDS-DMA request has landed only if the N operations allowed to stay in flight
// are YOUNGER LDS-DMA requests.  LDS-DMA requests retire in issue order among themselves, but stores and loads into registers retire out of
// order with respect to an older LDS-DMA request (tools/microbench/vmorder.hip: with 4 younger stores, or 4 younger register loads, vmcnt(4)
// returns while the older request's data is still on its way in > 90 % of the cases; with 4 younger LDS-DMA requests in none), so they must
// never be among the counted ones -- rounds 2-3 counted them, and were saved only by the operands having been requested a whole step earlier.
// hipcc does not know this: it models vector memory as ONE in-order queue, and behind [LDS-DMA requests, loads into registers] it guards
// `__syncthreads()` with e.g. `s_waitcnt vmcnt(2)` -- "everything but the two youngest loads" -- which proves nothing about the requests.
// Hence two forms, and tools/scan_dma_waits.py checks the compiled code of every kernel for them:
//   * wait_vmcnt<N>() with a hand-counted N, where the N youngest operations are LDS-DMA requests by construction (register loads retired
//     before, stores issued behind the wait);
//   * OPD_DMA_BARRIER(), an explicit drain and then the barrier, wherever a barrier publishes LDS-DMA data with younger register loads or
//     stores possibly in flight.
template <int N_OUTSTANDING>
__device__ __forceinline__ void wait_vmcnt() {
    static_assert(N_OUTSTANDING >= 0 && N_OUTSTANDING <= 63, "vmcnt range");
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N_OUTSTANDING) : "memory");
}
#if defined(__HIP_DEVICE_COMPILE__)
#define OPD_DMA_BARRIER()                                        \
    do {                                                         \
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");         \
        __syncthreads();                                         \
    } while (0)
#else
#define OPD_DMA_BARRIER() __syncthreads()
#endif
__device__ __forceinline__ void compiler_fence() { asm volatile("" ::: "memory"); }
// LDS reads / writes of this wave retired, then the workgroup barrier; nothing moves across it
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// ---- LDS-DMA requests: 16 bytes per lane, global -> LDS without passing through VGPRs; a wave's 64 lanes fill 1 KiB from `lds` on -------
// flat-address form
__device__ __forceinline__ void dma16(const void* gsrc, unsigned char* lds) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gsrc, (__attribute__((address_space(3))) void*)lds, 16, 0, 0);
}
// a per-lane byte offset at or beyond the end of every descriptor: the bounds check turns the request into a zero fill
constexpr unsigned DMA_ZERO_FILL = 0x80000000u;
// raw buffer descriptor of `bytes` bytes at `ptr` (stride 0: offsets are bytes, checked against `bytes`)
constexpr int BUF_RSRC_FLAGS = 0x00020000;   // descriptor word 3: DATA_FORMAT (bits 15-18) = 4, a 32-bit element; every other field 0
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buf_rsrc(const void* ptr, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(ptr), 0, bytes, BUF_RSRC_FLAGS);
}
// buffer form: per-lane offset `voff` (VGPR), wave-uniform displacement `soff` (SGPR)
__device__ __forceinline__ void dma16_buf(__amdgpu_buffer_rsrc_t rsrc, const unsigned char* lds, unsigned voff, int soff) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void*)lds, 16, voff, soff, 0, 0);
}

// ---- tile-row coordinates of the convolutions: output row m = (b, oh, ow) -> byte offset of the lane's 16-byte chunk `lchunk` at the input
//      pixel (oh * stride, ow * stride) of a descriptor based one padding (pad rows + pad pixels) BEFORE the tensor, so that tap (kh, kw) is a
//      non-negative scalar displacement; and a mask with bit kh * KW + kw set where that tap lies inside the image (rows >= M: no tap).
//      Two formulations; their arithmetic differs and each kernel keeps the one it was built and measured with. -----------------------------
// 3x3, pad 1, C1 channels, loop form (kernels_btail.hip, kernels_btail3.hip)
template <int C1>
__device__ __forceinline__ void tail_row_coords(const BtailParams& p, const int m, const int ohw, const int lchunk, unsigned& rowoff, unsigned& rowmask) {
    const bool okm = m < p.M;
    const int mm = okm ? m : 0;
    const int b = fdiv(mm, p.fd_ohw);
    const int r = mm - b * ohw;
    const int oh = fdiv(r, p.fd_ow);
    const int ow = r - oh * p.OW;
    rowoff = (unsigned)(((b * p.H + oh * p.stride) * p.W + ow * p.stride) * C1) * 2u + (unsigned)lchunk * 16u;
    unsigned kwmask = 0, mask = 0;
#pragma unroll
    for (int kw = 0; kw < 3; ++kw)
        if ((unsigned)(ow * p.stride - 1 + kw) < (unsigned)p.W) kwmask |= 1u << kw;
#pragma unroll
    for (int kh = 0; kh < 3; ++kh)
        if ((unsigned)(oh * p.stride - 1 + kh) < (unsigned)p.H) mask |= kwmask << (kh * 3);
    rowmask = okm ? mask : 0u;
}
// KH x KW, any stride / pad, closed form (kernels_gemm.hip, kernels_w8.hip).  In three pieces, for a caller with an input layout of its own:
// the stem branch of conv_gemm_dma_kernel chooses its offset between the pixel and the mask, as a conditional with both arms evaluated
// lazily -- any other arrangement compiles to other instructions (profiles/NOTES.md) ...
struct RowPixel { int b, oh, ow; };
__device__ __forceinline__ RowPixel conv_row_pixel(const ConvGemmParams& p, const int mm, const int ohw) {   // 0 <= mm < M
    const int b = fdiv(mm, p.fd_ohw);
    const int r = mm - b * ohw;
    const int oh = fdiv(r, p.fd_ow);
    const int ow = r - oh * p.OW;
    return RowPixel{b, oh, ow};
}
__device__ __forceinline__ unsigned conv_row_off(const ConvGemmParams& p, const RowPixel& px, const int lchunk) {
    return (unsigned)(((px.b * p.H + px.oh * p.stride) * p.W + px.ow * p.stride) * p.Cin) * 2u + (unsigned)lchunk * 16u;
}
// separable validity (no loops, no branches): the valid kw form a contiguous range [lo_w, hi_w], likewise kh; the row bits are
// replicated to every valid kh by a multiplication with the matching bits of p.tap_rep = sum 1 << kh*KW (opd_tap_rep)
__device__ __forceinline__ unsigned conv_tap_mask(const ConvGemmParams& p, const RowPixel& px) {
    const int iw0 = px.ow * p.stride - p.pad, ih0 = px.oh * p.stride - p.pad;
    const int lo_w = max(0, -iw0), hi_w = min(p.KW - 1, p.W - 1 - iw0);
    const int lo_h = max(0, -ih0), hi_h = min(p.KH - 1, p.H - 1 - ih0);
    auto below = [](const int n) { return n > 0 ? 0xffffffffu >> (32 - n) : 0u; };   // bits [0, n), n <= 32
    const unsigned kwmask = hi_w >= lo_w ? below(hi_w + 1) & ~below(lo_w) : 0u;
    const unsigned hsel = hi_h >= lo_h ? below((hi_h + 1) * p.KW) & ~below(lo_h * p.KW) : 0u;
    return kwmask * (p.tap_rep & hsel);
}
// ... and whole.  PW (1x1 stride 1 / linear): row m of [M][Cin]; rows >= M read zeros through the descriptor's bounds check
template <bool PW>
__device__ __forceinline__ void conv_row_coords(const ConvGemmParams& p, const int m, const int ohw, const int lchunk, unsigned& rowoff, unsigned& rowmask) {
    if constexpr (PW) {
        rowoff = m < p.M ? (unsigned)m * (unsigned)(p.Cin * 2) + (unsigned)lchunk * 16u : DMA_ZERO_FILL;
        rowmask = 1u;
        return;
    }
    const bool okm = m < p.M;
    const RowPixel px = conv_row_pixel(p, okm ? m : 0, ohw);
    rowoff = conv_row_off(p, px, lchunk);
    const unsigned mask = conv_tap_mask(p, px);   // (outside the conditional: evaluated for every row, selected afterwards)
    rowmask = okm ? mask : 0u;
}

// ---- reductions over the 64 lanes of a wave, MFMA wrapper -----------------------------------------------------------------------------------
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);   // a + b == b + a: all 64 lanes end with the same bits
    return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
// Every lane of a 16-lane row <- lane `src` (0..15) of its own row: one DPP move (row_newbcast) per dword, no LDS and no memory instruction.
// `src` must fold to a constant where the call is inlined (an unrolled loop index); all 64 lanes must be active.
__device__ __forceinline__ float row_bcast(const float v, const int src) {
#define OPD_ROW_BCAST_CASE(n) \
    case n: return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x150 + n, 0xf, 0xf, false))
    switch (src & 15) {
        OPD_ROW_BCAST_CASE(0); OPD_ROW_BCAST_CASE(1); OPD_ROW_BCAST_CASE(2); OPD_ROW_BCAST_CASE(3);
        OPD_ROW_BCAST_CASE(4); OPD_ROW_BCAST_CASE(5); OPD_ROW_BCAST_CASE(6); OPD_ROW_BCAST_CASE(7);
        OPD_ROW_BCAST_CASE(8); OPD_ROW_BCAST_CASE(9); OPD_ROW_BCAST_CASE(10); OPD_ROW_BCAST_CASE(11);
        OPD_ROW_BCAST_CASE(12); OPD_ROW_BCAST_CASE(13); OPD_ROW_BCAST_CASE(14);
        default: OPD_ROW_BCAST_CASE(15);
    }
#undef OPD_ROW_BCAST_CASE
}
__device__ __forceinline__ float4v row_bcast4(const float4v& v, const int src) {
    const float4v r = {row_bcast(v[0], src), row_bcast(v[1], src), row_bcast(v[2], src), row_bcast(v[3], src)};
    return r;
}
// Lane-packed bias of a tile's 64-channel chunks in the fused tails: lane (g, li) of set s holds the float4 that lane-row g needs for chunk
// 4 s + (li >> 2), accumulator tile li & 3; chunk j, tile nt is then row_bcast4(set j >> 2, bias_pack_lane(j, nt)).  One 16-byte load per
// lane and set for the whole tile instead of four per chunk step.
__device__ __forceinline__ int bias_pack_lane(const int j, const int nt) { return 4 * (j & 3) + nt; }

// D = A . B + C on 16 x 16 x 32 fragments of the translation unit's operand type
__device__ __forceinline__ float4v mfma16(const half8& a, const half8& b, const float4v& c) { return OPD_MFMA_16x16x32(a, b, c); }

// (host, for the launchers) grid size of a one-thread-per-element kernel
inline unsigned blocks_for(size_t n, unsigned threads) { return (unsigned)((n + threads - 1) / threads); }

}  // namespace
