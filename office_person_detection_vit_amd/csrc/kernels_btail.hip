// kernels_btail.hip — fused ResNet bottleneck tail for gfx950:   c1 (3x3) -> c2 (1x1 expand) + residual + ReLU -> c0' (1x1)
//
// SURVEY.md §8(a) row a4.  Reference arithmetic: HF:models/resnet/modeling_resnet.py:139-178 (ResNetBottleNeckLayer:
// shortcut + [1x1 reduce, 3x3, 1x1 expand] then activation), FrozenBN folded at load.
//
// In stages 1-2 of the trunk (C1 = 64 / 128 channels inside the block, C2 = 4*C1 outside) the unfused layers are HBM
// bound: the 3x3 output and the expand output each make a round trip through HBM only to be re-read by a 1x1 whose whole
// reduction dimension fits in one wave's registers.  The natural fusion boundary of a ResNet-v1.5 trunk is the INPUT of a
// 3x3 convolution (the only operator that needs a halo), so one kernel runs
//     x1 --3x3(C1->C1)+ReLU-->  a1  --1x1(C1->C2) + residual + ReLU-->  y  --1x1(C2->C3)+ReLU--> z
// where z is the NEXT block's reduce output (c0' of block i+1, or the first block of the next stage).  a1 never leaves
// registers, y is written once (it is the next residual) and never re-read for c0'.  HBM traffic per block drops from
// 1091 MB to 682 MB (stage 1, batch 8), and three launches' latency chains become one.
//
// Work decomposition: a workgroup owns 128 output pixels, wave w the 32 pixels 32w..32w+31 with ALL channels, so every
// reduction of the two 1x1s is wave-local.  MFMA orientation as in kernels_gemm.hip: weights are the A operand, pixels
// the B operand, D[row = channel][col = pixel]: lane (g = lane>>4, i = lane&15) holds channels 4g..4g+3 of pixel i.
// Channel ownership: the weight rows of every 32-channel block are STAGED into LDS in the order  LDS row 16t+4g+r <- channel 8g+4t+r
// (`own_row`; the staging offsets are per lane, so the permutation costs nothing), i.e. accumulator tile t of the block holds, in lane
// (g, i), channels 8g+4t .. +3 of pixel i.  The two tiles of a block, rounded to fp16, are then 8 CONSECUTIVE channels per lane:
// (1) they ARE the B operand of the next 16x16x32 MFMA in natural k order (no K-permuted weight copies), (2) y, z and the residual move as
// 16 bytes per lane with the four lanes of a pixel covering 64 contiguous bytes (16 pixels x 64 B per wave instruction; the accumulator
// layout of plain row order gives 8 bytes per lane, and a lane-pair exchange 32 rows x 32 B).
//
// Pipeline: the 3x3 main loop is the LDS-DMA loop of conv_gemm_dma_kernel (two stage buffers, buffer-descriptor
// staging, XOR-swizzled 128-byte rows).  It continues seamlessly into C2/64 "chunk steps": chunk j stages the 64 rows of
// W2 and the 64-column slice of W3 that chunk needs into the stage buffer the previous step has left, computes 64
// channels of y for the wave's 32 pixels, applies bias/residual/ReLU, stores them, and feeds them straight into the z
// accumulators.  The residual for chunk j+2 is fetched during chunk j; the wait that ends a chunk step counts only younger LDS-DMA
// requests (see `res_dma` below), and the step's y stores are issued behind it.
//
// Measured (tools/bench_btail.py, batch 8): stage-1 tail 188 us against 287 us for the three launches it replaces,
// stage-2 tail 135 against 170.  What does NOT move it further (each built, measured, removed):
// the residual staged through LDS by a dedicated fifth wave (SIMD imbalance: 238 us) or by one of the four waves with the
// operand staging split over the other three (190 us), whole-line y/z stores transposed through LDS (190 us), an
// input-stationary 3x3 loop on 8 x 16 pixel tiles with the halo patch of x1 in LDS (43 % fewer staged bytes: 188 us), a
// start-up stagger between workgroups sharing a CU (no phase locking), three instead of two workgroups per CU (185 vs
// 189 us).  PMC: no HBM credit stalls, the vector-memory address FIFO is full 45 % of the busy cycles.
#include "opd_kprims.h"

namespace {

constexpr int NW = 4;   // waves per workgroup = 32-pixel row groups of a tile: 128-pixel tiles, two workgroups per CU

// LDS row -> weight row (output channel) of the tails' channel ownership: bits [t][g1 g0][r1 r0] <- [g1 g0][t][r1 r0] within a 32-block
__device__ __forceinline__ int own_row(const int rho) { return (rho & ~31) | (((rho >> 2) & 3) << 3) | (((rho >> 4) & 1) << 2) | (rho & 3); }
// first of the four consecutive channels lane group g holds in accumulator tile nt
__device__ __forceinline__ int own_ch(const int nt, const int g) { return (nt >> 1) * 32 + g * 8 + (nt & 1) * 4; }

// Four 16-byte LDS reads the compiler does not see as such: in front of a `ds_read` whose address it cannot tell apart from the destinations
// of the LDS-DMA requests in flight it waits vmcnt(0), which here would drain the operand requests a chunk step has just issued.  The caller
// owns the vmcnt that proves the data has landed.  The reads and their lgkmcnt(0) are ONE statement: with the wait in a statement of its own
// the compiler is free to copy the destination registers in between, i.e. before the data has arrived.
__device__ __forceinline__ void lds_read16x4_raw(const unsigned char* const (&ptr)[4], uint4 (&r)[4]) {
    uint4v v0, v1, v2, v3;
    auto lds = [](const unsigned char* q) { return (unsigned)(size_t)(__attribute__((address_space(3))) const unsigned char*)q; };
    asm volatile("ds_read_b128 %0, %4\n\tds_read_b128 %1, %5\n\tds_read_b128 %2, %6\n\tds_read_b128 %3, %7\n\ts_waitcnt lgkmcnt(0)"
                 : "=&v"(v0), "=&v"(v1), "=&v"(v2), "=&v"(v3)
                 : "v"(lds(ptr[0])), "v"(lds(ptr[1])), "v"(lds(ptr[2])), "v"(lds(ptr[3]))
                 : "memory");
    r[0] = make_uint4(v0[0], v0[1], v0[2], v0[3]);
    r[1] = make_uint4(v1[0], v1[1], v1[2], v1[3]);
    r[2] = make_uint4(v2[0], v2[1], v2[2], v2[3]);
    r[3] = make_uint4(v3[0], v3[1], v3[2], v3[3]);
}

// RDMA = true: the residual travels global -> LDS through LDS-DMA instead of global -> VGPR.  Loads through
// VGPRs move ~16 B/clk/CU, LDS-DMA 33-42 (tools/microbench/ldpath.hip); each wave stages only ITS OWN 32 rows (four
// 8-row x 128-byte pieces per 64-channel chunk) into a wave-private quarter of two 16-KiB buffers, so no barrier and no
// special wave are involved: chunk j+2 is requested right after the wave has read chunk j out of the same buffer.
// C1 == 128 (RB1 below): the 32-KiB stage buffers leave room for ONE such buffer at two workgroups per CU, so chunk j+1 is requested right
// after chunk j has been read, and read behind a wait that counts only the operand requests issued in between (`res_dma` below).
// SC = true (first block of stage 1: C1 == 64, shortcut input of 64 channels at the output resolution): the block's 1x1 SHORTCUT
// convolution is a second GEMM into the same accumulators, y = relu(a1 . W2^T + xs . Wsc^T + (b2 + bsc)), instead of a residual
// that a separate launch wrote (274 MB at batch 8) and this kernel read back: the 64 shortcut channels of the wave's 32 pixels sit
// in 16 VGPRs as B fragments, the 64 x 64 slice of Wsc travels with the W2 / W3 chunk operands.  The shortcut is no longer
// rounded to fp16 on the way (one rounding fewer than the unfused path; the reference rounds nothing).
// SC at C1 == 128 (SC2; first block of stage 2: stride-2 3x3, shortcut input of 256 channels on the 3x3's input grid, read at (2 oh, 2 ow)):
// the same second GEMM, with the 256 channels in 64 VGPRs.  A chunk's operands (W2 16 KiB + Wsc 32 KiB + W3 16 KiB) do not fit a 32-KiB stage
// buffer, so a chunk runs as two HALF STEPS with a barrier each (see `issue_w2` / `issue_wsc_w3`): 80 KiB of LDS, two workgroups per CU.  The k
// order -- bias, a1's blocks, then the shortcut input's -- is that of the dual-source expand it replaces (Block::w2sc = [W2 | Wsc]): same bits.
// Measured (tools/bench_btail.py --sc2, batch 8): 149 us against 55 + 83 + 34 us for 3x3, dual-source expand and the next reduce.
// TRACE (tools/trace_btail.py): wave 0 stamps the shader clock at the phase boundaries and writes p.trace[blockIdx.x][16] at the end:
// {wall clock in, entry, prologue done, 3x3 loop done, chunk 0 .. NCH-1 done, stores retired, ..., [15] wall clock out}.
// RC = 1 (round 5; second block of stage 1): the residual is not read but REBUILT.  The previous block's output y' = relu(W2' . a1' + Wsc . xs +
// b') is 256 channels wide, its ingredients a1' and xs 64 each, and a 1x1 needs no halo: this kernel reads a1' and xs of its own 32 pixels per
// wave as B fragments (32 KiB per workgroup instead of the 64-KiB residual), streams the 64 x 64 slices of W2' and Wsc with its own chunk
// operands and runs the previous tail's chunk arithmetic -- same operands, same MFMA order, same fp16 rounding -- so the residual it adds has
// the bits that tail would have stored.  The previous tail then stores a1' (68 MB at batch 8) instead of y' (274 MB), and nobody reads y'.
template <int C1, int C3, bool RDMA, bool SC = false, bool TRACE = false, int RC = 0>
__global__ __launch_bounds__(64 * NW, 8 / NW) void btail_kernel(BtailParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
    unsigned long long tstamp[16] = {};
    auto stamp = [&](const int i) {
        if constexpr (TRACE) asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(tstamp[i])::"memory");
    };
    if constexpr (TRACE) asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(tstamp[0])::"memory");
    stamp(1);
    static_assert(!RDMA || C1 == 64 || C1 == 128, "residual staging buffers are budgeted for C1 == 64 and C1 == 128 (80 KiB of LDS per workgroup)");
    static_assert(!RDMA || RC == 0, "a rebuilt residual is not staged");
    static_assert(!SC || ((C1 == 64 || C1 == 128) && !RDMA), "fused shortcut: first block of stage 1 or 2; it replaces the residual");
    constexpr bool SC2 = SC && C1 == 128;      // first block of stage 2: stride-2 shortcut over 256 channels, chunk operands in half steps (below)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int C2 = 4 * C1;
    constexpr int NT1 = C1 / 16;               // c1 accumulator tiles per wave (all C1 channels)
    constexpr int KK1 = C1 / 32;               // 32-channel k-blocks of a1
    constexpr int BM = 32 * NW;                // pixels per tile
    constexpr int A_BYTES = BM * ROW_BYTES;    // BM pixels x 64 halfs
    constexpr int RC_BYTES = RC ? 2 * 64 * ROW_BYTES : 0;    // chunks of the previous block's W2 and Wsc: [64 rows][64 halfs] each
    constexpr int W1_PIECES = C1 / (8 * NW);   // 1-KiB pieces of the W1 tile per wave
    constexpr int NCH = C2 / 64;               // 64-channel chunks of y
    constexpr int W2C_BYTES = 64 * C1 * 2;     // chunk of W2: C1/64 sub-tiles of [64 rows][64 halfs]
    constexpr int W2_PIECES = W2C_BYTES / (1024 * NW);
    constexpr int W3_PIECES = C3 / (8 * NW);   // slice of W3: [C3 rows][64 halfs]
    constexpr int SC_PIECES = 8 / NW;          // a [64 rows][64 halfs] slice (Wsc; RC: the previous block's W2 and Wsc): pieces per wave
    static_assert(W1_PIECES >= 1 && W2_PIECES >= 1 && (C3 == 0 || W3_PIECES >= 1), "every wave stages at least one piece of every operand");
    constexpr int NT3 = C3 / 16;
    constexpr int WSC_BYTES = SC ? 64 * ROW_BYTES : 0;   // chunk of Wsc: [64 rows][64 halfs]
    constexpr int CHUNK_BYTES = W2C_BYTES + C3 * ROW_BYTES + WSC_BYTES + RC_BYTES;
    // a stage buffer holds a 3x3 k-step's tiles or a chunk's operands (SC2: a half step's, with the W3 slice behind the two buffers)
    constexpr int STAGE_BYTES = SC2 || (A_BYTES + C1 * ROW_BYTES) > CHUNK_BYTES ? (A_BYTES + C1 * ROW_BYTES) : CHUNK_BYTES;
    static_assert(!SC2 || 2 * STAGE_BYTES + C3 * ROW_BYTES <= 80 * 1024, "SC2 tails: at most 80 KiB of LDS, two workgroups per CU");
    static_assert(RC == 0 || (RC == 1 && C1 == 64 && !RDMA && !SC), "residual rebuild: second block of stage 1");
    // RDMA at C1 == 128: the stage buffers are 32 KiB each, which leaves room for ONE wave-private residual buffer (RB1) at two workgroups per CU
    constexpr bool RB1 = RDMA && C1 == 128;
    constexpr int RES_BUFS = RDMA ? (RB1 ? 1 : 2) : 0;
    static_assert(!RDMA || 2 * STAGE_BYTES + RES_BUFS * NW * 4096 == 80 * 1024, "RDMA tails: 80 KiB of LDS, two workgroups per CU");
    constexpr int OP_PIECES = W2_PIECES + W3_PIECES;   // LDS-DMA requests per wave of one chunk's operands (RB1 has neither SC nor RC)

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, li = lane & 15;
    // p.rev: every XCD walks its range of tiles backwards, so that a kernel starts on the rows its predecessor wrote LAST (the ones still
    // in the 256-MiB Infinity Cache; a 274-MB tensor written and re-read in the same order never hits)
    const int m_base = (p.rev ? xcd_logical_block_rev(blockIdx.x, gridDim.x) : xcd_logical_block(blockIdx.x, gridDim.x)) * BM;
    const int wm0 = m_base + wave * 32;        // this wave's 32 pixels

    // ---- staging coordinates (see conv_gemm_dma_kernel): piece = 8 tile rows x 128 B, lane -> (row lane>>3, slot lane&7)
    const int lrow = lane >> 3;
    const int lchunk = (lane & 7) ^ lrow;
    const unsigned backoff = (unsigned)(p.W + 1) * (unsigned)C1 * 2u;  // pad = 1: every in-image tap gets a non-negative offset
    const __amdgpu_buffer_rsrc_t rsrc_a = buf_rsrc(reinterpret_cast<const char*>(p.x1) - backoff, (unsigned)((size_t)p.B * p.H * p.W * C1 * 2) + backoff);
    const __amdgpu_buffer_rsrc_t rsrc_w1 = buf_rsrc(p.w1, (unsigned)(C1 * 9 * C1 * 2));
    const __amdgpu_buffer_rsrc_t rsrc_w2 = buf_rsrc(p.w2p, (unsigned)(C2 * C1 * 2));
    const __amdgpu_buffer_rsrc_t rsrc_w3 = buf_rsrc(C3 ? p.w3p : p.w2p, (unsigned)((C3 ? C3 : 1) * C2 * 2));
    const __amdgpu_buffer_rsrc_t rsrc_sc = buf_rsrc(SC ? p.wsc : RC ? p.rc_wsc : p.w2p, (unsigned)(C2 * (SC2 ? 256 : 64) * 2));
    const __amdgpu_buffer_rsrc_t rsrc_rw = buf_rsrc(RC ? p.rc_w2 : p.w2p, (unsigned)(C2 * 64 * 2));
    unsigned rowoff[4], rowmask[4], woff1[W1_PIECES], woff2[W2_PIECES], woff3[W3_PIECES ? W3_PIECES : 1], woffsc[2];
#pragma unroll
    for (int i = 0; i < 2; ++i)   // rows 8 (SC_PIECES wave + i) + lrow of the 64-row chunk
        woffsc[i] = (unsigned)(own_row(((wave * SC_PIECES + i) & 7) * 8 + lrow) * 64) * 2u + (unsigned)lchunk * 16u;
    {
        const int ohw = p.OH * p.OW;
#pragma unroll
        for (int i = 0; i < 4; ++i) tail_row_coords<C1>(p, m_base + (wave * 4 + i) * 8 + lrow, ohw, lchunk, rowoff[i], rowmask[i]);
#pragma unroll
        for (int i = 0; i < W1_PIECES; ++i)
            woff1[i] = (unsigned)(own_row((wave * W1_PIECES + i) * 8 + lrow) * (9 * C1)) * 2u + (unsigned)lchunk * 16u;
#pragma unroll
        for (int i = 0; i < W2_PIECES; ++i) {
            const int q = wave * W2_PIECES + i;   // sub-tile q>>3 (64 k each), rows 8*(q&7)..+7 of the 64-row chunk
            woff2[i] = (unsigned)(own_row((q & 7) * 8 + lrow) * C1 + (q >> 3) * 64) * 2u + (unsigned)lchunk * 16u;
        }
#pragma unroll
        for (int i = 0; i < W3_PIECES; ++i)
            woff3[i] = (unsigned)(own_row((wave * W3_PIECES + i) * 8 + lrow) * C2) * 2u + (unsigned)lchunk * 16u;
    }

    constexpr int kpc = C1 / 64;   // k-steps per filter tap
    constexpr int nk = 9 * kpc;
    int tap_kh = 0, tap_kw = 0, tap_c = 0;
    auto issue_main = [&](int ks, int buf) {
        unsigned char* As = smem + buf * STAGE_BYTES;
        unsigned char* Ws = As + A_BYTES;
        const int tap = tap_kh * 3 + tap_kw;
        const int soff_a = ((tap_kh * p.W + tap_kw) * C1 + tap_c * 64) * 2;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const unsigned vo = ((rowmask[i] >> tap) & 1u) ? rowoff[i] : DMA_ZERO_FILL;  // out of range -> zero fill
            dma16_buf(rsrc_a, As + (wave * 4 + i) * 1024, vo, soff_a);
        }
#pragma unroll
        for (int i = 0; i < W1_PIECES; ++i)
            dma16_buf(rsrc_w1, Ws + (wave * W1_PIECES + i) * 1024, woff1[i], ks * 128);
        if (++tap_c == kpc) {
            tap_c = 0;
            if (++tap_kw == 3) { tap_kw = 0; ++tap_kh; }
        }
    };
    auto issue_chunk = [&](int j, int buf) {
        unsigned char* W2s = smem + buf * STAGE_BYTES;
#pragma unroll
        for (int i = 0; i < W2_PIECES; ++i)
            dma16_buf(rsrc_w2, W2s + (wave * W2_PIECES + i) * 1024, woff2[i], j * (64 * C1 * 2));
        if constexpr (C3 > 0) {
            unsigned char* W3s = W2s + W2C_BYTES;
#pragma unroll
            for (int i = 0; i < W3_PIECES; ++i)
                dma16_buf(rsrc_w3, W3s + (wave * W3_PIECES + i) * 1024, woff3[i], j * 128);
        }
        if constexpr (SC) {
            unsigned char* Wscs = W2s + W2C_BYTES + C3 * ROW_BYTES;
#pragma unroll
            for (int i = 0; i < SC_PIECES; ++i)
                dma16_buf(rsrc_sc, Wscs + (wave * SC_PIECES + i) * 1024, woffsc[i], j * (64 * 64 * 2));
        }
        if constexpr (RC) {   // the previous block's expand and shortcut slices: [64 rows][64 k] each, rows in this kernel's ownership order
            unsigned char* Wr = W2s + W2C_BYTES + C3 * ROW_BYTES;
#pragma unroll
            for (int i = 0; i < SC_PIECES; ++i) {
                dma16_buf(rsrc_rw, Wr + (wave * SC_PIECES + i) * 1024, woffsc[i], j * (64 * 64 * 2));
                dma16_buf(rsrc_sc, Wr + 8192 + (wave * SC_PIECES + i) * 1024, woffsc[i], j * (64 * 64 * 2));
            }
        }
    };
    // y / z / residual: lane (g, li) moves 8 channels (16 B) at 8g of each 32-channel block, for its pixels li and 16 + li
    const bool pr_ok[2] = {wm0 + li < p.M, wm0 + 16 + li < p.M};
    // y: not stored at all (p.y == null: the consumer rebuilds it), or only where a stride-2 1x1 of the next stage reads it (even oh, ow)
    bool y_ok[2] = {pr_ok[0] && p.y != nullptr, pr_ok[1] && p.y != nullptr};
    if (p.y_stride2) {
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            const int m = wm0 + mt * 16 + li;
            const int r = m - fdiv(m, p.fd_ohw) * (p.OH * p.OW);
            const int oh = fdiv(r, p.fd_ow), ow = r - oh * p.OW;
            y_ok[mt] = y_ok[mt] && !((oh | ow) & 1);
        }
    }
    const size_t pr_row[2] = {(size_t)(wm0 + li) * C2 + g * 8, (size_t)(wm0 + 16 + li) * C2 + g * 8};
    // RDMA: wave-private residual staging: rows of this wave, whole 128-byte rows, swizzled like every other tile
    constexpr int RES_BUF = NW * 4096;
    unsigned char* const res_lds = smem + 2 * STAGE_BYTES + wave * 4096;   // + (j & 1) * RES_BUF for chunk j (RB1: one buffer)
    const __amdgpu_buffer_rsrc_t rsrc_r = buf_rsrc(p.res ? p.res : p.x1, p.res ? (unsigned)((size_t)p.M * C2 * 2) : 0u);   // rows >= M: zeros
    const unsigned res_voff = (unsigned)((wm0 + lrow) * C2) * 2u + (unsigned)lchunk * 16u;
    auto issue_res = [&](int j) {
#pragma unroll
        for (int i = 0; i < 4; ++i)   // (spelled out, not dma16_buf: through the function the RB1 kernels schedule three address instructions in another order)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_r, (__attribute__((address_space(3))) void*)(res_lds + (RB1 ? 0 : (j & 1) * RES_BUF) + i * 1024), 16,
                                                     res_voff + (unsigned)(i * 8 * C2 * 2), j * 128, 0, 0);
    };
    const bool has_res = RC ? true : (!SC && p.res != nullptr && !(p.dbg & 4));
    // Counted waits (the rule: opd_kprims.h -- only YOUNGER LDS-DMA requests may be among the N operations a vmcnt(N) leaves in flight).
    // Here: N = the residual pieces of chunk j + 2 when they travel by LDS-DMA, otherwise 0; and the y stores of a step are issued AFTER its
    // wait, so that a vmcnt(0) never waits for them.  The chunk steps issue no loads into registers: the biases come once per tile (`b2p`).
    // RB1 (one residual buffer): chunk j+1's pieces are requested in step j, right after chunk j has been read out of the buffer.  The barrier
    // wait of step j leaves those four in flight (wave-private, the youngest requests); the wait in front of step j+1's read leaves the
    // OP_PIECES operand requests of chunk j+2 in flight, which step j+1 has issued just before.  Nothing but LDS-DMA requests may sit among the
    // counted ones, so a step's y stores are fenced in front of its operand requests.
    const bool res_dma = RDMA && has_res;
    auto load_res = [&](int j, uint4 (&r)[4]) {
        if constexpr (RDMA) {
            if (has_res) issue_res(j);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {   // i = 2 q + mt: 32-channel block q of the chunk, pixel half mt
                r[i] = make_uint4(0u, 0u, 0u, 0u);
                if (has_res && pr_ok[i & 1]) r[i] = *reinterpret_cast<const uint4*>(p.res + pr_row[i & 1] + j * 64 + (i >> 1) * 32);
            }
        }
    };

    // ---- 3x3 main loop ------------------------------------------------------------------------------------------------
    const int ks_first = (p.dbg & 1) ? nk - 1 : 0;  // dbg: timing ablations (tools/bench_btail.py --ablate), never set by the model
    if (ks_first) { tap_kh = 2; tap_kw = 2; tap_c = kpc - 1; }
    // SC: the shortcut's input channels of this wave's 32 pixels as B fragments (k in natural order: Wsc is not permuted);
    // loaded in front of everything else, complete at the first barrier's vmcnt(0)
    half8 xs[2][2], a1p[2][2];   // RC: the same for the previous block: its shortcut input and its a1
    if constexpr ((SC && !SC2) || RC != 0) {
        const f16_t* xsrc = SC ? p.xs : p.rc_xs;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            const int m = wm0 + mt * 16 + li;
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                half8 v = {}, u = {};
                if (m < p.M) v = *reinterpret_cast<const half8*>(xsrc + (size_t)m * 64 + kk * 32 + g * 8);
                if constexpr (RC != 0)
                    if (m < p.M) u = *reinterpret_cast<const half8*>(p.rc_a1 + (size_t)m * 64 + kk * 32 + g * 8);
                xs[mt][kk] = v;
                a1p[mt][kk] = u;
            }
        }
    }
    stamp(2);
    issue_main(ks_first, ks_first & 1);
    float4v acc1[NT1][2];
#pragma unroll
    for (int nt = 0; nt < NT1; ++nt) {
        const float4v b = *reinterpret_cast<const float4v*>(p.b1 + own_ch(nt, g));
        acc1[nt][0] = b;
        acc1[nt][1] = b;
    }
    // The expand bias of the WHOLE tile, once: within a lane-row every lane needs the same 16 floats per chunk, so lane (g, li) fetches the
    // float4 of (chunk, tile) = (li >> 2, li & 3) and a chunk step takes its four from lane 4 (j & 3) + nt of its own row (row_bcast4: a DPP
    // move, no vector-memory instruction in the chunk steps).  C1 == 128: a second set for chunks 4-7.  RC: the previous block's bias likewise.
    constexpr int NB2 = NCH / 4;   // sets of four chunks
    float4v b2p[NB2], rcbp = {};
#pragma unroll
    for (int s = 0; s < NB2; ++s) b2p[s] = *reinterpret_cast<const float4v*>(p.b2 + s * 256 + (li >> 2) * 64 + own_ch(li & 3, g));
    if constexpr (RC != 0) rcbp = *reinterpret_cast<const float4v*>(p.rc_b + (li >> 2) * 64 + own_ch(li & 3, g));
    OPD_DMA_BARRIER();   // (the bias loads above are younger than the first stage's requests: the compiler's own wait would let them fly)
    uint4 res[3][4];  // residual of chunk j lives in res[j % 3], fetched two chunk steps ahead
    auto compute_main = [&](int buf) {
        const unsigned char* As = smem + buf * STAGE_BYTES;
        const unsigned char* Ws = As + A_BYTES;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            half8 xf[2], wf[NT1];
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) xf[mt] = *reinterpret_cast<const half8*>(As + swz(wave * 32 + mt * 16 + li, kk * 4 + g));
#pragma unroll
            for (int nt = 0; nt < NT1; ++nt) wf[nt] = *reinterpret_cast<const half8*>(Ws + swz(nt * 16 + li, kk * 4 + g));
#pragma unroll
            for (int nt = 0; nt < NT1; ++nt)
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) acc1[nt][mt] = OPD_MFMA_16x16x32(wf[nt], xf[mt], acc1[nt][mt]);
        }
    };
#pragma unroll 1
    for (int ks = ks_first; ks + 1 < nk; ++ks) {
        issue_main(ks + 1, (ks + 1) & 1);
        compute_main(ks & 1);
        __syncthreads();
    }
    // last k-step: the free stage buffer receives chunk 0's operands; residual chunks 0 and 1 (RB1: chunk 0) start their trip
    // SC2: the shortcut's 256 input channels of this wave's 32 pixels as B fragments, gathered at (stride oh, stride ow) of the H x W grid of
    // the previous stage's output.  Requested here, where acc1 is about to die; complete at the vmcnt(0) that ends the 3x3 loop.
    half8 xs2[2][SC2 ? 8 : 1];
    if constexpr (SC2) {
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            const int m = wm0 + mt * 16 + li;
            const int mm = m < p.M ? m : 0;   // (rows >= M: any valid pixel, never stored)
            const int b = fdiv(mm, p.fd_ohw);
            const int r = mm - b * (p.OH * p.OW);
            const int oh = fdiv(r, p.fd_ow), ow = r - oh * p.OW;
            const f16_t* src = p.xs + ((size_t)(b * p.H + oh * p.stride) * p.W + ow * p.stride) * 256 + g * 8;
#pragma unroll
            for (int kb = 0; kb < 8; ++kb) xs2[mt][kb] = *reinterpret_cast<const half8*>(src + kb * 32);
        }
    }
    // SC2 half steps.  A chunk's operands are W2 16 KiB + Wsc 32 KiB + W3 16 KiB against 32-KiB stage buffers, so chunk j runs as two steps
    // with a barrier each: the EVEN step reads W2[j] (buffer 0) while Wsc[j] (buffer 1) and the W3 slice (behind the buffers) are on their way,
    // the ODD step reads those while W2[j + 1] is.  One per-lane offset per matrix: own_row of a piece's rows is (piece part) + (lane part),
    // and the piece part is a wave-uniform displacement.
    const unsigned own_lrow = (unsigned)(8 * (lrow >> 2) + (lrow & 3));
    const unsigned voff2 = ((32u * (wave & 1) + own_lrow) * C1 + (wave >> 1) * 64u) * 2u + (unsigned)lchunk * 16u;   // wave: sub-tile wave >> 1, rows 32 (wave & 1) ..
    const unsigned voffw = (own_lrow * 256u + wave * 64u) * 2u + (unsigned)lchunk * 16u;                            // wave: the whole sub-tile `wave` of Wsc
    const unsigned voff3 = (32u * wave + own_lrow) * (unsigned)C2 * 2u + (unsigned)lchunk * 16u;                    // wave: rows 32 wave .. of W3
    auto piece_rows = [](const int i) { return 16 * (i & 1) + 4 * ((i >> 1) & 1) + 32 * (i >> 2); };                // own_row(8 i) for i < 8
    auto issue_w2 = [&](int j) {
#pragma unroll
        for (int i = 0; i < 4; ++i) dma16_buf(rsrc_w2, smem + (wave * 4 + i) * 1024, voff2, j * (64 * C1 * 2) + piece_rows(i) * C1 * 2);
    };
    auto issue_wsc_w3 = [&](int j) {
#pragma unroll
        for (int i = 0; i < 8; ++i) dma16_buf(rsrc_sc, smem + STAGE_BYTES + (wave * 8 + i) * 1024, voffw, j * (64 * 256 * 2) + piece_rows(i) * 256 * 2);
        if constexpr (C3 > 0) {
#pragma unroll
            for (int i = 0; i < 4; ++i) dma16_buf(rsrc_w3, smem + 2 * STAGE_BYTES + (wave * 4 + i) * 1024, voff3, j * 128 + piece_rows(i) * C2 * 2);
        }
    };
    if constexpr (SC2) {
        static_assert((nk & 1) == 0, "SC2: chunk 0's W2 goes into buffer 0, the one the last k-step does not read");
        issue_w2(0);
    } else {
        issue_chunk(0, nk & 1);
    }
    compiler_fence();
    if constexpr (RC == 0) {
        load_res(0, res[0]);
        if constexpr (!RB1) load_res(1, res[1]);
    }
    compiler_fence();
    compute_main((nk - 1) & 1);
    if (res_dma) wait_vmcnt<4>();   // chunk 0 operands and residual chunk 0 landed (chunk 1's 4 pieces, younger LDS-DMA requests, may still fly);
                                    // RB1: chunk 0's operands landed, its 4 residual pieces may still fly
    else wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();
    stamp(3);

    // ---- a1 = relu(c1) as fp16 B operands: k-block kk <- accumulator tiles 2kk, 2kk+1 -----------------------------------
    half8 a1[2][KK1];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int kk = 0; kk < KK1; ++kk) {
            float4v u = acc1[2 * kk][mt], v = acc1[2 * kk + 1][mt];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                u[r] = u[r] > 0.f ? u[r] : 0.f;
                v[r] = v[r] > 0.f ? v[r] : 0.f;
            }
            a1[mt][kk] = as_half8(pack2h(u[0], u[1]), pack2h(u[2], u[3]), pack2h(v[0], v[1]), pack2h(v[2], v[3]));
        }

    if (p.a1_out) {   // for the next tail, which rebuilds this block's output from it (lane (g, li): channels 32 kk + 8 g .. + 7 of its two pixels)
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int kk = 0; kk < KK1; ++kk)
                if (pr_ok[mt]) *reinterpret_cast<half8*>(p.a1_out + (size_t)(wm0 + mt * 16 + li) * C1 + kk * 32 + g * 8) = a1[mt][kk];
    }

    float4v accz[NT3 ? NT3 : 1][2];
    if constexpr (C3 > 0) {
#pragma unroll
        for (int nt = 0; nt < NT3; ++nt) {
            const float4v b = *reinterpret_cast<const float4v*>(p.b3 + own_ch(nt, g));
            accz[nt][0] = b;
            accz[nt][1] = b;
        }
    }

    // ---- chunk steps: 64 channels of y each ------------------------------------------------------------------------------
    if (p.dbg & 8) return;
    if constexpr (SC2) {
        // ---- SC2: y = relu((b2 + bsc) + W2 . a1 + Wsc . xs), k order a1's blocks then xs's (the dual-source expand's), in half steps ---------
        const unsigned char* const W2s = smem;
        const unsigned char* const Wscs = smem + STAGE_BYTES;
        const unsigned char* const W3s = smem + 2 * STAGE_BYTES;
        float4v acc2[4][2];
#pragma unroll
        for (int j = 0; j < NCH; ++j) {
            // even step: W2[j] has landed (the barrier before); buffer 1 and the W3 slice were last read before that barrier
            issue_wsc_w3(j);
            compiler_fence();
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                const float4v b = row_bcast4(b2p[j >> 2], bias_pack_lane(j, nt));
                acc2[nt][0] = b;
                acc2[nt][1] = b;
            }
#pragma unroll
            for (int kk = 0; kk < KK1; ++kk) {
                half8 wf[4];
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) wf[nt] = *reinterpret_cast<const half8*>(W2s + (kk >> 1) * 8192 + swz(nt * 16 + li, (kk & 1) * 4 + g));
#pragma unroll
                for (int nt = 0; nt < 4; ++nt)
#pragma unroll
                    for (int mt = 0; mt < 2; ++mt) acc2[nt][mt] = OPD_MFMA_16x16x32(wf[nt], a1[mt][kk], acc2[nt][mt]);
            }
            wait_vmcnt<0>();   // Wsc[j] and the W3 slice landed (and the previous step's y stores retired: nothing else is in flight)
            __builtin_amdgcn_s_barrier();
            // odd step: W2[j + 1] into buffer 0
            compiler_fence();
            if (j + 1 < NCH) issue_w2(j + 1);
            compiler_fence();
#pragma unroll
            for (int kb = 0; kb < 8; ++kb) {
                half8 wf[4];
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) wf[nt] = *reinterpret_cast<const half8*>(Wscs + (kb >> 1) * 8192 + swz(nt * 16 + li, (kb & 1) * 4 + g));
#pragma unroll
                for (int nt = 0; nt < 4; ++nt)
#pragma unroll
                    for (int mt = 0; mt < 2; ++mt) acc2[nt][mt] = OPD_MFMA_16x16x32(wf[nt], xs2[mt][kb], acc2[nt][mt]);
            }
            half8 yf[2][2];   // [q][mt]
#pragma unroll
            for (int q = 0; q < 2; ++q)
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) {
                    float4v v0 = acc2[2 * q][mt], v1 = acc2[2 * q + 1][mt];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        v0[r] = v0[r] > 0.f ? v0[r] : 0.f;
                        v1[r] = v1[r] > 0.f ? v1[r] : 0.f;
                    }
                    yf[q][mt] = as_half8(pack2h(v0[0], v0[1]), pack2h(v0[2], v0[3]), pack2h(v1[0], v1[1]), pack2h(v1[2], v1[3]));
                }
            if constexpr (C3 > 0) {
#pragma unroll
                for (int kk = 0; kk < 2; ++kk) {
#pragma unroll
                    for (int nt = 0; nt < NT3; ++nt) {
                        const half8 wf = *reinterpret_cast<const half8*>(W3s + swz(nt * 16 + li, kk * 4 + g));
#pragma unroll
                        for (int mt = 0; mt < 2; ++mt) accz[nt][mt] = OPD_MFMA_16x16x32(wf, yf[kk][mt], accz[nt][mt]);
                    }
                }
            }
            if (j + 1 < NCH) {
                wait_vmcnt<0>();   // W2[j + 1] landed
                __builtin_amdgcn_s_barrier();
            }
            // the y stores go out behind the wait: they fly during the next even step
#pragma unroll
            for (int q = 0; q < 2; ++q)
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
                    if (y_ok[mt] && !(p.dbg & 2)) *reinterpret_cast<half8*>(p.y + pr_row[mt] + j * 64 + q * 32) = yf[q][mt];
            stamp(4 + j);
        }
    }
    if constexpr (!SC2)
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        const int buf = (nk + j) & 1;
        uint4 (&res_cur)[4] = res[j % 3];
        if constexpr (RB1) compiler_fence();   // (the previous step's y stores stay in front of this step's requests: they must not be among the counted ones)
        if (j + 1 < NCH) issue_chunk(j + 1, buf ^ 1);
        compiler_fence();
        if constexpr (RDMA) {
            if (has_res) {   // paired layout out of this wave's rows of the staged chunk; then the buffer is free for chunk j+2 (RB1: j+1)
                if constexpr (RB1) {   // chunk j's pieces have landed: only the operand requests just issued are younger
                    if (j + 1 < NCH) wait_vmcnt<OP_PIECES>();
                    else wait_vmcnt<0>();
                }
                const unsigned char* src[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    src[i] = res_lds + (RB1 ? 0 : (j & 1) * RES_BUF) + swz((i & 1) * 16 + li, (i >> 1) * 4 + g);
                    if constexpr (!RB1) res_cur[i] = *reinterpret_cast<const uint4*>(src[i]);
                }
                if constexpr (RB1) {
                    lds_read16x4_raw(src, res_cur);   // (read and waited for: the buffer is free again)
                    if (j + 1 < NCH) issue_res(j + 1);
                } else {
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                    if (j + 2 < NCH) issue_res(j + 2);
                }
            }
        } else if constexpr (RC == 0) {
            if (j + 2 < NCH) load_res(j + 2, res[(j + 2) % 3]);
        }
        compiler_fence();
        const unsigned char* W2s = smem + buf * STAGE_BYTES;
        if constexpr (RC != 0) {   // the previous block's chunk, as its own tail computes it (btail_kernel<64, 64, false, SC>): bias, W2' . a1', Wsc . xs
            const unsigned char* Wr = W2s + W2C_BYTES + C3 * ROW_BYTES;
            float4v accr[4][2];
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                const float4v b = row_bcast4(rcbp, bias_pack_lane(j, nt));
                accr[nt][0] = b;
                accr[nt][1] = b;
            }
#pragma unroll
            for (int half = 0; half < 2; ++half)
#pragma unroll
                for (int kk = 0; kk < 2; ++kk) {
                    half8 wf[4];
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt) wf[nt] = *reinterpret_cast<const half8*>(Wr + half * 8192 + swz(nt * 16 + li, kk * 4 + g));
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
                        for (int mt = 0; mt < 2; ++mt) accr[nt][mt] = OPD_MFMA_16x16x32(wf[nt], half ? xs[mt][kk] : a1p[mt][kk], accr[nt][mt]);
                }
#pragma unroll
            for (int q = 0; q < 2; ++q)
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) {
                    float4v v0 = accr[2 * q][mt], v1 = accr[2 * q + 1][mt];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        v0[r] = v0[r] > 0.f ? v0[r] : 0.f;
                        v1[r] = v1[r] > 0.f ? v1[r] : 0.f;
                    }
                    res_cur[2 * q + mt] = make_uint4(pack2h(v0[0], v0[1]), pack2h(v0[2], v0[3]), pack2h(v1[0], v1[1]), pack2h(v1[2], v1[3]));
                }
        }
        float4v acc2[4][2];
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            const float4v b = row_bcast4(b2p[j >> 2], bias_pack_lane(j, nt));
            acc2[nt][0] = b;
            acc2[nt][1] = b;
        }
#pragma unroll
        for (int kk = 0; kk < KK1; ++kk) {
            half8 wf[4];
#pragma unroll
            for (int nt = 0; nt < 4; ++nt)
                wf[nt] = *reinterpret_cast<const half8*>(W2s + (kk >> 1) * 8192 + swz(nt * 16 + li, (kk & 1) * 4 + g));
#pragma unroll
            for (int nt = 0; nt < 4; ++nt)
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) acc2[nt][mt] = OPD_MFMA_16x16x32(wf[nt], a1[mt][kk], acc2[nt][mt]);
        }
        if constexpr (SC) {   // + Wsc[chunk] . xs: the block's shortcut convolution
            const unsigned char* Wscs = W2s + W2C_BYTES + C3 * ROW_BYTES;
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                half8 wf[4];
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) wf[nt] = *reinterpret_cast<const half8*>(Wscs + swz(nt * 16 + li, kk * 4 + g));
#pragma unroll
                for (int nt = 0; nt < 4; ++nt)
#pragma unroll
                    for (int mt = 0; mt < 2; ++mt) acc2[nt][mt] = OPD_MFMA_16x16x32(wf[nt], xs[mt][kk], acc2[nt][mt]);
            }
        }
        // residual, ReLU, fp16; store y; keep the fp16 values as the next B operand (block q of the chunk = k-block q of W3's slice)
        half8 yf[2][2];   // [q][mt]
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                float4v v0 = acc2[2 * q][mt], v1 = acc2[2 * q + 1][mt];
                if (has_res) {
                    const uint4 r = res_cur[2 * q + mt];
                    float a, b;
                    unpack2h(r.x, a, b); v0[0] += a; v0[1] += b;
                    unpack2h(r.y, a, b); v0[2] += a; v0[3] += b;
                    unpack2h(r.z, a, b); v1[0] += a; v1[1] += b;
                    unpack2h(r.w, a, b); v1[2] += a; v1[3] += b;
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    v0[r] = v0[r] > 0.f ? v0[r] : 0.f;
                    v1[r] = v1[r] > 0.f ? v1[r] : 0.f;
                }
                yf[q][mt] = as_half8(pack2h(v0[0], v0[1]), pack2h(v0[2], v0[3]), pack2h(v1[0], v1[1]), pack2h(v1[2], v1[3]));
            }
        if constexpr (C3 > 0) {
            const unsigned char* W3s = W2s + W2C_BYTES;
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
#pragma unroll
                for (int nt = 0; nt < NT3; ++nt) {
                    const half8 wf = *reinterpret_cast<const half8*>(W3s + swz(nt * 16 + li, kk * 4 + g));
#pragma unroll
                    for (int mt = 0; mt < 2; ++mt) accz[nt][mt] = OPD_MFMA_16x16x32(wf, yf[kk][mt], accz[nt][mt]);
                }
            }
        }
        if (j + 1 < NCH) {
            // chunk j+1's operands (requested at the top of this step) have landed; only the residual pieces of chunk j+2 (LDS-DMA requests
            // younger than the operands') may stay in flight; RB1: the pieces of chunk j+1
            if (res_dma && (RB1 || j + 2 < NCH)) wait_vmcnt<4>();
            else wait_vmcnt<0>();
            __builtin_amdgcn_s_barrier();
        }
        // the y stores go out behind the wait: they fly during the next chunk step
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
                if (y_ok[mt] && !(p.dbg & 2)) *reinterpret_cast<half8*>(p.y + pr_row[mt] + j * 64 + q * 32) = yf[q][mt];
        stamp(4 + j);
    }

    // ---- z = relu(c0') -----------------------------------------------------------------------------------------------------
    if constexpr (C3 > 0) {
#pragma unroll
        for (int q = 0; q < NT3 / 2; ++q)
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                float4v v0 = accz[2 * q][mt], v1 = accz[2 * q + 1][mt];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    v0[r] = v0[r] > 0.f ? v0[r] : 0.f;
                    v1[r] = v1[r] > 0.f ? v1[r] : 0.f;
                }
                if (pr_ok[mt] && !(p.dbg & 2))
                    *reinterpret_cast<uint4*>(p.z + (size_t)(wm0 + mt * 16 + li) * C3 + q * 32 + g * 8) =
                        make_uint4(pack2h(v0[0], v0[1]), pack2h(v0[2], v0[3]), pack2h(v1[0], v1[1]), pack2h(v1[2], v1[3]));
            }
    }
    if constexpr (TRACE) {
        stamp(4 + NCH);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        stamp(5 + NCH);
        asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(tstamp[15])::"memory");
        if (threadIdx.x == 0 && p.trace) {
#pragma unroll
            for (int i = 0; i < 16; ++i) p.trace[(size_t)blockIdx.x * 16 + i] = tstamp[i];
        }
    }
#endif
}

template <int C1, int C3, bool RDMA, bool SC = false, bool TRACE = false, int RC = 0>
hipError_t launch_btail_t(const BtailParams& p, hipStream_t stream) {
    constexpr int BM = 32 * NW;
    constexpr int MAIN = (BM + C1) * ROW_BYTES, CHUNK = 64 * C1 * 2 + C3 * ROW_BYTES + (SC ? 64 * ROW_BYTES : 0) + (RC ? 2 * 64 * ROW_BYTES : 0);
    constexpr int LDS = SC && C1 == 128 ? 2 * MAIN + C3 * ROW_BYTES                                           // half steps: the W3 slice behind the stage buffers
                                        : 2 * (MAIN > CHUNK ? MAIN : CHUNK) + (RDMA ? (C1 == 128 ? 1 : 2) * NW * 4096 : 0);   // C1 == 128: one residual buffer
    static_assert(LDS <= 160 * 1024 && (!RDMA || LDS == 80 * 1024), "LDS per workgroup");
    OPD_SET_MAX_LDS_ONCE((btail_kernel<C1, C3, RDMA, SC, TRACE, RC>), LDS);
    OPD_LAUNCH((btail_kernel<C1, C3, RDMA, SC, TRACE, RC>), dim3((p.M + BM - 1) / BM), dim3(64 * NW), LDS, stream, p);
    static const char* const kname = opd_kernel_name("btail_kernel<%d, %d, %s, %s, %s, %d>", C1, C3, OPD_BOOLSTR(RDMA), OPD_BOOLSTR(SC), OPD_BOOLSTR(TRACE), RC);
    opd_last_kernel_name = kname;
    return hipGetLastError();
}

}  // namespace

hipError_t OPD_SYM(opd_launch_btail)(const BtailParams& p_in, hipStream_t stream) {
    if (!opd_btail_supported(p_in.C1, p_in.C3) || p_in.OH <= 0 || p_in.OW <= 0) return hipErrorInvalidValue;
    BtailParams p = p_in;
    p.fd_ohw = opd_make_fastdiv((unsigned)p.OH * (unsigned)p.OW);
    p.fd_ow = opd_make_fastdiv((unsigned)p.OW);
    // 31-bit byte offsets in the buffer descriptors
    if ((size_t)p.B * p.H * p.W * p.C1 * 2 + (size_t)(p.W + 1) * p.C1 * 2 >= 0x7fffff00ull) return hipErrorInvalidValue;
    if ((size_t)p.M * p.C1 * 8 >= 0x7fffff00ull) return hipErrorInvalidValue;
    if (p.C1 == 256) return OPD_SYM(opd_launch_btail256)(p, stream);   // stage 3: kernels_btail3.hip
    if (p.y_stride2 && (p.stride != 1 || p.C3 == 0)) return hipErrorInvalidValue;   // (only next to a fused reduce: nobody else may need y)
    if (!p.y && !p.a1_out) return hipErrorInvalidValue;   // an output nobody could rebuild
    if (p.rc) {   // residual rebuilt from the previous block's a1 and shortcut input (second block of stage 1)
        if (p.rc != 1 || p.C1 != 64 || p.C3 != 64 || p.stride != 1 || p.res || p.xs || !p.rc_a1 || !p.rc_xs || !p.rc_w2 || !p.rc_wsc || !p.rc_b ||
            p.trace || (size_t)p.M * 64 * 2 >= 0x7fffff00ull)
            return hipErrorInvalidValue;
        return launch_btail_t<64, 64, false, false, false, 1>(p, stream);
    }
    if (p.xs && p.C1 == 128) {   // fused shortcut convolution: stride 2, 256 -> 512 channels next to a 128-channel 3x3 (first block of stage 2)
        if (!opd_btail_sc_supported(p.C1, p.C3, 256, p.stride) || !p.wsc || p.res || !p.y || p.a1_out || p.trace) return hipErrorInvalidValue;
        return p.C3 ? launch_btail_t<128, 128, false, true>(p, stream) : launch_btail_t<128, 0, false, true>(p, stream);
    }
    if (p.xs) {   // fused shortcut convolution: stride 1, 64 -> 256 channels next to a 64-channel 3x3 (first block of stage 1)
        if (p.C1 != 64 || p.C3 != 64 || p.stride != 1 || !p.wsc || p.res || (size_t)p.M * 64 * 2 >= 0x7fffff00ull) return hipErrorInvalidValue;
        return launch_btail_t<64, 64, false, true>(p, stream);
    }
    if (p.trace) {   // tools/trace_btail.py: the two shapes that dominate stages 1 and 2
        if (p.C1 == 64 && p.C3 == 64 && (p.dbg & 16)) return launch_btail_t<64, 64, false, false, true>(p, stream);
        if (p.C1 == 64 && p.C3 == 64) return launch_btail_t<64, 64, true, false, true>(p, stream);
        if (p.C1 == 128 && p.C3 == 128 && (p.dbg & 16)) return launch_btail_t<128, 128, false, false, true>(p, stream);
        if (p.C1 == 128 && p.C3 == 128) return launch_btail_t<128, 128, true, false, true>(p, stream);
        return hipErrorInvalidValue;
    }
    if (p.C1 == 64) {
        const bool rdma = !(p.dbg & 16);   // dbg 16: residual through VGPR loads (the first form: cross-check / timing)
        if (p.C3 == 0) return rdma ? launch_btail_t<64, 0, true>(p, stream) : launch_btail_t<64, 0, false>(p, stream);
        if (p.C3 == 64) return rdma ? launch_btail_t<64, 64, true>(p, stream) : launch_btail_t<64, 64, false>(p, stream);
        return rdma ? launch_btail_t<64, 128, true>(p, stream) : launch_btail_t<64, 128, false>(p, stream);
    }
    const bool rdma = !(p.dbg & 16);
    if (p.C3 == 0) return rdma ? launch_btail_t<128, 0, true>(p, stream) : launch_btail_t<128, 0, false>(p, stream);
    return rdma ? launch_btail_t<128, 128, true>(p, stream) : launch_btail_t<128, 128, false>(p, stream);
}
