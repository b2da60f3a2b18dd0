// opd_test_api.cpp — kernel-level test hooks (host buffers in, host buffers out).  NOT part of the drop-in boundary
// (include/opd_detr.h) and NOT part of the product library: this file is linked only into libopd_hip_test.so (csrc/build.py), which
// tests/ and tools/ load instead of libopd_hip.so, so that tests/test_kernels_gpu.py can check each hand-written kernel against the
// oracle on identical inputs.  Every kernel hook allocates its own device buffers, runs ONE kernel on the null stream and frees; the hooks of
// the kernels that order LDS-DMA by counted waits launch through launch_repeated (opd_test_util.h), which is that one launch unless
// opd_test_set_repeat turned the race screen on.
// Beside it: opd_test_bench_api.cpp (the timing and trace hooks of tools/) and opd_test_model_api.cpp (host-only helpers, and the hooks
// that reach into a model handle).
#include <string.h>

#include <algorithm>
#include <vector>

#include "opd_test_util.h"

using namespace opd;

// the launch options of the hooks below (opd_test_util.h) and their setters
int opd::g_conv_flags = 0, opd::g_gemm_ln_kloop = 0, opd::g_test_dtype = 0, opd::g_encffn_wprefetch = 0, opd::g_pos_frames = 0, opd::g_btail_dbg = 0;
TAPI int opd_test_set_encffn_wprefetch(int on) { g_encffn_wprefetch = on ? 1 : 0; return OPD_OK; }
TAPI int opd_test_set_pos_frames(int frames) { g_pos_frames = frames > 0 ? frames : 0; return OPD_OK; }
TAPI int opd_test_set_elem_bf16(int on) { g_test_dtype = on ? OPD_DT_BF16 : OPD_DT_F16; return OPD_OK; }
TAPI int opd_test_set_conv_flags(int flags) { g_conv_flags = flags; return OPD_OK; }
TAPI int opd_test_set_gemm_ln_kloop(int on) { g_gemm_ln_kloop = on ? 1 : 0; return OPD_OK; }
// opd_test_btail / opd_test_btail_repeat: the residual of the 64 / 128-channel tails through register loads (BtailParams::dbg bit 16) instead of LDS-DMA
TAPI int opd_test_set_btail_res_regs(int on) { g_btail_dbg = on ? 16 : 0; return OPD_OK; }

// ---- the race screen (opd_test_util.h: launch_repeated) ----------------------------------------------------------------------------------
// g_repeat: the repeat count of the hooks (0 = off); g_rep_launches / g_rep_diff: what the last launch_repeated did and found;
// g_rep_keep: the self-test's switch that leaves the in-place buffers as the previous repetition left them
static int g_repeat = 0, g_rep_launches = 0, g_rep_diff = 0, g_rep_keep = 0;
TAPI int opd_test_set_repeat(int reps) {
    g_repeat = reps >= 2 ? reps : 0;
    g_rep_launches = g_rep_diff = 0;
    return OPD_OK;
}
// (launches, n_diff) of the last hook call, 0 launches when that hook did not launch through launch_repeated.  The hooks that do not use it
// cannot clear the record, so the READ clears it (as does opd_test_set_repeat): a test sets the count, calls ONE hook and reads once.
TAPI int opd_test_repeat_result(int* launches, int* n_diff) {
    if (!launches || !n_diff) return fail(OPD_EINVAL, "repeat_result: null pointer");
    *launches = g_rep_launches; *n_diff = g_rep_diff;
    g_rep_launches = g_rep_diff = 0;
    return OPD_OK;
}

const char* opd::g_launch_expr = nullptr;
// launch(rep), a failure reported under the text of the launcher call that failed (LAUNCHED)
static int launch_checked(const std::function<hipError_t(int)>& launch, int rep) {
    g_launch_expr = nullptr;
    const hipError_t e = launch(rep);
    if (e == hipSuccess) return OPD_OK;
    return fail(OPD_EHIP, std::string(g_launch_expr ? g_launch_expr : "launch") + " failed: " + hipGetErrorString(e) + " (" + __FILE__ + ", repetition " +
                              std::to_string(rep) + ")");
}

int opd::launch_repeated(const std::function<hipError_t(int)>& launch, const std::vector<RepOut>& outs, const std::vector<RepInPlace>& inplace,
                         int reps) {
    if (reps == REPEAT_DEFAULT) reps = g_repeat;
    g_rep_launches = g_rep_diff = 0;
    if (reps < 2) {
        RCCHK(launch_checked(launch, 0));
        g_rep_launches = 1;
        return OPD_OK;
    }
    struct Buf { void* ptr; size_t bytes; int fill; void* pristine; };
    std::vector<Buf> bufs;
    for (const RepOut& o : outs)
        if (o.ptr && o.bytes) bufs.push_back({o.ptr, o.bytes, o.fill, nullptr});
    const size_t n_out = bufs.size();
    for (const RepInPlace& b : inplace)
        if (b.ptr && b.bytes) bufs.push_back({b.ptr, b.bytes, 0, nullptr});
    if (bufs.empty()) return fail(OPD_EINVAL, "launch_repeated: no buffer to compare");
    for (const Buf& b : bufs)
        if (b.bytes % 4) return fail(OPD_EINVAL, "launch_repeated: a buffer of " + std::to_string(b.bytes) + " bytes is no multiple of 4; the checksum would pass over its tail");
    DevMem dm;
    for (size_t i = n_out; i < bufs.size(); ++i) {
        bufs[i].pristine = dm.alloc<unsigned char>(bufs[i].bytes);
        if (bufs[i].pristine) HIPCHK(hipMemcpy(bufs[i].pristine, bufs[i].ptr, bufs[i].bytes, hipMemcpyDeviceToDevice));
    }
    const size_t noise_bytes = (size_t)256 << 20, block = bufs.size() * OPD_TAP_BLOCKS;
    unsigned char* noise = dm.alloc<unsigned char>(2 * noise_bytes);
    std::vector<unsigned long long> h((size_t)reps * block);
    unsigned long long* sums = dm.alloc<unsigned long long>(h.size());
    if (!dm.ok) return fail(OPD_ENOMEM, "test alloc failed");
    hipStream_t side = nullptr;
    HIPCHK(hipStreamCreateWithFlags(&side, hipStreamNonBlocking));
    auto run = [&]() -> int {
        for (int r = 0; r < reps; ++r) {
            for (size_t i = 0; i < bufs.size(); ++i) {
                if (i < n_out) HIPCHK(hipMemsetAsync(bufs[i].ptr, bufs[i].fill, bufs[i].bytes, nullptr));
                else if (!g_rep_keep) HIPCHK(hipMemcpyAsync(bufs[i].ptr, bufs[i].pristine, bufs[i].bytes, hipMemcpyDeviceToDevice, nullptr));
            }
            (void)hipMemcpyAsync(noise + ((r & 1) ? noise_bytes : 0), noise + ((r & 1) ? 0 : noise_bytes), noise_bytes, hipMemcpyDeviceToDevice, side);
            RCCHK(launch_checked(launch, r));
            for (size_t i = 0; i < bufs.size(); ++i)
                HIPCHK(opd_launch_checksum(bufs[i].ptr, bufs[i].bytes, sums + (size_t)r * block + i * OPD_TAP_BLOCKS, nullptr));
        }
        HIPCHK(hipDeviceSynchronize());
        return OPD_OK;
    };
    const int rc = run();
    if (rc != OPD_OK) (void)hipDeviceSynchronize();   // (nothing of this call is in flight when its buffers go)
    (void)hipStreamDestroy(side);
    RCCHK(rc);
    RCCHK(down(h.data(), sums, h.size()));
    for (int r = 1; r < reps; ++r)
        if (memcmp(h.data() + (size_t)r * block, h.data(), block * sizeof(unsigned long long)) != 0) ++g_rep_diff;
    g_rep_launches = reps;
    return OPD_OK;
}

// The screen's own test: launch_repeated on `bytes` of a fixed pattern written by plain copies instead of a kernel, with the repeat count of
// opd_test_set_repeat (>= 8).  mode 0: every repetition writes the pattern (*n_diff = 0); 1: repetition 7 differs in the buffer's last 16-bit
// value (1); 2: repetition 3 writes nothing, the 0xff refill survives (1); 3: repetitions 5 and 6 swap words 1 and 2, which share a checksum
// slot (2); 4: an IN-PLACE buffer that every launch advances from what it finds (rotates by one word): 0 because of the restore, and the hook
// runs it once more without the restore and fails unless every later repetition then differs; 5: that second run alone (reps - 1).
TAPI int opd_test_repeat_selftest(int mode, int bytes, int* n_diff) {
    if (mode < 0 || mode > 5 || bytes < 16 || !n_diff || g_repeat < 8) return fail(OPD_EINVAL, "repeat_selftest: bad arguments");
    DevMem dm;
    const size_t n = (size_t)bytes, words = (n + 3) / 4;
    std::vector<uint32_t> pat(words + 1);
    for (size_t i = 0; i < pat.size(); ++i) pat[i] = (uint32_t)(i * 2654435761u + 12345u) & 0x7f7f7f7fu;   // (no 0xff byte: the refill differs everywhere)
    pat[words] = (pat[words - 1] >> 16) ^ 1u;   // the spare word: the buffer's last 16-bit value with one bit turned
    unsigned char* src = (unsigned char*)dm.up(pat.data(), pat.size());
    unsigned char* buf = (unsigned char*)dm.up(pat.data(), pat.size());
    unsigned char* tmp = (unsigned char*)dm.alloc<uint32_t>(pat.size());
    if (!dm.ok) return fail(OPD_ENOMEM, "test alloc failed");
    auto copy = [](void* dst, const void* from, size_t count) { return hipMemcpyAsync(dst, from, count, hipMemcpyDeviceToDevice, nullptr); };
    auto write = [&](int rep) -> hipError_t {
        if (mode == 2 && rep == 3) return hipSuccess;
        hipError_t e = copy(buf, src, n);
        if (e == hipSuccess && mode == 1 && rep == 7) e = copy(buf + n - 2, src + 4 * words, 2);   // (the pattern's spare word)
        if (e == hipSuccess && mode == 3 && (rep == 5 || rep == 6)) {
            e = copy(buf + 4, src + 8, 4);
            if (e == hipSuccess) e = copy(buf + 8, src + 4, 4);
        }
        return e;
    };
    auto advance = [&](int) -> hipError_t {
        hipError_t e = copy(tmp, buf + 4, n - 4);
        if (e == hipSuccess) e = copy(tmp + n - 4, buf, 4);
        return e == hipSuccess ? copy(buf, tmp, n) : e;
    };
    int rc = OPD_OK;
    if (mode <= 3) rc = launch_repeated(write, {{buf, n, 0xff}});
    if (mode == 4) rc = launch_repeated(advance, {}, {{buf, n}});
    *n_diff = g_rep_diff;
    if (rc == OPD_OK && mode >= 4) {
        const int with_restore = g_rep_diff;
        HIPCHK(copy(buf, src, n));
        g_rep_keep = 1;
        rc = launch_repeated(advance, {}, {{buf, n}});
        g_rep_keep = 0;
        if (rc == OPD_OK && g_rep_diff != g_repeat - 1)
            return fail(OPD_ESTATE, "repeat_selftest: without the restore " + std::to_string(g_rep_diff) + " repetitions differ, not all but the first");
        if (mode == 4) g_rep_diff = with_restore;
        *n_diff = g_rep_diff;
    }
    return rc;
}

// B per-frame tables [B][rows][cols] fp32 -> one device copy and a device array of B pointers into it (bias_ptrs / pos_ptrs)
static const float* const* upload_frame_tables(DevMem& dm, const float* tables, int B, size_t rows, size_t cols, const float** first) {
    const float* d = dm.up(tables, (size_t)B * rows * cols);
    if (!d) return nullptr;
    std::vector<const float*> h((size_t)B);
    for (int b = 0; b < B; ++b) h[(size_t)b] = d + (size_t)b * rows * cols;
    *first = d;
    return dm.up(h.data(), h.size());
}
// The position shadow of opd_test_gemm_ln_deep / opd_test_enc_ffn: `pos` is one [period][256] table, or (opd_test_set_pos_frames) one per
// frame read through a device array of pointers; the single table then stays set to frame 0's, as in the model
static int upload_pos(DevMem& dm, const float* pos, int period, int M, const char* who, const float** table, const float* const** ptrs) {
    if (pos && g_pos_frames) {
        if ((size_t)g_pos_frames * period < (size_t)M) return fail(OPD_EINVAL, std::string(who) + ": fewer position tables than frames");
        *ptrs = upload_frame_tables(dm, pos, g_pos_frames, (size_t)period, 256, table);
    } else {
        *table = pos ? dm.up(pos, (size_t)period * 256) : nullptr;
    }
    return OPD_OK;
}

// x: NHWC fp16 bits [B][H][W][Cin] (stem: NHWC4); w: [N][K] fp16 bits; bias fp32 [N] (or [period][N]);
// res16/res32 optional; out fp16 bits or fp32 [M][N].
TAPI int opd_test_conv_gemm(const uint16_t* x, const uint16_t* w, const float* bias, const uint16_t* res16, const float* res32,
                            void* out, int B, int H, int W, int Cin, int OH, int OW, int N, int KH, int KW, int stride, int pad,
                            int relu, int bias_period, int out_f32, int stem) {
    DevMem dm;
    ConvGemmParams p{}; p.dtype = g_test_dtype;
    conv_geometry(p, B, H, W, Cin, OH, OW, N, KH, KW, stride, pad);
    if (stem) p.K = 256;
    const size_t MN = (size_t)p.M * N;
    p.x = dm.up(x, (size_t)B * H * W * (stem ? 4 : Cin));
    p.w = dm.up(w, (size_t)N * p.K);
    p.bias = dm.up(bias, (size_t)N * (bias_period > 0 ? bias_period : 1));
    p.res16 = res16 ? dm.up(res16, MN) : nullptr;
    p.res32 = res32 ? dm.up(res32, MN) : nullptr;
    p.out = alloc_out(dm, MN, out_f32);
    p.zero16 = zeros<uint32_t>(dm, 8);
    if (!dm.ok) return fail(OPD_ENOMEM, "test alloc failed");
    p.relu = relu; p.bias_period = bias_period; p.out_f32 = out_f32; p.stem = stem;
    apply_conv_flags(p, g_conv_flags);
    const bool w8 = g_conv_flags & (1 << 12);   // the eight-wave kernel (kernels_w8.hip)
    if (w8 && !opd_conv_w8_supported(p)) return fail(OPD_EINVAL, "conv_w8: shape outside the kernel's contract");
    RCCHK(launch_repeated([&](int) { return w8 ? LAUNCHED(opd_launch_conv_w8(p, nullptr)) : LAUNCHED(opd_launch_conv_gemm(p, nullptr)); },
                          {{p.out, MN * (out_f32 ? 4 : 2), 0xff}}));
    HIPCHK(hipDeviceSynchronize());
    return down_out(out, p.out, MN, out_f32);
}

// dual-source GEMM: out = relu( conv(x, w1; KH x KH, stride, pad) + conv1x1(x2, w2; stride2) + bias ): w1 [N][KH*KH*Cin], w2 [N][Cin2]
// (the hook concatenates them along K), out fp16 [M][N]
TAPI int opd_test_conv_dual(const uint16_t* x, const uint16_t* w1, const uint16_t* x2, const uint16_t* w2, const float* bias, uint16_t* out,
                            int B, int H, int W, int Cin, int KH, int stride, int pad, int N, int H2, int W2, int Cin2, int stride2, int relu) {
    DevMem dm;
    const int OH = (H + 2 * pad - KH) / stride + 1, OW = (W + 2 * pad - KH) / stride + 1;
    const int K1 = KH * KH * Cin, K = K1 + Cin2;
    std::vector<uint16_t> wc((size_t)N * K);
    for (int n = 0; n < N; ++n) {
        memcpy(&wc[(size_t)n * K], w1 + (size_t)n * K1, (size_t)K1 * 2);
        memcpy(&wc[(size_t)n * K + K1], w2 + (size_t)n * Cin2, (size_t)Cin2 * 2);
    }
    ConvGemmParams p{}; p.dtype = g_test_dtype;
    conv_geometry(p, B, H, W, Cin, OH, OW, N, KH, KH, stride, pad);
    p.K = K; p.K1 = K1; p.relu = relu; p.H2 = H2; p.W2 = W2; p.Cin2 = Cin2; p.stride2 = stride2;
    const size_t MN = (size_t)p.M * N;
    p.x = dm.up(x, (size_t)B * H * W * Cin);
    p.x2 = dm.up(x2, (size_t)B * H2 * W2 * Cin2);
    p.w = dm.up(wc.data(), wc.size());
    p.bias = dm.up(bias, (size_t)N);
    uint16_t* dout = dm.alloc<uint16_t>(MN);
    p.out = dout;
    p.zero16 = zeros<uint32_t>(dm, 8);
    if (!dm.ok) return fail(OPD_ENOMEM, "test alloc failed");
    apply_conv_flags(p, g_conv_flags);
    RCCHK(launch_repeated([&](int) { return LAUNCHED(opd_launch_conv_gemm(p, nullptr)); }, {{dout, MN * 2, 0xff}}));
    HIPCHK(hipDeviceSynchronize());
    return down(out, dout, MN);
}

// Split-K convolution the way the model's run_conv runs it: `splits` K slices into fp32 slabs (slab stride M * N, bias in slab 0), then
// opd_launch_reduce_act16 sums them in slice order, applies the ReLU and rounds once.  Launch options as opd_test_conv_gemm.
TAPI int opd_test_conv_splitk(const uint16_t* x, const uint16_t* w, const float* bias, uint16_t* out16, int B, int H, int W, int Cin, int OH, int OW,
                              int N, int KH, int KW, int stride, int pad, int relu, int splits) {
    if (splits < 2) return fail(OPD_EINVAL, "conv_splitk: splits must be >= 2");
    DevMem dm;
    ConvGemmParams p{}; p.dtype = g_test_dtype;
    conv_geometry(p, B, H, W, Cin, OH, OW, N, KH, KW, stride, pad);
    p.out_f32 = 1; p.relu = 0; p.split_k = splits;
    const size_t MN = (size_t)p.M * N;
    p.x = dm.up(x, (size_t)B * H * W * Cin);
    p.w = dm.up(w, (size_t)N * p.K);
    p.bias = dm.up(bias, (size_t)N);
    p.zero16 = zeros<float>(dm, (size_t)N);   // (slices > 0 take their "bias" from here)
    float* slab = dm.alloc<float>((size_t)splits * MN);
    uint16_t* dout = dm.alloc<uint16_t>(MN);
    if (!dm.ok) return fail(OPD_ENOMEM, "test alloc failed");
    p.out = slab;
    apply_conv_flags(p, g_conv_flags);
    RCCHK(launch_repeated(
        [&](int) {
            const hipError_t e = LAUNCHED(opd_launch_conv_gemm(p, nullptr));
            return e != hipSuccess ? e : LAUNCHED(opd_launch_reduce_act16(slab, splits, MN, dout, MN, relu ? 1 : 0, nullptr, g_test_dtype));
        },
        {{slab, (size_t)splits * MN * 4, 0xff}, {dout, MN * 2, 0xff}}));
    HIPCHK(hipDeviceSynchronize());
    return down(out16, dout, MN);
}

// reduce_act16_kernel alone: partials [nsplit] slabs of n floats, slab_stride floats apart (host array of (nsplit - 1) * slab_stride + n floats)
TAPI int opd_test_reduce_act16(const float* partials, int nsplit, long long slab_stride, long long n, int relu, uint16_t* out16) {
    if (nsplit < 1 || n <= 0 || slab_stride < n) return fail(OPD_EINVAL, "reduce_act16: bad arguments");
    DevMem dm;
    const float* dp = dm.up(partials, (size_t)(nsplit - 1) * slab_stride + n);
    uint16_t* dout = dm.alloc<uint16_t>((size_t)n);
    if (!dm.ok) return fail(OPD_ENOMEM, "test alloc failed");
    HIPCHK(opd_launch_reduce_act16(dp, nsplit, (size_t)slab_stride, dout, (size_t)n, relu, nullptr, g_test_dtype));
    HIPCHK(hipDeviceSynchronize());
    return down(out16, dout, (size_t)n);
}

// pointwise GEMM with two activation sources (the fused q | k | v projection): out[:, n] = (n mod alt_mod < alt_cols ? x : x_alt) . w[n] + bias[n]
TAPI int opd_test_gemm_alt(const uint16_t* x, const uint16_t* x_alt, const uint16_t* w, const float* bias, uint16_t* out16, int M, int N, int K,
                           int alt_mod, int alt_cols) {
    DevMem dm;
    ConvGemmParams p{}; p.dtype = g_test_dtype;
    pointwise_geometry(p, M, N, K);
    p.alt_mod = alt_mod; p.alt_cols = alt_cols;
    p.x = dm.up(x, (size_t)M * K);
    p.x_alt = dm.up(x_alt, (size_t)M * K);
    p.w = dm.up(w, (size_t)N * K);
    p.bias = dm.up(bias, (size_t)N);
    p.zero16 = zeros<uint32_t>(dm, 8);
    uint16_t* dout = dm.alloc<uint16_t>((size_t)M * N);
    p.out = dout;
    if (!dm.ok) return fail(OPD_ENOMEM, "test alloc failed");
    apply_conv_flags(p, g_conv_flags);
    HIPCHK(opd_launch_conv_gemm(p, nullptr));
    HIPCHK(hipDeviceSynchronize());
    return down(out16, dout, (size_t)M * N);
}

// pointwise GEMM with one row-periodic bias table PER FRAME of `period` rows (ragged batches): tables [B][period][N] fp32, B = ceil(M / period);
// the kernel reads them through a device array of B pointers (bias_ptrs), `bias` is table 0 as in the model.  out fp16 bits or fp32 [M][N].
TAPI int opd_test_gemm_frame_bias(const uint16_t* x, const uint16_t* w, const float* tables, void* out, int M, int N, int K, int period, int pmod,
                                  int pcols, int out_f32) {
    if (M <= 0 || period <= 0) return fail(OPD_EINVAL, "gemm_frame_bias: bad arguments");
    DevMem dm;
    ConvGemmParams p{}; p.dtype = g_test_dtype;
    pointwise_geometry(p, M, N, K);
    p.bias_period = period; p.bias_pmod = pmod; p.bias_pcols = pcols; p.out_f32 = out_f32;
    p.x = dm.up(x, (size_t)M * K);
    p.w = dm.up(w, (size_t)N * K);
    p.bias_ptrs = upload_frame_tables(dm, tables, (M + period - 1) / period, (size_t)period, (size_t)N, &p.bias);
    p.zero16 = zeros<uint32_t>(dm, 8);
    p.out = alloc_out(dm, (size_t)M * N, out_f32);
    if (!dm.ok) return fail(OPD_ENOMEM, "test alloc failed");
    apply_conv_flags(p, g_conv_flags);
    HIPCHK(opd_launch_conv_gemm(p, nullptr));
    HIPCHK(hipDeviceSynchronize());
    return down_out(out, p.out, (size_t)M * N, out_f32);
}

// reduce_ln256_kernel with the position shadow: y = LN(sum_z partials[z] + res) (gamma == null: the plain sum), y16 = fp16(y),
// yp16 = fp16(y + table[row / period][row % period]).  partials: nsplit slabs of M * 256 floats; pos: one [period][256] table, or
// pos_tables [B][period][256] (B > 0) read through a device array of B pointers, with table 0 as `pos`.
TAPI int opd_test_reduce_ln_pos(const float* partials, int nsplit, const float* res32, const float* gamma, const float* beta, const float* pos,
                                const float* pos_tables, int B, int period, float* y, uint16_t* y16, uint16_t* yp16, int M) {
    if (M <= 0 || nsplit < 1 || period <= 0 || (!pos && !pos_tables) || (pos_tables && (size_t)B * period < (size_t)M))
        return fail(OPD_EINVAL, "reduce_ln_pos: bad arguments");
    DevMem dm;
    const size_t MN = (size_t)M * 256;
    const float* dp = dm.up(partials, (size_t)nsplit * MN);
    const float* dres = res32 ? dm.up(res32, MN) : nullptr;
    const float* dg = gamma ? dm.up(gamma, 256) : nullptr;
    const float* db = beta ? dm.up(beta, 256) : nullptr;
    const float* dpos = nullptr;
    const float* const* dptrs = nullptr;
    if (pos_tables) dptrs = upload_frame_tables(dm, pos_tables, B, (size_t)period, 256, &dpos);
    else dpos = dm.up(pos, (size_t)period * 256);
    float* dy = dm.alloc<float>(MN);
    uint16_t* dy16 = dm.alloc<uint16_t>(MN);
    uint16_t* dyp16 = dm.alloc<uint16_t>(MN);
    if (!dm.ok) return fail(OPD_ENOMEM, "test alloc failed");
    HIPCHK(opd_launch_reduce_ln_pos(dp, nsplit, MN, dres, dg, db, dy, dy16, M, dpos, dptrs, period, dyp16, nullptr, g_test_dtype));
    HIPCHK(hipDeviceSynchronize());
    RCCHK(down(y, dy, MN));
    RCCHK(down(y16, dy16, MN));
    return down(yp16, dyp16, MN);
}

// split-K linear + fused reduce / residual / LayerNorm: y = LN(x.W^T + bias + res) (gamma == null: no LN), N == 256
TAPI int opd_test_gemm_splitk_ln(const uint16_t* x, const uint16_t* w, const float* bias, const float* res32, const float* gamma,
                                 const float* beta, float* y, uint16_t* y16, int M, int K, int splits) {
    DevMem dm;
    const int N = 256;
    const size_t MN = (size_t)M * N;
    ConvGemmParams p{}; p.dtype = g_test_dtype;
    pointwise_geometry(p, M, N, K);
    p.out_f32 = 1; p.split_k = splits;
    p.x = dm.up(x, (size_t)M * K);
    p.w = dm.up(w, (size_t)N * K);
    p.bias = dm.up(bias, N);
    p.zero16 = zeros<float>(dm, N);   // (slices > 0 take their "bias" from here)
    float* slab = dm.alloc<float>((size_t)splits * MN);
    const float* dres = res32 ? dm.up(res32, MN) : nullptr;
    const float* dg = gamma ? dm.up(gamma, N) : nullptr;
    const float* db = beta ? dm.up(beta, N) : nullptr;
    float* dy = dm.alloc<float>(MN);
    uint16_t* dy16 = dm.alloc<uint16_t>(MN);
    if (!dm.ok) return fail(OPD_ENOMEM, "test alloc failed");
    p.out = slab;
    RCCHK(launch_repeated(
        [&](int) {
            const hipError_t e = LAUNCHED(opd_launch_conv_gemm(p, nullptr));
            return e != hipSuccess ? e : LAUNCHED(opd_launch_reduce_ln(slab, splits, MN, dres, dg, db, dy, dy16, M, nullptr, g_test_dtype));
        },
        {{slab, (size_t)splits * MN * 4, 0xff}, {dy, MN * 4, 0xff}, {dy16, MN * 2, 0xff}}));
    HIPCHK(hipDeviceSynchronize());
    RCCHK(down(y, dy, MN));
    return down(y16, dy16, MN);
}

// fused Linear(K->256) + bias + residual + LayerNorm (kernels_rowln.hip)
TAPI int opd_test_gemm_ln(const uint16_t* x, const uint16_t* w, const float* bias, const float* res32, const float* gamma,
                          const float* beta, float* y, uint16_t* y16, int M, int K) {
    DevMem dm;
    const size_t MN = (size_t)M * 256;
    GemmLnParams p{}; p.dtype = g_test_dtype;
    p.x = dm.up(x, (size_t)M * K);
    p.w = dm.up(w, (size_t)256 * K);
    p.bias = dm.up(bias, 256);
    p.res32 = res32 ? dm.up(res32, MN) : nullptr;
    p.gamma = dm.up(gamma, 256);
    p.beta = dm.up(beta, 256);
    p.y32 = dm.alloc<float>(MN);
    p.y16 = dm.alloc<uint16_t>(MN);
    if (!dm.ok) return fail(OPD_ENOMEM, "test alloc failed");
    p.M = M; p.K = K; p.kloop = g_gemm_ln_kloop;
    RCCHK(launch_repeated([&](int) { return LAUNCHED(opd_launch_gemm_ln(p, nullptr)); }, {{p.y32, MN * 4, 0xff}, {p.y16, MN * 2, 0xff}}));
    HIPCHK(hipDeviceSynchronize());
    RCCHK(down(y, p.y32, MN));
    return down(y16, p.y16, MN);
}

// deep-K row-owner form (gemm_ln256_ring_kernel) with the optional position shadow: pos [period][256] fp32, yp16 = fp16(y + pos[row % period])
TAPI int opd_test_gemm_ln_deep(const uint16_t* x, const uint16_t* w, const float* bias, const float* res32, const float* gamma, const float* beta,
                               const float* pos, int period, float* y, uint16_t* y16, uint16_t* yp16, int M, int K, int in_place) {
    DevMem dm;
    const size_t MN = (size_t)M * 256;
    GemmLnParams p{}; p.dtype = g_test_dtype;
    p.x = dm.up(x, (size_t)M * K);
    p.w = dm.up(w, (size_t)256 * K);
    p.bias = dm.up(bias, 256);
    float* res = res32 ? dm.up(res32, MN) : nullptr;
    p.res32 = res;
    p.gamma = gamma ? dm.up(gamma, 256) : nullptr;   // null: no LayerNorm (the input projection)
    p.beta = beta ? dm.up(beta, 256) : nullptr;
    p.y32 = (in_place && res) ? res : dm.alloc<float>(MN);   // the model writes the residual stream in place
    p.y16 = dm.alloc<uint16_t>(MN);
    RCCHK(upload_pos(dm, pos, period, M, "gemm_ln_deep", &p.pos, &p.pos_ptrs));
    p.pos_period = period;
    p.yp16 = pos ? dm.alloc<uint16_t>(MN) : nullptr;
    if (!dm.ok) return fail(OPD_ENOMEM, "test alloc failed");
    p.M = M; p.K = K; p.deep_k = 1;
    const bool alias = p.y32 == res;   // (in place: the launch reads the residual stream it overwrites)
    RCCHK(launch_repeated([&](int) { return LAUNCHED(opd_launch_gemm_ln(p, nullptr)); },
                          {{alias ? nullptr : p.y32, MN * 4, 0xff}, {p.y16, MN * 2, 0xff}, {p.yp16, MN * 2, 0xff}},
                          {{alias ? p.y32 : nullptr, MN * 4}}));
    HIPCHK(hipDeviceSynchronize());
    RCCHK(down(y, p.y32, MN));
    RCCHK(down(y16, p.y16, MN));
    return pos ? down(yp16, p.yp16, MN) : OPD_OK;
}

// the encoder's FFN block in one launch (enc_ffn_kernel): x [M][256], w1 [F][256], w2 [256][F] as 16-bit elements of the current test element
// type, b1 [F], b2 / gamma / beta [256], res32 [M][256]; y = LayerNorm(res32 + relu(x . w1^T + b1) . w2^T + b2); optional position shadow as in
// opd_test_gemm_ln_deep.  in_place: y32 aliases res32 and y16 aliases x, as in the model.  Optional tail projection: wt [tail * 256][256],
// tail_bias [tail * 256], the first tail_pos passes on y + pos; tail_out [M][tail * 256] (pass t at columns 256 t).  Optional FRONT phase
// (wo != null): x is the ATTENTION output; x' = LayerNorm1(res32 + x . wo^T + bo) * g1 + be1 is computed inside, returned in x1_out [M][256]
// (fp32), and the FFN runs on fp16(x') with the residual x' (always in place on res32 then).
TAPI int opd_test_enc_ffn(const uint16_t* x, const uint16_t* w1, const float* b1, const uint16_t* w2, const float* b2, const float* res32, const float* gamma,
                          const float* beta, const float* pos, int period, float* y, uint16_t* y16, uint16_t* yp16, int M, int F, int in_place,
                          const uint16_t* wt, const float* tail_bias, int tail, int tail_pos, uint16_t* tail_out, const uint16_t* wo, const float* bo,
                          const float* g1, const float* be1, int pack_front) {
    if (M <= 0 || F <= 0 || F % 128 || tail < 0 || tail > 16) return fail(OPD_EINVAL, "enc_ffn: F must be a multiple of 128, tail <= 16");
    if (wo && !pack_front) return fail(OPD_EINVAL, "enc_ffn: the front phase needs a stream packed with it");
    DevMem dm;
    const size_t MN = (size_t)M * 256;
    std::vector<unsigned char> pk(opd_encffn_pack_bytes(F, tail, pack_front));
    std::vector<uint16_t> wo_dummy((size_t)256 * 256, 0);
    opd_encffn_pack(w1, b1, w2, F, wt, tail_bias, tail, pack_front ? (wo ? wo : wo_dummy.data()) : nullptr, pk.data());
    EncFfnParams p{}; p.dtype = g_test_dtype;
    uint16_t* dx = dm.up(x, MN);
    float* res = dm.up(res32, MN);
    p.wpack = dm.up(pk.data(), pk.size()); p.b2 = dm.up(b2, 256); p.res32 = res; p.gamma = dm.up(gamma, 256); p.beta = dm.up(beta, 256);
    p.pack_front = pack_front;
    if (wo) {
        p.attn = dx; p.bo = dm.up(bo, 256); p.gamma1 = dm.up(g1, 256); p.beta1 = dm.up(be1, 256);
        in_place = 1;
    } else {
        p.x = dx;
    }
    p.y32 = in_place ? res : dm.alloc<float>(MN);
    p.y16 = (in_place && !wo) ? dx : dm.alloc<uint16_t>(MN);
    RCCHK(upload_pos(dm, pos, period, M, "enc_ffn", &p.pos, &p.pos_ptrs));   // per-frame tables as in opd_test_gemm_ln_deep
    p.pos_period = period;
    p.wprefetch = g_encffn_wprefetch;
    p.yp16 = pos ? dm.alloc<uint16_t>(MN) : nullptr;
    p.M = M; p.F = F; p.pack_tail = tail; p.tail = tail; p.tail_pos = tail_pos;
    if (tail) {
        p.tail_ld = tail * 256;
        p.tail_out = dm.alloc<uint16_t>((size_t)M * p.tail_ld);
        for (int t = 0; t < tail; ++t) p.tail_col[t] = 256 * t;
    }
    if (!dm.ok) return fail(OPD_ENOMEM, "test alloc failed");
    const bool a32 = p.y32 == res, a16 = p.y16 == dx;   // (in place: the launch reads what it overwrites)
    RCCHK(launch_repeated([&](int) { return LAUNCHED(opd_launch_enc_ffn(p, nullptr)); },
                          {{a32 ? nullptr : p.y32, MN * 4, 0xff}, {a16 ? nullptr : p.y16, MN * 2, 0xff}, {p.yp16, MN * 2, 0xff},
                           {p.tail_out, (size_t)M * p.tail_ld * 2, 0xff}},
                          {{a32 ? p.y32 : nullptr, MN * 4}, {a16 ? p.y16 : nullptr, MN * 2}}));
    HIPCHK(hipDeviceSynchronize());
    RCCHK(down(y, p.y32, MN));
    RCCHK(down(y16, p.y16, MN));
    if (pos) RCCHK(down(yp16, p.yp16, MN));
    return tail ? down(tail_out, p.tail_out, (size_t)M * p.tail_ld) : OPD_OK;
}

TAPI int opd_test_gemm_k256(const uint16_t* x, const uint16_t* w, const float* bias, uint16_t* out16, float* out32, int M, int N,
                            int K, int bias_period, int relu) {
    DevMem dm;
    const size_t MN = (size_t)M * N;
    GemmK256Params p{}; p.dtype = g_test_dtype;
    const int slices = K / 256;
    if (slices > 1 && N != 256) return fail(OPD_EINVAL, "sliced test needs N == 256");
    p.x = dm.up(x, (size_t)M * K);
    p.w = dm.up(w, (size_t)N * K);
    p.bias = dm.up(bias, (size_t)N * (bias_period > 0 ? bias_period : 1));
    p.out16 = slices == 1 ? dm.alloc<uint16_t>(MN) : nullptr;
    p.out32 = slices > 1 ? dm.alloc<float>((size_t)slices * MN) : nullptr;
    float* sum = slices > 1 ? dm.alloc<float>(MN) : nullptr;
    if (!dm.ok) return fail(OPD_ENOMEM, "test alloc failed");
    p.M = M; p.N = N; p.ldx = K; p.ldw = K; p.slices = slices; p.bias_period = bias_period; p.relu = relu;
    RCCHK(launch_repeated(
        [&](int) {
            const hipError_t e = LAUNCHED(opd_launch_gemm_k256(p, nullptr));
            if (e != hipSuccess || slices == 1) return e;
            return LAUNCHED(opd_launch_reduce_ln(p.out32, slices, MN, nullptr, nullptr, nullptr, sum, nullptr, M, nullptr));
        },
        {{p.out16, MN * 2, 0xff}, {p.out32, (size_t)slices * MN * 4, 0xff}, {sum, MN * 4, 0xff}}));
    HIPCHK(hipDeviceSynchronize());
    return slices > 1 ? down(out32, sum, MN) : down(out16, p.out16, MN);
}

// fused bottleneck tail vs. the caller's reference: x1 [B][H][W][C1], w1 [C1][3][3][C1], w2 [4*C1][C1], w3 [C3][4*C1]
// (plain K order: btail_weights applies opd_permute_k32 where the kernel wants it), res [M][4*C1] or null; outputs y [M][4*C1], z [M][C3] (C3 > 0).
TAPI int opd_test_btail(const uint16_t* x1, const uint16_t* w1, const float* b1, const uint16_t* w2, const float* b2,
                        const uint16_t* res, const uint16_t* w3, const float* b3, uint16_t* y, uint16_t* z, int B, int H, int W,
                        int C1, int C3, int stride) {
    if (!opd_btail_supported(C1, C3)) return fail(OPD_EINVAL, "btail: unsupported (C1, C3)");
    DevMem dm;
    const int C2 = 4 * C1;
    BtailParams p{}; p.dtype = g_test_dtype;
    btail_geometry(p, B, H, W, stride, C1, C3);
    p.dbg = g_btail_dbg;
    const size_t M = (size_t)p.M;
    p.x1 = dm.up(x1, (size_t)B * H * W * C1);
    p.w1 = dm.up(w1, (size_t)C1 * 9 * C1);
    p.b1 = dm.up(b1, C1);
    btail_weights(dm, p, C1, C3, w2, w3);
    p.b2 = dm.up(b2, C2);
    p.res = res ? dm.up(res, M * C2) : nullptr;
    p.y = dm.alloc<uint16_t>(M * C2);
    p.b3 = C3 ? dm.up(b3, C3) : nullptr;
    p.z = C3 ? dm.alloc<uint16_t>(M * C3) : nullptr;
    if (!dm.ok) return fail(OPD_ENOMEM, "test alloc failed");
    RCCHK(launch_repeated([&](int) { return LAUNCHED(opd_launch_btail(p, nullptr)); }, {{p.y, M * C2 * 2, 0xff}, {p.z, M * C3 * 2, 0xff}}));
    HIPCHK(hipDeviceSynchronize());
    RCCHK(down(y, p.y, M * C2));
    return C3 ? down(z, p.z, M * C3) : OPD_OK;
}

// Race screen for the fused tails (the stage-3 kernel reads LDS-DMA data by counted waits and raw barriers: a misplaced wait shows as a
// rare wrong tile that comes and goes with timing): `reps` launches on the same device-resident operands, position-weighted checksums of
// y and z after each, *n_diff = number of launches whose checksums differ from the first launch's.  A second stream keeps the memory system
// busy meanwhile (a 256-MiB device-to-device copy per launch) so that DMA latencies vary between launches.
TAPI int opd_test_btail_repeat(const uint16_t* x1, const uint16_t* w1, const float* b1, const uint16_t* w2, const float* b2, const uint16_t* res,
                               const uint16_t* w3, const float* b3, int B, int H, int W, int C1, int C3, int reps, int* n_diff) {
    if (!opd_btail_supported(C1, C3) || !C3 || reps < 2 || !n_diff) return fail(OPD_EINVAL, "btail_repeat: bad arguments");
    DevMem dm;
    const int C2 = 4 * C1;
    const size_t M = (size_t)B * H * W;
    BtailParams p{}; p.dtype = g_test_dtype;
    btail_geometry(p, B, H, W, 1, C1, C3);
    p.dbg = g_btail_dbg;
    p.x1 = dm.up(x1, M * C1); p.w1 = dm.up(w1, (size_t)C1 * 9 * C1); p.b1 = dm.up(b1, C1);
    btail_weights(dm, p, C1, C3, w2, w3);
    p.b2 = dm.up(b2, C2); p.res = dm.up(res, M * C2); p.y = dm.alloc<uint16_t>(M * C2);
    p.b3 = dm.up(b3, C3); p.z = dm.alloc<uint16_t>(M * C3);
    if (!dm.ok) return fail(OPD_ENOMEM, "test alloc failed");
    // (the tile walk alternates between repetitions: the outputs do not depend on it, the timing of every tile does)
    RCCHK(launch_repeated([&](int rep) { p.rev = rep & 1; return LAUNCHED(opd_launch_btail(p, nullptr)); }, {{p.y, M * C2 * 2, 0xff}, {p.z, M * C3 * 2, 0xff}}, {},
                          reps));
    *n_diff = g_rep_diff;
    return OPD_OK;
}

// fused tail WITH the block's shortcut convolution inside (first block of stage 1): xs [M][64] = the shortcut's input at the output
// resolution, wsc [256][64]; b2sc = b2 + the shortcut's bias.  C1 = 64, C3 = 64, stride 1.
TAPI int opd_test_btail_sc(const uint16_t* x1, const uint16_t* w1, const float* b1, const uint16_t* w2, const float* b2sc, const uint16_t* xs,
                           const uint16_t* wsc, const uint16_t* w3, const float* b3, uint16_t* y, uint16_t* z, int B, int H, int W) {
    DevMem dm;
    const int C1 = 64, C2 = 256, C3 = 64;
    const size_t M = (size_t)B * H * W;
    BtailParams p{}; p.dtype = g_test_dtype;
    btail_geometry(p, B, H, W, 1, C1, C3);
    p.x1 = dm.up(x1, M * C1);
    p.w1 = dm.up(w1, (size_t)C1 * 9 * C1);
    p.b1 = dm.up(b1, C1);
    btail_weights(dm, p, C1, C3, w2, w3);
    p.b2 = dm.up(b2sc, C2);
    p.xs = dm.up(xs, M * 64);
    p.wsc = dm.up(wsc, (size_t)C2 * 64);
    p.y = dm.alloc<uint16_t>(M * C2);
    p.b3 = dm.up(b3, C3);
    p.z = dm.alloc<uint16_t>(M * C3);
    if (!dm.ok) return fail(OPD_ENOMEM, "test alloc failed");
    RCCHK(launch_repeated([&](int) { return LAUNCHED(opd_launch_btail(p, nullptr)); }, {{p.y, M * C2 * 2, 0xff}, {p.z, M * C3 * 2, 0xff}}));
    HIPCHK(hipDeviceSynchronize());
    RCCHK(down(y, p.y, M * C2));
    return down(z, p.z, M * C3);
}

// ... and the first block of stage 2 (kernels_btail.hip, SC2): x1 [B][H][W][128] under a stride-2 3x3, xs [B][H][W][256] = the shortcut's input on
// the same grid (read at (2 oh, 2 ow)), wsc [512][256]; b2sc = b2 + the shortcut's bias.  C3 = 128, or 0: no z.
TAPI int opd_test_btail_sc2(const uint16_t* x1, const uint16_t* w1, const float* b1, const uint16_t* w2, const float* b2sc, const uint16_t* xs,
                            const uint16_t* wsc, const uint16_t* w3, const float* b3, uint16_t* y, uint16_t* z, int B, int H, int W, int C3) {
    const int C1 = 128, C2 = 512, Csc = 256;
    if (!opd_btail_sc_supported(C1, C3, Csc, 2) || B < 1 || H < 1 || W < 1) return fail(OPD_EINVAL, "btail_sc2: unsupported C3 or shape");
    DevMem dm;
    BtailParams p{}; p.dtype = g_test_dtype;
    btail_geometry(p, B, H, W, 2, C1, C3);
    const size_t M = (size_t)p.M, HW = (size_t)B * H * W;
    p.x1 = dm.up(x1, HW * C1);
    p.w1 = dm.up(w1, (size_t)C1 * 9 * C1);
    p.b1 = dm.up(b1, C1);
    btail_weights(dm, p, C1, C3, w2, w3);
    p.b2 = dm.up(b2sc, C2);
    p.xs = dm.up(xs, HW * Csc);
    p.wsc = dm.up(wsc, (size_t)C2 * Csc);
    p.y = dm.alloc<uint16_t>(M * C2);
    p.b3 = C3 ? dm.up(b3, C3) : nullptr;
    p.z = C3 ? dm.alloc<uint16_t>(M * C3) : nullptr;
    if (!dm.ok) return fail(OPD_ENOMEM, "test alloc failed");
    RCCHK(launch_repeated([&](int rep) { p.rev = rep & 1; return LAUNCHED(opd_launch_btail(p, nullptr)); }, {{p.y, M * C2 * 2, 0xff}, {p.z, M * C3 * 2, 0xff}}));
    HIPCHK(hipDeviceSynchronize());
    RCCHK(down(y, p.y, M * C2));
    return C3 ? down(z, p.z, M * C3) : OPD_OK;
}

// Stage 1's first two tails and its last one, both ways (kernels_btail.hip, round 5).  Blocks a (shortcut inside), b, c on x1 [B][H][W][64] /
// xs [M][64]; weights as in opd_test_btail_sc / opd_test_btail (w3a, w3b: [64][256], w3c: [128][256]).
//   old: tail a stores y_a -> tail b reads it back as its residual -> tail c stores all of y_c;
//   new: tail a stores a1 only -> tail b REBUILDS y_a (rc = 1) -> tail c stores y_c at even (oh, ow) only (y_stride2; the buffer is pre-filled
//        with `fill` so the caller sees what was not written).
// Outputs: yb / zb [M][256] / [M][64], yc / zc [M][256] / [M][128], once per route (index 0 old, 1 new).
TAPI int opd_test_btail_chain(const uint16_t* x1, const uint16_t* xs, const uint16_t* const* w1, const float* const* b1, const uint16_t* const* w2,
                              const float* const* b2, const uint16_t* wsc, const uint16_t* const* w3, const float* const* b3, uint16_t* const* yb,
                              uint16_t* const* zb, uint16_t* const* yc, uint16_t* const* zc, int B, int H, int W, int fill) {
    DevMem dm;
    const size_t M = (size_t)B * H * W;
    const uint16_t* d_x1 = dm.up(x1, M * 64);
    const uint16_t* d_xs = dm.up(xs, M * 64);
    const uint16_t* d_wsc = dm.up(wsc, (size_t)256 * 64);
    const uint16_t *d_w1[3], *d_w2[3], *d_w3[3];
    const float *d_b1[3], *d_b2[3], *d_b3[3];
    for (int i = 0; i < 3; ++i) {
        const int c3 = i == 2 ? 128 : 64;
        d_w1[i] = dm.up(w1[i], (size_t)64 * 9 * 64); d_b1[i] = dm.up(b1[i], 64);
        d_w2[i] = dm.up(w2[i], (size_t)256 * 64); d_b2[i] = dm.up(b2[i], 256);
        d_w3[i] = dm.up(w3[i], (size_t)c3 * 256); d_b3[i] = dm.up(b3[i], c3);
    }
    uint16_t* ya = dm.alloc<uint16_t>(M * 256);
    uint16_t* za = dm.alloc<uint16_t>(M * 64);
    uint16_t* a1a = dm.alloc<uint16_t>(M * 64);
    uint16_t* d_yb = dm.alloc<uint16_t>(M * 256);
    uint16_t* d_zb = dm.alloc<uint16_t>(M * 64);
    uint16_t* d_yc = dm.alloc<uint16_t>(M * 256);
    uint16_t* d_zc = dm.alloc<uint16_t>(M * 128);
    if (!dm.ok) return fail(OPD_ENOMEM, "test alloc failed");
    for (int route = 0; route < 2; ++route) {
        HIPCHK(hipMemset(ya, 0xEE, M * 256 * 2));
        HIPCHK(hipMemset(d_yc, fill, M * 256 * 2));
        auto base = [&](int i, const uint16_t* in, uint16_t* y, uint16_t* z, int c3) {
            BtailParams p{}; p.dtype = g_test_dtype;
            p.x1 = in; p.w1 = d_w1[i]; p.b1 = d_b1[i]; p.w2p = d_w2[i]; p.b2 = d_b2[i]; p.y = y; p.w3p = d_w3[i]; p.b3 = d_b3[i]; p.z = z;
            btail_geometry(p, B, H, W, 1, 64, c3);
            return p;
        };
        BtailParams pa = base(0, d_x1, ya, za, 64);
        pa.xs = d_xs; pa.wsc = d_wsc;
        if (route) { pa.y = nullptr; pa.a1_out = a1a; }
        HIPCHK(opd_launch_btail(pa, nullptr));
        BtailParams pb = base(1, za, d_yb, d_zb, 64);
        if (route) { pb.rc = 1; pb.rc_a1 = a1a; pb.rc_xs = d_xs; pb.rc_w2 = d_w2[0]; pb.rc_wsc = d_wsc; pb.rc_b = d_b2[0]; }
        else pb.res = ya;
        HIPCHK(opd_launch_btail(pb, nullptr));
        BtailParams pc = base(2, d_zb, d_yc, d_zc, 128);
        pc.y_stride2 = route;
        pc.res = d_yb;
        HIPCHK(opd_launch_btail(pc, nullptr));
        HIPCHK(hipDeviceSynchronize());
        RCCHK(down(yb[route], d_yb, M * 256));
        RCCHK(down(zb[route], d_zb, M * 64));
        RCCHK(down(yc[route], d_yc, M * 256));
        RCCHK(down(zc[route], d_zc, M * 128));
    }
    return OPD_OK;
}

// attention on q [B][Lq][D], k / v [B][Lk][D], D = heads * 32; key_valid (nullable): the per-frame key mask of opd_test_attention_masked
static int attention_params(DevMem& dm, AttnParams& p, const uint16_t* q, const uint16_t* k, const uint16_t* v, int B, int heads, int Lq, int Lk,
                            float scale, const int32_t* key_valid, int key_row) {
    const int D = heads * 32;
    p.dtype = g_test_dtype;
    p.q = dm.up(q, (size_t)B * Lq * D);
    p.k = dm.up(k, (size_t)B * Lk * D);
    p.v = dm.up(v, (size_t)B * Lk * D);
    p.key_valid = key_valid ? dm.up(key_valid, (size_t)B * 2) : nullptr;
    p.B = B; p.heads = heads; p.Lq = Lq; p.Lk = Lk; p.ldq = p.ldk = p.ldv = p.ldo = D; p.scale = scale; p.key_row = key_row;
    return D;
}
static int run_attention(const uint16_t* q, const uint16_t* k, const uint16_t* v, uint16_t* o, int B, int heads, int Lq, int Lk, float scale,
                         const int32_t* key_valid, int key_row) {
    DevMem dm;
    AttnParams p{};
    const size_t n = (size_t)B * Lq * attention_params(dm, p, q, k, v, B, heads, Lq, Lk, scale, key_valid, key_row);
    p.o = dm.alloc<uint16_t>(n);
    if (!dm.ok) return fail(OPD_ENOMEM, "test alloc failed");
    RCCHK(launch_repeated([&](int) { return LAUNCHED(opd_launch_attention(p, nullptr)); }, {{p.o, n * 2, 0xff}}));
    HIPCHK(hipDeviceSynchronize());
    return down(o, p.o, n);
}
TAPI int opd_test_attention(const uint16_t* q, const uint16_t* k, const uint16_t* v, uint16_t* o, int B, int heads, int Lq, int Lk,
                            float scale) {
    return run_attention(q, k, v, o, B, heads, Lq, Lk, scale, nullptr, 0);
}
// attention with a per-frame key mask: key k = (k / key_row, k % key_row) is valid inside key_valid[b] = (rows, cols)
TAPI int opd_test_attention_masked(const uint16_t* q, const uint16_t* k, const uint16_t* v, uint16_t* o, int B, int heads, int Lq,
                                   int Lk, float scale, const int32_t* key_valid, int key_row) {
    return run_attention(q, k, v, o, B, heads, Lq, Lk, scale, key_valid, key_row);
}
// key-split attention partials: part_o [splits][B * Lq][heads * 32], part_ml [splits][B * Lq][heads][2]
TAPI int opd_test_attention_split(const uint16_t* q, const uint16_t* k, const uint16_t* v, int B, int heads, int Lq, int Lk, float scale, int splits,
                                  const int32_t* key_valid, int key_row, float* part_o, float* part_ml) {
    DevMem dm;
    AttnParams p{};
    const int D = attention_params(dm, p, q, k, v, B, heads, Lq, Lk, scale, key_valid, key_row);
    const size_t no = (size_t)splits * B * Lq * D, nm = (size_t)splits * B * Lq * heads * 2;
    p.part_o = dm.alloc<float>(no); p.part_ml = dm.alloc<float>(nm); p.splits = splits;
    if (!dm.ok) return fail(OPD_ENOMEM, "test alloc failed");
    RCCHK(launch_repeated([&](int) { return LAUNCHED(opd_launch_attention(p, nullptr)); }, {{p.part_o, no * 4, 0xff}, {p.part_ml, nm * 4, 0xff}}));
    HIPCHK(hipDeviceSynchronize());
    RCCHK(down(part_o, p.part_o, no));
    return down(part_ml, p.part_ml, nm);
}

// the cross-attention map of ONE frame and layer (attn_map_*_kernel): q [rows][ldq], k [Lk][ldk] (head h at columns 32 h; the hook sizes q by
// the largest selected row), sel [nsel] rows of q, key_valid2 (nullable) = (rows, cols) of the valid keys; out [Lk]
TAPI int opd_test_attention_map(const uint16_t* q, int ldq, const uint16_t* k, int ldk, const int32_t* sel, int nsel, int heads, int Lk, float scale,
                                const int32_t* key_valid2, int key_row, float* out) {
    if (!q || !k || !sel || !out || nsel <= 0 || heads <= 0 || Lk <= 0 || key_row <= 0 || ldq < heads * 32 || ldk < heads * 32)
        return fail(OPD_EINVAL, "attention_map: bad arguments");
    int qrows = 0;
    for (int i = 0; i < nsel; ++i) {
        if (sel[i] < 0) return fail(OPD_EINVAL, "attention_map: negative query index");
        qrows = std::max(qrows, sel[i] + 1);
    }
    DevMem dm;
    const uint16_t* dq = dm.up(q, (size_t)qrows * ldq);
    const uint16_t* dk = dm.up(k, (size_t)Lk * ldk);
    const int32_t* dsel = dm.up(sel, (size_t)nsel);
    const int32_t* dvalid = key_valid2 ? dm.up(key_valid2, 2) : nullptr;
    float* stat = dm.alloc<float>((size_t)nsel * heads * 2);
    float* dout = dm.alloc<float>((size_t)Lk);
    if (!dm.ok) return fail(OPD_ENOMEM, "test alloc failed");
    HIPCHK(opd_launch_attention_map(dq, ldq, dk, ldk, dsel, nsel, heads, Lk, scale, dvalid, key_row, stat, dout, nullptr, g_test_dtype));
    HIPCHK(hipDeviceSynchronize());
    return down(out, dout, (size_t)Lk);
}

TAPI int opd_test_layernorm(const float* x, const float* g, const float* b, float* y, uint16_t* y16, int rows) {
    DevMem dm;
    const size_t n = (size_t)rows * 256;
    const float* dx = dm.up(x, n);
    const float* dg = dm.up(g, 256);
    const float* db = dm.up(b, 256);
    float* dy = dm.alloc<float>(n);
    uint16_t* dy16 = dm.alloc<uint16_t>(n);
    if (!dm.ok) return fail(OPD_ENOMEM, "test alloc failed");
    HIPCHK(opd_launch_layernorm(dx, dg, db, dy, dy16, rows, nullptr, g_test_dtype));
    HIPCHK(hipDeviceSynchronize());
    RCCHK(down(y, dy, n));
    return down(y16, dy16, n);
}

TAPI int opd_test_maxpool(const uint16_t* x, uint16_t* out, int B, int H, int W, int C, int OH, int OW) {
    DevMem dm;
    const size_t n = (size_t)B * OH * OW * C;
    const uint16_t* dx = dm.up(x, (size_t)B * H * W * C);
    uint16_t* dout = dm.alloc<uint16_t>(n);
    if (!dm.ok) return fail(OPD_ENOMEM, "test alloc failed");
    HIPCHK(opd_launch_maxpool(dx, dout, B, H, W, C, OH, OW, nullptr, g_test_dtype));
    HIPCHK(hipDeviceSynchronize());
    return down(out, dout, n);
}

// valid_hw (nullable): host [B][2] per-frame (h, w) inside the H x W canvas
TAPI int opd_test_preprocess_u8(const uint8_t* frames, uint16_t* out, int B, int H, int W, int Hp, int Wp, const int32_t* valid_hw) {
    DevMem dm;
    const size_t n = (size_t)B * Hp * Wp * 4;
    const uint8_t* din = dm.up(frames, (size_t)B * H * W * 3);
    uint16_t* dout = dm.alloc<uint16_t>(n);
    const int32_t* dvalid = valid_hw ? dm.up(valid_hw, (size_t)B * 2) : nullptr;
    if (!dm.ok) return fail(OPD_ENOMEM, "test alloc failed");
    HIPCHK(opd_launch_preprocess_u8(din, dout, B, H, W, Hp, Wp, dvalid, nullptr, g_test_dtype));
    HIPCHK(hipDeviceSynchronize());
    return down(out, dout, n);
}

// Stem on the zero-bordered NHWC4 image through the LDS-DMA kernel (stem mode 2): x4p [B][Hp][Wp][4], w [64][8][8][4].
TAPI int opd_test_stem2(const uint16_t* x4p, const uint16_t* w, const float* bias, uint16_t* out, int B, int Hp, int Wp, int OH, int OW) {
    DevMem dm;
    ConvGemmParams p{}; p.dtype = g_test_dtype;
    conv_geometry(p, B, Hp, Wp, 256, OH, OW, 64, 1, 1, 2, 0);
    p.K = 256; p.relu = 1; p.stem = 2;
    const size_t n = (size_t)p.M * 64;
    p.x = dm.up(x4p, (size_t)B * Hp * Wp * 4);
    p.w = dm.up(w, (size_t)64 * 256);
    p.bias = dm.up(bias, 64);
    p.zero16 = zeros<float>(dm, 64);
    uint16_t* dout = dm.alloc<uint16_t>(n);
    p.out = dout;
    if (!dm.ok) return fail(OPD_ENOMEM, "test alloc failed");
    HIPCHK(opd_launch_conv_gemm(p, nullptr));
    HIPCHK(hipDeviceSynchronize());
    return down(out, dout, n);
}

// Fused stem + max-pool on the zero-bordered NHWC4 image: out = pooled [B][PH][PW][64] fp16
TAPI int opd_test_stem_pool(const uint16_t* x4p, const uint16_t* w, const float* bias, uint16_t* out, int B, int Hp, int Wp, int OH, int OW,
                            int PH, int PW) {
    DevMem dm;
    const size_t n = (size_t)B * PH * PW * 64;
    const uint16_t* dx = dm.up(x4p, (size_t)B * Hp * Wp * 4);
    const uint16_t* dw = dm.up(w, (size_t)64 * 256);
    const float* db = dm.up(bias, 64);
    uint16_t* dout = dm.alloc<uint16_t>(n);
    if (!dm.ok) return fail(OPD_ENOMEM, "test alloc failed");
    HIPCHK(opd_launch_stem_pool(dx, dw, db, dout, B, Hp, Wp, OH, OW, PH, PW, nullptr, g_test_dtype));
    HIPCHK(hipDeviceSynchronize());
    return down(out, dout, n);
}

// Pre-processing + stem + max-pool in one launch against the two-kernel path on the same uint8 frames: out_fused / out_split =
// pooled [B][PH][PW][64] fp16 (the caller checks bit-equality); valid_hw nullable [B][2]
TAPI int opd_test_stem_pool_u8(const uint8_t* frames, const int32_t* valid_hw, const uint16_t* w, const float* bias, uint16_t* out_fused,
                               uint16_t* out_split, int B, int H, int W) {
    DevMem dm;
    const int OH = (H - 1) / 2 + 1, OW = (W - 1) / 2 + 1, PH = (OH - 1) / 2 + 1, PW = (OW - 1) / 2 + 1, Hp = 2 * OH + 6, Wp = 2 * OW + 6;
    const size_t n = (size_t)B * PH * PW * 64;
    const uint8_t* df = dm.up(frames, (size_t)B * H * W * 3);
    const int32_t* dv = valid_hw ? dm.up(valid_hw, (size_t)2 * B) : nullptr;
    const uint16_t* dw = dm.up(w, (size_t)64 * 256);
    const float* db = dm.up(bias, 64);
    uint16_t* dx = dm.alloc<uint16_t>((size_t)B * Hp * Wp * 4);
    uint16_t* d1 = dm.alloc<uint16_t>(n);
    uint16_t* d2 = dm.alloc<uint16_t>(n);
    if (!dm.ok) return fail(OPD_ENOMEM, "test alloc failed");
    RCCHK(launch_repeated(
        [&](int) {
            hipError_t e = LAUNCHED(opd_launch_stem_pool_u8(df, dv, dw, db, d1, B, H, W, OH, OW, PH, PW, nullptr, g_test_dtype));
            if (e == hipSuccess) e = LAUNCHED(opd_launch_preprocess_u8(df, dx, B, H, W, Hp, Wp, dv, nullptr, g_test_dtype));
            return e != hipSuccess ? e : LAUNCHED(opd_launch_stem_pool(dx, dw, db, d2, B, Hp, Wp, OH, OW, PH, PW, nullptr, g_test_dtype));
        },
        {{d1, n * 2, 0xff}, {d2, n * 2, 0xff}}));
    HIPCHK(hipDeviceSynchronize());
    RCCHK(down(out_fused, d1, n));
    return down(out_split, d2, n);
}

// The stem launch with stage 1's first 1x1 reduce inside (StemReduce) against the same launch without it followed by opd_launch_conv_gemm
// (64 -> 64, ReLU) on the pooled map: frames [B][H][W][3] uint8 BGR (valid_hw nullable [B][2]); u8 = 1: the kernel that pre-processes the
// frames itself, 0: preprocess_u8_kernel first, then the kernel that reads the fp16 image.  w [64][256], w0 [64][64] in the hooks' element
// type; pool_* / z_* [B][PH][PW][64] (the caller checks bit-equality).
TAPI int opd_test_stem_reduce(const uint8_t* frames, const int32_t* valid_hw, const uint16_t* w, const float* bias, const uint16_t* w0, const float* b0,
                              uint16_t* pool_fused, uint16_t* z_fused, uint16_t* pool_ref, uint16_t* z_ref, int B, int H, int W, int u8) {
    DevMem dm;
    const int OH = (H - 1) / 2 + 1, OW = (W - 1) / 2 + 1, PH = (OH - 1) / 2 + 1, PW = (OW - 1) / 2 + 1, Hp = 2 * OH + 6, Wp = 2 * OW + 6;
    const size_t n = (size_t)B * PH * PW * 64;
    const uint8_t* df = dm.up(frames, (size_t)B * H * W * 3);
    const int32_t* dv = valid_hw ? dm.up(valid_hw, (size_t)2 * B) : nullptr;
    const uint16_t* dw = dm.up(w, (size_t)64 * 256);
    const float* db = dm.up(bias, 64);
    uint16_t* dx = dm.alloc<uint16_t>((size_t)B * Hp * Wp * 4);
    uint16_t *p1 = dm.alloc<uint16_t>(n), *z1 = dm.alloc<uint16_t>(n), *p2 = dm.alloc<uint16_t>(n), *z2 = dm.alloc<uint16_t>(n);
    StemReduce red;
    red.z0 = z1; red.w0 = dm.up(w0, (size_t)64 * 64); red.b0 = dm.up(b0, 64);
    ConvGemmParams c{}; c.dtype = g_test_dtype;
    conv_geometry(c, B, PH, PW, 64, PH, PW, 64, 1, 1, 1, 0);
    c.x = p2; c.w = red.w0; c.bias = red.b0; c.out = z2; c.zero16 = zeros<uint32_t>(dm, 8); c.relu = 1;
    if (!dm.ok) return fail(OPD_ENOMEM, "test alloc failed");
    HIPCHK(hipMemsetAsync(z1, 0xff, n * 2, nullptr));   // (a pixel the fused launch forgets stays NaN)
    RCCHK(launch_repeated(
        [&](int) {
            hipError_t e;
            if (u8) {
                e = LAUNCHED(opd_launch_stem_pool_u8(df, dv, dw, db, p1, B, H, W, OH, OW, PH, PW, nullptr, g_test_dtype, red));
                if (e == hipSuccess) e = LAUNCHED(opd_launch_stem_pool_u8(df, dv, dw, db, p2, B, H, W, OH, OW, PH, PW, nullptr, g_test_dtype));
            } else {
                e = LAUNCHED(opd_launch_preprocess_u8(df, dx, B, H, W, Hp, Wp, dv, nullptr, g_test_dtype));
                if (e == hipSuccess) e = LAUNCHED(opd_launch_stem_pool(dx, dw, db, p1, B, Hp, Wp, OH, OW, PH, PW, nullptr, g_test_dtype, red));
                if (e == hipSuccess) e = LAUNCHED(opd_launch_stem_pool(dx, dw, db, p2, B, Hp, Wp, OH, OW, PH, PW, nullptr, g_test_dtype));
            }
            return e != hipSuccess ? e : LAUNCHED(opd_launch_conv_gemm(c, nullptr));
        },
        {{p1, n * 2, 0xff}, {z1, n * 2, 0xff}, {p2, n * 2, 0xff}, {z2, n * 2, 0xff}}));
    HIPCHK(hipDeviceSynchronize());
    RCCHK(down(pool_fused, p1, n));
    RCCHK(down(z_fused, z1, n));
    RCCHK(down(pool_ref, p2, n));
    return down(z_ref, z2, n);
}

// heads_kernel alone: hs [rows][256] fp32 (+ optional final LayerNorm), weights in the reference's [out][in] layout (the hooks
// transpose them as opd_model.cpp does); logits [rows][ncls], boxes [rows][4]
static int g_test_heads2 = 1;   // heads hooks: 1 = heads2_kernel (split fp16 operands), 0 = heads_kernel (fp32 matrix pipe)
TAPI int opd_test_set_heads2(int on) { g_test_heads2 = on; return OPD_OK; }
// heads hooks: `logits` / `boxes` carry this many rows behind `rows`; the device buffers start as the caller's arrays (a sentinel in the spare
// rows) and come back whole, so that a store past the last row shows
static int g_test_heads_spare = 0;
TAPI int opd_test_set_heads_spare_rows(int rows) { g_test_heads_spare = rows > 0 ? rows : 0; return OPD_OK; }
// which kernel the heads hooks run: heads2_kernel where it is selected and holds the class matrix (128 rows), else heads_kernel
static bool heads_split16(int ncls) { return g_test_heads2 && ncls <= 128; }
// (the three 256-wide layers as split fp16 pairs in fragment order, class matrix padded to 128 rows)
static void heads_frags(DevMem& dm, HeadParams& p, const float* wc, const float* w1, const float* w2, int ncls) {
    if (!heads_split16(ncls)) return;
    std::vector<float> wcp((size_t)128 * 256, 0.f);
    std::copy(wc, wc + (size_t)ncls * 256, wcp.begin());
    std::vector<uint16_t> f((size_t)2 * 128 * 256);
    opd_split_f16_frag(wcp.data(), 128, 256, f.data());
    p.wc_f = dm.up(f.data(), f.size());
    std::vector<uint16_t> f2((size_t)2 * 256 * 256);
    opd_split_f16_frag(w1, 256, 256, f2.data());
    p.w1_f = dm.up(f2.data(), f2.size());
    opd_split_f16_frag(w2, 256, 256, f2.data());
    p.w2_f = dm.up(f2.data(), f2.size());
}
// what both heads hooks fill: the rows, the four layers ([out][in] -> [in][out]), the outputs, the fragment forms
static void heads_params(DevMem& dm, HeadParams& p, const float* hs, const float* wc, const float* bc, const float* w1, const float* b1,
                         const float* w2, const float* b2, const float* w3, const float* b3, int rows, int ncls, const float* logits, const float* boxes) {
    auto tr = [&](const float* w, int O, int I) -> const float* {
        std::vector<float> t((size_t)O * I);
        for (int o = 0; o < O; ++o)
            for (int i = 0; i < I; ++i) t[(size_t)i * O + o] = w[(size_t)o * I + i];
        return dm.up(t.data(), t.size());
    };
    p.hs = dm.up(hs, (size_t)rows * 256);
    p.wc = tr(wc, ncls, 256); p.bc = dm.up(bc, ncls);
    p.w1 = tr(w1, 256, 256); p.b1 = dm.up(b1, 256);
    p.w2 = tr(w2, 256, 256); p.b2 = dm.up(b2, 256);
    p.w3 = tr(w3, 4, 256); p.b3 = dm.up(b3, 4);
    const size_t all = (size_t)rows + g_test_heads_spare;
    p.logits = g_test_heads_spare ? dm.up(logits, all * ncls) : dm.alloc<float>(all * ncls);
    p.boxes = g_test_heads_spare ? dm.up(boxes, all * 4) : dm.alloc<float>(all * 4);
    p.rows = rows; p.ncls = ncls;
    heads_frags(dm, p, wc, w1, w2, ncls);
}
static int run_heads(DevMem& dm, const HeadParams& p, float* logits, float* boxes) {
    if (!dm.ok) return fail(OPD_ENOMEM, "test alloc failed");
    const size_t all = (size_t)p.rows + g_test_heads_spare;
    // (with spare rows the outputs start as the caller's arrays, which only a restore brings back; else they are merely allocated)
    const bool spare = g_test_heads_spare > 0;
    std::vector<RepOut> outs;
    std::vector<RepInPlace> kept;
    if (spare) kept = {{p.logits, all * p.ncls * 4}, {p.boxes, all * 16}};
    else outs = {{p.logits, all * p.ncls * 4, 0xff}, {p.boxes, all * 16, 0xff}};
    RCCHK(launch_repeated([&](int) { return heads_split16(p.ncls) ? LAUNCHED(opd_launch_heads2(p, nullptr)) : LAUNCHED(opd_launch_heads(p, nullptr)); }, outs, kept));
    HIPCHK(hipDeviceSynchronize());
    RCCHK(down(logits, p.logits, all * p.ncls));
    return down(boxes, p.boxes, all * 4);
}
TAPI int opd_test_heads(const float* hs, const float* ln_g, const float* ln_b, const float* wc, const float* bc, const float* w1, const float* b1,
                        const float* w2, const float* b2, const float* w3, const float* b3, float* logits, float* boxes, int rows, int ncls) {
    DevMem dm;
    HeadParams p{};
    p.ln_gamma = ln_g ? dm.up(ln_g, 256) : nullptr;
    p.ln_beta = ln_b ? dm.up(ln_b, 256) : nullptr;
    heads_params(dm, p, hs, wc, bc, w1, b1, w2, b2, w3, b3, rows, ncls, logits, boxes);
    return run_heads(dm, p, logits, boxes);
}
// heads_kernel with the fused decoder's prologue: rows = LN3(hs + b2f + sum partials), then the final LayerNorm, then the heads
TAPI int opd_test_heads_fused(const float* hs, const float* partials, int nsplit, const float* b2f, const float* ln3_g, const float* ln3_b, const float* ln_g,
                              const float* ln_b, const float* wc, const float* bc, const float* w1, const float* b1, const float* w2, const float* b2,
                              const float* w3, const float* b3, int rows, int ncls, float* logits, float* boxes) {
    DevMem dm;
    HeadParams p{};
    p.partials = dm.up(partials, (size_t)nsplit * rows * 256); p.nsplit = nsplit; p.ffn_b2 = dm.up(b2f, 256);
    p.ln3_gamma = dm.up(ln3_g, 256); p.ln3_beta = dm.up(ln3_b, 256);
    p.ln_gamma = dm.up(ln_g, 256); p.ln_beta = dm.up(ln_b, 256);
    heads_params(dm, p, hs, wc, bc, w1, b1, w2, b2, w3, b3, rows, ncls, logits, boxes);
    return run_heads(dm, p, logits, boxes);
}

// postprocess_kernel alone: logits [B][Q][ncls], boxes [B][Q][4] cxcywh, orig_hw [B][2] -> records [B][Q] (compacted) + counts [B]
TAPI int opd_test_postprocess(const float* logits, const float* boxes, const int32_t* orig_hw, int B, int Q, int ncls, float threshold,
                              opd_det* records, int32_t* counts) {
    DevMem dm;
    PostParams p{};
    p.logits = dm.up(logits, (size_t)B * Q * ncls);
    p.boxes = dm.up(boxes, (size_t)B * Q * 4);
    p.orig_hw = dm.up(orig_hw, (size_t)B * 2);
    opd_det* rec = zeros<opd_det>(dm, (size_t)B * Q);
    p.counts = dm.alloc<int32_t>(B);
    if (!dm.ok) return fail(OPD_ENOMEM, "test alloc failed");
    p.records = rec; p.B = B; p.Q = Q; p.ncls = ncls; p.threshold = threshold;
    HIPCHK(opd_launch_postprocess(p, nullptr));
    HIPCHK(hipDeviceSynchronize());
    RCCHK(down(records, rec, (size_t)B * Q));
    return down(counts, p.counts, (size_t)B);
}

// roi_features_kernel alone: enc [h][w][256] fp32, rois [n][4] = (x0, y0, x1, y1) in map cells -> out [n][256]
TAPI int opd_test_roi_features(const float* enc, const int32_t* rois, int n, int h, int w, float* out) {
    DevMem dm;
    const float* d_enc = dm.up(enc, (size_t)h * w * 256);
    const int32_t* d_rois = dm.up(rois, (size_t)n * 4);
    float* d_out = dm.alloc<float>((size_t)n * 256);
    if (!dm.ok) return fail(OPD_ENOMEM, "test alloc failed");
    HIPCHK(opd_launch_roi_features(d_enc, d_rois, d_out, n, h, w, nullptr));
    HIPCHK(hipDeviceSynchronize());
    return down(out, d_out, (size_t)n * 256);
}

// ---- fused decoder kernels (kernels_dec.hip), one launch each; weights arrive as fp32 and are split here like the loader does ----------
static const f16_t* up_frag(DevMem& dm, const float* w, int N, int K) {
    std::vector<f16_t> f((size_t)N * K * 2);
    opd_split_f16_frag(w, N, K, f.data());
    return dm.up(f.data(), f.size());
}
// h_out / q16 [M][256]; k16 / vT [M / Q][8][8][512] in fragment order (host; returned as the device wrote them: padding keys untouched = zero-filled here)
TAPI int opd_test_dec_qkv(const float* h_in, const float* partials, int nsplit, const float* b2, const float* ln_g, const float* ln_b, const float* w,
                          const float* bias, int M, int Q, float* h_out, uint16_t* q16, uint16_t* k16, uint16_t* vT) {
    DevMem dm;
    DecQkvParams p{};
    const size_t n = (size_t)M * 256, nv = (size_t)(M / Q) * 8 * 8 * 512;
    if (partials) {
        p.h_in = dm.up(h_in, n); p.partials = dm.up(partials, n * nsplit); p.nsplit = nsplit; p.b2 = dm.up(b2, 256); p.ln_g = dm.up(ln_g, 256); p.ln_b = dm.up(ln_b, 256);
        p.h_out = dm.alloc<float>(n);
    } else {
        p.h_out = dm.up(h_in, n);
    }
    p.w = up_frag(dm, w, 768, 256);
    p.bias = dm.up(bias, (size_t)Q * 768);
    p.q16 = dm.alloc<uint16_t>(n); p.k16 = zeros<uint16_t>(dm, nv); p.vT = zeros<uint16_t>(dm, nv);
    if (!dm.ok) return fail(OPD_ENOMEM, "test alloc failed");
    p.M = M; p.Q = Q;
    // (without the prologue the launch reads h_out; the padding keys of k16 / vT must keep the zero fill)
    RCCHK(launch_repeated([&](int) { return LAUNCHED(opd_launch_dec_qkv(p, nullptr)); },
                          {{partials ? p.h_out : nullptr, n * 4, 0xff}, {p.q16, n * 2, 0xff}, {p.k16, nv * 2, 0}, {p.vT, nv * 2, 0}},
                          {{partials ? nullptr : p.h_out, n * 4}}));
    HIPCHK(hipDeviceSynchronize());
    RCCHK(down(h_out, p.h_out, n));
    RCCHK(down(q16, p.q16, n));
    RCCHK(down(k16, p.k16, nv));
    return down(vT, p.vT, nv);
}
// h [B * Q][256] in / out, qc16 [B * Q][256] out
TAPI int opd_test_dec_self(const uint16_t* q16, const uint16_t* k16, const uint16_t* vT, float* h, const float* wo, const float* bo, const float* ln_g,
                           const float* ln_b, const float* wq, const float* rbq, int B, int Q, float scale, uint16_t* qc16) {
    DevMem dm;
    DecSelfParams p{};
    const size_t n = (size_t)B * Q * 256, nv = (size_t)B * 8 * 8 * 512;
    p.q16 = dm.up(q16, n); p.k16 = dm.up(k16, nv); p.vT = dm.up(vT, nv); p.h = dm.up(h, n);
    p.bo = dm.up(bo, 256); p.ln_g = dm.up(ln_g, 256); p.ln_b = dm.up(ln_b, 256); p.rbq = dm.up(rbq, (size_t)Q * 256);
    p.qc16 = dm.alloc<uint16_t>(n);
    p.wo = up_frag(dm, wo, 256, 256); p.wq = up_frag(dm, wq, 256, 256);
    if (!dm.ok) return fail(OPD_ENOMEM, "test alloc failed");
    p.B = B; p.Q = Q; p.scale = scale; p.qc_bf16 = (g_test_dtype == OPD_DT_BF16);
    RCCHK(launch_repeated([&](int) { return LAUNCHED(opd_launch_dec_self(p, nullptr)); }, {{p.qc16, n * 2, 0xff}}, {{p.h, n * 4}}));
    HIPCHK(hipDeviceSynchronize());
    RCCHK(down(h, p.h, n));
    return down(qc16, p.qc16, n);
}
TAPI int opd_test_dec_cross_out(const float* part_o, const float* part_ml, int splits, const float* res, int res_period, const float* wo, const float* bo,
                                const float* ln_g, const float* ln_b, int M, float* h) {
    DevMem dm;
    DecCrossOutParams p{};
    const size_t n = (size_t)M * 256;
    p.part_o = dm.up(part_o, n * splits); p.part_ml = dm.up(part_ml, (size_t)splits * M * 16); p.splits = splits;
    p.res = dm.up(res, res_period > 0 ? (size_t)res_period * 256 : n); p.res_period = res_period;
    p.h = dm.alloc<float>(n); p.bo = dm.up(bo, 256); p.ln_g = dm.up(ln_g, 256); p.ln_b = dm.up(ln_b, 256); p.M = M;
    p.wo = up_frag(dm, wo, 256, 256);
    if (!dm.ok) return fail(OPD_ENOMEM, "test alloc failed");
    RCCHK(launch_repeated([&](int) { return LAUNCHED(opd_launch_dec_cross_out(p, nullptr)); }, {{p.h, n * 4, 0xff}}));
    HIPCHK(hipDeviceSynchronize());
    return down(h, p.h, n);
}
// partials [F / 128][M][256]
TAPI int opd_test_dec_ffn(const float* h, const float* w1, const float* b1, const float* w2, int M, int F, float* partials) {
    DevMem dm;
    DecFfnParams p{};
    const size_t n = (size_t)M * 256, np = n * (F / OPD_DEC_FFN_CHUNK);
    p.h = dm.up(h, n); p.b1 = dm.up(b1, (size_t)F); p.partials = dm.alloc<float>(np); p.M = M; p.F = F;
    p.w1 = up_frag(dm, w1, F, 256); p.w2 = up_frag(dm, w2, 256, F);
    if (!dm.ok) return fail(OPD_ENOMEM, "test alloc failed");
    RCCHK(launch_repeated([&](int) { return LAUNCHED(opd_launch_dec_ffn(p, nullptr)); }, {{p.partials, np * 4, 0xff}}));
    HIPCHK(hipDeviceSynchronize());
    return down(partials, p.partials, np);
}
