// opd_test_bench_api.cpp — the timing (opd_test_bench_*) and trace (opd_test_trace_*) hooks of tools/: device-resident operands of arbitrary
// data, launches on the null stream, microseconds or per-workgroup stamps back.  Exported from libopd_hip_test.so only; no test calls these.
#include <vector>

#include "opd_test_util.h"

using namespace opd;

// Times `iters` launches of Linear(K -> 256) + residual + LayerNorm (deep != 0: the row-owner ring kernel) on M rows of arbitrary data.
TAPI int opd_test_bench_gemm_ln(int M, int K, int deep, int iters, float* us_out) {
    DevMem dm;
    GemmLnParams p{}; p.dtype = g_test_dtype;
    p.x = filled16(dm, (size_t)M * K, 0x2c);
    p.w = filled16(dm, (size_t)256 * K, 0x1c);
    float* f = zeros<float>(dm, 1024);
    float* res = zeros<float>(dm, (size_t)M * 256);
    p.y16 = dm.alloc<uint16_t>((size_t)M * 256);
    if (!dm.ok) return fail(OPD_ENOMEM, "bench alloc failed");
    p.bias = f; p.gamma = f + 256; p.beta = f + 512; p.res32 = res; p.y32 = res; p.M = M; p.K = K; p.deep_k = deep;
    return time_launches(3, iters, [&] { return opd_launch_gemm_ln(p, nullptr); }, us_out);
}

// Times `iters` launches of the fused encoder FFN on M rows of arbitrary data.
TAPI int opd_test_bench_enc_ffn(int M, int F, int iters, int dbg, int tail, int front, float* us_out) {
    if (M <= 0 || F <= 0 || F % 128) return fail(OPD_EINVAL, "bench_enc_ffn: F must be a multiple of 128");
    DevMem dm;
    EncFfnParams p{}; p.dtype = g_test_dtype;
    uint16_t* x = filled16(dm, (size_t)M * 256, 0x2c);
    p.wpack = filled<unsigned char>(dm, opd_encffn_pack_bytes(F, tail, 1), 0x1c);
    p.tail_out = tail ? dm.alloc<uint16_t>((size_t)M * tail * 256) : nullptr;
    float* f = zeros<float>(dm, 1024);
    float* res = zeros<float>(dm, (size_t)M * 256);
    p.y16 = dm.alloc<uint16_t>((size_t)M * 256);
    if (!dm.ok) return fail(OPD_ENOMEM, "bench alloc failed");
    p.x = x; p.b2 = f; p.gamma = f + 256; p.beta = f + 512; p.res32 = res; p.y32 = res; p.M = M; p.F = F; p.dbg = dbg;
    p.pack_tail = tail; p.tail = tail; p.tail_pos = 0; p.tail_ld = tail * 256; p.pack_front = 1;
    if (front) { p.attn = x; p.x = nullptr; p.bo = f; p.gamma1 = f + 256; p.beta1 = f + 512; }
    for (int t = 0; t < tail && t < 16; ++t) p.tail_col[t] = 256 * t;
    return time_launches(3, iters, [&] { return opd_launch_enc_ffn(p, nullptr); }, us_out);
}

// The operands of one conv_gemm layer shape on device-resident arbitrary data (KH x KH, pad KH / 2, ReLU); `out` holds out_scale x [M][N] 16-bit elements
static void conv_layer(DevMem& dm, ConvGemmParams& p, int B, int H, int W, int Cin, int N, int KH, int stride, int with_res, size_t out_scale) {
    const int pad = KH / 2, OH = (H + 2 * pad - KH) / stride + 1, OW = (W + 2 * pad - KH) / stride + 1;
    p.dtype = g_test_dtype;
    conv_geometry(p, B, H, W, Cin, OH, OW, N, KH, KH, stride, pad);
    const size_t MN = (size_t)p.M * N;
    p.x = filled16(dm, (size_t)B * H * W * Cin, 0x2c);
    p.w = filled16(dm, (size_t)N * p.K, 0x1c);
    p.bias = zeros<float>(dm, N);
    p.res16 = with_res ? filled16(dm, MN, 0x2c) : nullptr;
    p.out = dm.alloc<uint16_t>(MN * out_scale);
    p.zero16 = zeros<float>(dm, 4096);
    p.relu = 1;
}

// Times one conv_gemm launch shape on device-resident random data (no host copies): average microseconds over `iters`.
TAPI int opd_test_bench_conv(int B, int H, int W, int Cin, int N, int KH, int stride, int with_res, int variant, int dbg, int iters,
                             float* us_out) {
    DevMem dm;
    ConvGemmParams p{};
    conv_layer(dm, p, B, H, W, Cin, N, KH, stride, with_res, 1);
    if (!dm.ok) return fail(OPD_ENOMEM, "bench alloc failed");
    p.dbg = dbg;
    apply_conv_flags(p, variant);   // (`variant`: the flag word of opd_test_set_conv_flags)
    return time_launches(2, iters, [&] { return opd_launch_conv_gemm(p, nullptr); }, us_out);
}

// `warm` traced launches of a layer shape back to back, then three more whose stamps are kept: trace_out [3][max_wgs][8] receives the
// per-workgroup phase stamps of conv_gemm_dma_kernel<..., TRACE> (the spacing of their wall-clock stamps is the cost of a launch boundary --
// drain of one kernel, dispatch of the next -- on a busy stream).  The launcher's grid is not exported: *wgs_out = max_wgs, and the caller
// reads stamps until the first all-zero row.
TAPI int opd_test_trace_conv(int B, int H, int W, int Cin, int N, int KH, int stride, int with_res, int split_k, int warm, unsigned long long* trace_out,
                             int max_wgs, int* wgs_out) {
    DevMem dm;
    ConvGemmParams p{};
    conv_layer(dm, p, B, H, W, Cin, N, KH, stride, with_res, split_k > 1 ? 2 * (size_t)split_k : 1);   // split-K: fp32 slabs
    const size_t per = (size_t)max_wgs * 8;
    p.trace = zeros<unsigned long long>(dm, per);
    unsigned long long* tr3 = zeros<unsigned long long>(dm, 3 * per);
    if (!dm.ok) return fail(OPD_ENOMEM, "trace alloc failed");
    if (split_k > 1) { p.split_k = split_k; p.out_f32 = 1; p.relu = 0; }
    for (int i = 0; i < warm; ++i) HIPCHK(opd_launch_conv_gemm(p, nullptr));
    for (int i = 0; i < 3; ++i) {
        p.trace = tr3 + (size_t)i * per;
        HIPCHK(opd_launch_conv_gemm(p, nullptr));
    }
    HIPCHK(hipDeviceSynchronize());
    *wgs_out = max_wgs;
    return down(trace_out, tr3, 3 * per);
}

// The operands of a fused tail on device-resident arbitrary data; C3 == 0: w3 / z sized for 64 channels (the unfused c0' of opd_test_bench_btail)
static void btail_layer(DevMem& dm, BtailParams& p, int B, int H, int W, int C1, int C3, int stride, int dbg) {
    const int C2 = 4 * C1, C3a = C3 ? C3 : 64;
    p.dtype = g_test_dtype;
    btail_geometry(p, B, H, W, stride, C1, C3);
    const size_t M = (size_t)p.M;
    p.x1 = filled16(dm, (size_t)B * H * W * C1, 0x2c);
    p.w1 = filled16(dm, (size_t)C1 * 9 * C1, 0x1c);
    p.w2p = filled16(dm, (size_t)C2 * C1, 0x1c);
    p.w3p = filled16(dm, (size_t)C3a * C2, 0x1c);
    p.b1 = p.b2 = p.b3 = zeros<float>(dm, C2);
    p.res = filled16(dm, M * C2, 0x2c);
    p.y = dm.alloc<uint16_t>(M * C2);
    p.z = dm.alloc<uint16_t>(M * C3a);
    p.dbg = dbg;
}

// Two warm launches, then one traced launch of a fused tail: trace_out [wgs][16] (kernels_btail.hip, TRACE), *wgs_out = grid size
TAPI int opd_test_trace_btail(int B, int H, int W, int C1, int C3, int dbg, unsigned long long* trace_out, int max_wgs, int* wgs_out) {
    if (!opd_btail_supported(C1, C3)) return fail(OPD_EINVAL, "btail: unsupported (C1, C3)");
    DevMem dm;
    const int wgs = (int)(((size_t)B * H * W + 127) / 128);
    if (wgs > max_wgs) return fail(OPD_EINVAL, "trace buffer too small");
    BtailParams p{};
    btail_layer(dm, p, B, H, W, C1, C3, 1, dbg);
    unsigned long long* tr = zeros<unsigned long long>(dm, (size_t)wgs * 16);
    if (!dm.ok) return fail(OPD_ENOMEM, "trace alloc failed");
    for (int i = 0; i < 2; ++i) HIPCHK(opd_launch_btail(p, nullptr));
    p.trace = tr;
    HIPCHK(opd_launch_btail(p, nullptr));
    HIPCHK(hipDeviceSynchronize());
    *wgs_out = wgs;
    return down(trace_out, tr, (size_t)wgs * 16);
}

// Times the fused tail (us_out[0]) and the three unfused launches it replaces (us_out[1..3]: c1, c2, c0') on device-resident data of the
// given shape.
TAPI int opd_test_bench_btail(int B, int H, int W, int C1, int C3, int stride, int dbg, int iters, float* us_out) {
    if (!opd_btail_supported(C1, C3)) return fail(OPD_EINVAL, "btail: unsupported (C1, C3)");
    DevMem dm;
    const int C2 = 4 * C1;
    BtailParams p{};
    btail_layer(dm, p, B, H, W, C1, C3, stride, dbg);
    uint16_t* a1 = dm.alloc<uint16_t>((size_t)p.M * C1);
    float* zero = zeros<float>(dm, 4096);
    if (!dm.ok) return fail(OPD_ENOMEM, "bench alloc failed");
    ConvGemmParams c[3] = {};
    c[0].x = p.x1; c[0].w = p.w1; c[0].out = a1;
    conv_geometry(c[0], B, H, W, C1, p.OH, p.OW, C1, 3, 3, stride, 1);
    c[1].x = a1; c[1].w = p.w2p; c[1].res16 = p.res; c[1].out = p.y;
    conv_geometry(c[1], B, p.OH, p.OW, C1, p.OH, p.OW, C2, 1, 1, 1, 0);
    c[2].x = p.y; c[2].w = p.w3p; c[2].out = p.z;
    conv_geometry(c[2], B, p.OH, p.OW, C2, p.OH, p.OW, C3 ? C3 : 64, 1, 1, 1, 0);
    for (auto& q : c) { q.bias = p.b1; q.zero16 = zero; q.relu = 1; }
    for (int k = 0; k < 4; ++k) {
        us_out[k] = 0.f;
        if (k == 3 && !C3) break;
        if (k > 0 && dbg) continue;
        RCCHK(time_launches(2, iters, [&] { return k == 0 ? opd_launch_btail(p, nullptr) : opd_launch_conv_gemm(c[k - 1], nullptr); }, &us_out[k]));
    }
    return OPD_OK;
}

// Stage 2's first block: the fused tail with the stride-2 shortcut inside (us_out[0]; kernels_btail.hip, SC2) and the three launches it replaces
// (us_out[1..3]: 3x3 stride 2, dual-source expand over [a1 | block input], the next block's reduce) on x1 [B][H][W][128], xs [B][H][W][256].
TAPI int opd_test_bench_btail_sc2(int B, int H, int W, int C3, int dbg, int iters, float* us_out) {
    const int C1 = 128, C2 = 512, Csc = 256;
    if (!opd_btail_sc_supported(C1, C3, Csc, 2)) return fail(OPD_EINVAL, "btail_sc2: unsupported C3");
    DevMem dm;
    BtailParams p{};
    btail_layer(dm, p, B, H, W, C1, C3, 2, dbg);
    p.res = nullptr;
    p.xs = filled16(dm, (size_t)B * H * W * Csc, 0x2c);
    p.wsc = filled16(dm, (size_t)C2 * Csc, 0x1c);
    uint16_t* a1 = dm.alloc<uint16_t>((size_t)p.M * C1);
    uint16_t* w2sc = filled16(dm, (size_t)C2 * (C1 + Csc), 0x1c);
    float* zero = zeros<float>(dm, 4096);
    if (!dm.ok) return fail(OPD_ENOMEM, "bench alloc failed");
    ConvGemmParams c[3] = {};
    c[0].x = p.x1; c[0].w = p.w1; c[0].out = a1;
    conv_geometry(c[0], B, H, W, C1, p.OH, p.OW, C1, 3, 3, 2, 1);
    c[1].x = a1; c[1].w = w2sc; c[1].out = p.y; c[1].x2 = p.xs;
    conv_geometry(c[1], B, p.OH, p.OW, C1, p.OH, p.OW, C2, 1, 1, 1, 0);
    c[1].K = C1 + Csc; c[1].K1 = C1; c[1].H2 = H; c[1].W2 = W; c[1].Cin2 = Csc; c[1].stride2 = 2;
    c[2].x = p.y; c[2].w = p.w3p; c[2].out = p.z;
    conv_geometry(c[2], B, p.OH, p.OW, C2, p.OH, p.OW, C3 ? C3 : 64, 1, 1, 1, 0);
    for (auto& q : c) { q.dtype = g_test_dtype; q.bias = p.b1; q.zero16 = zero; q.relu = 1; }
    for (int k = 0; k < 4; ++k) {
        us_out[k] = 0.f;
        if (k > 0 && dbg) continue;
        RCCHK(time_launches(2, iters, [&] { return k == 0 ? opd_launch_btail(p, nullptr) : opd_launch_conv_gemm(c[k - 1], nullptr); }, &us_out[k]));
    }
    return OPD_OK;
}

// The operands of an attention launch with leading dimension ldq / ldkv (768 = the fused QKV buffer) from the caller's q, k, v
static void attention_operands(DevMem& dm, AttnParams& p, const uint16_t* q, const uint16_t* k, const uint16_t* v, int B, int heads, int Lq, int Lk,
                               int ldq, int ldkv, float scale) {
    p.dtype = g_test_dtype;
    p.q = dm.up(q, (size_t)B * Lq * ldq);
    p.k = dm.up(k, (size_t)B * Lk * ldkv);
    p.v = dm.up(v, (size_t)B * Lk * ldkv);
    p.o = dm.alloc<uint16_t>((size_t)B * Lq * heads * 32);
    p.B = B; p.heads = heads; p.Lq = Lq; p.Lk = Lk; p.ldq = ldq; p.ldk = p.ldv = ldkv; p.ldo = heads * 32; p.scale = scale;
}

// Times `iters` launches of the attention kernel on caller-supplied operands with leading dimension ld (768 = the fused QKV buffer).
TAPI int opd_test_bench_attention(const uint16_t* q, const uint16_t* k, const uint16_t* v, int B, int heads, int Lq, int Lk, int ldq, int ldkv,
                                  float scale, int iters, float* us_out) {
    DevMem dm;
    AttnParams p{};
    attention_operands(dm, p, q, k, v, B, heads, Lq, Lk, ldq, ldkv, scale);
    if (!dm.ok) return fail(OPD_ENOMEM, "bench alloc failed");
    return time_launches(3, iters, [&] { return opd_launch_attention(p, nullptr); }, us_out);
}

// One traced launch (after 2 untraced ones): trace_out [max_wgs][8] = per-workgroup sums of wave 0's cycles in the five phases of a
// key tile (loads issued | S + max + branch | exp + PV | wait for the next tile's loads | LDS stores | barrier), total, tiles.
TAPI int opd_test_trace_attention(const uint16_t* q, const uint16_t* k, const uint16_t* v, int B, int heads, int Lq, int Lk, int ldq, int ldkv,
                                  float scale, unsigned long long* trace_out, int max_wgs, int* wgs_out) {
    DevMem dm;
    AttnParams p{};
    attention_operands(dm, p, q, k, v, B, heads, Lq, Lk, ldq, ldkv, scale);
    const int total = ((Lq + 63) / 64) * heads * B, grid = 8 * ((total + 7) / 8);
    unsigned long long* tr = zeros<unsigned long long>(dm, (size_t)grid * 12);
    if (!dm.ok) return fail(OPD_ENOMEM, "trace alloc failed");
    for (int i = 0; i < 2; ++i) HIPCHK(opd_launch_attention(p, nullptr));
    p.trace = tr;
    HIPCHK(opd_launch_attention(p, nullptr));
    HIPCHK(hipDeviceSynchronize());
    const int n = grid < max_wgs ? grid : max_wgs;
    *wgs_out = n;
    return down(trace_out, tr, (size_t)n * 12);
}

// isolated timing of the fused decoder's kernels on zero-filled operands at M = B x Q rows, Lk keys: us per launch of
// [qkv, self, cross-split, cross-out, ffn] (tools/bench_dec.py)
TAPI int opd_test_bench_dec(int B, int Q, int Lk, int F, int splits, int iters, float* us5) {
    DevMem dm;
    const int M = B * Q, nchunk = F / OPD_DEC_FFN_CHUNK;
    const size_t n = (size_t)M * 256;
    DecQkvParams a{}; DecSelfParams b{}; AttnParams c{}; DecCrossOutParams d{}; DecFfnParams e{};
    float *vec = zeros<float>(dm, 4096), *h0 = zeros<float>(dm, n), *h1 = zeros<float>(dm, n), *part = zeros<float>(dm, n * nchunk), *tabs = zeros<float>(dm, (size_t)Q * 768), *po = zeros<float>(dm, n * splits),
          *pml = zeros<float>(dm, (size_t)splits * M * 16);
    const size_t nv = (size_t)B * 8 * 8 * 512;
    uint16_t *q16 = zeros<uint16_t>(dm, n), *k16 = zeros<uint16_t>(dm, nv), *vT = zeros<uint16_t>(dm, nv), *qc = zeros<uint16_t>(dm, n);
    uint16_t *w768 = zeros<uint16_t>(dm, 2 * 768 * 256), *w256 = zeros<uint16_t>(dm, 2 * 65536), *wf = zeros<uint16_t>(dm, (size_t)2 * F * 256), *mem = zeros<uint16_t>(dm, (size_t)B * Lk * 512);
    if (!dm.ok) return fail(OPD_ENOMEM, "test alloc failed");
    a.h_in = h0; a.partials = part; a.nsplit = nchunk; a.b2 = vec; a.ln_g = vec; a.ln_b = vec; a.h_out = h1; a.w = w768; a.bias = tabs;
    a.q16 = q16; a.k16 = k16; a.vT = vT; a.M = M; a.Q = Q;
    b.q16 = q16; b.k16 = k16; b.vT = vT; b.h = h1; b.wo = w256; b.bo = vec; b.ln_g = vec; b.ln_b = vec; b.wq = w256;
    b.rbq = tabs; b.qc16 = qc; b.B = B; b.Q = Q; b.scale = 0.17677669f;
    c.q = qc; c.k = mem; c.v = mem + 256; c.B = B; c.heads = 8; c.Lq = Q; c.Lk = Lk; c.ldq = 256; c.ldk = c.ldv = 512; c.ldo = 256; c.scale = 0.17677669f;
    c.splits = splits; c.part_o = po; c.part_ml = pml;
    d.part_o = po; d.part_ml = pml; d.splits = splits; d.res = h1; d.h = h1; d.wo = w256; d.bo = vec; d.ln_g = vec; d.ln_b = vec; d.M = M;
    e.h = h1; e.w1 = wf; e.b1 = vec; e.w2 = wf; e.partials = part; e.M = M; e.F = F;
    for (int k = 0; k < 5; ++k) {
        auto run = [&]() -> hipError_t {
            switch (k) {
                case 0: return opd_launch_dec_qkv(a, nullptr);
                case 1: return opd_launch_dec_self(b, nullptr);
                case 2: return opd_launch_attention(c, nullptr);
                case 3: return opd_launch_dec_cross_out(d, nullptr);
                default: return opd_launch_dec_ffn(e, nullptr);
            }
        };
        RCCHK(time_launches(3, iters, run, &us5[k]));
    }
    return OPD_OK;
}

// phase stamps of dec_self_kernel (wave 0 of every workgroup, shader clocks): trace_out [ceil(Q / 16) * B][8]
TAPI int opd_test_trace_dec_self(int B, int Q, unsigned long long* trace_out) {
    DevMem dm;
    DecSelfParams b{};
    const size_t n = (size_t)B * Q * 256, nv = (size_t)B * 8 * 8 * 512, stamps = (size_t)((Q + 15) / 16) * B * 8;
    b.q16 = zeros<uint16_t>(dm, n); b.k16 = zeros<uint16_t>(dm, nv); b.vT = zeros<uint16_t>(dm, nv); b.h = zeros<float>(dm, n);
    b.wo = zeros<uint16_t>(dm, 2 * 65536); b.wq = zeros<uint16_t>(dm, 2 * 65536);
    b.bo = b.ln_g = b.ln_b = zeros<float>(dm, 4096);
    b.rbq = zeros<float>(dm, (size_t)Q * 256); b.qc16 = zeros<uint16_t>(dm, n); b.B = B; b.Q = Q; b.scale = 0.17677669f;
    unsigned long long* tr = dm.alloc<unsigned long long>(stamps);
    if (!dm.ok) return fail(OPD_ENOMEM, "test alloc failed");
    for (int i = 0; i < 3; ++i) HIPCHK(opd_launch_dec_self(b, nullptr));   // warm: code and weights in the caches
    b.trace = tr;
    HIPCHK(opd_launch_dec_self(b, nullptr));
    HIPCHK(hipDeviceSynchronize());
    return down(trace_out, tr, stamps);
}
