// opd_model.cpp — workspace, per-resolution plans, per-launch timing, the trunk and transformer plans and the forward with its graph cache (the weights under it:
// opd_weights.cpp; the C-ABI on top of it: opd_api.cpp).
//
// Host-side orchestration of the DETR detect path:
//   preprocess -> stem 7x7 -> maxpool -> 16/33 bottlenecks -> input_projection -> 6 x encoder layer ->
//   (memory K/V of all decoder layers in one GEMM) -> 6 x decoder layer -> final LN -> heads -> post-process.
// Data layout in HBM: activations NHWC fp16 ([B*H*W][C] matrices), FrozenBN folded into fp16 [Cout][KH][KW][Cin]
// kernels + fp32 bias, transformer residual stream fp32 [tokens][256] with an fp16 shadow feeding the MFMA GEMMs.
// The sine position embedding is constant per (h, w), so pos.Wq / pos.Wk (+ biases) are folded into row-periodic
// fp32 bias matrices at plan-build time and q/k/v become ONE GEMM over x per layer.
#include <algorithm>

#include "opd_model.h"

namespace opd {

std::atomic<int> g_alloc_poison{-1};   // opd_model.h: diagnostic allocation mode

static void compute_dims(int B, int H, int W, Dims* d) {
    d->B = B; d->H = H; d->W = W;
    d->H1 = down2(H); d->W1 = down2(W);
    d->H2 = down2(d->H1); d->W2 = down2(d->W1);
    d->stage_h[0] = d->H2; d->stage_w[0] = d->W2;
    for (int s = 1; s < 4; ++s) { d->stage_h[s] = down2(d->stage_h[s - 1]); d->stage_w[s] = down2(d->stage_w[s - 1]); }
}

// Layer 0's cross-attention queries do not depend on the frames (build_weights: qc0): the fused decoder reads them from layer 0's region of
// d_qd16, where opd_detr_attention_map finds them too; written once per handle, every frame slot (and again by the test hooks that
// switch between the fused and the unfused decoder, whose layer 0 writes its own rounding of the same values there).
int fill_qc0(opd_detr* m) {
    if (!m->qc0 || !m->d_qd16) return OPD_OK;
    const size_t QD = (size_t)m->arch.queries * m->arch.d_model;
    for (int b = 0; b < m->cfg.max_batch; ++b) HIPCHK(hipMemcpy(m->d_qd16 + b * QD, m->qc0, QD * 2, hipMemcpyDeviceToDevice));
    return OPD_OK;
}

// Split-K plan of a deep convolution for SMALL handles (round 5).  A max_batch = 1 handle at 800 x 1333 runs stage 4's 3x3 as 72 workgroups
// that each walk 72 k-steps (50 us: the launch lasts one workgroup's life, 184 CUs idle); cut eight ways it is 576 workgroups of 9 k-steps
// plus a 3-us reduction.  The split follows the handle's CONFIGURATION (max_batch, the frame-size bounds, the layer), never the batch or frame
// at hand -- a frame's low-order bits must not depend on the call it travels in -- and applies only where the unsplit launch would leave most
// CUs without a workgroup.  Returns 1 (no split) or a divisor of the k-step count.
static int conv_splits(const opd_detr* m, const Conv& c, int stage) {
    if (!m->sw.small_splitk || stage < 0 || stage > 3 || c.stem || c.K % 64 != 0 || c.Cout % 64 != 0) return 1;
    const long long px = (long long)m->cfg.max_batch * (long long)m->stage_px[stage];
    const long long tiles = ((px + 127) / 128) * (c.Cout / 64);
    const int nk = c.K / 64;
    if (tiles > 160 || nk < 24) return 1;
    int best = 1;
    for (int s : {2, 3, 4, 6, 8})
        if (nk % s == 0 && nk / s >= 6 && tiles * s <= 640) best = s;
    return best;
}

// Frames may come in either orientation (the HF size rule maps a portrait camera frame to about 1333 x 750): the handle
// accepts every H x W with H, W <= max(max_height, max_width) and H * W <= max_height * max_width, so the buffers are sized by
// bounds on the pixel COUNT of each pyramid level, not by one shape: down2(n) <= (n + 1) / 2, hence
// H1 * W1 <= (H * W + H + W + 1) / 4 <= (n + 2 * L + 1) / 4 for a level with n pixels and sides <= L.
FrameBounds frame_bounds(const opd_config& cfg) {
    FrameBounds f;
    f.lvl[0] = (size_t)cfg.max_height * cfg.max_width; f.side[0] = (size_t)std::max(cfg.max_height, cfg.max_width);
    for (int k = 1; k < 6; ++k) { f.lvl[k] = (f.lvl[k - 1] + 2 * f.side[k - 1] + 1) / 4 + 1; f.side[k] = (size_t)down2((int)f.side[k - 1]); }
    return f;
}

int build_workspace(opd_detr* m) {
    const Arch& a = m->arch;
    const size_t B = m->cfg.max_batch;
    const size_t npix = B * (size_t)m->cfg.max_height * m->cfg.max_width;
    const FrameBounds fb = frame_bounds(m->cfg);
    const size_t *lvl = fb.lvl, *side = fb.side;
    RCCHK(dalloc(m, &m->d_u8, npix * 3, false));
    RCCHK(dalloc(m, &m->d_pv, npix * 3, false));
    RCCHK(dalloc(m, &m->d_x4, B * (4 * lvl[1] + 24 * side[1] + 36) * 4, false));  // zero-bordered NHWC4: (2 H1 + 6) x (2 W1 + 6)
    RCCHK(dalloc(m, &m->d_stem, B * lvl[1] * 64, false));
    RCCHK(dalloc(m, &m->d_pool, B * lvl[2] * 64, false));
    size_t trunk = 0, mid = 0;
    for (int s = 0; s < 4; ++s) {
        const size_t hw = lvl[2 + s];
        trunk = std::max(trunk, B * hw * a.hidden[s]);
        // first block of a stage runs its 1x1 reduce at the INPUT resolution of the stage
        const size_t hw_in = s == 0 ? hw : lvl[1 + s];
        mid = std::max(mid, B * hw_in * (a.hidden[s] / 4));
    }
    RCCHK(dalloc(m, &m->d_t0, trunk, false));
    RCCHK(dalloc(m, &m->d_t1, trunk, false));
    RCCHK(dalloc(m, &m->d_sc, trunk, false));
    RCCHK(dalloc(m, &m->d_m0, mid, false));
    RCCHK(dalloc(m, &m->d_m1, mid, false));
    const size_t M = B * lvl[5];
    const size_t D = a.d_model, Md = B * a.queries;
    RCCHK(dalloc(m, &m->d_x32, M * D, false));
    RCCHK(dalloc(m, &m->d_y32, M * D, false));
    for (int s = 0; s < 4; ++s) m->stage_px[s] = lvl[2 + s];
    m->slab_floats = std::max(M * D * 8, Md * D * 8);   // (split-K slabs of the encoder side: 4 slices, 8 for small handles)
    for (size_t bi = 0; bi < m->blocks.size(); ++bi) {   // split-K plans of small handles (conv_splits): room for their fp32 slabs
        int s = 0;
        while (s + 1 < 4 && (int)bi >= m->stage_first[s + 1]) ++s;
        const Block& b = m->blocks[bi];
        const bool first = (int)bi == m->stage_first[s];
        // c0 runs at the stage's INPUT resolution in its first block, c1 / c2 at the output resolution
        const int s_c0 = first && s > 0 ? s - 1 : s;
        m->slab_floats = std::max(m->slab_floats, (size_t)conv_splits(m, b.c0, s_c0) * B * m->stage_px[s_c0] * b.c0.Cout);
        m->slab_floats = std::max(m->slab_floats, (size_t)conv_splits(m, b.c1, s) * B * m->stage_px[s] * b.c1.Cout);
    }
    RCCHK(dalloc(m, &m->d_slab, m->slab_floats, false));
    RCCHK(dalloc(m, &m->d_x16, M * D, false));
    RCCHK(dalloc(m, &m->d_xp16, M * D, false));
    RCCHK(dalloc(m, &m->d_qkv16, M * 3 * D, false));
    RCCHK(dalloc(m, &m->d_attn16, M * D, false));
    RCCHK(dalloc(m, &m->d_ffn16, M * a.ffn, false));
    RCCHK(dalloc(m, &m->d_memkv16, M * 2 * D * a.dec_layers, false));
    RCCHK(dalloc(m, &m->d_h32, Md * D, false));
    RCCHK(dalloc(m, &m->d_yd32, Md * D, false));
    RCCHK(dalloc(m, &m->d_hs32, Md * D, false));
    RCCHK(dalloc(m, &m->d_h16, Md * D, false));
    RCCHK(dalloc(m, &m->d_qkvd16, Md * 3 * D, false));
    RCCHK(dalloc(m, &m->d_qd16, Md * D * a.dec_layers, false));   // (every layer's cross-attention queries stay: opd_detr_attention_map)
    RCCHK(dalloc(m, &m->d_amap, (size_t)lvl[5] + 64, false));
    RCCHK(dalloc(m, &m->d_amap_stat, (size_t)a.queries * a.heads * 2, false));
    RCCHK(dalloc(m, &m->d_amap_sel, (size_t)a.queries, false));
    RCCHK(dalloc(m, &m->d_attnd16, Md * D, false));
    RCCHK(dalloc(m, &m->d_ffnd16, Md * a.ffn, false));
    RCCHK(dalloc(m, &m->d_dq16, Md * D, false));
    RCCHK(dalloc(m, &m->d_dk16, B * 8 * 8 * 512, false));   // (fragment order: 8 heads x 8 key tiles x 1 KiB per frame)
    RCCHK(dalloc(m, &m->d_dvT, B * 8 * 8 * 512, false));
    RCCHK(dalloc(m, &m->d_part_o, (size_t)m->sw.dec_splits * Md * D, false));
    RCCHK(dalloc(m, &m->d_part_ml, (size_t)m->sw.dec_splits * Md * a.heads * 2, false));
    RCCHK(dalloc(m, &m->d_ffn_part, (size_t)(a.ffn / OPD_DEC_FFN_CHUNK + 1) * Md * D, false));
    RCCHK(fill_qc0(m));
    RCCHK(dalloc(m, &m->d_logits, Md * a.ncls, false));
    RCCHK(dalloc(m, &m->d_boxes, Md * 4, false));
    // records of max_batch frames, the per-frame counts right behind them: ONE device-to-host copy fetches both
    // (and behind the counts, 32-byte aligned, room for one feature row per record: opd_detr_detect_frames_features fetches all three at once)
    const size_t cnt_units = ((size_t)B * 4 + sizeof(opd_det) - 1) / sizeof(opd_det);
    RCCHK(dalloc(m, &m->d_records, Md + cnt_units + Md * D * 4 / sizeof(opd_det), false));
    m->d_counts = reinterpret_cast<int32_t*>(m->d_records + Md);
    m->d_feat_all = reinterpret_cast<float*>(m->d_records + Md + cnt_units);
    RCCHK(dalloc(m, &m->d_orig_hw, B * 2, false));
    RCCHK(dalloc(m, &m->d_valid_hw, B * 2, false));
    RCCHK(dalloc(m, &m->d_key_valid, B * 2, false));
    RCCHK(dalloc(m, &m->d_bias_ptrs, (size_t)(a.enc_layers + 2) * B, false));
    RCCHK(dalloc(m, &m->d_rois, (size_t)128 * 4, false));
    RCCHK(dalloc(m, &m->d_roi_out, (size_t)128 * D, false));
    return OPD_OK;
}

static int get_plan(opd_detr* m, int fh, int fw, int vh, int vw, Plan** out) {
    // the cache lives with the weights; a fold is built once, on the calling handle's stream, and is complete (stream
    // synchronised) before the lock is released.  Its buffers belong to the WeightSet: they may outlive this handle.
    std::lock_guard<std::mutex> plan_lock(m->weights->plan_mu);
    auto& plans = m->weights->plans;
    for (auto& p : plans)
        if (p->fh == fh && p->fw == fw && p->vh == vh && p->vw == vw) { *out = p.get(); return OPD_OK; }
    struct Unseal {
        opd_detr* m;
        explicit Unseal(opd_detr* mm) : m(mm) { m->weights_sealed = false; }
        ~Unseal() { m->weights_sealed = true; }
    } unseal(m);
    const Arch& a = m->arch;
    const int D = a.d_model, hw = fh * fw;
    std::unique_ptr<Plan> p(new Plan());
    p->fh = fh; p->fw = fw; p->vh = vh; p->vw = vw;
    std::vector<float> pos;
    sine_pos_embed(fh, fw, vh, vw, D, &pos);
    float* d_pos = nullptr;
    RCCHK(upload_f32(m, &d_pos, pos));
    p->d_pos = d_pos;
    p->rb_enc.resize(a.enc_layers);
    for (int i = 0; i < a.enc_layers; ++i) RCCHK(upload_fold(m, d_pos, m->h_enc_cat_w[i], m->h_enc_cat_b[i], hw, 768, D, &p->rb_enc[i]));
    RCCHK(upload_fold(m, d_pos, m->h_kv_cat_w, m->h_kv_cat_b, hw, a.dec_layers * 512, D, &p->rb_kv));
    HIPCHK(hipStreamSynchronize(m->stream));
    *out = p.get();
    plans.push_back(std::move(p));
    return OPD_OK;
}

// ---- one launch of the forward (opd_model.h: launch) ---------------------------------------------------------------
static int tap(opd_detr* m, hipStream_t s, const Tap& t) {
    if (!m->taps || !m->d_taps || m->tap_next >= OPD_MAX_TAPS) return OPD_OK;
    HIPCHK(opd_launch_checksum(t.p, t.bytes, m->d_taps + (size_t)m->tap_next * OPD_TAP_BLOCKS, s));
    if ((int)m->tap_names.size() <= m->tap_next) m->tap_names.resize(m->tap_next + 1);
    m->tap_names[m->tap_next++] = t.name;
    return OPD_OK;
}
int launch_end(opd_detr* m, hipStream_t s, std::initializer_list<Tap> taps) {
    if (m->profiling == 1) RCCHK(m->timer.end(s));
    for (const Tap& t : taps)
        if (t.name && t.p) RCCHK(tap(m, s, t));
    return OPD_OK;
}
// profiling mode 1: the timer's marks of the calls since the last forward began -> the kernel table (longest first) and the class sums
void timed_collect(opd_detr* m) {
    static const char* const cls_name[4] = {"(convolution)", "(linear layer)", "(attention)", "(other)"};
    for (int c = 0; c < 4; ++c) { m->class_ms[c] = 0.f; m->class_launches[c] = 0; m->class_flops[c] = 0.0; }
    m->ktable.clear();
    (void)m->timer.fold(&m->ktable, cls_name);
    for (const auto& t : m->timer.marks)
        if (t.ms >= 0.f) { m->class_ms[t.cls] += t.ms; m->class_launches[t.cls] += 1; m->class_flops[t.cls] += t.flops; }
    std::sort(m->ktable.begin(), m->ktable.end(), [](const KernelRow& a, const KernelRow& b) { return a.ms > b.ms; });
    for (auto& r : m->ktable) {   // OPD_LAUNCH((kernel<a, b>), ...): the name without its parentheses (the class labels keep theirs)
        const bool label = std::find_if(cls_name, cls_name + 4, [&](const char* c) { return r.name == c; }) != cls_name + 4;
        if (!label && r.name.size() > 1 && r.name.front() == '(' && r.name.back() == ')') r.name = r.name.substr(1, r.name.size() - 2);
    }
}

// ---- the per-call context of one forward ---------------------------------------------------------------------------
struct PosShadow { const float* pos; const float* const* pos_ptrs; int period; f16_t* yp16; };   // second fp16 output of a reduce + LN
struct Fwd {
    opd_detr* m;
    hipStream_t stream;   // where this chain of the forward launches: m->stream, or m->stream2 for the stage-3 split's second chain
    int B, H, W;
    Dims d;
    int D, F, Q, Md, NKV;   // d_model, FFN width, queries, decoder rows (B x Q), columns of the memory K/V projection
    Plan* plan = nullptr;
    // ragged batches only: device arrays of B per-frame pointers (bias folds per encoder layer, K/V fold, position embeddings), valid sizes
    const float* const* enc_bias_ptrs[16] = {};
    const float* const* kv_bias_ptrs = nullptr;
    const float* const* pos_ptrs = nullptr;
    const int32_t *d_valid = nullptr, *d_keyv = nullptr;
    // from the trunk on: the feature map [B][fh][fw][proj.K], its tokens per frame and in all
    const f16_t* feat = nullptr;
    int fh = 0, fw = 0, hw = 0, M = 0;
    bool shadow = false;   // the position shadow is in use (fwd_encoder)
    PosShadow psh{};
    const PosShadow* ps() const { return shadow ? &psh : nullptr; }
    template <typename Fn>
    int launch(int cls, double flops, Fn&& issue, std::initializer_list<Tap> taps = {}) const { return opd::launch(m, stream, cls, flops, issue, taps); }
};

// ---- parameter builders: what every implicit-GEMM / attention launch of the forward has in common ------------------
// a pointwise GEMM out[M][N] = x[M][K] . w[N][K]^T + bias, as a 1x1 "convolution" over M pixels
static ConvGemmParams gemm_params(const opd_detr* m, const f16_t* x, const f16_t* w, const float* bias, void* out, int M, int N, int K) {
    ConvGemmParams p{}; p.dtype = m->dtype;
    p.x = x; p.w = w; p.bias = bias; p.out = out; p.zero16 = m->zero_bias;
    p.B = M; p.H = 1; p.W = 1; p.Cin = K; p.OH = 1; p.OW = 1; p.N = N; p.KH = 1; p.KW = 1; p.stride = 1; p.pad = 0;
    p.M = M; p.K = K; p.dbg = m->sw.dbg_gemm; p.wprefetch = m->sw.wprefetch & 1;
    return p;
}
static ConvGemmParams conv_params(const opd_detr* m, const Conv& c, const f16_t* x, int B, int H, int W, int OH, int OW, void* out, bool relu) {
    ConvGemmParams p = gemm_params(m, x, c.w, c.bias, out, B * OH * OW, c.Cout, c.K);
    p.B = B; p.H = H; p.W = W; p.Cin = c.Cin; p.OH = OH; p.OW = OW; p.KH = c.KH; p.KW = c.KW; p.stride = c.stride; p.pad = c.pad;
    p.relu = relu ? 1 : 0; p.stem = c.stem ? 1 : 0;
    return p;
}
static AttnParams attn_params(const Fwd& c, const f16_t* q, int ldq, const f16_t* k, int ldk, const f16_t* v, int ldv, f16_t* o, int ldo, int Lq, int Lk,
                              const int32_t* key_valid, int key_row) {
    AttnParams p{}; p.dtype = c.m->dtype;
    p.key_valid = key_valid; p.key_row = key_row;
    p.q = q; p.k = k; p.v = v; p.o = o; p.B = c.B; p.heads = c.m->arch.heads; p.Lq = Lq; p.Lk = Lk;
    p.ldq = ldq; p.ldk = ldk; p.ldv = ldv; p.ldo = ldo;
    p.scale = 1.0f / sqrtf((float)(c.m->arch.d_model / c.m->arch.heads));
    return p;
}
static double attn_flops(const AttnParams& p) { return 4.0 * p.B * (double)p.heads * p.Lq * p.Lk * 32; }

// a convolution of `B` frames (the stage-3 split's chains run part of the batch)
static int run_conv(const Fwd& c, const Conv& cv, const f16_t* x, int B, int H, int W, int OH, int OW, void* out, bool relu, const f16_t* res16, int stage = -1) {
    opd_detr* m = c.m;
    ConvGemmParams p = conv_params(m, cv, x, B, H, W, OH, OW, out, relu);
    p.res16 = res16;
    // algorithmic FLOPs (2 x MAC over the real taps/channels; the stem's zero padding is not counted)
    const double flops = 2.0 * p.M * (double)cv.Cout * cv.KH * cv.KW * cv.Cin;
    const size_t n = (size_t)p.M * cv.Cout;
    const Tap t{cv.KH == 3 ? "conv3x3" : "conv1x1", out, n * 2};
    if (const int splits = res16 ? 1 : conv_splits(m, cv, stage); splits > 1 && (size_t)splits * n <= m->slab_floats) {
        p.out = m->d_slab; p.out_f32 = 1; p.relu = 0; p.split_k = splits;
        RCCHK(c.launch(CLS_CONV, flops, [&] { return opd_launch_conv_gemm(p, c.stream); }));
        return c.launch(CLS_OTHER, 0.0, [&] { return opd_launch_reduce_act16(m->d_slab, splits, n, reinterpret_cast<f16_t*>(out), n, relu ? 1 : 0, c.stream, m->dtype); }, {t});
    }
    // Wide layers with few row tiles (stage 4) through the eight-wave kernel (kernels_w8.hip; identical bits).  The choice follows the handle's
    // CONFIGURATION (max_batch and the layer), never the batch at hand.  OPD_W8: bit 0 = 3x3, bit 1 = 1x1 with K >= 1024, bit 2 = 1x1 with K = 512.
    bool w8 = false;
    if (m->sw.w8 && cv.Cout % 256 == 0 && cv.Cout >= 512) {
        const long long tiles = (((long long)OH * OW * m->cfg.max_batch + 127) / 128) * (cv.Cout / 256);
        const bool few = tiles <= 3LL * m->num_cus;
        const int kind = cv.KH == 3 ? (m->sw.w8 & 1) : (cv.K >= 1024 ? (m->sw.w8 & 2) : (cv.K == 512 ? (m->sw.w8 & 4) : 0));
        w8 = few && kind && opd_conv_w8_supported(p);
    }
    return c.launch(CLS_CONV, flops, [&] { return w8 ? opd_launch_conv_w8(p, c.stream) : opd_launch_conv_gemm(p, c.stream); }, {t});
}

// a pointwise GEMM the caller has described (gemm_params + what differs)
static int run_gemm(const Fwd& c, const ConvGemmParams& p) {
    return c.launch(CLS_GEMM, 2.0 * p.M * (double)p.N * p.K, [&] { return opd_launch_conv_gemm(p, c.stream); }, {{"gemm", p.out, (size_t)p.M * p.N * (p.out_f32 ? 4 : 2)}});
}
// out16 = x16 . w^T + bias, bias a vector or (period > 0) a row-periodic table; optionally ReLU
static int run_linear(const Fwd& c, const f16_t* x, const f16_t* w, const float* bias, int bias_period, int M, int N, int K, f16_t* out, bool relu) {
    ConvGemmParams p = gemm_params(c.m, x, w, bias, out, M, N, K);
    p.bias_period = bias_period; p.relu = relu ? 1 : 0;
    return run_gemm(c, p);
}
// A projection of the encoder's tokens whose first `pos_cols` of every `mod` output columns see x + pos and the others x: either from the position
// shadow with the plain bias vector, or from x alone with the [hw][N] table W.pos + b (`table_ptrs`: one table per frame, ragged batches)
static int run_pos_proj(const Fwd& c, const f16_t* w, const float* bias_vec, const float* table, const float* const* table_ptrs, int N, int mod, int pos_cols, f16_t* out) {
    opd_detr* m = c.m;
    ConvGemmParams p = gemm_params(m, c.shadow ? m->d_xp16 : m->d_x16, w, c.shadow ? bias_vec : table, out, c.M, N, c.D);
    if (c.shadow) { p.x_alt = m->d_x16; p.alt_mod = mod; p.alt_cols = pos_cols; }
    else { p.bias_period = c.hw; p.bias_ptrs = table_ptrs; p.bias_pmod = mod; p.bias_pcols = pos_cols; }
    return run_gemm(c, p);
}

// Split-K flavour for skinny / deep-K linears: slices write fp32 slabs, then ONE fused kernel reduces them in slice
// order, adds the residual stream and applies the post-LayerNorm (gamma == nullptr: plain sum, e.g. input_projection).
static int run_gemm_splitk_ln(const Fwd& c, const f16_t* x, const f16_t* w, const float* bias, int M, int N, int K, int splits, const float* res32,
                              const LNp* ln, float* y32, f16_t* y16, int cls, const PosShadow* ps = nullptr) {
    opd_detr* m = c.m;
    ConvGemmParams p = gemm_params(m, x, w, bias, m->d_slab, M, N, K);
    p.out_f32 = 1; p.split_k = splits; p.dbg = 0; p.wprefetch = 0;   // (the sliced launch takes neither the ablation bits nor the weight warm-up)
    RCCHK(c.launch(cls, 2.0 * M * (double)N * K, [&] { return opd_launch_conv_gemm(p, c.stream); }, {{"splitk_slabs", m->d_slab, (size_t)splits * M * N * 4}}));
    return c.launch(CLS_OTHER, 0.0, [&] {
        return opd_launch_reduce_ln_pos(m->d_slab, splits, (size_t)M * N, res32, ln ? ln->g : nullptr, ln ? ln->b : nullptr, y32, y16, M, ps ? ps->pos : nullptr,
                                        ps ? ps->pos_ptrs : nullptr, ps ? ps->period : 0, ps ? ps->yp16 : nullptr, c.stream, m->dtype);
    }, {{"reduce_ln", y32, (size_t)M * N * 4}});
}

// y = LayerNorm(x16 . w^T + bias + res32): one launch (kernels_rowln.hip); y32 may alias res32
static int run_gemm_ln(const Fwd& c, const f16_t* x, const f16_t* w, const float* bias, int M, int K, const float* res32, const LNp& ln, float* y32, f16_t* y16) {
    GemmLnParams p{}; p.dtype = c.m->dtype;
    p.x = x; p.w = w; p.bias = bias; p.res32 = res32; p.gamma = ln.g; p.beta = ln.b; p.y32 = y32; p.y16 = y16; p.M = M; p.K = K;
    return c.launch(CLS_GEMM, 2.0 * M * 256.0 * K, [&] { return opd_launch_gemm_ln(p, c.stream); }, {{"gemm_ln", y32, (size_t)M * 256 * 4}});
}
// Deep-K row-owner launches (kernels_rowln.hip::gemm_ln256_ring_kernel) for the two K = 2048 -> 256 linears of the encoder side:
// the input projection (no LayerNorm) and every layer's FFN-2 (+ residual + LayerNorm); both also write the position shadow
static int run_deep(const Fwd& c, const f16_t* x, const f16_t* w, const float* bias, int K, const float* res32, const LNp* ln, int cls) {
    opd_detr* m = c.m;
    GemmLnParams gp{}; gp.dtype = m->dtype;
    gp.x = x; gp.w = w; gp.bias = bias; gp.res32 = res32; gp.gamma = ln ? ln->g : nullptr; gp.beta = ln ? ln->b : nullptr;
    gp.y32 = m->d_x32; gp.y16 = m->d_x16; gp.M = c.M; gp.K = K; gp.deep_k = 1;
    if (const PosShadow* ps = c.ps()) { gp.pos = ps->pos; gp.pos_ptrs = ps->pos_ptrs; gp.pos_period = ps->period; gp.yp16 = ps->yp16; }
    return c.launch(cls, 2.0 * c.M * (double)c.D * K, [&] { return opd_launch_gemm_ln(gp, c.stream); }, {{ln ? "fc2_ln_ring" : "input_proj_ring", m->d_x32, (size_t)c.M * c.D * 4}});
}

// Decoder-sized linear layer (M = B x queries, K a multiple of 256): the one-shot kernel of kernels_rowln.hip; K > 256 is
// cut into 256-wide slices whose fp32 slabs are summed by the fused reduce + residual + LayerNorm kernel.
static int run_small_gemm(const Fwd& c, const f16_t* x, const f16_t* w, const float* bias, int bias_period, int M, int N, int K, f16_t* out16, bool relu) {
    GemmK256Params p{}; p.dtype = c.m->dtype;
    p.x = x; p.w = w; p.bias = bias; p.out16 = out16; p.M = M; p.N = N; p.ldx = K; p.ldw = K; p.slices = 1;
    p.bias_period = bias_period; p.relu = relu ? 1 : 0;
    return c.launch(CLS_GEMM, 2.0 * M * (double)N * K, [&] { return opd_launch_gemm_k256(p, c.stream); }, {{"gemm_k256", out16, (size_t)M * N * 2}});
}
static int run_small_gemm_ln(const Fwd& c, const f16_t* x, const f16_t* w, const float* bias, int M, int K, const float* res32, const LNp& ln, float* y32, f16_t* y16) {
    opd_detr* m = c.m;
    GemmK256Params p{}; p.dtype = m->dtype;
    p.x = x; p.w = w; p.bias = bias; p.out32 = m->d_slab; p.M = M; p.N = 256; p.ldx = K; p.ldw = K; p.slices = K / 256;
    RCCHK(c.launch(CLS_GEMM, 2.0 * M * 256.0 * K, [&] { return opd_launch_gemm_k256(p, c.stream); }));
    return c.launch(CLS_OTHER, 0.0, [&] { return opd_launch_reduce_ln(m->d_slab, p.slices, (size_t)M * 256, res32, ln.g, ln.b, y32, y16, M, c.stream, m->dtype); },
                    {{"small_gemm_ln", y32, (size_t)M * 256 * 4}});
}

// attention into [B][Lq][d_model] rows
static int run_attn(const Fwd& c, const f16_t* q, int ldq, const f16_t* k, int ldk, const f16_t* v, int ldv, f16_t* o, int Lq, int Lk,
                    const int32_t* key_valid = nullptr, int key_row = 0) {
    const int D = c.m->arch.d_model;
    const AttnParams p = attn_params(c, q, ldq, k, ldk, v, ldv, o, D, Lq, Lk, key_valid, key_row);
    return c.launch(CLS_ATTN, attn_flops(p), [&] { return opd_launch_attention(p, c.stream); }, {{"attention", o, (size_t)c.B * Lq * D * 2}});
}

// The trunk plan (opd_model.h).  Every decision about how a bottleneck block runs is made here, from shapes and configuration only;
// trunk_blocks walks the steps and launches.
TrunkPlan plan_trunk(const Arch& a, const std::vector<Block>& blocks, const opd_config& cfg, const Switches& sw, int B, int H2, int W2, int num_cus,
                     bool taps, int profiling, bool has_stream2) {
    TrunkPlan plan;
    plan.steps.resize(blocks.size());
    plan.split = B;
    const bool multi = (cfg.flags & OPD_FLAG_MULTI_STREAM) != 0;
    int ch = H2, cw = W2, oh3 = 0, ow3 = 0;
    for (int s = 0, bi = 0; s < 4; ++s) {
        for (int l = 0; l < a.depths[s]; ++l, ++bi) {
            const Block& b = blocks[bi];
            const Block* nbk = bi + 1 < (int)blocks.size() ? &blocks[bi + 1] : nullptr;
            const int oh = (b.c1.stride == 2) ? down2(ch) : ch, ow = (b.c1.stride == 2) ? down2(cw) : cw;
            const int C1 = b.c1.Cin;
            // first block of stage 1 (64 -> 256 channels, stride 1): the shortcut runs inside the fused tail (kernels_btail.hip, SC)
            const bool sc_in_tail = b.has_sc && sw.fuse_shortcut && sw.fuse_btail && block_has_bias2sc(b) && b.sc.KH == 1 && b.sc.stride == 1 &&
                                    b.sc.Cin == 64 && b.c1.Cin == 64 && b.c1.stride == 1 && b.c2.Cout == 256 && nbk && conv_has_kperm(nbk->c0) &&
                                    nbk->c0.Cin == 256 && nbk->c0.Cout == 64;
            bool tail = sw.fuse_btail && b.c1.KH == 3 && b.c1.Cout == C1 && b.c2.Cin == C1 && b.c2.Cout == 4 * C1 && conv_has_kperm(b.c2) &&
                        opd_btail_supported(C1, 0);
            // what the one-launch form of the dual-source route needs of the block (below): a 128-channel tail shape
            const bool tail128 = tail && C1 == 128;
            // first block of stage 2: 3x3 + dual-source expand (+ the next reduce on its own) beats shortcut launch + fused tail
            // (stage 2: 0.674 -> 0.657 ms; OPD_DUAL_OVER_TAIL=0 restores the tail)
            if (sw.dual_over_tail && tail && b.has_sc && !sc_in_tail && block_has_w2sc(b)) tail = false;
            // Stage 3: the eight-wave tail holds one 160-KiB workgroup per CU, so a launch costs whole ROUNDS of ~70 us whatever they hold.
            // Rounds that are only partly filled because the batch does not divide into them are dealt with by the frame split below; what
            // remains is the case of too few tiles for even one round (small frames / batches: the three launches win there).  The choice is
            // made from the handle's configuration (max_batch and the frame size), never from the batch at hand: the two paths differ in
            // the last bit (kernels_btail3.hip), and a frame's low-order bits must not depend on the batch it travels in.  Handles that
            // keep several batches in flight (OPD_FLAG_MULTI_STREAM) always take the fused tail: other streams fill its idle CUs.
            if (C1 == 256 && tail) {
                const long long tiles = ((long long)cfg.max_batch * oh * ow + 127) / 128;
                const bool pays = tiles * 10 >= (long long)num_cus * 6;
                if (sw.tail3 == 0 || (sw.tail3 == 1 && !pays && !multi)) tail = false;
            }
            // first block of stages 3 / 4: the shortcut is extra K of the 1x1 expand (conv_gemm_dma_kernel, DUAL)
            const bool sc_in_expand = b.has_sc && sw.fuse_shortcut && block_has_w2sc(b) && !sc_in_tail && !tail;
            tail = tail && (size_t)B * ch * cw * C1 * 2 < 0x7ff00000ull;
            TrunkStep& t = plan.steps[bi];
            t.path = tail ? PATH_TAIL : sc_in_expand ? PATH_DUAL : PATH_CONVS;
            t.sc = !b.has_sc ? SC_NONE : (sc_in_tail && tail) ? SC_TAIL : sc_in_expand ? SC_EXPAND : SC_LAUNCH;
            t.res = (t.sc == SC_TAIL || t.sc == SC_EXPAND) ? RES_NONE : t.sc == SC_LAUNCH ? RES_SHORTCUT : RES_TRUNK;
            t.store = STORE_Y;
            t.C3 = 0;
            if (tail && nbk && conv_has_kperm(nbk->c0) && nbk->c0.Cin == 4 * C1 && opd_btail_supported(C1, nbk->c0.Cout)) t.C3 = nbk->c0.Cout;
            // First block of stage 2 (256 -> 512 channels, stride 2) on the dual-source route: its 3x3, its expand over [a1 | block input] and the
            // next block's reduce are issued as ONE launch of the fused tail with the shortcut inside (kernels_btail.hip, SC2).  The route is
            // still the dual-source one -- same operands (bias2sc), same K order, same rounding points, hence the same bits -- so the step stays
            // PATH_DUAL / SC_EXPAND and `one_launch` says how it is issued; OPD_SC2_TAIL=0 restores the three launches.
            t.one_launch = t.one_C3 = t.one_rev = 0;
            if (t.path == PATH_DUAL && sw.sc2_tail && sw.fuse_btail && tail128 && b.sc.KH == 1 && b.sc.stride == b.c1.stride &&
                opd_btail_sc_supported(C1, 0, b.sc.Cin, b.c1.stride) && (size_t)B * ch * cw * b.sc.Cin * 2 < 0x7ff00000ull) {
                t.one_launch = 1;
                if (nbk && conv_has_kperm(nbk->c0) && nbk->c0.Cin == 4 * C1 && opd_btail_sc_supported(C1, nbk->c0.Cout, b.sc.Cin, b.c1.stride)) t.one_C3 = nbk->c0.Cout;
                t.one_rev = sw.tail_rev ? 1 : 0;   // from the rows stage 1's last tail wrote last (measured: the other direction reads the same)
            }
            // The last block of stage 1 hands the next stage its reduce output z (fused above); the block output itself is then read
            // by that stage's stride-2 shortcut only, i.e. at even (oh, ow): the other three quarters of its 274 MB are not stored.
            if (tail && sw.y_stride2 && t.C3 && b.c1.stride == 1 && l + 1 == a.depths[s] && nbk && nbk->has_sc && nbk->sc.stride == 2 && nbk->sc.KH == 1 &&
                nbk->c1.stride == 2 && !taps)
                t.store = STORE_Y_STRIDE2;
            // Stage 1, residual rebuild (BtailParams::rc), decided per pair: the previous block stores its a1 (64 channels) instead of its output
            // (256) only if THIS block rebuilds that output chunk by chunk from a1 and the previous block's input (the shortcut's input) as its
            // residual -- which the rc kernel does for a 64 -> 64 tail without a shortcut behind a tail with the shortcut inside.  Bit-identical
            // results (tests/test_kernels_gpu.py, OPD_TAIL_RC=0/1 end to end); 344 MB less HBM traffic per forward at batch 8.
            if (l > 0 && sw.tail_rc && !taps) {
                TrunkStep& prev = plan.steps[bi - 1];
                if (prev.path == PATH_TAIL && prev.sc == SC_TAIL && prev.C3 == 64 && prev.store == STORE_Y && tail && C1 == 64 && t.C3 == 64 &&
                    t.res == RES_TRUNK) {
                    prev.store = STORE_A1;
                    t.res = RES_REBUILD;
                }
            }
            if (s == 2 && l == 0) { oh3 = oh; ow3 = ow; }
            ch = oh; cw = ow;
        }
    }
    // Stage 3.  Frame split: with the fused tails a launch of T tiles costs ceil(T / CUs) rounds, and batch 8 at 800x1333 is 263 tiles on
    // 256 CUs.  Frames are independent, so blocks 1 .. n-1 of the stage (all tensors there have one per-frame size, the buffers of the
    // two chains never overlap) run as TWO chains on two streams -- frames [0, split) = whole rounds, the rest on `stream2` -- whose
    // workgroups the hardware packs onto whatever CU is free: 5 tails of 263 workgroup-lives take ~5.3 rounds instead of 10.  Per-row
    // arithmetic does not depend on the tiling, so this is invisible in the results (any batch, any split).  Captured into the graph
    // as a fork / join; not under profiling (event pairs on one stream) or diagnostic taps, and not for handles that keep several batches
    // in flight (there other handles' kernels fill the idle CUs; measured on one box, 1000 steps x 2: three streams 2841 frames/s with
    // one launch per tail, 2783 with the split, 2793 unfused; one stream 2045 / 2112 / 2090).
    const int s3 = a.depths[0] + a.depths[1], s4 = s3 + a.depths[2];
    bool fused3 = a.depths[2] > 2 && profiling != 1 && !taps && has_stream2 && sw.tail3_split && !multi && B >= 2;
    for (int bi = s3 + 1; bi < s4 && fused3; ++bi) fused3 = plan.steps[bi].path == PATH_TAIL;
    if (fused3) {
        auto tiles_of = [&](int frames) { return ((long long)frames * oh3 * ow3 + 127) / 128; };
        const long long total = tiles_of(B), cus = num_cus, last = total % cus;
        if (total > cus && last > 0 && last < cus / 2) {
            const long long whole = (total / cus) * cus;
            int bA = B - 1;
            while (bA > 1 && tiles_of(bA) > whole) --bA;
            if (tiles_of(bA) <= whole) plan.split = bA;
        }
    }
    // consecutive fused tails walk their tiles in alternating directions (Switches::tail_rev), counted in launch order: the split's second
    // chain comes between the first chain and stage 4
    int n = 0;
    auto rev = [&](const TrunkStep& t) { return t.path == PATH_TAIL && sw.tail_rev ? (n++ & 1) : 0; };
    for (int bi = 0; bi < s4; ++bi) plan.steps[bi].rev = rev(plan.steps[bi]);
    for (int bi = s3 + 1; bi < s4 && plan.split < B; ++bi) plan.steps[bi].rev_b = rev(plan.steps[bi]);
    for (int bi = s4; bi < (int)blocks.size(); ++bi) plan.steps[bi].rev = rev(plan.steps[bi]);
    return plan;
}

// The transformer plan (opd_model.h).  Every decision about the launch sequence behind the trunk is made here; fwd_encoder, fwd_memory_kv,
// fwd_decoder_fused / fwd_decoder_chain and fwd_heads walk it and launch.  Which packed weights exist comes from the rules build_weights
// reads (opd_model.h); what build_weights makes unconditionally (bqkv, bkv_all, dec0_h, qc0) is not tested for.
TransformerPlan plan_transformer(const Arch& a, const opd_config& cfg, const Switches& sw, size_t stage4_px, int B, int fh, int fw) {
    TransformerPlan t;
    const int D = a.d_model, F = a.ffn, Q = a.queries, Kp = a.hidden[3];
    const size_t M = (size_t)B * fh * fw, NKV = (size_t)a.dec_layers * 2 * D;
    const bool row256 = D == 256;   // the row-owner kernels' width (kernels_rowln.hip, kernels_dec.hip)
    // pos_shadow: whoever writes x (input projection, each layer's last LayerNorm) also writes fp16(x + pos); the fused QKV projection
    // reads that for its q / k column tiles and x for its v tiles, with a plain bias vector -- instead of x everywhere plus a [hw][768]
    // fp32 table W.pos + b added per output tile (two divisions and 16 dependent table loads per lane in front of the first MFMA:
    // 14.2 us per launch against 9.4 for the same GEMM with a bias vector; decoder K/V 44.7 against 24-27)
    t.shadow = sw.pos_shadow && row256;
    // Small handles (round 5): the row-owner launches of the encoder side own 48 / 64 rows per workgroup and stream a whole weight matrix through
    // each -- at max_batch = 1 that is 22 workgroups walking 2.2 MB apiece (42 us per layer, 27 us for the input projection).  Where the handle's
    // CONFIGURATION bounds the token count below ~1400 the same linears run as tiled GEMMs with the reduction split eight ways over workgroups
    // and the fixed-order reduce + LayerNorm kernel (the round-1 path): encoder stage 0.41 -> 0.32 ms at batch 1.  Never per batch.
    t.small_enc = sw.small_enc && (size_t)cfg.max_batch * stage4_px <= 1400;
    t.enc_splits = t.small_enc ? 8 : 4;
    auto splits_of = [&](int K) { return (K / 64) % t.enc_splits == 0 ? t.enc_splits : 4; };
    // the deep-K row-owner launch of a K -> 256 linear over the M tokens (32-bit offsets into its input)
    auto deep = [&](int K) { return sw.deep_fc2 && row256 && !t.small_enc && K % 64 == 0 && M * K * 2 < 0x7fffff00ull; };
    t.proj_splits = deep(Kp) ? 0 : splits_of(Kp);
    // the whole FFN block as ONE row-owner launch: the [M][F] hidden tensor never leaves LDS (kernels_rowln.hip::enc_ffn_kernel)
    const bool ffn_one = sw.fused_enc_ffn && sw.fuse_gemm_ln && enc_has_ffn_pack(a) && !t.small_enc;
    // fc2 + residual + LayerNorm (+ the position shadow) as ONE row-owner launch of the three-stage ring kernel: 36.9 us in the
    // forward against 19.4 + 12.2 us for split-K slabs + reduce, but 514 MB less HBM traffic per forward and half the CUs left to
    // other batches (+1.3 % with three streams, -5 us per layer for a lone stream; profiles/NOTES.md "Deep-K row owners")
    const int ffn_two = deep(F) ? FFN_FC1_DEEP : FFN_FC1_SPLITK;
    t.enc.resize(a.enc_layers);
    bool prev_tail = false;
    for (int i = 0; i < a.enc_layers; ++i) {
        EncStep& e = t.enc[i];
        const bool last = i + 1 == a.enc_layers;
        e.qkv = prev_tail ? QKV_PREV_TAIL : QKV_LAUNCH;
        e.oproj = ffn_one && sw.enc_front ? OPROJ_IN_FFN : sw.fuse_gemm_ln && row256 ? OPROJ_GEMM_LN : OPROJ_GEMM_THEN_LN;
        e.ffn = ffn_one ? FFN_ONE_LAUNCH : ffn_two;
        e.splits = e.ffn == FFN_FC1_SPLITK ? splits_of(F) : 0;
        // the tail projection: what consumes this block's output (only on the position-shadow path: x + pos with plain bias vectors; the
        // memory K/V rows are addressed with 32-bit byte offsets)
        e.tail = ffn_one && t.shadow && sw.enc_tail && (!last || M * NKV * 2 < (1ull << 32)) ? enc_pack_tail(a, i) : 0;
        prev_tail = e.tail > 0;
    }
    t.kv_launch = !prev_tail;
    t.dec0 = sw.fuse_dec0 && row256;
    // the fused decoder is taken when the architecture fits its kernels' fixed shapes
    t.dec_fused = sw.fused_dec && t.dec0 && a.heads == 8 && Q <= 128 && (Q & 3) == 0 && F % OPD_DEC_FFN_CHUNK == 0 && F / OPD_DEC_FFN_CHUNK <= 16 &&
                  sw.dec_splits <= 6 && dec_has_frag_weights(a) && M * NKV * 2 < (1ull << 32);
    t.dec_splits = sw.dec_splits;
    t.dec_small_m = sw.small_m_gemm && row256 && F % 256 == 0 && F / 256 <= 8;
    t.dec_oproj = sw.fuse_gemm_ln && row256 ? OPROJ_GEMM_LN : OPROJ_GEMM_THEN_LN;
    t.heads = sw.heads2 && heads_have_frag_weights(a) ? HEADS_SPLIT16 : HEADS_F32;
    t.heads_ln3 = t.dec_fused;
    t.heads_ln = t.dec_fused || sw.fuse_gemm_ln;
    return t;
}

// True when some frame of the batch does not fill the H x W canvas (a ragged batch: padding mask path).
static bool is_ragged(const int32_t* valid_hw, int B, int H, int W) {
    if (!valid_hw) return false;
    for (int b = 0; b < B; ++b)
        if (valid_hw[2 * b] != H || valid_hw[2 * b + 1] != W) return true;
    return false;
}

// ---- the forward, stage by stage (enqueue_forward below lists them) ------------------------------------------------
// A ragged batch: one plan per frame's valid feature map, their fold pointers and the valid sizes uploaded for the kernels that mask
static int fwd_prepare_ragged(Fwd& c, const int32_t* valid_hw) {
    opd_detr* m = c.m;
    const Arch& a = m->arch;
    const int B = c.B, fh = c.d.stage_h[3], fw = c.d.stage_w[3];
    if (a.enc_layers > 16) return fail(OPD_EINVAL, "ragged batches: at most 16 encoder layers");
    m->h_valid_hw.assign(valid_hw, valid_hw + 2 * B);
    m->h_key_valid.resize((size_t)2 * B);
    m->h_bias_ptrs.assign((size_t)(a.enc_layers + 2) * B, nullptr);
    for (int b = 0; b < B; ++b) {
        const int vh = valid_hw[2 * b], vw = valid_hw[2 * b + 1];
        if (vh < 1 || vw < 1 || vh > c.H || vw > c.W) return fail(OPD_EINVAL, "valid_hw outside the frame canvas");
        const int vfh = valid_prefix(vh, c.H, fh), vfw = valid_prefix(vw, c.W, fw);
        if (vfh < 1 || vfw < 1) return fail(OPD_EINVAL, "frame too small: no valid feature-map position");
        m->h_key_valid[2 * b] = vfh; m->h_key_valid[2 * b + 1] = vfw;
        Plan* pb = nullptr;
        RCCHK(get_plan(m, fh, fw, vfh, vfw, &pb));
        if (b == 0) c.plan = pb;
        for (int i = 0; i < a.enc_layers; ++i) m->h_bias_ptrs[(size_t)i * B + b] = pb->rb_enc[i];
        m->h_bias_ptrs[(size_t)a.enc_layers * B + b] = pb->rb_kv;
        m->h_bias_ptrs[(size_t)(a.enc_layers + 1) * B + b] = pb->d_pos;
    }
    // (member vectors: they outlive the asynchronous copies; every entry point synchronises before it returns)
    HIPCHK(hipMemcpyAsync(m->d_valid_hw, m->h_valid_hw.data(), (size_t)2 * B * 4, hipMemcpyHostToDevice, c.stream));
    HIPCHK(hipMemcpyAsync(m->d_key_valid, m->h_key_valid.data(), (size_t)2 * B * 4, hipMemcpyHostToDevice, c.stream));
    HIPCHK(hipMemcpyAsync(m->d_bias_ptrs, m->h_bias_ptrs.data(), m->h_bias_ptrs.size() * sizeof(float*), hipMemcpyHostToDevice, c.stream));
    for (int i = 0; i < a.enc_layers; ++i) c.enc_bias_ptrs[i] = m->d_bias_ptrs + (size_t)i * B;
    c.kv_bias_ptrs = m->d_bias_ptrs + (size_t)a.enc_layers * B;
    c.pos_ptrs = m->d_bias_ptrs + (size_t)(a.enc_layers + 1) * B;
    c.d_valid = m->d_valid_hw;
    c.d_keyv = m->d_key_valid;
    return OPD_OK;
}

// Stage 1's first 1x1 reduce (64 -> 64 on the pooled map) inside the fused stem launch (Switches::stem_reduce; kernels_gemm.hip, StemReduce):
// the stem writes that block's c0 output into the buffer the launch would have written, and the trunk starts with it in hand.  Every other
// case keeps the launch: another architecture, the two-kernel stem, diagnostic taps (which checksum every launch's own output).
static bool stem_reduces(const opd_detr* m) {
    if (!m->sw.stem_reduce || !m->sw.fuse_stem_pool || m->taps || m->blocks.empty() || m->arch.depths[0] < 1) return false;
    const Conv& c0 = m->blocks[0].c0;
    return c0.KH == 1 && c0.KW == 1 && c0.stride == 1 && c0.pad == 0 && c0.Cin == 64 && c0.Cout == 64 && c0.w && c0.bias;
}

// pre-processing, stem 7x7 and max-pool -> d_pool (and, stem_reduces: the first block's reduce -> d_m0)
static int fwd_stem(const Fwd& c, const void* d_pixels, int pixel_format) {
    opd_detr* m = c.m;
    const Dims& d = c.d;
    const int B = c.B, H = c.H, W = c.W;
    const int Hp = 2 * d.H1 + 6, Wp = 2 * d.W1 + 6;  // padded image seen by the stem: rows/cols 2*o + k, k = 0..7
    const bool u8 = pixel_format == OPD_PIXELS_U8_BGR_HWC;
    StemReduce red;
    if (stem_reduces(m)) { red.z0 = m->d_m0; red.w0 = m->blocks[0].c0.w; red.b0 = m->blocks[0].c0.bias; }
    const double flops = 2.0 * B * d.H1 * d.W1 * 64.0 * 147.0 + (red.z0 ? 2.0 * B * d.H2 * d.W2 * 64.0 * 64.0 : 0.0);
    if (m->sw.fuse_prep && m->sw.fuse_stem_pool && u8)
        return c.launch(CLS_CONV, flops, [&] {
            return opd_launch_stem_pool_u8(reinterpret_cast<const uint8_t*>(d_pixels), c.d_valid, m->stem.w, m->stem.bias, m->d_pool, B, H, W, d.H1, d.W1, d.H2, d.W2,
                                           c.stream, m->dtype, red);
        }, {{"stem_pool_u8", m->d_pool, (size_t)B * d.H2 * d.W2 * 64 * 2}});
    RCCHK(c.launch(CLS_OTHER, 0.0, [&] {
        return u8 ? opd_launch_preprocess_u8(reinterpret_cast<const uint8_t*>(d_pixels), m->d_x4, B, H, W, Hp, Wp, c.d_valid, c.stream, m->dtype)
                  : opd_launch_preprocess_f32(reinterpret_cast<const float*>(d_pixels), m->d_x4, B, H, W, Hp, Wp, c.d_valid, c.stream, m->dtype);
    }));
    if (m->sw.fuse_stem_pool)
        return c.launch(CLS_CONV, flops, [&] { return opd_launch_stem_pool(m->d_x4, m->stem.w, m->stem.bias, m->d_pool, B, Hp, Wp, d.H1, d.W1, d.H2, d.W2, c.stream, m->dtype, red); });
    // two kernels, for cross-checking: the stem as a stride-2 pointwise GEMM over the padded NHWC4 image's 8 x 8 x 4 windows, then the pool
    ConvGemmParams p = gemm_params(m, m->d_x4, m->stem.w, m->stem.bias, m->d_stem, B * d.H1 * d.W1, 64, 256);
    p.B = B; p.H = Hp; p.W = Wp; p.OH = d.H1; p.OW = d.W1; p.stride = 2; p.relu = 1; p.stem = 2;
    p.dbg = 0; p.wprefetch = 0;   // (this launch takes neither the ablation bits nor the weight warm-up)
    RCCHK(c.launch(CLS_CONV, 2.0 * p.M * 64.0 * 147.0, [&] { return opd_launch_conv_gemm(p, c.stream); }));
    return c.launch(CLS_OTHER, 0.0, [&] { return opd_launch_maxpool(m->d_stem, m->d_pool, B, d.H1, d.W1, 64, d.H2, d.W2, c.stream, m->dtype); });
}

// ---- trunk: the blocks of stages 1-4 as plan_trunk decided.  trunk_blocks launches blocks [l_begin, l_end) of stage s for frames
// [b0, b0 + nb) on c.stream: every tensor of those frames lives at frame offset b0 of its buffer (b0 > 0: the stage-3 split's second chain).
struct TrunkState { int cur_id; int ch, cw; int z_id; int prev_id; };   // cur_id / prev_id (the previous block's input) 0 = pool, 1 = t0, 2 = t1;
                                                                        // z_id -1 / 0 = m0 / 1 = m1: the z a fused tail computed for the next block
static int trunk_blocks(const Fwd& c, const TrunkPlan& tp, int s, int b0, int nb, TrunkState& st, int l_begin = 0, int l_end = 1 << 30) {
    opd_detr* m = c.m;
    auto trunk = [&](int id, size_t per_frame) { return (id == 0 ? m->d_pool : id == 1 ? m->d_t0 : m->d_t1) + (size_t)b0 * per_frame; };
    auto mid = [&](int id, size_t per_frame) { return (id ? m->d_m1 : m->d_m0) + (size_t)b0 * per_frame; };
    for (int l = l_begin; l < m->arch.depths[s] && l < l_end; ++l) {
        const int bi = m->stage_first[s] + l;
        const Block& b = m->blocks[bi];
        const TrunkStep& t = tp.steps[bi];
        const int ch = st.ch, cw = st.cw;
        const int oh = (b.c1.stride == 2) ? down2(ch) : ch, ow = (b.c1.stride == 2) ? down2(cw) : cw;
        const int C1 = b.c1.Cin, C2 = b.c2.Cout, C3 = t.one_launch ? t.one_C3 : t.C3;
        const f16_t* cur = trunk(st.cur_id, (size_t)ch * cw * b.c0.Cin);
        const int out_id = st.cur_id == 1 ? 2 : 1;
        f16_t* out = trunk(out_id, (size_t)oh * ow * C2);
        f16_t* const scb = m->d_sc + (size_t)b0 * oh * ow * C2;
        if (t.sc == SC_LAUNCH) RCCHK(run_conv(c, b.sc, cur, nb, ch, cw, oh, ow, scb, false, nullptr));
        const f16_t* res = t.res == RES_TRUNK ? cur : t.res == RES_SHORTCUT ? scb : nullptr;
        int x1_id = st.z_id;
        const f16_t* x1 = nullptr;
        if (x1_id >= 0) {
            x1 = mid(x1_id, (size_t)ch * cw * C1);
        } else {
            x1_id = 0;
            f16_t* c0out = mid(0, (size_t)ch * cw * b.c0.Cout);
            RCCHK(run_conv(c, b.c0, cur, nb, ch, cw, ch, cw, c0out, true, nullptr, (l == 0 && s > 0) ? s - 1 : s));
            x1 = c0out;
        }
        st.z_id = -1;
        if (t.path == PATH_TAIL || t.one_launch) {
            const Block* nbk = C3 ? &m->blocks[bi + 1] : nullptr;
            BtailParams p{}; p.dtype = m->dtype;
            p.x1 = x1; p.w1 = b.c1.w; p.b1 = b.c1.bias; p.w2p = C1 == 256 ? b.c2.wp : b.c2.w; p.b2 = b.c2.bias; p.res = res;   // (K-permuted copies: stage-3 kernel only)
            p.y = t.store == STORE_A1 ? nullptr : out;
            if (t.sc == SC_TAIL || t.one_launch) { p.xs = cur; p.wsc = b.sc.w; p.b2 = b.bias2sc; }
            f16_t* z = mid(1 - x1_id, (size_t)oh * ow * C3);
            if (C3) { p.w3p = C1 == 256 ? nbk->c0.wp : nbk->c0.w; p.b3 = nbk->c0.bias; p.z = z; }
            // stage 1's a1 hand-over (STORE_A1 -> RES_REBUILD) lives in the shortcut buffer, which a fused shortcut leaves unused
            f16_t* const a1_keep = m->d_sc + (size_t)b0 * oh * ow * C1;
            if (t.store == STORE_A1) p.a1_out = a1_keep;
            if (t.res == RES_REBUILD) {
                const Block& pb = m->blocks[bi - 1];
                p.rc = 1; p.rc_a1 = a1_keep; p.rc_xs = trunk(st.prev_id, (size_t)ch * cw * pb.c0.Cin); p.rc_w2 = pb.c2.w; p.rc_wsc = pb.sc.w; p.rc_b = pb.bias2sc;
            }
            p.y_stride2 = t.store == STORE_Y_STRIDE2;
            p.B = nb; p.H = ch; p.W = cw; p.OH = oh; p.OW = ow; p.stride = b.c1.stride; p.M = nb * oh * ow; p.C1 = C1; p.C3 = C3;
            p.rev = t.one_launch ? t.one_rev : b0 ? t.rev_b : t.rev;
            p.dbg = m->sw.dbg_btail | (C1 == 128 && !m->sw.res_dma128 ? 16 : 0);   // (bit 16: the residual through register loads)
            RCCHK(c.launch(CLS_CONV, 2.0 * p.M * ((double)C1 * 9 * C1 + 4.0 * C1 * C1 + 4.0 * C1 * C3 + (p.xs ? (double)b.sc.Cin * C2 : 0.0)),
                           [&] { return opd_launch_btail(p, c.stream); },
                           {{"btail_y", p.y ? out : nullptr, (size_t)p.M * 4 * C1 * 2}, {"btail_z", C3 ? z : nullptr, (size_t)p.M * C3 * 2}}));
            if (C3) st.z_id = 1 - x1_id;
        } else {
            f16_t* a1 = mid(1 - x1_id, (size_t)oh * ow * C1);
            RCCHK(run_conv(c, b.c1, x1, nb, ch, cw, oh, ow, a1, true, nullptr, s));
            if (t.path == PATH_DUAL) {   // the 1x1 expand over [a1 | the block input]: the shortcut as extra K
                ConvGemmParams p = gemm_params(m, a1, b.w2sc, b.bias2sc, out, nb * oh * ow, C2, C1 + b.sc.Cin);
                p.B = nb; p.H = oh; p.W = ow; p.OH = oh; p.OW = ow; p.Cin = C1; p.K1 = C1; p.relu = 1;
                p.x2 = cur; p.H2 = ch; p.W2 = cw; p.Cin2 = b.sc.Cin; p.stride2 = b.sc.stride;
                RCCHK(c.launch(CLS_CONV, 2.0 * p.M * (double)C2 * p.K, [&] { return opd_launch_conv_gemm(p, c.stream); }, {{"dual_expand", out, (size_t)p.M * C2 * 2}}));
            } else {
                RCCHK(run_conv(c, b.c2, a1, nb, oh, ow, oh, ow, out, true, res));
            }
        }
        st.prev_id = st.cur_id; st.cur_id = out_id; st.ch = oh; st.cw = ow;
    }
    return OPD_OK;
}

// Stage 3 with the frame split of plan_trunk: its first block (stride 2, shortcut) for the whole batch, then blocks 1.. as two chains of frames
static int trunk_stage3_split(const Fwd& c, const TrunkPlan& tp, TrunkState& st) {
    opd_detr* m = c.m;
    RCCHK(trunk_blocks(c, tp, 2, 0, c.B, st, 0, 1));
    if (tp.split == c.B) return trunk_blocks(c, tp, 2, 0, c.B, st, 1);
    TrunkState ta = st, tb = st;
    Fwd c2 = c;   // the second chain: the same call, launching on the branch stream
    c2.stream = m->stream2;
    HIPCHK(hipEventRecord(m->ev_fork, c.stream));
    HIPCHK(hipStreamWaitEvent(m->stream2, m->ev_fork, 0));
    // whatever happens in either chain, `stream2` is rejoined before this function returns (an unjoined fork would leak into
    // the next forward's events, or leave a capture with a dangling branch)
    const int rc_a = trunk_blocks(c, tp, 2, 0, tp.split, ta, 1);
    const int rc_b = rc_a == OPD_OK ? trunk_blocks(c2, tp, 2, tp.split, c.B - tp.split, tb, 1) : OPD_OK;
    const hipError_t ej = hipEventRecord(m->ev_join, m->stream2);
    const hipError_t ew = ej == hipSuccess ? hipStreamWaitEvent(c.stream, m->ev_join, 0) : ej;
    RCCHK(rc_a);
    RCCHK(rc_b);
    HIPCHK(ew);
    st = ta;
    return OPD_OK;
}

static int fwd_trunk(Fwd& c) {
    opd_detr* m = c.m;
    const TrunkPlan tp = plan_trunk(m->arch, m->blocks, m->cfg, m->sw, c.B, c.d.H2, c.d.W2, m->num_cus, m->taps != 0, m->profiling, m->stream2 != nullptr);
    TrunkState st{0, c.d.H2, c.d.W2, stem_reduces(m) ? 0 : -1, -1};   // (z_id 0: the stem launch has written the first block's reduce into d_m0)
    for (int s = 0; s < 4; ++s) {
        RCCHK(s == 2 ? trunk_stage3_split(c, tp, st) : trunk_blocks(c, tp, s, 0, c.B, st));
        MARK(2 + s);   // (stage 3 ends at the join of its two chains)
    }
    c.feat = st.cur_id == 1 ? m->d_t0 : m->d_t1;
    c.fh = st.ch; c.fw = st.cw; c.hw = st.ch * st.cw; c.M = c.B * c.hw;
    return OPD_OK;
}

// ---- input projection -> encoder, as plan_transformer decided
static int fwd_encoder(Fwd& c, const TransformerPlan& tp) {
    opd_detr* m = c.m;
    const Arch& a = m->arch;
    const int M = c.M, D = c.D, F = c.F;
    c.shadow = tp.shadow;
    c.psh = PosShadow{c.plan->d_pos, c.pos_ptrs, c.hw, m->d_xp16};
    const PosShadow* ps = c.ps();
    if (!tp.proj_splits) RCCHK(run_deep(c, c.feat, m->proj.w, m->proj.bias, m->proj.K, nullptr, nullptr, CLS_CONV));
    else RCCHK(run_gemm_splitk_ln(c, c.feat, m->proj.w, m->proj.bias, M, D, m->proj.K, tp.proj_splits, nullptr, nullptr, m->d_x32, m->d_x16, CLS_CONV, ps));
    for (int i = 0; i < a.enc_layers; ++i) {
        const EncLayer& L = m->enc[i];
        const EncStep& e = tp.enc[i];
        if (e.qkv == QKV_LAUNCH) RCCHK(run_pos_proj(c, L.wqkv, L.bqkv, c.plan->rb_enc[i], c.enc_bias_ptrs[i], 3 * D, 3 * D, 2 * D, m->d_qkv16));   // (pos enters q and k only)
        RCCHK(run_attn(c, m->d_qkv16, 3 * D, m->d_qkv16 + D, 3 * D, m->d_qkv16 + 2 * D, 3 * D, m->d_attn16, c.hw, c.hw, c.d_keyv, c.fw));
        if (e.oproj == OPROJ_GEMM_LN) {
            RCCHK(run_gemm_ln(c, m->d_attn16, L.o.w, L.o.b, M, D, m->d_x32, L.ln1, m->d_x32, m->d_x16));
        } else if (e.oproj == OPROJ_GEMM_THEN_LN) {
            ConvGemmParams p = gemm_params(m, m->d_attn16, L.o.w, L.o.b, m->d_y32, M, D, D);
            p.out_f32 = 1; p.res32 = m->d_x32;
            RCCHK(run_gemm(c, p));
            RCCHK(c.launch(CLS_OTHER, 0.0, [&] { return opd_launch_layernorm(m->d_y32, L.ln1.g, L.ln1.b, m->d_x32, m->d_x16, M, c.stream, m->dtype); }));
        }
        if (e.ffn == FFN_ONE_LAUNCH) {
            const bool front = e.oproj == OPROJ_IN_FFN, last = i + 1 == a.enc_layers;
            EncFfnParams fp{}; fp.dtype = m->dtype; fp.wprefetch = (m->sw.wprefetch >> 1) & 1;
            fp.x = m->d_x16; fp.wpack = L.ffn_pack; fp.b2 = L.fc2.b; fp.res32 = m->d_x32; fp.gamma = L.ln2.g; fp.beta = L.ln2.b;
            fp.y32 = m->d_x32; fp.y16 = m->d_x16; fp.M = M; fp.F = F; fp.pack_tail = enc_pack_tail(a, i); fp.pack_front = 1;
            if (front) { fp.attn = m->d_attn16; fp.bo = L.o.b; fp.gamma1 = L.ln1.g; fp.beta1 = L.ln1.b; }
            if (ps) { fp.pos = ps->pos; fp.pos_ptrs = ps->pos_ptrs; fp.pos_period = ps->period; fp.yp16 = ps->yp16; }
            if (e.tail) {   // the next layer's q | k | v, or the decoder's memory K/V
                fp.tail = e.tail; fp.tail_pos = L.tail_pos; fp.tail_ld = L.tail_ld;
                fp.tail_out = last ? m->d_memkv16 : m->d_qkv16;
                for (int t = 0; t < e.tail; ++t) fp.tail_col[t] = L.tail_col[t];
            }
            RCCHK(c.launch(CLS_GEMM, 4.0 * M * (double)D * F + 2.0 * M * (double)D * 256 * (fp.tail + (front ? 1 : 0)), [&] { return opd_launch_enc_ffn(fp, c.stream); },
                           {{"enc_ffn", m->d_x32, (size_t)M * D * 4}}));
        } else {
            RCCHK(run_linear(c, m->d_x16, L.fc1.w, L.fc1.b, 0, M, F, D, m->d_ffn16, true));
            if (e.ffn == FFN_FC1_DEEP) RCCHK(run_deep(c, m->d_ffn16, L.fc2.w, L.fc2.b, F, m->d_x32, &L.ln2, CLS_GEMM));
            else RCCHK(run_gemm_splitk_ln(c, m->d_ffn16, L.fc2.w, L.fc2.b, M, D, F, e.splits, m->d_x32, &L.ln2, m->d_x32, m->d_x16, CLS_GEMM, ps));
        }
    }
    return OPD_OK;
}

// memory keys / values of all decoder layers in one GEMM (per layer [k | v]: pos enters k only), unless the encoder's last launch wrote them
static int fwd_memory_kv(const Fwd& c, const TransformerPlan& tp) {
    if (!tp.kv_launch) return OPD_OK;
    return run_pos_proj(c, c.m->wkv_all, c.m->bkv_all, c.plan->rb_kv, c.kv_bias_ptrs, c.NKV, 2 * c.D, c.D, c.m->d_memkv16);
}

// The fused decoder (kernels_dec.hip): five launches per layer on split fp16 operands; layer 0 starts at its cross-attention (its
// self-attention block and its queries are constants of the weights).  *final_h: the state the heads read (before the last FFN, whose
// partial sums travel with it)
static int fwd_decoder_fused(const Fwd& c, const TransformerPlan& tp, const float** final_h) {
    opd_detr* m = c.m;
    const Arch& a = m->arch;
    const int B = c.B, D = c.D, F = c.F, Q = c.Q, Md = c.Md;
    const int S = tp.dec_splits, nchunk = F / OPD_DEC_FFN_CHUNK;
    float* hbuf[2] = {m->d_h32, m->d_yd32};
    int cur = 0;   // hbuf[cur] holds the layer's state from its self-attention block on
    for (int i = 0; i < a.dec_layers && i < m->sw.dbg_dec_layers; ++i) {
        const DecLayer& L = m->dec[i];
        f16_t* qd = m->d_qd16 + (size_t)i * m->cfg.max_batch * Q * D;   // (per-layer regions of max_batch frames: layer 0's constants stay put)
        if (i > 0) {
            const DecLayer& P = m->dec[i - 1];
            DecQkvParams qp{};
            qp.h_in = hbuf[cur]; qp.partials = m->d_ffn_part; qp.nsplit = nchunk; qp.b2 = P.fc2.b; qp.ln_g = P.ln3.g; qp.ln_b = P.ln3.b;
            qp.h_out = hbuf[cur ^ 1]; qp.w = L.wqkv_f; qp.bias = L.rb_self;
            qp.q16 = m->d_dq16; qp.k16 = m->d_dk16; qp.vT = m->d_dvT; qp.M = Md; qp.Q = Q;
            cur ^= 1;
            RCCHK(c.launch(CLS_GEMM, 2.0 * Md * 768.0 * D, [&] { return opd_launch_dec_qkv(qp, c.stream); }, {{"dec_qkv_h", hbuf[cur], (size_t)Md * D * 4}}));
            DecSelfParams sp{};
            sp.q16 = m->d_dq16; sp.k16 = m->d_dk16; sp.vT = m->d_dvT; sp.h = hbuf[cur]; sp.wo = L.so_f; sp.bo = L.so.b;
            sp.ln_g = L.ln1.g; sp.ln_b = L.ln1.b; sp.wq = L.wqc_f; sp.rbq = L.rb_q; sp.qc16 = qd; sp.qc_bf16 = m->dtype == OPD_DT_BF16; sp.B = B; sp.Q = Q;
            sp.scale = 1.0f / sqrtf((float)(D / a.heads));
            RCCHK(c.launch(CLS_GEMM, 4.0 * Md * (double)D * D + 4.0 * B * (double)a.heads * Q * Q * 32, [&] { return opd_launch_dec_self(sp, c.stream); },
                           {{"dec_self_h", hbuf[cur], (size_t)Md * D * 4}}));
        }
        // cross-attention over S key ranges: unnormalised partials
        AttnParams ap = attn_params(c, qd, D, m->d_memkv16 + (size_t)i * 2 * D, c.NKV, m->d_memkv16 + (size_t)i * 2 * D + D, c.NKV, nullptr, D, Q, c.hw, c.d_keyv, c.fw);
        ap.splits = S; ap.part_o = m->d_part_o; ap.part_ml = m->d_part_ml;
        RCCHK(c.launch(CLS_ATTN, attn_flops(ap), [&] { return opd_launch_attention(ap, c.stream); }, {{"dec_cross_part", m->d_part_o, (size_t)S * Md * D * 4}}));
        DecCrossOutParams cp{};
        cp.part_o = m->d_part_o; cp.part_ml = m->d_part_ml; cp.splits = S;
        cp.res = i == 0 ? m->dec0_h : hbuf[cur]; cp.res_period = i == 0 ? 1 : 0; cp.h = hbuf[cur];
        cp.wo = L.co_f; cp.bo = L.co.b; cp.ln_g = L.ln2.g; cp.ln_b = L.ln2.b; cp.M = Md;
        RCCHK(c.launch(CLS_GEMM, 2.0 * Md * (double)D * D, [&] { return opd_launch_dec_cross_out(cp, c.stream); }, {{"dec_cross_h", hbuf[cur], (size_t)Md * D * 4}}));
        DecFfnParams fp{};
        fp.h = hbuf[cur]; fp.w1 = L.fc1_f; fp.b1 = L.fc1.b; fp.w2 = L.fc2_f;
        fp.partials = m->d_ffn_part; fp.M = Md; fp.F = F;
        RCCHK(c.launch(CLS_GEMM, 4.0 * Md * (double)D * F, [&] { return opd_launch_dec_ffn(fp, c.stream); }, {{"dec_ffn_part", m->d_ffn_part, (size_t)nchunk * Md * D * 4}}));
    }
    *final_h = hbuf[cur];
    return OPD_OK;
}

// The unfused decoder: the round-3 chain of nine launches per layer on single fp16 operands (the cross-check of the fused one); state in d_h32 / d_h16
static int fwd_decoder_chain(const Fwd& c, const TransformerPlan& tp) {
    opd_detr* m = c.m;
    const Arch& a = m->arch;
    const int D = c.D, F = c.F, Q = c.Q, Md = c.Md;
    if (tp.dec0) {
        RCCHK(c.launch(CLS_OTHER, 0.0, [&] { return opd_launch_broadcast_rows(m->dec0_h, m->d_h32, m->d_h16, Md, c.stream, m->dtype); },
                       {{"dec0_broadcast", m->d_h32, (size_t)Md * D * 4}}));
    } else {
        HIPCHK(hipMemsetAsync(m->d_h32, 0, (size_t)Md * D * 4, c.stream));
        HIPCHK(hipMemsetAsync(m->d_h16, 0, (size_t)Md * D * 2, c.stream));
    }
    auto linear = [&](const f16_t* x, const f16_t* w, const float* bias, int bias_period, int N, int K, f16_t* out, bool relu) {
        return tp.dec_small_m ? run_small_gemm(c, x, w, bias, bias_period, Md, N, K, out, relu) : run_linear(c, x, w, bias, bias_period, Md, N, K, out, relu);
    };
    auto out_proj_ln = [&](const Lin& o, const LNp& ln) {   // attention output projection + residual + LayerNorm on the state
        return tp.dec_oproj == OPROJ_GEMM_LN ? run_gemm_ln(c, m->d_attnd16, o.w, o.b, Md, D, m->d_h32, ln, m->d_h32, m->d_h16)
                                              : run_gemm_splitk_ln(c, m->d_attnd16, o.w, o.b, Md, D, D, 4, m->d_h32, &ln, m->d_h32, m->d_h16, CLS_GEMM);
    };
    for (int i = 0; i < a.dec_layers && i < m->sw.dbg_dec_layers; ++i) {
        const DecLayer& L = m->dec[i];
        if (!(tp.dec0 && i == 0)) {   // (layer 0's self-attention block is the broadcast above)
            RCCHK(linear(m->d_h16, L.wqkv, L.rb_self, Q, 3 * D, D, m->d_qkvd16, false));
            RCCHK(run_attn(c, m->d_qkvd16, 3 * D, m->d_qkvd16 + D, 3 * D, m->d_qkvd16 + 2 * D, 3 * D, m->d_attnd16, Q, Q));
            RCCHK(out_proj_ln(L.so, L.ln1));
        }
        f16_t* qd = m->d_qd16 + (size_t)i * m->cfg.max_batch * Q * D;
        RCCHK(linear(m->d_h16, L.wq_c, L.rb_q, Q, D, D, qd, false));
        RCCHK(run_attn(c, qd, D, m->d_memkv16 + (size_t)i * 2 * D, c.NKV, m->d_memkv16 + (size_t)i * 2 * D + D, c.NKV, m->d_attnd16, Q, c.hw, c.d_keyv, c.fw));
        RCCHK(out_proj_ln(L.co, L.ln2));
        RCCHK(linear(m->d_h16, L.fc1.w, L.fc1.b, 0, F, D, m->d_ffnd16, true));
        if (tp.dec_small_m) RCCHK(run_small_gemm_ln(c, m->d_ffnd16, L.fc2.w, L.fc2.b, Md, F, m->d_h32, L.ln3, m->d_h32, m->d_h16));
        else RCCHK(run_gemm_splitk_ln(c, m->d_ffnd16, L.fc2.w, L.fc2.b, Md, D, F, 8, m->d_h32, &L.ln3, m->d_h32, m->d_h16, CLS_GEMM));
    }
    return OPD_OK;
}

// final LayerNorm + class / box heads on the decoder's state `h`
static int fwd_heads(const Fwd& c, const TransformerPlan& tp, const float* h) {
    opd_detr* m = c.m;
    const Arch& a = m->arch;
    HeadParams hp{};
    hp.hs = h;
    if (tp.heads_ln3) {   // the last layer's FFN sum + LN3 run inside the heads kernel
        const DecLayer& P = m->dec[a.dec_layers - 1];
        hp.partials = m->d_ffn_part; hp.nsplit = c.F / OPD_DEC_FFN_CHUNK; hp.ffn_b2 = P.fc2.b; hp.ln3_gamma = P.ln3.g; hp.ln3_beta = P.ln3.b;
    }
    if (tp.heads_ln) {   // the final LayerNorm runs inside the heads kernel
        hp.ln_gamma = m->dec_ln.g; hp.ln_beta = m->dec_ln.b;
    } else {
        RCCHK(c.launch(CLS_OTHER, 0.0, [&] { return opd_launch_layernorm(h, m->dec_ln.g, m->dec_ln.b, m->d_hs32, nullptr, c.Md, c.stream, m->dtype); }));
        hp.hs = m->d_hs32;
    }
    hp.wc = m->wc; hp.bc = m->bc; hp.w1 = m->w1; hp.b1 = m->b1; hp.w2 = m->w2; hp.b2 = m->b2;
    hp.w3 = m->w3; hp.b3 = m->b3; hp.logits = m->d_logits; hp.boxes = m->d_boxes; hp.rows = c.Md; hp.ncls = a.ncls;
    const bool split16 = tp.heads == HEADS_SPLIT16;
    if (split16) { hp.wc_f = m->wc_f; hp.w1_f = m->w1_f; hp.w2_f = m->w2_f; }
    return c.launch(CLS_OTHER, 2.0 * c.Md * 256.0 * (a.ncls + 256 + 256 + 4), [&] { return split16 ? opd_launch_heads2(hp, c.stream) : opd_launch_heads(hp, c.stream); },
                    {{"heads_logits", m->d_logits, (size_t)c.Md * a.ncls * 4}});
}

// Enqueues the whole forward on m->stream.  `d_pixels` must already be on the device.  `valid_hw` (host, nullable): [B][2] = (h, w) of each
// frame inside the H x W canvas.
static int enqueue_forward(opd_detr* m, const void* d_pixels, int pixel_format, int B, int H, int W, const int32_t* valid_hw = nullptr) {
    const Arch& a = m->arch;
    Fwd c{};
    c.m = m; c.stream = m->stream; c.B = B; c.H = H; c.W = W;
    compute_dims(B, H, W, &c.d);
    c.D = a.d_model; c.F = a.ffn; c.Q = a.queries; c.Md = B * c.Q; c.NKV = a.dec_layers * 2 * c.D;
    const bool ragged = is_ragged(valid_hw, B, H, W);
    if (ragged) RCCHK(fwd_prepare_ragged(c, valid_hw));
    else RCCHK(get_plan(m, c.d.stage_h[3], c.d.stage_w[3], c.d.stage_h[3], c.d.stage_w[3], &c.plan));
    m->tap_next = 0;   // the taps of the last forward (its event pairs: the pipeline call resets the launch timer in front of its source step, opd_api.cpp)
    if (pixel_format == OPD_PIXELS_U8_BGR_HWC) RCCHK(tap(m, c.stream, {"pixels_u8", d_pixels, (size_t)B * H * W * 3}));
    MARK(0);
    RCCHK(fwd_stem(c, d_pixels, pixel_format));
    MARK(1);
    RCCHK(fwd_trunk(c));   // (marks 2 .. 5: one behind each stage)
    const TransformerPlan tp = plan_transformer(a, m->cfg, m->sw, m->stage_px[3], B, c.fh, c.fw);
    RCCHK(fwd_encoder(c, tp));
    MARK(6);
    RCCHK(fwd_memory_kv(c, tp));
    const float* h = m->d_h32;   // the state the heads read: the chain's, or what the fused decoder hands back
    if (tp.dec_fused) RCCHK(fwd_decoder_fused(c, tp, &h));
    else RCCHK(fwd_decoder_chain(c, tp));
    RCCHK(fwd_heads(c, tp, h));
    MARK(7);
    m->last_B = B; m->last_H = H; m->last_W = W; m->last_fh = c.fh; m->last_fw = c.fw;
    m->last_ragged = ragged;
    return OPD_OK;
}

std::atomic<unsigned> g_handle_epoch{0};
std::atomic<int> g_graph_guard{1};   // opd_test_set_graph_guard(0): leave stale-epoch graphs alone (diagnosis only)

// Every captured graph of the handle holds the launch sequence of the switches, taps and profiling mode it was captured under
void drop_graphs(opd_detr* m) {
    for (auto& g : m->graphs) g.slot.drop();
    m->graphs.clear();
}

// Forward through the graph cache.  First call of a (shape, pixel pointer) key runs eagerly (one-time function-attribute
// setup and plan building are not capturable); the second call captures the stream into a hipGraph; later calls replay it.
int run_forward(opd_detr* m, const void* d_pixels, int pixel_format, int B, int H, int W, const int32_t* valid_hw) {
    m->graph_marks = false;
    // ragged batches run eagerly: their launch sequence depends on per-call host data (fold pointers, valid sizes)
    if (is_ragged(valid_hw, B, H, W)) return enqueue_forward(m, d_pixels, pixel_format, B, H, W, valid_hw);
    if (m->profiling == 1 || (m->cfg.flags & OPD_FLAG_NO_GRAPH)) return enqueue_forward(m, d_pixels, pixel_format, B, H, W);
    opd_detr::GraphEntry* e = nullptr;
    for (auto& g : m->graphs)
        if (g.B == B && g.H == H && g.W == W && g.fmt == pixel_format && g.pixels == d_pixels) e = &g;
    if (!e) {
        if (m->graphs.size() >= 8) {  // bounded cache: drop the oldest entry
            m->graphs.front().slot.drop();
            m->graphs.erase(m->graphs.begin());
        }
        m->graphs.push_back({B, H, W, pixel_format, 0, 0, d_pixels, 0, GraphSlot{}});
        e = &m->graphs.back();
    }
    if (!e->slot.ready() && e->uses++ == 0) return enqueue_forward(m, d_pixels, pixel_format, B, H, W);   // (a stale graph is captured again at once; a failed capture, by the next call)
    RCCHK(e->slot.run(m->stream, "the forward", [&]() -> int {
        RCCHK(enqueue_forward(m, d_pixels, pixel_format, B, H, W));
        e->fh = m->last_fh; e->fw = m->last_fw;
        return OPD_OK;
    }));
    if (m->profiling == 2) { HIPCHK(hipEventRecord(m->ev[9], m->stream)); m->graph_marks = true; }   // eager mark behind the graph: the post-process stage is timed between eager events
    m->last_B = B; m->last_H = H; m->last_W = W; m->last_fh = e->fh; m->last_fw = e->fw; m->last_ragged = false;   // (a replay ran no host code of the forward)
    return OPD_OK;
}

}  // namespace opd
