// opd_weights.cpp — build_weights: the checkpoint's tensors folded, rounded, packed and uploaded into the DetrWeights of a handle (opd_model.h).
// Runs once per opd_detr_create; everything it allocates belongs to the handle's WeightSet.  The forward that reads them: opd_model.cpp.
#include <algorithm>

#include "opd_model.h"

namespace opd {

template <typename E>
static int upload(opd_detr* m, E** dst, const std::vector<E>& v) {
    RCCHK(dalloc(m, dst, v.size(), true));
    HIPCHK(hipMemcpy(*dst, v.data(), v.size() * sizeof(E), hipMemcpyHostToDevice));
    return OPD_OK;
}
int upload_f32(opd_detr* m, float** dst, const std::vector<float>& v) { return upload(m, dst, v); }
int upload_fold(opd_detr* m, const float* d_x, const std::vector<float>& w, const std::vector<float>& b, int rows, int N, int K, float** out) {
    float *d_w = nullptr, *d_b = nullptr;
    RCCHK(upload_f32(m, &d_w, w));
    RCCHK(upload_f32(m, &d_b, b));
    RCCHK(dalloc(m, out, (size_t)rows * N, true));
    HIPCHK(opd_launch_gemm_f32(d_x, d_w, d_b, *out, rows, N, K, N, m->stream));
    return OPD_OK;
}
// the 16-bit operand type of this handle: fp16, or bf16 under OPD_FLAG_BF16
static std::vector<f16_t> to_h16(const opd_detr* m, const std::vector<float>& v) {
    std::vector<f16_t> h(v.size());
    if (m->dtype == OPD_DT_BF16) for (size_t i = 0; i < v.size(); ++i) h[i] = f32_to_bf16(v[i]);
    else for (size_t i = 0; i < v.size(); ++i) h[i] = f32_to_f16(v[i]);
    return h;
}
static int upload_f16(opd_detr* m, f16_t** dst, const std::vector<float>& v) { return upload(m, dst, to_h16(m, v)); }

// a linear layer's weights [N][K] as the fused decoder's split pair in MFMA-fragment order (opd_split_f16_frag)
static int upload_frag(opd_detr* m, f16_t** dst, const std::vector<float>& v, int N, int K) {
    if ((size_t)N * K != v.size() || N % 16 || K % 32) return fail(OPD_ESCHEMA, "decoder weight matrix does not tile into 16 x 32 fragments");
    std::vector<f16_t> f(v.size() * 2);
    opd_split_f16_frag(v.data(), N, K, f.data());
    return upload(m, dst, f);
}

static const HostTensor& T(const StateDict& sd, const std::string& k) { return sd.at(k); }

// the encoder FFN's weights (+ the rows of its tail projection, pass order) as enc_ffn_kernel's per-wave fragment streams, in the handle's 16-bit
// operand type
static int upload_encffn(opd_detr* m, unsigned char** dst, const std::vector<float>& w1, const std::vector<float>& b1, const std::vector<float>& w2, int F,
                         const std::vector<float>& wt, const std::vector<float>& bt, int tail, const std::vector<float>& wo) {
    const std::vector<f16_t> h1 = to_h16(m, w1), h2 = to_h16(m, w2), ht = to_h16(m, wt), ho = to_h16(m, wo);
    if (!ho.empty() && ho.size() != (size_t)256 * 256) return fail(OPD_ESCHEMA, "encoder front projection: unexpected weight shape");
    if (ht.size() != (size_t)tail * 256 * 256 || bt.size() != (size_t)tail * 256) return fail(OPD_ESCHEMA, "encoder tail projection: unexpected weight shape");
    std::vector<unsigned char> pk(opd_encffn_pack_bytes(F, tail, ho.empty() ? 0 : 1));
    opd_encffn_pack(h1.data(), b1.data(), h2.data(), F, ht.data(), bt.data(), tail, ho.empty() ? nullptr : ho.data(), pk.data());
    return upload(m, dst, pk);
}

// conv + FrozenBN -> folded fp16 [Cout][KH][KW][Cin] + fp32 bias (HF:models/detr/modeling_detr.py:207-215).  `host` (nullable) receives the
// two host images as they were uploaded (the 16-bit one after its one rounding): what Block::bias2sc / Block::w2sc are assembled from.
struct ConvHost { std::vector<f16_t> w16; std::vector<float> bias; };
static int make_conv(opd_detr* m, const StateDict& sd, const std::string& prefix, int stride, Conv* c, ConvHost* host = nullptr) {
    const HostTensor& w = T(sd, prefix + ".convolution.weight");
    const int Cout = (int)w.shape[0], Cin = (int)w.shape[1], KH = (int)w.shape[2], KW = (int)w.shape[3];
    const std::string n = prefix + ".normalization";
    const auto& g = T(sd, n + ".weight").data;
    const auto& bt = T(sd, n + ".bias").data;
    const auto& mu = T(sd, n + ".running_mean").data;
    const auto& var = T(sd, n + ".running_var").data;
    std::vector<float> scale(Cout), bias(Cout);
    for (int o = 0; o < Cout; ++o) {
        scale[o] = g[o] * (1.0f / sqrtf(var[o] + 1e-5f));
        bias[o] = bt[o] - mu[o] * scale[o];
    }
    c->Cin = Cin; c->Cout = Cout; c->KH = KH; c->KW = KW; c->stride = stride; c->pad = KH / 2;
    c->stem = Cin == 3;
    c->K = c->stem ? 256 : KH * KW * Cin;
    const size_t Kt = (size_t)KH * KW * Cin;
    std::vector<float> wt((size_t)Cout * Kt);   // folded, [o][kh][kw][ci] (the stem's without its padding): what gets rounded
    for (int o = 0; o < Cout; ++o)
        for (int ci = 0; ci < Cin; ++ci)
            for (int kh = 0; kh < KH; ++kh)
                for (int kw = 0; kw < KW; ++kw) wt[o * Kt + (size_t)(kh * KW + kw) * Cin + ci] = w.data[(((size_t)o * Cin + ci) * KH + kh) * KW + kw] * scale[o];
    // the fp16 image of the folded kernel: error diffusion along the reduction (opd_host.h) instead of round-to-nearest
    if (m->sw.wround) round_f16_diffused(wt.data(), (size_t)Cout, KH * KW, Cin, m->dtype == OPD_DT_BF16);
    if (c->stem) {  // stem: [64][8][8][4], zero padded (kh = 7, kw = 7, c = 3)
        std::vector<float> padded((size_t)Cout * 256, 0.f);
        for (int o = 0; o < Cout; ++o)
            for (int kh = 0; kh < 7; ++kh)
                for (int kw = 0; kw < 7; ++kw)
                    for (int ci = 0; ci < 3; ++ci) padded[(size_t)o * 256 + kh * 32 + kw * 4 + ci] = wt[(size_t)o * 147 + (kh * 7 + kw) * 3 + ci];
        wt.swap(padded);
    }
    std::vector<f16_t> w16 = to_h16(m, wt);
    RCCHK(upload(m, &c->w, w16));
    if (conv_has_kperm(*c)) {  // operands of kernels_btail.hip / kernels_btail3.hip (stages 1-3): the same image in opd_permute_k32's order
        std::vector<f16_t> wp(w16.size());
        opd_permute_k32(w16.data(), wp.data(), Cout, Cin);
        RCCHK(upload(m, &c->wp, wp));
    }
    RCCHK(upload_f32(m, &c->bias, bias));
    if (host) { host->w16 = std::move(w16); host->bias = std::move(bias); }
    return OPD_OK;
}

static int make_lin(opd_detr* m, const StateDict& sd, const std::string& prefix, Lin* l) {
    const HostTensor& w = T(sd, prefix + ".weight");
    l->N = (int)w.shape[0]; l->K = (int)w.shape[1];
    RCCHK(upload_f16(m, &l->w, w.data));
    RCCHK(upload_f32(m, &l->b, T(sd, prefix + ".bias").data));
    return OPD_OK;
}
static int make_ln(opd_detr* m, const StateDict& sd, const std::string& prefix, LNp* l) {
    RCCHK(upload_f32(m, &l->g, T(sd, prefix + ".weight").data));
    RCCHK(upload_f32(m, &l->b, T(sd, prefix + ".bias").data));
    return OPD_OK;
}
static void append(std::vector<float>& dst, const std::vector<float>& src) { dst.insert(dst.end(), src.begin(), src.end()); }

// w_full = [Wq;Wk;Wv] (GEMM weights), w_pos = [Wq;Wk;0] and b_cat = [bq;bk;bv] (row-bias fold) of the attention block `p`
static void cat3(const StateDict& sd, const std::string& p, int D, std::vector<float>* w_full, std::vector<float>* w_pos, std::vector<float>* b_cat) {
    w_full->clear(); w_pos->clear(); b_cat->clear();
    for (const char* pr : {".q_proj", ".k_proj", ".v_proj"}) { append(*w_full, T(sd, p + pr + ".weight").data); append(*b_cat, T(sd, p + pr + ".bias").data); }
    append(*w_pos, T(sd, p + ".q_proj.weight").data); append(*w_pos, T(sd, p + ".k_proj.weight").data);
    w_pos->resize(w_pos->size() + (size_t)D * D, 0.f);
}

// ResNet trunk (stem, bottleneck blocks with their packed forms) and the input projection
static int build_backbone(opd_detr* m, const StateDict& sd) {
    const std::string bb = "model.backbone.model.";
    RCCHK(make_conv(m, sd, bb + "embedder.embedder", 2, &m->stem));
    for (int s = 0; s < 4; ++s) {
        m->stage_first.push_back((int)m->blocks.size());
        for (int l = 0; l < m->arch.depths[s]; ++l) {
            const std::string p = bb + "encoder.stages." + std::to_string(s) + ".layers." + std::to_string(l);
            const int stride = (l == 0 && s > 0) ? 2 : 1;
            Block b;
            ConvHost h2, hs;   // the expand's and the shortcut's images, as uploaded
            b.has_sc = sd.count(p + ".shortcut.convolution.weight") > 0;
            if (b.has_sc) RCCHK(make_conv(m, sd, p + ".shortcut", stride, &b.sc, &hs));
            RCCHK(make_conv(m, sd, p + ".layer.0", 1, &b.c0));
            RCCHK(make_conv(m, sd, p + ".layer.1", stride, &b.c1));
            RCCHK(make_conv(m, sd, p + ".layer.2", 1, &b.c2, &h2));
            if (block_has_bias2sc(b)) {
                std::vector<float> b2 = h2.bias;
                for (size_t j = 0; j < b2.size(); ++j) b2[j] += hs.bias[j];
                RCCHK(upload_f32(m, &b.bias2sc, b2));
                if (block_has_w2sc(b)) {   // stages 2-4: [W2 | Wsc]
                    const size_t K1 = (size_t)b.c2.K, K2 = (size_t)b.sc.K, N = (size_t)b.c2.Cout;
                    std::vector<f16_t> cat(N * (K1 + K2));
                    for (size_t n = 0; n < N; ++n) {
                        memcpy(&cat[n * (K1 + K2)], &h2.w16[n * K1], K1 * 2);
                        memcpy(&cat[n * (K1 + K2) + K1], &hs.w16[n * K2], K2 * 2);
                    }
                    RCCHK(upload(m, &b.w2sc, cat));
                }
            }
            m->blocks.push_back(b);
        }
    }
    // input_projection: plain 1x1 conv with bias, no BN
    const HostTensor& w = T(sd, "model.input_projection.weight");
    m->proj.Cin = (int)w.shape[1]; m->proj.Cout = (int)w.shape[0]; m->proj.K = m->proj.Cin;
    RCCHK(upload_f16(m, &m->proj.w, w.data));
    RCCHK(upload_f32(m, &m->proj.bias, T(sd, "model.input_projection.bias").data));
    return OPD_OK;
}

static int build_encoder(opd_detr* m, const StateDict& sd) {
    const Arch& a = m->arch;
    m->enc.resize(a.enc_layers); m->h_enc_cat_w.resize(a.enc_layers); m->h_enc_cat_b.resize(a.enc_layers);
    for (int i = 0; i < a.enc_layers; ++i) {
        const std::string p = "model.encoder.layers." + std::to_string(i);
        EncLayer& L = m->enc[i];
        std::vector<float> wfull;
        cat3(sd, p + ".self_attn", a.d_model, &wfull, &m->h_enc_cat_w[i], &m->h_enc_cat_b[i]);
        RCCHK(upload_f16(m, &L.wqkv, wfull));
        RCCHK(upload_f32(m, &L.bqkv, m->h_enc_cat_b[i]));
        RCCHK(make_lin(m, sd, p + ".self_attn.o_proj", &L.o));
        RCCHK(make_ln(m, sd, p + ".self_attn_layer_norm", &L.ln1));
        RCCHK(make_lin(m, sd, p + ".mlp.fc1", &L.fc1));
        RCCHK(make_lin(m, sd, p + ".mlp.fc2", &L.fc2));
        RCCHK(make_ln(m, sd, p + ".final_layer_norm", &L.ln2));
    }
    return OPD_OK;
}

// The encoder FFN blocks as single launches, each with the projection that consumes its output.  `kv_full`: build_decoder's [k_l | v_l] rows.
static int build_encoder_ffn_packs(opd_detr* m, const StateDict& sd, const std::vector<float>& kv_full) {
    const Arch& a = m->arch;
    if (!enc_has_ffn_pack(a)) return OPD_OK;
    const int D = 256, L = a.dec_layers;
    for (int i = 0; i < a.enc_layers; ++i) {
        EncLayer& E = m->enc[i];
        const std::string p = "model.encoder.layers." + std::to_string(i);
        std::vector<float> wt, bt;
        const int tail = enc_pack_tail(a, i, &E.tail_pos);
        E.tail_ld = tail * D;
        if (i + 1 < a.enc_layers) {   // the next layer's q, k (on x + pos), v
            const std::string n = "model.encoder.layers." + std::to_string(i + 1) + ".self_attn.";
            for (const char* pr : {"q_proj", "k_proj", "v_proj"}) { append(wt, T(sd, n + pr + ".weight").data); append(bt, T(sd, n + pr + ".bias").data); }
            for (int t = 0; t < 3; ++t) E.tail_col[t] = t * D;
        } else if (tail) {
            // the decoder's memory projections, [k_l | v_l] per layer in wkv_all: passes k_0 .. k_{L-1} (on x + pos), then v_0 .. v_{L-1}
            for (int kv = 0; kv < 2; ++kv)
                for (int l = 0; l < L; ++l) {
                    wt.insert(wt.end(), kv_full.begin() + (size_t)(2 * l + kv) * D * D, kv_full.begin() + (size_t)(2 * l + kv + 1) * D * D);
                    bt.insert(bt.end(), m->h_kv_cat_b.begin() + (size_t)(2 * l + kv) * D, m->h_kv_cat_b.begin() + (size_t)(2 * l + kv + 1) * D);
                    E.tail_col[kv * L + l] = (2 * l + kv) * D;
                }
        }
        RCCHK(upload_encffn(m, &E.ffn_pack, T(sd, p + ".mlp.fc1.weight").data, T(sd, p + ".mlp.fc1.bias").data, T(sd, p + ".mlp.fc2.weight").data, a.ffn, wt, bt, tail,
                            T(sd, p + ".self_attn.o_proj.weight").data));
    }
    return OPD_OK;
}

// The decoder starts from h = 0 (HF:models/detr/modeling_detr.py:1243-1251), so in layer 0 the self-attention values are the
// same row for every query, v = 0 . Wv^T + bv, the softmax weights of a row sum to one, and the block's output
// LN(0 + Wo . bv + bo) is ONE vector, whatever the frame shows: computed here once in fp32, broadcast at run time instead of
// two memsets, the QKV projection, the attention and the output projection + LayerNorm of that layer.
static int build_decoder_layer0(opd_detr* m, const StateDict& sd) {
    const int D = m->arch.d_model, Q = m->arch.queries;
    const std::string p0 = "model.decoder.layers.0";
    const auto& bv = T(sd, p0 + ".self_attn.v_proj.bias").data;
    const auto& wo = T(sd, p0 + ".self_attn.o_proj.weight").data;
    const auto& bo = T(sd, p0 + ".self_attn.o_proj.bias").data;
    const auto& g = T(sd, p0 + ".self_attn_layer_norm.weight").data;
    const auto& be = T(sd, p0 + ".self_attn_layer_norm.bias").data;
    std::vector<float> x(D), c(D);
    for (int n = 0; n < D; ++n) {
        float acc = 0.f;
        for (int k = 0; k < D; ++k) acc += wo[(size_t)n * D + k] * bv[k];
        x[n] = acc + bo[n];
    }
    float mean = 0.f, var = 0.f;
    for (int n = 0; n < D; ++n) mean += x[n];
    mean /= (float)D;
    for (int n = 0; n < D; ++n) var += (x[n] - mean) * (x[n] - mean);
    var /= (float)D;
    const float rstd = 1.0f / sqrtf(var + 1e-5f);
    for (int n = 0; n < D; ++n) c[n] = (x[n] - mean) * rstd * g[n] + be[n];
    RCCHK(upload_f32(m, &m->dec0_h, c));
    // ... and so are layer 0's cross-attention queries, (h1 + qpos) . Wq_c^T + bq_c: one [Q][D] table (fp32 sums, stored as the fp16 operand
    // the attention kernel reads)
    const auto& qpos = T(sd, "model.query_position_embeddings.weight").data;
    const auto& wq = T(sd, p0 + ".encoder_attn.q_proj.weight").data;
    const auto& bq = T(sd, p0 + ".encoder_attn.q_proj.bias").data;
    std::vector<float> q0((size_t)Q * D);
    for (int q = 0; q < Q; ++q)
        for (int n = 0; n < D; ++n) {
            double acc = bq[n];
            for (int k = 0; k < D; ++k) acc += ((double)c[k] + qpos[(size_t)q * D + k]) * wq[(size_t)n * D + k];
            q0[(size_t)q * D + n] = (float)acc;
        }
    return upload_f16(m, &m->qc0, q0);
}

// Decoder layers and the memory K/V projection of all of them (`kv_full`: its fp32 rows, which the last encoder FFN pack needs too)
static int build_decoder(opd_detr* m, const StateDict& sd, std::vector<float>* kv_full) {
    const Arch& a = m->arch;
    const int D = a.d_model, Q = a.queries;
    const std::vector<float> zerosW((size_t)D * D, 0.f);
    // query-position folds are resolution independent -> build them now with the fp32 plan GEMM
    float* d_qpos = nullptr;
    RCCHK(upload_f32(m, &d_qpos, T(sd, "model.query_position_embeddings.weight").data));
    m->dec.resize(a.dec_layers);
    for (int i = 0; i < a.dec_layers; ++i) {
        const std::string p = "model.decoder.layers." + std::to_string(i);
        DecLayer& L = m->dec[i];
        std::vector<float> wfull, wpos, bcat;
        cat3(sd, p + ".self_attn", D, &wfull, &wpos, &bcat);
        RCCHK(upload_f16(m, &L.wqkv, wfull));
        RCCHK(upload_fold(m, d_qpos, wpos, bcat, Q, 768, D, &L.rb_self));
        RCCHK(make_lin(m, sd, p + ".self_attn.o_proj", &L.so));
        RCCHK(make_ln(m, sd, p + ".self_attn_layer_norm", &L.ln1));
        // cross attention: q from the decoder state, k/v from the encoder memory
        RCCHK(upload_f16(m, &L.wq_c, T(sd, p + ".encoder_attn.q_proj.weight").data));
        RCCHK(upload_fold(m, d_qpos, T(sd, p + ".encoder_attn.q_proj.weight").data, T(sd, p + ".encoder_attn.q_proj.bias").data, Q, D, D, &L.rb_q));
        append(*kv_full, T(sd, p + ".encoder_attn.k_proj.weight").data);
        append(*kv_full, T(sd, p + ".encoder_attn.v_proj.weight").data);
        append(m->h_kv_cat_w, T(sd, p + ".encoder_attn.k_proj.weight").data);
        append(m->h_kv_cat_w, zerosW);
        append(m->h_kv_cat_b, T(sd, p + ".encoder_attn.k_proj.bias").data);
        append(m->h_kv_cat_b, T(sd, p + ".encoder_attn.v_proj.bias").data);
        RCCHK(make_lin(m, sd, p + ".encoder_attn.o_proj", &L.co));
        RCCHK(make_ln(m, sd, p + ".encoder_attn_layer_norm", &L.ln2));
        RCCHK(make_lin(m, sd, p + ".mlp.fc1", &L.fc1));
        RCCHK(make_lin(m, sd, p + ".mlp.fc2", &L.fc2));
        RCCHK(make_ln(m, sd, p + ".final_layer_norm", &L.ln3));
        // split pairs for the fused decoder
        if (dec_has_frag_weights(a)) {
            RCCHK(upload_frag(m, &L.wqkv_f, wfull, 3 * D, D));
            RCCHK(upload_frag(m, &L.so_f, T(sd, p + ".self_attn.o_proj.weight").data, D, D));
            RCCHK(upload_frag(m, &L.wqc_f, T(sd, p + ".encoder_attn.q_proj.weight").data, D, D));
            RCCHK(upload_frag(m, &L.co_f, T(sd, p + ".encoder_attn.o_proj.weight").data, D, D));
            RCCHK(upload_frag(m, &L.fc1_f, T(sd, p + ".mlp.fc1.weight").data, a.ffn, D));
            RCCHK(upload_frag(m, &L.fc2_f, T(sd, p + ".mlp.fc2.weight").data, D, a.ffn));
        }
    }
    RCCHK(upload_f16(m, &m->wkv_all, *kv_full));
    return upload_f32(m, &m->bkv_all, m->h_kv_cat_b);
}

// the decoder's final LayerNorm, class and box heads
static int build_heads(opd_detr* m, const StateDict& sd) {
    const Arch& a = m->arch;
    auto transposed = [&](const std::string& key) {  // [out][in] -> [in][out] (coalesced reads in heads_kernel)
        const HostTensor& w = T(sd, key);
        const int O = (int)w.shape[0], I = (int)w.shape[1];
        std::vector<float> t((size_t)O * I);
        for (int o = 0; o < O; ++o)
            for (int i = 0; i < I; ++i) t[(size_t)i * O + o] = w.data[(size_t)o * I + i];
        return t;
    };
    RCCHK(make_ln(m, sd, "model.decoder.layernorm", &m->dec_ln));
    RCCHK(upload_f32(m, &m->wc, transposed("class_labels_classifier.weight")));
    RCCHK(upload_f32(m, &m->bc, T(sd, "class_labels_classifier.bias").data));
    if (heads_have_frag_weights(a)) {   // the heads on split fp16 operands (kernels_dec.hip::heads2_kernel): class matrix padded to 128 rows
        std::vector<float> wcp((size_t)128 * 256, 0.f);
        const auto& wcs = T(sd, "class_labels_classifier.weight").data;
        std::copy(wcs.begin(), wcs.end(), wcp.begin());
        RCCHK(upload_frag(m, &m->wc_f, wcp, 128, 256));
        RCCHK(upload_frag(m, &m->w1_f, T(sd, "bbox_predictor.layers.0.weight").data, 256, 256));
        RCCHK(upload_frag(m, &m->w2_f, T(sd, "bbox_predictor.layers.1.weight").data, 256, 256));
    }
    float** const box_w[3] = {&m->w1, &m->w2, &m->w3};
    float** const box_b[3] = {&m->b1, &m->b2, &m->b3};
    for (int l = 0; l < 3; ++l) {
        RCCHK(upload_f32(m, box_w[l], transposed("bbox_predictor.layers." + std::to_string(l) + ".weight")));
        RCCHK(upload_f32(m, box_b[l], T(sd, "bbox_predictor.layers." + std::to_string(l) + ".bias").data));
    }
    return upload_f32(m, &m->zero_bias, std::vector<float>(4096, 0.f));
}

int build_weights(opd_detr* m, const StateDict& sd) {
    std::vector<float> kv_full;
    RCCHK(build_backbone(m, sd));
    RCCHK(build_encoder(m, sd));
    RCCHK(build_decoder(m, sd, &kv_full));
    RCCHK(build_encoder_ffn_packs(m, sd, kv_full));
    RCCHK(build_decoder_layer0(m, sd));
    RCCHK(build_heads(m, sd));
    HIPCHK(hipStreamSynchronize(m->stream));
    return OPD_OK;
}

}  // namespace opd
