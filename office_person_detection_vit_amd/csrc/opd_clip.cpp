// opd_clip.cpp — the CLIP ViT image tower behind an opd_reid handle created with OPD_REID_MODEL_CLIP: schema and sizes of a Hugging Face
// CLIP state dict, weight folding and packing, workspace layout and the forward's launch sequence (kernels_reid.hip).  Staging, graphs
// and the API live in opd_reid.cpp and are shared with the OSNet model.
//
// Forward of nb crops (nb = the bucket of the call, padded crops are zero images whose features are discarded):
//   reid_preprocess -> patch GEMM (+ class / position bias table) -> pre_layrnorm (fp32 stream rewritten)
//   per layer: LN1 -> QKV GEMM (q pre-scaled by 1/8) -> attention -> out-proj GEMM + residual -> LN2 -> fc1 GEMM + quick_gelu
//              -> fc2 GEMM + residual
//   post_layernorm of each class-token row -> projection GEMM -> L2 normalisation
#include <math.h>
#include <string.h>

#include <fstream>
#include <sstream>

#include "opd_clip.h"

namespace opd {

namespace {

struct ReidArch {
    int H = 0, L = 0, T = 0, P = 0, E = 0, F = 0, heads = 0, KP = 0;
};

struct ReidLayer {
    const f16_t *wqkv, *wo, *w1, *w2;
    const float *ln1g, *ln1b, *ln2g, *ln2b, *bqkv, *bo, *b1, *b2;
};

int heads_from_config(const std::string& weights_path, int* heads) {
    const size_t slash = weights_path.find_last_of('/');
    const std::string dir = slash == std::string::npos ? "." : weights_path.substr(0, slash);
    std::ifstream f(dir + "/config.json");
    if (!f) return 0;
    std::stringstream ss;
    ss << f.rdbuf();
    std::string s = ss.str();
    size_t lo = 0, hi = s.size();
    const size_t vc = s.find("\"vision_config\"");
    if (vc != std::string::npos) {   // CLIPModel: only the vision tower's object
        const size_t open = s.find('{', vc);
        if (open == std::string::npos) return 0;
        int depth = 0;
        size_t i = open;
        for (; i < s.size(); ++i) {
            if (s[i] == '{') ++depth;
            if (s[i] == '}' && --depth == 0) break;
        }
        lo = open;
        hi = i;
    }
    const size_t k = s.find("\"num_attention_heads\"", lo);
    if (k == std::string::npos || k >= hi) return 0;
    const size_t colon = s.find(':', k);
    if (colon == std::string::npos) return 0;
    *heads = atoi(s.c_str() + colon + 1);
    return 1;
}

int shape_is(const StateDict& sd, const std::string& k, std::initializer_list<int64_t> shape) {
    auto it = sd.find(k);
    if (it == sd.end()) return fail(OPD_ESCHEMA, "CLIP weight file lacks tensor '" + k + "'");
    if (it->second.shape != std::vector<int64_t>(shape)) return fail(OPD_ESCHEMA, "CLIP tensor '" + k + "' has an unexpected shape");
    return OPD_OK;
}

int infer_reid_arch(const StateDict& sd, const std::string& path, ReidArch* a) {
    const std::string vm = "vision_model.";
    auto get = [&](const std::string& k) -> const HostTensor* { auto it = sd.find(k); return it == sd.end() ? nullptr : &it->second; };
    const HostTensor* pe = get(vm + "embeddings.patch_embedding.weight");
    const HostTensor* pos = get(vm + "embeddings.position_embedding.weight");
    const HostTensor* proj = get("visual_projection.weight");
    if (!pe || pe->shape.size() != 4 || pe->shape[1] != 3 || pe->shape[2] != pe->shape[3])
        return fail(OPD_ESCHEMA, "CLIP weight file lacks a [hidden][3][P][P] 'vision_model.embeddings.patch_embedding.weight'");
    if (!pos || pos->shape.size() != 2) return fail(OPD_ESCHEMA, "CLIP weight file lacks 'vision_model.embeddings.position_embedding.weight'");
    if (!proj || proj->shape.size() != 2) return fail(OPD_ESCHEMA, "CLIP weight file lacks 'visual_projection.weight'");
    a->H = (int)pe->shape[0];
    a->P = (int)pe->shape[2];
    a->T = (int)pos->shape[0];
    a->E = (int)proj->shape[0];
    a->KP = 3 * a->P * a->P;
    while (get(vm + "encoder.layers." + std::to_string(a->L) + ".self_attn.q_proj.weight")) ++a->L;
    if (a->L == 0) return fail(OPD_ESCHEMA, "CLIP weight file has no encoder layer");
    const HostTensor* fc1 = get(vm + "encoder.layers.0.mlp.fc1.weight");
    if (!fc1 || fc1->shape.size() != 2) return fail(OPD_ESCHEMA, "CLIP weight file lacks 'vision_model.encoder.layers.0.mlp.fc1.weight'");
    a->F = (int)fc1->shape[0];
    a->heads = a->H / 64;
    int h = 0;
    if (heads_from_config(path, &h)) a->heads = h;
    // limits of the kernels (kernels_reid.hip)
    if (a->heads <= 0 || a->H % a->heads || a->H / a->heads != 64)
        return fail(OPD_ESCHEMA, "CLIP head_dim " + std::to_string(a->heads > 0 ? a->H / a->heads : 0) + " is not supported (the attention kernel needs head_dim 64)");
    if (a->T > 64) return fail(OPD_ESCHEMA, "CLIP token count " + std::to_string(a->T) + " is above the attention kernel's limit of 64 tokens");
    if (a->H % 128 || a->H > 1024) return fail(OPD_ESCHEMA, "CLIP hidden size " + std::to_string(a->H) + " is not a multiple of 128 up to 1024");
    const int gw = (int)lround(sqrt((double)(a->T - 1)));
    if (a->T < 2 || gw * gw != a->T - 1 || gw * a->P != REID_IMG)
        return fail(OPD_ESCHEMA, "CLIP image size " + std::to_string(gw * a->P) + " (patch " + std::to_string(a->P) + ", " + std::to_string(a->T) +
                                     " tokens) is not the processor's 224");
    if (a->KP % 64 || a->F % 64 || a->E % 64)
        return fail(OPD_ESCHEMA, "CLIP patch row (" + std::to_string(a->KP) + "), MLP width (" + std::to_string(a->F) + ") and projection width (" +
                                     std::to_string(a->E) + ") must be multiples of 64");
    // every shape of the forward
    const int64_t H = a->H, F = a->F;
    RCCHK(shape_is(sd, vm + "embeddings.class_embedding", {H}));
    RCCHK(shape_is(sd, vm + "embeddings.position_embedding.weight", {a->T, H}));
    RCCHK(shape_is(sd, vm + "pre_layrnorm.weight", {H}));
    RCCHK(shape_is(sd, vm + "pre_layrnorm.bias", {H}));
    RCCHK(shape_is(sd, vm + "post_layernorm.weight", {H}));
    RCCHK(shape_is(sd, vm + "post_layernorm.bias", {H}));
    RCCHK(shape_is(sd, "visual_projection.weight", {a->E, H}));
    for (int l = 0; l < a->L; ++l) {
        const std::string p = vm + "encoder.layers." + std::to_string(l) + ".";
        for (const char* n : {"q_proj", "k_proj", "v_proj", "out_proj"}) {
            RCCHK(shape_is(sd, p + "self_attn." + n + ".weight", {H, H}));
            RCCHK(shape_is(sd, p + "self_attn." + n + ".bias", {H}));
        }
        for (const char* n : {"layer_norm1", "layer_norm2"}) {
            RCCHK(shape_is(sd, p + n + ".weight", {H}));
            RCCHK(shape_is(sd, p + n + ".bias", {H}));
        }
        RCCHK(shape_is(sd, p + "mlp.fc1.weight", {F, H}));
        RCCHK(shape_is(sd, p + "mlp.fc1.bias", {F}));
        RCCHK(shape_is(sd, p + "mlp.fc2.weight", {H, F}));
        RCCHK(shape_is(sd, p + "mlp.fc2.bias", {H}));
    }
    return OPD_OK;
}

struct ClipModel final : ReidModel {
    ReidArch a;
    std::vector<size_t> o16, o32;   // pack(): where each tensor starts in h16 / h32, in the order bind() resolves them
    const f16_t *lut = nullptr, *wpatch = nullptr, *wproj = nullptr;
    const float *pbias = nullptr, *preg = nullptr, *preb = nullptr, *postg = nullptr, *postb = nullptr;
    std::vector<ReidLayer> layers;
    // workspace (max_crops)
    f16_t *patches = nullptr, *xn = nullptr, *qkv = nullptr, *attn = nullptr, *mlp = nullptr, *cls = nullptr;
    float *x = nullptr, *feat = nullptr;

    const CropSpec& crop() const override { return CROP_CLIP; }
    int feature_dim() const override { return a.E; }
    const float* features() const override { return feat; }
    const void* image() const override { return patches; }
    size_t image_bytes() const override { return (size_t)a.T * a.KP * 2; }

    void fill_info(opd_reid_model_info* info) const override {
        info->model = OPD_REID_MODEL_CLIP;
        info->feature_dim = a.E; info->tokens = a.T; info->hidden = a.H; info->layers = a.L;
        info->heads = a.heads; info->mlp_dim = a.F; info->patch = a.P;
    }

    void pack(const StateDict& sd, std::vector<uint16_t>* h16, std::vector<float>* h32) override {
        const int H = a.H, F = a.F, P = a.P, KP = a.KP, E = a.E;
        const std::string vm = "vision_model.";
        auto T_ = [&](const std::string& k) -> const std::vector<float>& { return sd.at(k).data; };
        auto put16 = [&](const float* v, size_t n, float scale = 1.0f) { o16.push_back(h16->size()); for (size_t i = 0; i < n; ++i) h16->push_back(f32_to_f16(v[i] * scale)); };
        auto put32 = [&](const float* v, size_t n, float scale = 1.0f) { o32.push_back(h32->size()); for (size_t i = 0; i < n; ++i) h32->push_back(v[i] * scale); };
        o16.push_back(h16->size());
        h16->resize(h16->size() + 3 * 256);
        reid_pixel_lut(h16->data() + o16.back());
        // patch weight [H][3][P][P] -> [H][kh][kw][c]: one patch is one contiguous row of the pre-processed image
        std::vector<float> pw((size_t)H * KP);
        {
            const std::vector<float>& src = T_(vm + "embeddings.patch_embedding.weight");
            for (int n = 0; n < H; ++n)
                for (int c = 0; c < 3; ++c)
                    for (int kh = 0; kh < P; ++kh)
                        for (int kw = 0; kw < P; ++kw) pw[(size_t)n * KP + (kh * P + kw) * 3 + c] = src[(((size_t)n * 3 + c) * P + kh) * P + kw];
        }
        put16(pw.data(), pw.size());
        // row 0 = class_embedding + pos[0]; rows 1.. = pos[1..] (the patch convolution has no bias)
        std::vector<float> pb(T_(vm + "embeddings.position_embedding.weight"));
        for (int n = 0; n < H; ++n) pb[n] += T_(vm + "embeddings.class_embedding")[n];
        put32(pb.data(), pb.size());
        for (const char* n : {"pre_layrnorm.weight", "pre_layrnorm.bias", "post_layernorm.weight", "post_layernorm.bias"}) put32(T_(vm + n).data(), H);
        put16(T_("visual_projection.weight").data(), (size_t)E * H);
        const float qs = 0.125f;   // 1 / sqrt(head_dim 64), a power of two: folded into q exactly
        for (int l = 0; l < a.L; ++l) {
            const std::string p = vm + "encoder.layers." + std::to_string(l) + ".";
            put16(T_(p + "self_attn.q_proj.weight").data(), (size_t)H * H, qs);   // q | k | v: one [3H][H] weight, one [3H] bias
            put16(T_(p + "self_attn.k_proj.weight").data(), (size_t)H * H);
            put16(T_(p + "self_attn.v_proj.weight").data(), (size_t)H * H);
            put32(T_(p + "self_attn.q_proj.bias").data(), H, qs);
            put32(T_(p + "self_attn.k_proj.bias").data(), H);
            put32(T_(p + "self_attn.v_proj.bias").data(), H);
            put16(T_(p + "self_attn.out_proj.weight").data(), (size_t)H * H);
            put32(T_(p + "self_attn.out_proj.bias").data(), H);
            put16(T_(p + "mlp.fc1.weight").data(), (size_t)F * H);
            put32(T_(p + "mlp.fc1.bias").data(), F);
            put16(T_(p + "mlp.fc2.weight").data(), (size_t)H * F);
            put32(T_(p + "mlp.fc2.bias").data(), H);
            for (const char* n : {"layer_norm1.weight", "layer_norm1.bias", "layer_norm2.weight", "layer_norm2.bias"}) put32(T_(p + n).data(), H);
        }
    }

    void bind(const f16_t* w16, const float* w32) override {
        size_t i16 = 0, i32 = 0;
        auto n16 = [&] { return w16 + o16[i16++]; };
        auto n32 = [&] { return w32 + o32[i32++]; };
        lut = n16(); wpatch = n16(); pbias = n32();
        preg = n32(); preb = n32(); postg = n32(); postb = n32();
        wproj = n16();
        layers.assign(a.L, ReidLayer{});
        for (ReidLayer& L : layers) {
            L.wqkv = n16(); n16(); n16();   // (k and v follow q)
            L.bqkv = n32(); n32(); n32();
            L.wo = n16(); L.bo = n32(); L.w1 = n16(); L.b1 = n32(); L.w2 = n16(); L.b2 = n32();
            L.ln1g = n32(); L.ln1b = n32(); L.ln2g = n32(); L.ln2b = n32();
        }
    }

    size_t workspace(int max_crops, unsigned char* base) override {
        const size_t C = (size_t)max_crops, M = C * a.T, H = a.H;
        size_t ws = 0;
        auto take = [&](size_t bytes) { const size_t o = ws; ws = (ws + bytes + 255) / 256 * 256; return base ? base + o : nullptr; };
        patches = reinterpret_cast<f16_t*>(take(M * a.KP * 2));
        x = reinterpret_cast<float*>(take(M * H * 4));
        xn = reinterpret_cast<f16_t*>(take(M * H * 2));
        qkv = reinterpret_cast<f16_t*>(take(M * 3 * H * 2));
        attn = reinterpret_cast<f16_t*>(take(M * H * 2));
        mlp = reinterpret_cast<f16_t*>(take(M * a.F * 2));
        cls = reinterpret_cast<f16_t*>(take(C * H * 2));
        feat = reinterpret_cast<float*>(take(C * a.E * 4));
        return ws;
    }

    hipError_t preprocess(int nb, const ReidCrop* crops, const unsigned char* base, hipStream_t s) const override {
        return opd_launch_reid_preprocess(crops, base, lut, patches, nb, a.P, a.T, s);
    }

    int enqueue(int nb, const ReidCrop* crops, const unsigned char* base, ReidLauncher& Q) const override {
        const int M = nb * a.T;
        hipStream_t s = Q.stream;
        const double g2 = 2.0 * M;   // 2 M N K per GEMM
        LCHK(Q, preprocess(nb, crops, base, s), 0.0);
        LCHK(Q, opd_launch_reid_gemm(REID_EPI_F32_PBIAS, patches, wpatch, pbias, a.T, x, M, a.H, a.KP, s), g2 * a.H * a.KP);
        LCHK(Q, opd_launch_reid_layernorm(x, 1, preg, preb, x, xn, M, a.H, s), 0.0);
        for (const ReidLayer& L : layers) {
            LCHK(Q, opd_launch_reid_layernorm(x, 1, L.ln1g, L.ln1b, nullptr, xn, M, a.H, s), 0.0);
            LCHK(Q, opd_launch_reid_gemm(REID_EPI_F16_BIAS, xn, L.wqkv, L.bqkv, 0, qkv, M, 3 * a.H, a.H, s), g2 * 3 * a.H * a.H);
            LCHK(Q, opd_launch_reid_attention(qkv, attn, nb, a.T, a.H, s), 4.0 * nb * a.T * a.T * a.H);
            LCHK(Q, opd_launch_reid_gemm(REID_EPI_F32_RESID, attn, L.wo, L.bo, 0, x, M, a.H, a.H, s), g2 * a.H * a.H);
            LCHK(Q, opd_launch_reid_layernorm(x, 1, L.ln2g, L.ln2b, nullptr, xn, M, a.H, s), 0.0);
            LCHK(Q, opd_launch_reid_gemm(REID_EPI_F16_QGELU, xn, L.w1, L.b1, 0, mlp, M, a.F, a.H, s), g2 * a.F * a.H);
            LCHK(Q, opd_launch_reid_gemm(REID_EPI_F32_RESID, mlp, L.w2, L.b2, 0, x, M, a.H, a.F, s), g2 * a.H * a.F);
        }
        LCHK(Q, opd_launch_reid_layernorm(x, a.T, postg, postb, nullptr, cls, nb, a.H, s), 0.0);
        LCHK(Q, opd_launch_reid_gemm(REID_EPI_F32_PBIAS, cls, wproj, nullptr, 0, feat, nb, a.E, a.H, s), 2.0 * nb * a.E * a.H);
        LCHK(Q, opd_launch_reid_l2norm(feat, nb, a.E, s), 0.0);
        return OPD_OK;
    }
};

}  // namespace

int clip_create(const StateDict& sd, const std::string& weights_path, std::unique_ptr<ReidModel>* out) {
    std::unique_ptr<ClipModel> m(new ClipModel);
    RCCHK(infer_reid_arch(sd, weights_path, &m->a));
    *out = std::move(m);
    return OPD_OK;
}

void reid_pixel_lut(uint16_t* lut) {
    // HF: rescale = float32(float64(u8) * (1/255)); normalize = (x - float32(mean)) / float32(std) in float32 (OPENAI_CLIP_MEAN / STD)
    const double mean[3] = {0.48145466, 0.4578275, 0.40821073}, stdv[3] = {0.26862954, 0.26130258, 0.27577711};
    for (int c = 0; c < 3; ++c)
        for (int v = 0; v < 256; ++v) {
            const float x = (float)((double)v * (1.0 / 255.0));
            const volatile float d = x - (float)mean[c];   // (two roundings, as numpy's two array operations)
            lut[c * 256 + v] = f32_to_f16(d / (float)stdv[c]);
        }
}

void reid_preprocess_host(const uint8_t* frame, int W, const ReidGeom& g, int P, const uint16_t* lut, uint16_t* out) {
    const int KP = 3 * P * P, gw = REID_IMG / P;
    std::vector<uint8_t> rgb((size_t)REID_IMG * REID_IMG * 3);
    crop_resample_host(CROP_CLIP, frame, W, g, rgb.data());
    memset(out, 0, (size_t)KP * 2);
    for (int yo = 0; yo < REID_IMG; ++yo)
        for (int xo = 0; xo < REID_IMG; ++xo) {
            const int p = (yo / P) * gw + xo / P;
            for (int c = 0; c < 3; ++c)
                out[(size_t)(1 + p) * KP + ((yo % P) * P + xo % P) * 3 + c] = lut[c * 256 + rgb[((size_t)yo * REID_IMG + xo) * 3 + c]];
        }
}

}  // namespace opd
