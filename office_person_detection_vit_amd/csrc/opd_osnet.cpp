// opd_osnet.cpp — the OSNet model behind an opd_reid handle created with OPD_REID_MODEL_OSNET: schema and widths of a torchreid state dict,
// BN folding in fp32, workspace layout and the forward's launch sequence (kernels_osnet.hip).  Staging, graphs and the API live in
// opd_reid.cpp and are shared with the CLIP model.
//
// Forward of nb crops, NHWC fp16:
//   osnet_preprocess -> stem (7x7 / 2, BN, ReLU) -> max-pool 3x3 / 2
//   per OSBlock: conv1 GEMM (BN, ReLU) -> level 1: one GEMM for the four streams' 1x1 (N = 4 mid) -> depthwise (BN, ReLU)
//                -> levels 2 .. 4: grouped GEMM over the 5 - t streams still running -> depthwise -> gate (pooled means, fc1, fc2, sigmoid)
//                -> x2 = sum of gated streams -> [conv3 | downsample] GEMM (BN folded, biases summed, ReLU) or conv3 + identity + ReLU
//   transitions: 1x1 GEMM (BN, ReLU) -> 2x2 average pool;  conv5 GEMM (BN, ReLU) -> head (global mean, fc + BN1d, ReLU, L2)
#include <math.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "opd_osnet.h"

namespace opd {

namespace {

struct OsnetArchC {
    int widths[4] = {0, 0, 0, 0};   // stem, conv2, conv3, conv4 stage widths
    int blocks[3] = {0, 0, 0};      // OSBlocks per stage
    int feat = 0;                   // fc width
};

const char* STREAM_NAMES = "abcd";

std::string stream_module(const std::string& blk, int s, int t) {   // LightConv of stream s (0 = a) at level t (1-based)
    if (s == 0) return blk + ".conv2a";
    return blk + ".conv2" + STREAM_NAMES[s] + "." + std::to_string(t - 1);
}

std::string block_prefix(int stage, int i) { return "conv" + std::to_string(stage + 2) + "." + std::to_string(i); }

struct Spec { std::string key; std::vector<int64_t> shape; };

void specs_bn(std::vector<Spec>* v, const std::string& p, int64_t c) {
    for (const char* n : {"weight", "bias", "running_mean", "running_var"}) v->push_back({p + "." + n, {c}});
}

void specs_conv_bn(std::vector<Spec>* v, const std::string& p, int64_t cout, int64_t cin, int64_t k) {
    v->push_back({p + ".conv.weight", {cout, cin, k, k}});
    specs_bn(v, p + ".bn", cout);
}

std::vector<Spec> all_specs(const OsnetArchC& a) {
    std::vector<Spec> v;
    specs_conv_bn(&v, "conv1", a.widths[0], 3, 7);
    int cin = a.widths[0];
    for (int s = 0; s < 3; ++s) {
        const int cout = a.widths[s + 1], mid = cout / 4, hid = mid / 16;
        for (int i = 0; i < a.blocks[s]; ++i) {
            const std::string p = block_prefix(s, i);
            specs_conv_bn(&v, p + ".conv1", mid, cin, 1);
            for (int st = 0; st < 4; ++st)
                for (int t = 1; t <= st + 1; ++t) {
                    const std::string m = stream_module(p, st, t);
                    v.push_back({m + ".conv1.weight", {mid, mid, 1, 1}});
                    v.push_back({m + ".conv2.weight", {mid, 1, 3, 3}});
                    specs_bn(&v, m + ".bn", mid);
                }
            v.push_back({p + ".gate.fc1.weight", {hid, mid, 1, 1}});
            v.push_back({p + ".gate.fc1.bias", {hid}});
            v.push_back({p + ".gate.fc2.weight", {mid, hid, 1, 1}});
            v.push_back({p + ".gate.fc2.bias", {mid}});
            specs_conv_bn(&v, p + ".conv3", cout, mid, 1);
            if (cin != cout) specs_conv_bn(&v, p + ".downsample", cout, cin, 1);
            cin = cout;
        }
        if (s < 2) specs_conv_bn(&v, block_prefix(s, a.blocks[s]) + ".0", cout, cout, 1);
    }
    specs_conv_bn(&v, "conv5", a.widths[3], a.widths[3], 1);
    v.push_back({"fc.0.weight", {a.feat, a.widths[3]}});
    v.push_back({"fc.0.bias", {a.feat}});
    specs_bn(&v, "fc.1", a.feat);
    return v;
}

std::string shape_str(const std::vector<int64_t>& s) {
    std::string r = "[";
    for (size_t i = 0; i < s.size(); ++i) r += (i ? ", " : "") + std::to_string(s[i]);
    return r + "]";
}

}  // namespace

// device pointers of one OSBlock (all weights BN-folded; 16-bit = fp16)
struct OsnetBlockW {
    int cin, cout, mid, hid;
    bool down;
    const f16_t* w1; const float* b1;       // conv1 [mid][cin]
    const f16_t* wl[4];                     // level t: [(5 - t) streams][mid][mid] (level 1: [4 mid][mid])
    const float* dw[4]; const float* dwb[4];   // level t: depthwise [9][4 mid], bias [4 mid] (streams < t - 1 unused)
    const float *g1w, *g1b, *g2w, *g2b;     // gate fc1 [hid][mid], fc2 [mid][hid]
    const f16_t* w3; const float* b3;       // [conv3 | downsample] [cout][mid (+ cin)], bias summed
};

struct OsnetModel final : ReidModel {
    OsnetArchC a;
    std::vector<size_t> o16, o32;           // pack(): where each tensor starts in h16 / h32, in the order bind() resolves them
    // weights
    const f16_t* lut = nullptr;             // [3][256] fp16 normalisation table
    const f16_t* wstem = nullptr; const float* bstem = nullptr;   // [147][64] fp16 (channels padded to 64), bias [64]
    std::vector<OsnetBlockW> blocks;        // in forward order
    const f16_t* wtr[2] = {nullptr, nullptr}; const float* btr[2] = {nullptr, nullptr};   // transitions conv2 / conv3
    const f16_t* w5 = nullptr; const float* b5 = nullptr;
    const float* wfc = nullptr; const float* bfc = nullptr;   // fc^T [C][512] with BN1d folded
    // workspace (max_crops)
    f16_t *img = nullptr, *stem = nullptr, *act[3] = {nullptr, nullptr, nullptr}, *x1 = nullptr, *u = nullptr, *t = nullptr, *x2 = nullptr;
    float *gates = nullptr, *feat = nullptr;

    const CropSpec& crop() const override { return CROP_OSNET; }
    int feature_dim() const override { return OSNET_FEAT; }
    const float* features() const override { return feat; }
    const void* image() const override { return img; }
    size_t image_bytes() const override { return (size_t)OSNET_H * OSNET_W * 4 * 2; }
    void fill_info(opd_reid_model_info* info) const override {   // tokens, layers, heads, mlp_dim and patch stay 0
        info->model = OPD_REID_MODEL_OSNET;
        info->feature_dim = OSNET_FEAT;
        info->hidden = a.widths[3];
    }
    void pack(const StateDict& sd, std::vector<uint16_t>* h16, std::vector<float>* h32) override;
    void bind(const f16_t* w16, const float* w32) override;
    size_t workspace(int max_crops, unsigned char* base) override;
    hipError_t preprocess(int nb, const ReidCrop* crops, const unsigned char* base, hipStream_t s) const override {
        return opd_launch_osnet_preprocess(crops, base, lut, img, nb, s);
    }
    int enqueue(int nb, const ReidCrop* crops, const unsigned char* base, ReidLauncher& Q) const override;
};

// Infer and check the architecture of a torchreid OSNet state dict (every tensor the forward reads, with its shape).  OPD_ESCHEMA names
// a missing tensor or the kernel limit a width breaks.
static int osnet_infer(const StateDict& sd, OsnetArchC* a) {
    auto get = [&](const std::string& k) -> const HostTensor* { auto it = sd.find(k); return it == sd.end() ? nullptr : &it->second; };
    for (const auto& kv : sd)
        if (kv.first.find(".IN.") != std::string::npos || kv.first.rfind("IN.", 0) == 0)
            return fail(OPD_ESCHEMA, "OSNet weight file holds instance-norm tensor '" + kv.first + "' (osnet_ain / osnet_ibn variants are not supported)");
    if (get("conv1.bn.weight") && !get("conv1.bn.running_mean"))
        return fail(OPD_ESCHEMA, "OSNet 'conv1.bn' has affine parameters but no running statistics: an instance-norm variant (osnet_ain / "
                                 "osnet_ibn), which is not supported");
    const HostTensor* c1 = get("conv1.conv.weight");
    if (!c1) return fail(OPD_ESCHEMA, "OSNet weight file lacks tensor 'conv1.conv.weight'");
    if (c1->shape.size() != 4 || c1->shape[1] != 3 || c1->shape[2] != 7 || c1->shape[3] != 7)
        return fail(OPD_ESCHEMA, "OSNet tensor 'conv1.conv.weight' is not [C][3][7][7]");
    a->widths[0] = (int)c1->shape[0];
    for (int s = 0; s < 3; ++s) {
        int n = 0;
        while (get(block_prefix(s, n) + ".conv1.conv.weight")) ++n;
        if (n == 0) return fail(OPD_ESCHEMA, "OSNet weight file lacks tensor '" + block_prefix(s, 0) + ".conv1.conv.weight'");
        a->blocks[s] = n;
        const HostTensor* c3 = get(block_prefix(s, 0) + ".conv3.conv.weight");
        if (!c3 || c3->shape.size() != 4) return fail(OPD_ESCHEMA, "OSNet weight file lacks tensor '" + block_prefix(s, 0) + ".conv3.conv.weight'");
        a->widths[s + 1] = (int)c3->shape[0];
    }
    const HostTensor* fc = get("fc.0.weight");
    if (!fc) return fail(OPD_ESCHEMA, "OSNet weight file lacks tensor 'fc.0.weight'");
    if (fc->shape.size() != 2) return fail(OPD_ESCHEMA, "OSNet tensor 'fc.0.weight' is not 2-D");
    a->feat = (int)fc->shape[0];
    // limits of the kernels (kernels_osnet.hip)
    if (a->feat != OSNET_FEAT) return fail(OPD_ESCHEMA, "OSNet fc width " + std::to_string(a->feat) + " is not 512");
    if (a->widths[0] % 16 || a->widths[0] > 64 || a->widths[0] < 16)
        return fail(OPD_ESCHEMA, "OSNet stem width " + std::to_string(a->widths[0]) + " is not a multiple of 16 from 16 to 64");
    for (int s = 1; s < 4; ++s) {
        const int w = a->widths[s];
        if (w % 64 || w > 1024)
            return fail(OPD_ESCHEMA, "OSNet stage width " + std::to_string(w) + " is not supported: the kernels need stage widths that are multiples "
                                     "of 64 (block width / 4 a multiple of 16) up to 1024");
    }
    if (a->widths[3] > 512) return fail(OPD_ESCHEMA, "OSNet last stage width " + std::to_string(a->widths[3]) + " is above the head kernel's 512");
    for (const Spec& sp : all_specs(*a)) {
        const HostTensor* t = get(sp.key);
        if (!t) return fail(OPD_ESCHEMA, "OSNet weight file lacks tensor '" + sp.key + "'");
        if (t->shape != sp.shape)
            return fail(OPD_ESCHEMA, "OSNet tensor '" + sp.key + "' has shape " + shape_str(t->shape) + ", expected " + shape_str(sp.shape));
    }
    return OPD_OK;
}

void OsnetModel::pack(const StateDict& sd, std::vector<uint16_t>* h16, std::vector<float>* h32) {
    auto T = [&](const std::string& k) -> const std::vector<float>& { return sd.at(k).data; };
    // every tensor starts 16-byte aligned (the kernels read weights and biases as 8 halves / 4 floats)
    auto mark16 = [&] { h16->resize((h16->size() + 7) / 8 * 8, 0); o16.push_back(h16->size()); };
    auto mark32 = [&] { h32->resize((h32->size() + 3) / 4 * 4, 0.f); o32.push_back(h32->size()); };
    // BN (eval) as scale / shift in fp32
    auto bn = [&](const std::string& p, std::vector<float>* sc, std::vector<float>* sh) {
        const std::vector<float>&g = T(p + ".weight"), &b = T(p + ".bias"), &m = T(p + ".running_mean"), &v = T(p + ".running_var");
        sc->resize(g.size());
        sh->resize(g.size());
        for (size_t c = 0; c < g.size(); ++c) {
            (*sc)[c] = g[c] / sqrtf(v[c] + 1e-5f);
            (*sh)[c] = b[c] - m[c] * (*sc)[c];
        }
    };
    std::vector<float> sc, sh;
    // normalisation table, stem
    mark16();
    h16->resize(h16->size() + 768);
    osnet_pixel_lut(h16->data() + o16.back());
    const int c0 = a.widths[0];
    bn("conv1.bn", &sc, &sh);
    mark16();
    {
        const std::vector<float>& w = T("conv1.conv.weight");
        for (int ky = 0; ky < 7; ++ky)
            for (int kx = 0; kx < 7; ++kx)
                for (int c = 0; c < 3; ++c)
                    for (int o = 0; o < 64; ++o)
                        h16->push_back(o < c0 ? f32_to_f16(w[(((size_t)o * 3 + c) * 7 + ky) * 7 + kx] * sc[o]) : 0);
    }
    mark32();
    for (int o = 0; o < 64; ++o) h32->push_back(o < c0 ? sh[o] : 0.f);
    // 1x1 conv + BN: fp16 rows scaled, fp32 bias
    auto conv1x1 = [&](const std::string& p, bool with_bias) {
        bn(p + ".bn", &sc, &sh);
        const std::vector<float>& w = T(p + ".conv.weight");
        const size_t cout = sc.size(), cin = w.size() / cout;
        mark16();
        for (size_t n = 0; n < cout; ++n)
            for (size_t k = 0; k < cin; ++k) h16->push_back(f32_to_f16(w[n * cin + k] * sc[n]));
        if (with_bias) { mark32(); h32->insert(h32->end(), sh.begin(), sh.end()); }
    };
    int cin = c0;
    for (int s = 0; s < 3; ++s) {
        const int cout = a.widths[s + 1], mid = cout / 4;
        for (int i = 0; i < a.blocks[s]; ++i) {
            const std::string p = block_prefix(s, i);
            conv1x1(p + ".conv1", true);
            for (int t = 1; t <= 4; ++t) {   // level t: the 1x1 weights of streams t - 1 .. 3, unscaled (their BN follows the depthwise)
                mark16();
                for (int st = t - 1; st < 4; ++st) {
                    const std::vector<float>& w = T(stream_module(p, st, t) + ".conv1.weight");
                    for (float v : w) h16->push_back(f32_to_f16(v));
                }
            }
            for (int t = 1; t <= 4; ++t) {   // depthwise [9][4 mid] with the LightConv's BN scale; bias [4 mid]
                std::vector<float> dw((size_t)9 * 4 * mid, 0.f), db((size_t)4 * mid, 0.f);
                for (int st = t - 1; st < 4; ++st) {
                    const std::string m = stream_module(p, st, t);
                    bn(m + ".bn", &sc, &sh);
                    const std::vector<float>& w = T(m + ".conv2.weight");
                    for (int c = 0; c < mid; ++c) {
                        for (int k = 0; k < 9; ++k) dw[(size_t)k * 4 * mid + st * mid + c] = w[(size_t)c * 9 + k] * sc[c];
                        db[st * mid + c] = sh[c];
                    }
                }
                mark32();
                h32->insert(h32->end(), dw.begin(), dw.end());
                mark32();
                h32->insert(h32->end(), db.begin(), db.end());
            }
            for (const char* n : {".gate.fc1.weight", ".gate.fc1.bias", ".gate.fc2.weight", ".gate.fc2.bias"}) {
                mark32();
                const std::vector<float>& v = T(p + n);
                h32->insert(h32->end(), v.begin(), v.end());
            }
            // [conv3 | downsample] rows, biases summed
            const bool down = cin != cout;
            std::vector<float> sc3, sh3, scd, shd;
            bn(p + ".conv3.bn", &sc3, &sh3);
            if (down) bn(p + ".downsample.bn", &scd, &shd);
            const std::vector<float>& w3 = T(p + ".conv3.conv.weight");
            mark16();
            for (int n = 0; n < cout; ++n) {
                for (int k = 0; k < mid; ++k) h16->push_back(f32_to_f16(w3[(size_t)n * mid + k] * sc3[n]));
                if (down) {
                    const std::vector<float>& wd = T(p + ".downsample.conv.weight");
                    for (int k = 0; k < cin; ++k) h16->push_back(f32_to_f16(wd[(size_t)n * cin + k] * scd[n]));
                }
            }
            mark32();
            for (int n = 0; n < cout; ++n) h32->push_back(down ? sh3[n] + shd[n] : sh3[n]);
            cin = cout;
        }
        if (s < 2) conv1x1(block_prefix(s, a.blocks[s]) + ".0", true);
    }
    conv1x1("conv5", true);
    // fc + BN1d: wt[k][e] = W[e][k] scale[e]; b = (b - mean) scale + beta
    bn("fc.1", &sc, &sh);
    const std::vector<float>&wf = T("fc.0.weight"), &bf = T("fc.0.bias"), &mf = T("fc.1.running_mean");
    const int C = a.widths[3];
    mark32();
    for (int k = 0; k < C; ++k)
        for (int e = 0; e < OSNET_FEAT; ++e) h32->push_back(wf[(size_t)e * C + k] * sc[e]);
    mark32();
    for (int e = 0; e < OSNET_FEAT; ++e) h32->push_back((bf[e] - mf[e]) * sc[e] + T("fc.1.bias")[e]);
}

void OsnetModel::bind(const f16_t* w16, const float* w32) {
    size_t i16 = 0, i32 = 0;
    auto n16 = [&] { return w16 + o16[i16++]; };
    auto n32 = [&] { return w32 + o32[i32++]; };
    lut = n16();
    wstem = n16();
    bstem = n32();
    blocks.clear();
    int cin = a.widths[0];
    for (int s = 0; s < 3; ++s) {
        const int cout = a.widths[s + 1], mid = cout / 4;
        for (int i = 0; i < a.blocks[s]; ++i) {
            OsnetBlockW b{};
            b.cin = cin; b.cout = cout; b.mid = mid; b.hid = mid / 16; b.down = cin != cout;
            b.w1 = n16(); b.b1 = n32();
            for (int lv = 0; lv < 4; ++lv) b.wl[lv] = n16();
            for (int lv = 0; lv < 4; ++lv) { b.dw[lv] = n32(); b.dwb[lv] = n32(); }
            b.g1w = n32(); b.g1b = n32(); b.g2w = n32(); b.g2b = n32();
            b.w3 = n16(); b.b3 = n32();
            blocks.push_back(b);
            cin = cout;
        }
        if (s < 2) { wtr[s] = n16(); btr[s] = n32(); }
    }
    w5 = n16(); b5 = n32();
    wfc = n32(); bfc = n32();
}

size_t OsnetModel::workspace(int max_crops, unsigned char* base) {
    const size_t C = (size_t)max_crops;
    const int hw[3] = {64 * 32, 32 * 16, 16 * 8};
    size_t actsz = (size_t)hw[0] * a.widths[0], mid = 0;
    for (int s = 0; s < 3; ++s) {
        actsz = std::max(actsz, (size_t)hw[s] * a.widths[s + 1]);
        mid = std::max(mid, (size_t)hw[s] * (a.widths[s + 1] / 4));
    }
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off = (off + bytes + 255) / 256 * 256; return base ? base + o : nullptr; };
    img = reinterpret_cast<f16_t*>(take(C * OSNET_H * OSNET_W * 4 * 2));
    stem = reinterpret_cast<f16_t*>(take(C * (OSNET_H / 2) * (OSNET_W / 2) * a.widths[0] * 2));
    for (int i = 0; i < 3; ++i) act[i] = reinterpret_cast<f16_t*>(take(C * actsz * 2));
    x1 = reinterpret_cast<f16_t*>(take(C * mid * 2));
    x2 = reinterpret_cast<f16_t*>(take(C * mid * 2));
    u = reinterpret_cast<f16_t*>(take(C * mid * 4 * 2));
    t = reinterpret_cast<f16_t*>(take(C * mid * 4 * 2));
    const size_t maxmid = (size_t)std::max(a.widths[1], std::max(a.widths[2], a.widths[3])) / 4;
    gates = reinterpret_cast<float*>(take(C * 4 * maxmid * 4));
    feat = reinterpret_cast<float*>(take(C * OSNET_FEAT * 4));
    return off;
}

int OsnetModel::enqueue(int nb, const ReidCrop* crops, const unsigned char* base, ReidLauncher& Q) const {
    hipStream_t s = Q.stream;
    LCHK(Q, preprocess(nb, crops, base, s), 0.0);
    LCHK(Q, opd_launch_osnet_stem(img, wstem, bstem, stem, nb, a.widths[0], s), 2.0 * nb * (OSNET_H / 2) * (OSNET_W / 2) * a.widths[0] * 147);
    LCHK(Q, opd_launch_osnet_maxpool(stem, act[0], nb, OSNET_H / 2, OSNET_W / 2, a.widths[0], s), 0.0);
    auto gemm = [&](int epi, const OsnetGemm& p, int groups) -> int {
        LCHK(Q, opd_launch_osnet_gemm(epi, p, groups, s), 2.0 * p.M * p.N * (p.k1 + p.k2) * groups);
        return OPD_OK;
    };
    int cur = 0, H = OSNET_H / 4, W = OSNET_W / 4;
    size_t bi = 0;
    for (int st = 0; st < 3; ++st) {
        const int HW = H * W, M = nb * HW;
        for (int i = 0; i < a.blocks[st]; ++i) {
            const OsnetBlockW& b = blocks[bi++];
            const int mid = b.mid, ld = 4 * mid;
            f16_t* x = act[cur];
            f16_t* y = act[(cur + 1) % 3];
            OsnetGemm p{};
            p.M = M;
            // conv1: x -> x1
            p.a1 = x; p.lda1 = b.cin; p.k1 = b.cin; p.w = b.w1; p.bias = b.b1; p.out = x1; p.ldo = mid; p.N = mid;
            RCCHK(gemm(OSNET_EPI_RELU, p, 1));
            // level 1: the four streams' 1x1 on x1 as one GEMM, then the depthwise over all 4 mid channels
            p = OsnetGemm{};
            p.M = M; p.a1 = x1; p.lda1 = mid; p.k1 = mid; p.w = b.wl[0]; p.out = u; p.ldo = ld; p.N = ld;
            RCCHK(gemm(OSNET_EPI_NONE, p, 1));
            LCHK(Q, opd_launch_osnet_dwconv(u, t, b.dw[0], b.dwb[0], nb, H, W, ld, 0, ld, ld, s), 2.0 * M * ld * 9);
            // levels 2 .. 4: streams lv - 1 .. 3, one mid x mid weight each
            for (int lv = 2; lv <= 4; ++lv) {
                const int c0 = (lv - 1) * mid, S = 5 - lv;
                p = OsnetGemm{};
                p.M = M; p.a1 = t + c0; p.lda1 = ld; p.k1 = mid; p.a_gcol = mid; p.w = b.wl[lv - 1]; p.out = u + c0; p.ldo = ld; p.o_gcol = mid;
                p.N = mid;
                RCCHK(gemm(OSNET_EPI_NONE, p, S));
                LCHK(Q, opd_launch_osnet_dwconv(u, t, b.dw[lv - 1], b.dwb[lv - 1], nb, H, W, ld, c0, S * mid, ld, s), 2.0 * M * S * mid * 9);
            }
            LCHK(Q, opd_launch_osnet_gate(t, b.g1w, b.g1b, b.g2w, b.g2b, gates, nb, HW, mid, b.hid, s), 0.0);
            LCHK(Q, opd_launch_osnet_combine(t, gates, x2, nb, HW, mid, s), 0.0);
            p = OsnetGemm{};
            p.M = M; p.a1 = x2; p.lda1 = mid; p.k1 = mid; p.w = b.w3; p.bias = b.b3; p.out = y; p.ldo = b.cout; p.N = b.cout;
            if (b.down) {
                p.a2 = x; p.lda2 = b.cin; p.k2 = b.cin;
                RCCHK(gemm(OSNET_EPI_RELU, p, 1));
            } else {
                p.res = x; p.ldr = b.cin;
                RCCHK(gemm(OSNET_EPI_RESID_RELU, p, 1));
            }
            cur = (cur + 1) % 3;
        }
        if (st < 2) {   // transition: Conv1x1 -> 2x2 average pool
            const int C = a.widths[st + 1];
            OsnetGemm p{};
            p.M = M; p.a1 = act[cur]; p.lda1 = C; p.k1 = C; p.w = wtr[st]; p.bias = btr[st]; p.out = act[(cur + 1) % 3]; p.ldo = C; p.N = C;
            RCCHK(gemm(OSNET_EPI_RELU, p, 1));
            LCHK(Q, opd_launch_osnet_avgpool2(act[(cur + 1) % 3], act[(cur + 2) % 3], nb, H, W, C, s), 0.0);
            cur = (cur + 2) % 3;
            H /= 2;
            W /= 2;
        }
    }
    const int C = a.widths[3], HW = H * W;
    OsnetGemm p{};
    p.M = nb * HW; p.a1 = act[cur]; p.lda1 = C; p.k1 = C; p.w = w5; p.bias = b5; p.out = act[(cur + 1) % 3]; p.ldo = C; p.N = C;
    RCCHK(gemm(OSNET_EPI_RELU, p, 1));
    LCHK(Q, opd_launch_osnet_head(act[(cur + 1) % 3], wfc, bfc, feat, nb, HW, C, s), 2.0 * nb * C * OSNET_FEAT);
    return OPD_OK;
}

int osnet_create(const StateDict& sd, std::unique_ptr<ReidModel>* out) {
    std::unique_ptr<OsnetModel> m(new OsnetModel);
    RCCHK(osnet_infer(sd, &m->a));
    *out = std::move(m);
    return OPD_OK;
}

// ---- normalisation and the host restatement of the pre-processing ----------------------------------------------------------------------
void osnet_pixel_lut(uint16_t* lut) {
    // torchvision ToTensor: u8.float().div(255); Normalize: sub_(float32 mean).div_(float32 std), each one fp32 rounding
    const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};
    for (int c = 0; c < 3; ++c)
        for (int v = 0; v < 256; ++v) {
            const volatile float x = (float)v / 255.0f;
            const volatile float d = x - mean[c];
            lut[c * 256 + v] = f32_to_f16(d / stdv[c]);
        }
}

void osnet_preprocess_host(const uint8_t* frame, int W, const ReidGeom& g, const uint16_t* lut, uint16_t* out) {
    std::vector<uint8_t> rgb((size_t)OSNET_H * OSNET_W * 3);
    crop_resample_host(CROP_OSNET, frame, W, g, rgb.data());
    for (size_t i = 0; i < (size_t)OSNET_H * OSNET_W; ++i) {
        for (int c = 0; c < 3; ++c) out[4 * i + c] = lut[c * 256 + rgb[3 * i + c]];
        out[4 * i + 3] = 0;
    }
}

}  // namespace opd
