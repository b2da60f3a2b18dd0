// opd_reid.cpp — the Re-ID handle (include/opd_detr.h, opd_reid_*): CLIP ViT image tower weights, workspace sized once for max_crops,
// its own stream, one captured hipGraph per crop-count bucket, host staging of each crop's source window.  A handle created with
// OPD_REID_MODEL_OSNET holds an OsnetModel (opd_osnet.cpp) instead of the CLIP weights and shares everything else.
//
// CLIP forward of nb crops (nb = the bucket of the call, padded crops are zero images whose features are discarded):
//   reid_preprocess -> patch GEMM (+ class / position bias table) -> pre_layrnorm (fp32 stream rewritten)
//   per layer: LN1 -> QKV GEMM (q pre-scaled by 1/8) -> attention -> out-proj GEMM + residual -> LN2 -> fc1 GEMM + quick_gelu
//              -> fc2 GEMM + residual
//   post_layernorm of each class-token row -> projection GEMM -> L2 normalisation
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <fstream>
#include <map>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "opd_model.h"
#include "opd_osnet.h"
#include "opd_reid.h"

using namespace opd;

namespace {

struct ReidArch {
    int H = 0, L = 0, T = 0, P = 0, E = 0, F = 0, heads = 0, KP = 0;
};

struct ReidLayer {
    f16_t *wqkv, *wo, *w1, *w2;
    float *ln1g, *ln1b, *ln2g, *ln2b, *bqkv, *bo, *b1, *b2;
};

}  // namespace

struct opd_reid {
    int device = 0;
    opd_reid_config cfg{};
    ReidArch a;
    hipStream_t stream = nullptr;
    // weights
    void* wmem = nullptr;
    size_t wbytes = 0;
    f16_t *lut = nullptr, *wpatch = nullptr, *wproj = nullptr;
    float *pbias = nullptr, *preg = nullptr, *preb = nullptr, *postg = nullptr, *postb = nullptr;
    std::vector<ReidLayer> layers;
    std::unique_ptr<OsnetModel> os;   // OPD_REID_MODEL_OSNET: the OSNet weights and workspace (the CLIP pointers above stay null)
    // workspace (max_crops)
    void* ws = nullptr;
    size_t wsbytes = 0;
    f16_t *patches = nullptr, *xn = nullptr, *qkv = nullptr, *attn = nullptr, *mlp = nullptr, *cls = nullptr;
    float *x = nullptr, *feat = nullptr;
    // staging: [ReidCrop x max_crops][tables][windows], pinned host image + device copy, grown on demand
    unsigned char* h_up = nullptr;
    unsigned char* d_up = nullptr;
    size_t up_cap = 0;
    std::vector<int> buckets;
    struct Graph { hipGraphExec_t exec; unsigned epoch; };
    std::map<int, Graph> graphs;
    // per-launch timing of eager forwards (opd_test_reid_kernel_table): event pairs around every launch while `prof` is set
    bool prof = false;
    struct Mark { const char* name; double flops; hipEvent_t e0, e1; };
    std::vector<Mark> marks;
    std::vector<hipEvent_t> event_pool;
    size_t events_used = 0;
};

namespace {

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

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

#define SCHK(expr)                 \
    do {                           \
        const int rc_ = (expr);    \
        if (rc_) return rc_;       \
    } while (0)

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
    SCHK(shape_is(sd, vm + "embeddings.class_embedding", {H}));
    SCHK(shape_is(sd, vm + "embeddings.position_embedding.weight", {a->T, H}));
    SCHK(shape_is(sd, vm + "pre_layrnorm.weight", {H}));
    SCHK(shape_is(sd, vm + "pre_layrnorm.bias", {H}));
    SCHK(shape_is(sd, vm + "post_layernorm.weight", {H}));
    SCHK(shape_is(sd, vm + "post_layernorm.bias", {H}));
    SCHK(shape_is(sd, "visual_projection.weight", {a->E, H}));
    for (int l = 0; l < a->L; ++l) {
        const std::string p = vm + "encoder.layers." + std::to_string(l) + ".";
        for (const char* n : {"q_proj", "k_proj", "v_proj", "out_proj"}) {
            SCHK(shape_is(sd, p + "self_attn." + n + ".weight", {H, H}));
            SCHK(shape_is(sd, p + "self_attn." + n + ".bias", {H}));
        }
        for (const char* n : {"layer_norm1", "layer_norm2"}) {
            SCHK(shape_is(sd, p + n + ".weight", {H}));
            SCHK(shape_is(sd, p + n + ".bias", {H}));
        }
        SCHK(shape_is(sd, p + "mlp.fc1.weight", {F, H}));
        SCHK(shape_is(sd, p + "mlp.fc1.bias", {F}));
        SCHK(shape_is(sd, p + "mlp.fc2.weight", {H, F}));
        SCHK(shape_is(sd, p + "mlp.fc2.bias", {H}));
    }
    return OPD_OK;
}

void destroy_graphs(opd_reid* r) {
    for (auto& kv : r->graphs) (void)hipGraphExecDestroy(kv.second.exec);
    r->graphs.clear();
}

int ensure_upload(opd_reid* r, size_t bytes) {
    if (bytes <= r->up_cap) return OPD_OK;
    const size_t cap = std::max(bytes, r->up_cap * 2);
    destroy_graphs(r);   // the captured kernels hold the old base pointer
    if (r->h_up) (void)hipHostFree(r->h_up);
    if (r->d_up) (void)hipFree(r->d_up);
    r->h_up = r->d_up = nullptr;
    r->up_cap = 0;
    HIPCHK(hipHostMalloc((void**)&r->h_up, cap, hipHostMallocDefault));
    HIPCHK(hipMalloc((void**)&r->d_up, cap));
    r->up_cap = cap;
    return OPD_OK;
}

int bucket_of(const opd_reid* r, int n) {
    for (int b : r->buckets)
        if (b >= n) return b;
    return r->buckets.back();
}

int next_event(opd_reid* r, hipEvent_t* e) {
    if (r->events_used == r->event_pool.size()) {
        hipEvent_t ev;
        HIPCHK(hipEventCreate(&ev));
        r->event_pool.push_back(ev);
    }
    *e = r->event_pool[r->events_used++];
    return OPD_OK;
}

// one launch of the forward; with r->prof set it is bracketed by events and noted with its kernel name and algorithmic FLOPs
#define LCHK(expr, fl)                                                                                     \
    do {                                                                                                   \
        hipEvent_t e0_ = nullptr, e1_ = nullptr;                                                           \
        if (r->prof) { RCCHK(next_event(r, &e0_)); RCCHK(next_event(r, &e1_)); HIPCHK(hipEventRecord(e0_, s)); } \
        HIPCHK(expr);                                                                                      \
        if (r->prof) { HIPCHK(hipEventRecord(e1_, s)); r->marks.push_back({opd_last_kernel_name, (fl), e0_, e1_}); } \
    } while (0)

int enqueue_forward(opd_reid* r, int nb) {
    if (r->os) {
        hipStream_t s = r->stream;
        return osnet_enqueue(*r->os, nb, reinterpret_cast<const ReidCrop*>(r->d_up), r->d_up, s, [&](double fl, const std::function<hipError_t()>& fn) {
            LCHK(fn(), fl);
            return OPD_OK;
        });
    }
    const ReidArch& a = r->a;
    const int M = nb * a.T;
    hipStream_t s = r->stream;
    const double g2 = 2.0 * M;   // 2 M N K per GEMM
    LCHK(opd_launch_reid_preprocess(reinterpret_cast<const ReidCrop*>(r->d_up), r->d_up, r->lut, r->patches, nb, a.P, a.T, s), 0.0);
    LCHK(opd_launch_reid_gemm(REID_EPI_F32_PBIAS, r->patches, r->wpatch, r->pbias, a.T, r->x, M, a.H, a.KP, s), g2 * a.H * a.KP);
    LCHK(opd_launch_reid_layernorm(r->x, 1, r->preg, r->preb, r->x, r->xn, M, a.H, s), 0.0);
    for (const ReidLayer& L : r->layers) {
        LCHK(opd_launch_reid_layernorm(r->x, 1, L.ln1g, L.ln1b, nullptr, r->xn, M, a.H, s), 0.0);
        LCHK(opd_launch_reid_gemm(REID_EPI_F16_BIAS, r->xn, L.wqkv, L.bqkv, 0, r->qkv, M, 3 * a.H, a.H, s), g2 * 3 * a.H * a.H);
        LCHK(opd_launch_reid_attention(r->qkv, r->attn, nb, a.T, a.H, s), 4.0 * nb * a.T * a.T * a.H);
        LCHK(opd_launch_reid_gemm(REID_EPI_F32_RESID, r->attn, L.wo, L.bo, 0, r->x, M, a.H, a.H, s), g2 * a.H * a.H);
        LCHK(opd_launch_reid_layernorm(r->x, 1, L.ln2g, L.ln2b, nullptr, r->xn, M, a.H, s), 0.0);
        LCHK(opd_launch_reid_gemm(REID_EPI_F16_QGELU, r->xn, L.w1, L.b1, 0, r->mlp, M, a.F, a.H, s), g2 * a.F * a.H);
        LCHK(opd_launch_reid_gemm(REID_EPI_F32_RESID, r->mlp, L.w2, L.b2, 0, r->x, M, a.H, a.F, s), g2 * a.H * a.F);
    }
    LCHK(opd_launch_reid_layernorm(r->x, a.T, r->postg, r->postb, nullptr, r->cls, nb, a.H, s), 0.0);
    LCHK(opd_launch_reid_gemm(REID_EPI_F32_PBIAS, r->cls, r->wproj, nullptr, 0, r->feat, nb, a.E, a.H, s), 2.0 * nb * a.E * a.H);
    LCHK(opd_launch_reid_l2norm(r->feat, nb, a.E, s), 0.0);
    return OPD_OK;
}

int run_forward(opd_reid* r, int nb) {
    if (r->prof || (r->cfg.flags & OPD_FLAG_NO_GRAPH)) return enqueue_forward(r, nb);
    auto it = r->graphs.find(nb);
    if (it != r->graphs.end() && g_graph_guard.load() && it->second.epoch != g_handle_epoch.load()) {   // handles came or went since the
        (void)hipGraphExecDestroy(it->second.exec);                                                       // capture: capture again, as the
        r->graphs.erase(it);                                                                              // detector does (opd_model.h)
        it = r->graphs.end();
    }
    if (it == r->graphs.end()) {
        hipGraph_t graph = nullptr;
        int rc;
        hipError_t ec;
        {
            CaptureExclusive alone;
            HIPCHK(hipStreamBeginCapture(r->stream, hipStreamCaptureModeThreadLocal));
            rc = enqueue_forward(r, nb);
            ec = hipStreamEndCapture(r->stream, &graph);
        }
        if (rc != OPD_OK) { if (graph) (void)hipGraphDestroy(graph); return rc; }
        if (ec != hipSuccess || !graph) {
            (void)hipGetLastError();
            return fail(OPD_EHIP, std::string("hipStreamEndCapture refused the Re-ID forward: ") + hipGetErrorString(ec) + " (OPD_FLAG_NO_GRAPH runs eagerly)");
        }
        hipGraphExec_t exec = nullptr;
        const hipError_t ei = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        if (ei != hipSuccess) {
            (void)hipGetLastError();
            return fail(OPD_EHIP, std::string("hipGraphInstantiate failed for the Re-ID forward: ") + hipGetErrorString(ei));
        }
        it = r->graphs.emplace(nb, opd_reid::Graph{exec, g_handle_epoch.load()}).first;
    }
    HIPCHK(hipGraphLaunch(it->second.exec, r->stream));
    return OPD_OK;
}

// Crop records, coefficient tables and (host frames) source windows of boxes [0, n) into the pinned staging image; padded crops up to
// nb are zero images.  Returns the byte count to upload.
int stage(opd_reid* r, const uint8_t* const* frames, const int32_t* frame_hw, int n_frames, int mem_kind, const float* boxes,
          const int32_t* box_frame, int n, int nb, size_t* used) {
    struct Plan { ReidGeom g; int f; std::vector<int32_t> bx, by, ch, cv; int ksh = 0, ksv = 0; size_t toff = 0, woff = 0; };
    std::vector<Plan> plan((size_t)n);
    const bool os = r->os != nullptr;
    const int OW = os ? OSNET_W : REID_IMG, OH = os ? OSNET_H : REID_IMG;   // outputs per row / column of the pre-processed image
    size_t off = align_up(sizeof(ReidCrop) * (size_t)nb, 256);
    for (int i = 0; i < n; ++i) {
        Plan& p = plan[i];
        p.f = box_frame ? box_frame[i] : 0;
        if (p.f < 0 || p.f >= n_frames) return fail(OPD_EINVAL, "opd_reid_extract: box " + std::to_string(i) + " names frame " + std::to_string(p.f));
        const int H = frame_hw[2 * p.f], W = frame_hw[2 * p.f + 1];
        if (H < 1 || W < 1 || !frames[p.f]) return fail(OPD_EINVAL, "opd_reid_extract: frame " + std::to_string(p.f) + " has no pixels");
        if (os) osnet_geometry(boxes[4 * i], boxes[4 * i + 1], boxes[4 * i + 2], boxes[4 * i + 3], H, W, &p.g);
        else reid_geometry(boxes[4 * i], boxes[4 * i + 1], boxes[4 * i + 2], boxes[4 * i + 3], H, W, &p.g);
        if (p.g.zero) continue;
        if (os) {
            osnet_axis_tables(p.g.x2 - p.g.x1, OW, &p.bx, &p.ch, &p.ksh);
            osnet_axis_tables(p.g.y2 - p.g.y1, OH, &p.by, &p.cv, &p.ksv);
        } else {
            reid_axis_tables(p.g.x2 - p.g.x1, p.g.rw, p.g.left, REID_IMG, &p.bx, &p.ch, &p.ksh);
            reid_axis_tables(p.g.y2 - p.g.y1, p.g.rh, p.g.top, REID_IMG, &p.by, &p.cv, &p.ksv);
        }
        // first taps relative to the window
        for (int k = 0; k < OW; ++k) p.bx[2 * k] -= p.g.wx0 - p.g.x1;
        for (int k = 0; k < OH; ++k) p.by[2 * k] -= p.g.wy0 - p.g.y1;
        p.toff = off;
        off = align_up(off + 4 * (size_t)(2 * OW + 2 * OH + OW * p.ksh + OH * p.ksv), 16);
    }
    if (mem_kind == OPD_MEM_HOST)
        for (int i = 0; i < n; ++i) {
            Plan& p = plan[i];
            if (p.g.zero) continue;
            p.woff = off;
            off = align_up(off + (size_t)(p.g.wy1 - p.g.wy0) * (p.g.wx1 - p.g.wx0) * 3, 16);
        }
    RCCHK(ensure_upload(r, off));
    ReidCrop* rec = reinterpret_cast<ReidCrop*>(r->h_up);
    for (int i = 0; i < nb; ++i) {
        ReidCrop& c = rec[i];
        memset(&c, 0, sizeof c);
        c.zero = 1;
        if (i >= n || plan[i].g.zero) continue;
        const Plan& p = plan[i];
        const int W = frame_hw[2 * p.f + 1];
        c.zero = 0;
        c.ks_h = p.ksh;
        c.ks_v = p.ksv;
        c.tables = (int64_t)p.toff;
        int32_t* t = reinterpret_cast<int32_t*>(r->h_up + p.toff);
        memcpy(t, p.bx.data(), 4 * 2 * (size_t)OW);
        memcpy(t + 2 * OW, p.by.data(), 4 * 2 * (size_t)OH);
        memcpy(t + 2 * OW + 2 * OH, p.ch.data(), 4 * (size_t)OW * p.ksh);
        memcpy(t + 2 * OW + 2 * OH + (size_t)OW * p.ksh, p.cv.data(), 4 * (size_t)OH * p.ksv);
        const size_t fstart = ((size_t)p.g.wy0 * W + p.g.wx0) * 3;
        if (mem_kind == OPD_MEM_HOST) {
            const size_t rowb = (size_t)(p.g.wx1 - p.g.wx0) * 3;
            for (int y = p.g.wy0; y < p.g.wy1; ++y)
                memcpy(r->h_up + p.woff + (size_t)(y - p.g.wy0) * rowb, frames[p.f] + fstart + (size_t)(y - p.g.wy0) * W * 3, rowb);
            c.src = r->d_up + p.woff;
            c.pitch = (int32_t)rowb;
        } else {
            c.src = frames[p.f] + fstart;
            c.pitch = W * 3;
        }
    }
    *used = off;
    return OPD_OK;
}

int check_extract_args(opd_reid* r, const uint8_t* const* frames, const int32_t* frame_hw, int n_frames, int mem_kind, const float* boxes,
                       int n_boxes, const void* out) {
    if (!r) return fail(OPD_EINVAL, "opd_reid_extract: null handle");
    if (n_boxes < 0 || (n_boxes > 0 && (!boxes || !out || !frames || !frame_hw || n_frames < 1)))
        return fail(OPD_EINVAL, "opd_reid_extract: bad arguments");
    if (mem_kind != OPD_MEM_HOST && mem_kind != OPD_MEM_DEVICE) return fail(OPD_EINVAL, "opd_reid_extract: mem_kind must be OPD_MEM_HOST or OPD_MEM_DEVICE");
    return OPD_OK;
}

void destroy_impl(opd_reid* r) {
    if (!r) return;
    (void)hipSetDevice(r->device);
    if (r->stream) (void)hipStreamSynchronize(r->stream);
    destroy_graphs(r);
    for (hipEvent_t e : r->event_pool) (void)hipEventDestroy(e);
    if (r->h_up) (void)hipHostFree(r->h_up);
    if (r->d_up) (void)hipFree(r->d_up);
    if (r->ws) (void)hipFree(r->ws);
    if (r->wmem) (void)hipFree(r->wmem);
    if (r->stream) (void)hipStreamDestroy(r->stream);
    delete r;
}

struct ReidDeleter {
    void operator()(opd_reid* r) const { destroy_impl(r); }
};

int create_osnet(const opd_reid_config* cfg, const StateDict& sd, int device, opd_reid** out) {
    OsnetArchC a;
    RCCHK(osnet_infer(sd, &a));   // the schema is settled before the device is touched
    std::unique_ptr<opd_reid, ReidDeleter> r(new opd_reid);
    r->cfg = *cfg;
    r->device = device;
    r->os.reset(new OsnetModel);
    r->os->a = a;
    for (int b = 8; b < cfg->max_crops; b *= 2) r->buckets.push_back(b);
    r->buckets.push_back(cfg->max_crops);
    std::vector<uint16_t> h16;
    std::vector<float> h32;
    OsnetOffsets offs;
    osnet_pack(sd, a, &h16, &h32, &offs);
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipStreamCreateWithFlags(&r->stream, hipStreamNonBlocking));
    const size_t b16 = align_up(h16.size() * 2, 256), b32 = h32.size() * 4;
    r->wbytes = b16 + b32;
    HIPCHK(hipMalloc(&r->wmem, r->wbytes));
    unsigned char* wb = static_cast<unsigned char*>(r->wmem);
    HIPCHK(hipMemcpy(wb, h16.data(), h16.size() * 2, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(wb + b16, h32.data(), b32, hipMemcpyHostToDevice));
    osnet_bind(r->os.get(), offs, reinterpret_cast<const f16_t*>(wb), reinterpret_cast<const float*>(wb + b16));
    r->wsbytes = osnet_workspace(r->os.get(), cfg->max_crops, nullptr);
    HIPCHK(hipMalloc(&r->ws, r->wsbytes));
    osnet_workspace(r->os.get(), cfg->max_crops, static_cast<unsigned char*>(r->ws));
    RCCHK(ensure_upload(r.get(), align_up(sizeof(ReidCrop) * (size_t)cfg->max_crops, 256) + (size_t)cfg->max_crops * 4 * (OSNET_H + OSNET_W) * 8));
    *out = r.release();
    ++g_handle_epoch;
    return OPD_OK;
}

int create_impl(const opd_reid_config* cfg, const char* weights_path, int device, opd_reid** out) {
    if (!cfg || !weights_path || !out) return fail(OPD_EINVAL, "opd_reid_create: null argument");
    *out = nullptr;
    if (cfg->struct_size != (int32_t)sizeof(opd_reid_config)) return fail(OPD_EINVAL, "opd_reid_config.struct_size mismatch");
    if (cfg->max_crops < 1 || cfg->max_crops > 4096) return fail(OPD_EINVAL, "opd_reid_config.max_crops must be 1 .. 4096");
    if (cfg->model != OPD_REID_MODEL_CLIP && cfg->model != OPD_REID_MODEL_OSNET)
        return fail(OPD_EINVAL, "opd_reid_config.model " + std::to_string(cfg->model) + " is neither OPD_REID_MODEL_CLIP (0) nor OPD_REID_MODEL_OSNET (1)");
    StateDict sd;
    std::string err;
    int rc = load_safetensors(weights_path, &sd, &err, /*raw_keys=*/true);
    if (rc) return fail(rc, err);
    if (cfg->model == OPD_REID_MODEL_OSNET) return create_osnet(cfg, sd, device, out);
    ReidArch a;
    RCCHK(infer_reid_arch(sd, weights_path, &a));   // the schema is settled before the device is touched
    std::unique_ptr<opd_reid, ReidDeleter> r(new opd_reid);   // a failure below releases whatever was already made
    r->cfg = *cfg;
    r->a = a;
    r->device = device;
    for (int b = 8; b < cfg->max_crops; b *= 2) r->buckets.push_back(b);
    r->buckets.push_back(cfg->max_crops);
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipStreamCreateWithFlags(&r->stream, hipStreamNonBlocking));
    // ---- fold and convert the weights on the host -----------------------------------------------------------------------------------
    const int H = a.H, F = a.F, T = a.T, P = a.P, KP = a.KP, E = a.E;
    const std::string vm = "vision_model.";
    auto T_ = [&](const std::string& k) -> const std::vector<float>& { return sd.at(k).data; };
    std::vector<uint16_t> h16;
    std::vector<float> h32;
    auto put16 = [&](const float* v, size_t n, float scale = 1.0f) { const size_t o = h16.size(); for (size_t i = 0; i < n; ++i) h16.push_back(f32_to_f16(v[i] * scale)); return o; };
    auto put32 = [&](const float* v, size_t n, float scale = 1.0f) { const size_t o = h32.size(); for (size_t i = 0; i < n; ++i) h32.push_back(v[i] * scale); return o; };
    std::vector<uint16_t> lut(3 * 256);
    reid_pixel_lut(lut.data());
    const size_t o_lut = h16.size();
    h16.insert(h16.end(), lut.begin(), lut.end());
    // patch weight [H][3][P][P] -> [H][kh][kw][c]: one patch is one contiguous row of the pre-processed image
    std::vector<float> pw((size_t)H * KP);
    {
        const std::vector<float>& src = T_(vm + "embeddings.patch_embedding.weight");
        for (int n = 0; n < H; ++n)
            for (int c = 0; c < 3; ++c)
                for (int kh = 0; kh < P; ++kh)
                    for (int kw = 0; kw < P; ++kw) pw[(size_t)n * KP + (kh * P + kw) * 3 + c] = src[(((size_t)n * 3 + c) * P + kh) * P + kw];
    }
    const size_t o_wpatch = put16(pw.data(), pw.size());
    // row 0 = class_embedding + pos[0]; rows 1.. = pos[1..] (the patch convolution has no bias)
    std::vector<float> pb(T_(vm + "embeddings.position_embedding.weight"));
    for (int n = 0; n < H; ++n) pb[n] += T_(vm + "embeddings.class_embedding")[n];
    const size_t o_pbias = put32(pb.data(), pb.size());
    const size_t o_preg = put32(T_(vm + "pre_layrnorm.weight").data(), H), o_preb = put32(T_(vm + "pre_layrnorm.bias").data(), H);
    const size_t o_postg = put32(T_(vm + "post_layernorm.weight").data(), H), o_postb = put32(T_(vm + "post_layernorm.bias").data(), H);
    const size_t o_proj = put16(T_("visual_projection.weight").data(), (size_t)E * H);
    struct LOff { size_t wqkv, wo, w1, w2, ln1g, ln1b, ln2g, ln2b, bqkv, bo, b1, b2; };
    std::vector<LOff> lo(a.L);
    const float qs = 0.125f;   // 1 / sqrt(head_dim 64), a power of two: folded into q exactly
    for (int l = 0; l < a.L; ++l) {
        const std::string p = vm + "encoder.layers." + std::to_string(l) + ".";
        LOff& o = lo[l];
        o.wqkv = put16(T_(p + "self_attn.q_proj.weight").data(), (size_t)H * H, qs);
        put16(T_(p + "self_attn.k_proj.weight").data(), (size_t)H * H);
        put16(T_(p + "self_attn.v_proj.weight").data(), (size_t)H * H);
        o.bqkv = put32(T_(p + "self_attn.q_proj.bias").data(), H, qs);
        put32(T_(p + "self_attn.k_proj.bias").data(), H);
        put32(T_(p + "self_attn.v_proj.bias").data(), H);
        o.wo = put16(T_(p + "self_attn.out_proj.weight").data(), (size_t)H * H);
        o.bo = put32(T_(p + "self_attn.out_proj.bias").data(), H);
        o.w1 = put16(T_(p + "mlp.fc1.weight").data(), (size_t)F * H);
        o.b1 = put32(T_(p + "mlp.fc1.bias").data(), F);
        o.w2 = put16(T_(p + "mlp.fc2.weight").data(), (size_t)H * F);
        o.b2 = put32(T_(p + "mlp.fc2.bias").data(), H);
        o.ln1g = put32(T_(p + "layer_norm1.weight").data(), H);
        o.ln1b = put32(T_(p + "layer_norm1.bias").data(), H);
        o.ln2g = put32(T_(p + "layer_norm2.weight").data(), H);
        o.ln2b = put32(T_(p + "layer_norm2.bias").data(), H);
    }
    sd.clear();
    const size_t b16 = align_up(h16.size() * 2, 256), b32 = h32.size() * 4;
    r->wbytes = b16 + b32;
    HIPCHK(hipMalloc(&r->wmem, r->wbytes));
    unsigned char* wb = static_cast<unsigned char*>(r->wmem);
    HIPCHK(hipMemcpy(wb, h16.data(), h16.size() * 2, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(wb + b16, h32.data(), b32, hipMemcpyHostToDevice));
    f16_t* w16 = reinterpret_cast<f16_t*>(wb);
    float* w32 = reinterpret_cast<float*>(wb + b16);
    r->lut = w16 + o_lut;
    r->wpatch = w16 + o_wpatch;
    r->wproj = w16 + o_proj;
    r->pbias = w32 + o_pbias;
    r->preg = w32 + o_preg; r->preb = w32 + o_preb; r->postg = w32 + o_postg; r->postb = w32 + o_postb;
    for (const LOff& o : lo)
        r->layers.push_back({w16 + o.wqkv, w16 + o.wo, w16 + o.w1, w16 + o.w2, w32 + o.ln1g, w32 + o.ln1b, w32 + o.ln2g, w32 + o.ln2b,
                             w32 + o.bqkv, w32 + o.bo, w32 + o.b1, w32 + o.b2});
    // ---- workspace for max_crops --------------------------------------------------------------------------------------------------
    const size_t C = (size_t)cfg->max_crops, M = C * T;
    size_t ws = 0;
    auto take = [&](size_t bytes) { const size_t o = ws; ws = align_up(ws + bytes, 256); return o; };
    const size_t o_pat = take(M * KP * 2), o_x = take(M * H * 4), o_xn = take(M * H * 2), o_qkv = take(M * 3 * H * 2), o_attn = take(M * H * 2),
                 o_mlp = take(M * F * 2), o_cls = take(C * H * 2), o_feat = take(C * E * 4);
    r->wsbytes = ws;
    HIPCHK(hipMalloc(&r->ws, ws));
    unsigned char* w = static_cast<unsigned char*>(r->ws);
    r->patches = reinterpret_cast<f16_t*>(w + o_pat);
    r->x = reinterpret_cast<float*>(w + o_x);
    r->xn = reinterpret_cast<f16_t*>(w + o_xn);
    r->qkv = reinterpret_cast<f16_t*>(w + o_qkv);
    r->attn = reinterpret_cast<f16_t*>(w + o_attn);
    r->mlp = reinterpret_cast<f16_t*>(w + o_mlp);
    r->cls = reinterpret_cast<f16_t*>(w + o_cls);
    r->feat = reinterpret_cast<float*>(w + o_feat);
    RCCHK(ensure_upload(r.get(), align_up(sizeof(ReidCrop) * C, 256) + (size_t)C * 4 * REID_IMG * 16));
    *out = r.release();
    ++g_handle_epoch;
    return OPD_OK;
}

template <class F>
int reid_guarded(const char* what, F&& body) {
    try {
        return body();
    } catch (const std::bad_alloc&) {
        return fail(OPD_ENOMEM, std::string(what) + ": out of host memory");
    } catch (const std::out_of_range& e) {
        return fail(OPD_ESCHEMA, std::string(what) + ": weight file lacks a tensor the model needs (" + e.what() + ")");
    } catch (const std::exception& e) {
        return fail(OPD_EINVAL, std::string(what) + ": " + e.what());
    } catch (...) {
        return fail(OPD_EINVAL, std::string(what) + ": unknown C++ exception");
    }
}

}  // namespace

// ---- host-side geometry (opd_reid.h) ------------------------------------------------------------------------------------------------------
namespace opd {

static int py_int(double v) {   // Python's int() of a finite float (truncation), saturated far outside any frame
    if (!(v == v)) return 0;
    if (v > 1e9) return 1000000000;
    if (v < -1e9) return -1000000000;
    return (int)v;
}

void reid_geometry(double x, double y, double w, double h, int H, int W, ReidGeom* g) {
    memset(g, 0, sizeof *g);
    // fmax / fmin return the number when the other operand is NaN, as Python's max(0, x) / min(W, x) do
    g->x1 = py_int(fmax(0.0, x));
    g->y1 = py_int(fmax(0.0, y));
    g->x2 = py_int(fmin((double)W, x + w));
    g->y2 = py_int(fmin((double)H, y + h));
    g->zero = g->x2 <= g->x1 || g->y2 <= g->y1;
    if (g->zero) { g->rh = g->rw = REID_IMG; return; }
    const int ch = g->y2 - g->y1, cw = g->x2 - g->x1;
    const int shrt = cw <= ch ? cw : ch, lng = cw <= ch ? ch : cw;
    const int nl = (int)((double)((int64_t)REID_IMG * lng) / (double)shrt);   // int(224 * long / short)
    if (cw <= ch) { g->rw = REID_IMG; g->rh = nl; } else { g->rh = REID_IMG; g->rw = nl; }
    g->top = (g->rh - REID_IMG) / 2;
    g->left = (g->rw - REID_IMG) / 2;
    std::vector<int32_t> b, c;
    int ks;
    reid_axis_tables(cw, g->rw, g->left, REID_IMG, &b, &c, &ks);
    g->wx0 = g->x1 + b[0];
    g->wx1 = g->x1 + b[2 * (REID_IMG - 1)] + b[2 * (REID_IMG - 1) + 1];
    for (int k = 0; k < REID_IMG; ++k) { g->wx0 = std::min(g->wx0, g->x1 + b[2 * k]); g->wx1 = std::max(g->wx1, g->x1 + b[2 * k] + b[2 * k + 1]); }
    reid_axis_tables(ch, g->rh, g->top, REID_IMG, &b, &c, &ks);
    g->wy0 = g->y1 + b[0];
    g->wy1 = g->y1 + b[2 * (REID_IMG - 1)] + b[2 * (REID_IMG - 1) + 1];
    for (int k = 0; k < REID_IMG; ++k) { g->wy0 = std::min(g->wy0, g->y1 + b[2 * k]); g->wy1 = std::max(g->wy1, g->y1 + b[2 * k] + b[2 * k + 1]); }
}

void reid_axis_tables(int in_size, int out_size, int first, int count, std::vector<int32_t>* bounds, std::vector<int32_t>* coeffs, int* ksize) {
    opd_resize_coeffs_filter(in_size, out_size, /*bicubic=*/true, first, count, bounds, coeffs, ksize);
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

void reid_preprocess_host(const uint8_t* frame, int H, int W, const ReidGeom& g, int P, const uint16_t* lut, uint16_t* out) {
    (void)H;
    const int KP = 3 * P * P, gw = REID_IMG / P;
    memset(out, 0, (size_t)KP * 2);
    std::vector<int32_t> bx, by, chh, cvv;
    int ksh = 0, ksv = 0;
    if (!g.zero) {
        reid_axis_tables(g.x2 - g.x1, g.rw, g.left, REID_IMG, &bx, &chh, &ksh);
        reid_axis_tables(g.y2 - g.y1, g.rh, g.top, REID_IMG, &by, &cvv, &ksv);
    }
    for (int yo = 0; yo < REID_IMG; ++yo)
        for (int xo = 0; xo < REID_IMG; ++xo) {
            int rgb[3] = {0, 0, 0};
            if (!g.zero) {
                const int half = 1 << 21;
                int a[3] = {half, half, half};
                for (int j = 0; j < by[2 * yo + 1]; ++j) {
                    const uint8_t* row = frame + ((size_t)(g.y1 + by[2 * yo] + j) * W + g.x1 + bx[2 * xo]) * 3;
                    int s[3] = {half, half, half};
                    for (int k = 0; k < bx[2 * xo + 1]; ++k)
                        for (int c = 0; c < 3; ++c) s[c] += (int)row[3 * k + c] * chh[(size_t)xo * ksh + k];
                    for (int c = 0; c < 3; ++c) {
                        s[c] >>= 22;
                        s[c] = s[c] < 0 ? 0 : (s[c] > 255 ? 255 : s[c]);
                        a[c] += s[c] * cvv[(size_t)yo * ksv + j];
                    }
                }
                for (int c = 0; c < 3; ++c) {
                    a[c] >>= 22;
                    rgb[2 - c] = a[c] < 0 ? 0 : (a[c] > 255 ? 255 : a[c]);
                }
            }
            const int p = (yo / P) * gw + xo / P;
            for (int c = 0; c < 3; ++c) out[(size_t)(1 + p) * KP + ((yo % P) * P + xo % P) * 3 + c] = lut[c * 256 + rgb[c]];
        }
}

// test hook body (opd_reid_test_api.cpp): stage + pre-process only, patches [n][T][KP] back to the host
int reid_test_pixels(opd_reid* r, const uint8_t* const* frames, const int32_t* frame_hw, int n_frames, int mem_kind, const float* boxes,
                     const int32_t* box_frame, int n, uint16_t* out) {
    ApiScope api_scope;
    RCCHK(check_extract_args(r, frames, frame_hw, n_frames, mem_kind, boxes, n, out));
    if (n > r->cfg.max_crops) return fail(OPD_EINVAL, "reid_test_pixels: more boxes than max_crops");
    if (n == 0) return OPD_OK;
    HIPCHK(hipSetDevice(r->device));
    size_t used = 0;
    RCCHK(stage(r, frames, frame_hw, n_frames, mem_kind, boxes, box_frame, n, n, &used));
    HIPCHK(hipMemcpyAsync(r->d_up, r->h_up, used, hipMemcpyHostToDevice, r->stream));
    if (r->os) {   // OSNet: [n][256][128][4]
        HIPCHK(opd_launch_osnet_preprocess(reinterpret_cast<const ReidCrop*>(r->d_up), r->d_up, r->os->lut, r->os->img, n, r->stream));
        HIPCHK(hipMemcpyAsync(out, r->os->img, (size_t)n * OSNET_H * OSNET_W * 4 * 2, hipMemcpyDeviceToHost, r->stream));
        HIPCHK(hipStreamSynchronize(r->stream));
        return OPD_OK;
    }
    HIPCHK(opd_launch_reid_preprocess(reinterpret_cast<const ReidCrop*>(r->d_up), r->d_up, r->lut, r->patches, n, r->a.P, r->a.T, r->stream));
    HIPCHK(hipMemcpyAsync(out, r->patches, (size_t)n * r->a.T * r->a.KP * 2, hipMemcpyDeviceToHost, r->stream));
    HIPCHK(hipStreamSynchronize(r->stream));
    return OPD_OK;
}

int reid_test_kernel_table(opd_reid* r, const uint8_t* const* frames, const int32_t* frame_hw, int n_frames, const float* boxes,
                           const int32_t* box_frame, int n, int iters, opd_kernel_stat* out, int capacity, int* count) {
    ApiScope api_scope;
    RCCHK(check_extract_args(r, frames, frame_hw, n_frames, OPD_MEM_HOST, boxes, n, out));
    if (n < 1 || n > r->cfg.max_crops || iters < 1 || !count) return fail(OPD_EINVAL, "reid_test_kernel_table: bad arguments");
    HIPCHK(hipSetDevice(r->device));
    const int nb = bucket_of(r, n);
    size_t used = 0;
    RCCHK(stage(r, frames, frame_hw, n_frames, OPD_MEM_HOST, boxes, box_frame, n, nb, &used));
    HIPCHK(hipMemcpyAsync(r->d_up, r->h_up, used, hipMemcpyHostToDevice, r->stream));
    std::vector<std::string> names;
    std::vector<opd_kernel_stat> rows;
    r->prof = true;
    int rc = OPD_OK;
    for (int it = 0; it < iters && rc == OPD_OK; ++it) {
        r->marks.clear();
        r->events_used = 0;
        rc = enqueue_forward(r, nb);
        if (rc == OPD_OK && hipStreamSynchronize(r->stream) != hipSuccess) rc = fail(OPD_EHIP, "hipStreamSynchronize failed");
        for (size_t i = 0; rc == OPD_OK && i < r->marks.size(); ++i) {
            const opd_reid::Mark& mk = r->marks[i];
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, mk.e0, mk.e1) != hipSuccess) { rc = fail(OPD_EHIP, "hipEventElapsedTime failed"); break; }
            size_t k = 0;
            while (k < names.size() && names[k] != mk.name) ++k;
            if (k == names.size()) {
                names.push_back(mk.name);
                opd_kernel_stat z;
                memset(&z, 0, sizeof z);
                snprintf(z.name, sizeof z.name, "%s", mk.name);
                rows.push_back(z);
            }
            rows[k].launches += 1;
            rows[k].ms += ms;
            rows[k].flops += mk.flops;
        }
    }
    r->prof = false;
    r->marks.clear();
    RCCHK(rc);
    *count = (int)rows.size();
    for (int i = 0; i < (int)rows.size() && i < capacity; ++i) out[i] = rows[i];
    return OPD_OK;
}

}  // namespace opd

extern "C" {

int opd_reid_create(const opd_reid_config* cfg, const char* weights_path, int device_ordinal, opd_reid** out) {
    ApiScope api_scope;
    return reid_guarded("opd_reid_create", [&] { return create_impl(cfg, weights_path, device_ordinal, out); });
}

void opd_reid_destroy(opd_reid* r) {
    ApiScope api_scope;
    if (!r) return;
    destroy_impl(r);
    ++g_handle_epoch;
}

int opd_reid_info(const opd_reid* r, opd_reid_model_info* info) {
    if (!r || !info) return fail(OPD_EINVAL, "opd_reid_info: null argument");
    memset(info, 0, sizeof *info);
    if (r->os) {   // OSNet: tokens, layers, heads, mlp_dim and patch stay 0
        info->model = OPD_REID_MODEL_OSNET;
        info->feature_dim = OSNET_FEAT;
        info->hidden = r->os->a.widths[3];
        info->max_crops = r->cfg.max_crops;
        info->device_ordinal = r->device;
        info->weight_bytes_device = (int64_t)r->wbytes;
        info->workspace_bytes_device = (int64_t)(r->wsbytes + r->up_cap);
        return OPD_OK;
    }
    info->model = OPD_REID_MODEL_CLIP;
    info->feature_dim = r->a.E;
    info->tokens = r->a.T;
    info->hidden = r->a.H;
    info->layers = r->a.L;
    info->heads = r->a.heads;
    info->mlp_dim = r->a.F;
    info->patch = r->a.P;
    info->max_crops = r->cfg.max_crops;
    info->device_ordinal = r->device;
    info->weight_bytes_device = (int64_t)r->wbytes;
    info->workspace_bytes_device = (int64_t)(r->wsbytes + r->up_cap);
    return OPD_OK;
}

int opd_reid_extract(opd_reid* r, const uint8_t* const* frames, const int32_t* frame_hw, int n_frames, int mem_kind, const float* boxes_xywh,
                     const int32_t* box_frame, int n_boxes, float* out) {
    ApiScope api_scope;
    return reid_guarded("opd_reid_extract", [&]() -> int {
        RCCHK(check_extract_args(r, frames, frame_hw, n_frames, mem_kind, boxes_xywh, n_boxes, out));
        if (n_boxes == 0) return OPD_OK;
        HIPCHK(hipSetDevice(r->device));
        const int E = r->os ? OSNET_FEAT : r->a.E;
        const float* feat = r->os ? r->os->feat : r->feat;
        for (int c0 = 0; c0 < n_boxes; c0 += r->cfg.max_crops) {   // more boxes than max_crops: chunks of max_crops
            const int n = std::min(r->cfg.max_crops, n_boxes - c0);
            const int nb = bucket_of(r, n);
            size_t used = 0;
            RCCHK(stage(r, frames, frame_hw, n_frames, mem_kind, boxes_xywh + 4 * (size_t)c0, box_frame ? box_frame + c0 : nullptr, n, nb, &used));
            HIPCHK(hipMemcpyAsync(r->d_up, r->h_up, used, hipMemcpyHostToDevice, r->stream));
            RCCHK(run_forward(r, nb));
            HIPCHK(hipMemcpyAsync(out + (size_t)c0 * E, feat, (size_t)n * E * 4, hipMemcpyDeviceToHost, r->stream));
            HIPCHK(hipStreamSynchronize(r->stream));   // (the pinned staging image is rewritten by the next chunk)
        }
        return OPD_OK;
    });
}

}  // extern "C"
