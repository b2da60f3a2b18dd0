// opd_reid.cpp — the Re-ID handle (include/opd_detr.h, opd_reid_*): one ReidModel (opd_reid.h: the CLIP tower of opd_clip.cpp or the
// OSNet of opd_osnet.cpp), its weights and a workspace sized once for max_crops, its own stream, one captured hipGraph per crop-count
// bucket, and host staging of each crop's coefficient tables and source window.  Nothing here depends on which model it is, except
// the one line of create that constructs it.
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "opd_clip.h"
#include "opd_osnet.h"

using namespace opd;

struct opd_reid {
    int device = 0;
    opd_reid_config cfg{};
    std::unique_ptr<ReidModel> model;
    ReidLauncher launch;   // the stream, and per-launch timing of eager forwards (opd_test_reid_kernel_table)
    void* wmem = nullptr;   // weights
    size_t wbytes = 0;
    void* ws = nullptr;     // workspace (max_crops)
    size_t wsbytes = 0;
    // staging: [ReidCrop x max_crops][tables][windows], pinned host image + device copy, grown on demand
    Staging up;
    std::vector<int> buckets;
    std::map<int, GraphSlot> graphs;   // by crop-count bucket, captured on first use
    // One call at a time: opd_reid_extract and the fused detect call (opd_detr_detect_frames_reid) both rewrite the staging buffer and
    // replay the same graphs.  A second thread waits here, with its hold of the entry-point lock handed back meanwhile (a capture
    // inside the first call takes that lock exclusively).
    std::mutex call_mu;
    hipEvent_t ev_planned = nullptr, ev_done = nullptr;   // fused call: the detector's stream -> this handle's stream and back
};

namespace {

void destroy_graphs(opd_reid* r) {
    for (auto& kv : r->graphs) kv.second.drop();
    r->graphs.clear();
}

int ensure_upload(opd_reid* r, size_t bytes) {
    const size_t cap = bytes <= r->up.dev_cap ? bytes : std::max(bytes, r->up.dev_cap * 2);   // grows by doubling
    bool moved = false;
    const int rc = r->up.reserve("opd_reid", cap, cap, r->launch.stream, &moved);   // (nothing may be launched between this and the next line)
    if (moved) destroy_graphs(r);   // the captured kernels hold the old base pointer
    return rc;
}

struct CallLock {
    std::unique_lock<std::mutex> lk;
    explicit CallLock(opd_reid* r) : lk(r->call_mu, std::defer_lock) {
        ApiUnlocked waiting;
        lk.lock();
    }
};

int bucket_of(const opd_reid* r, int n) {
    for (int b : r->buckets)
        if (b >= n) return b;
    return r->buckets.back();
}

int enqueue_forward(opd_reid* r, int nb) { return r->model->enqueue(nb, reinterpret_cast<const ReidCrop*>(r->up.dev), r->up.dev, r->launch); }

int run_forward(opd_reid* r, int nb) {
    if (r->launch.prof || (r->cfg.flags & OPD_FLAG_NO_GRAPH)) return enqueue_forward(r, nb);
    return r->graphs[nb].run(r->launch.stream, "the Re-ID forward", [&] { return enqueue_forward(r, nb); });
}

// Crop records, coefficient tables and (host frames) source windows of boxes [0, n) into the pinned staging image; padded crops up to
// nb are zero images.  Returns the byte count to upload.
int stage(opd_reid* r, const uint8_t* const* frames, const int32_t* frame_hw, int n_frames, int mem_kind, const float* boxes,
          const int32_t* box_frame, int n, int nb, size_t* used) {
    struct Plan { ReidGeom g; int f; std::vector<int32_t> bx, by, ch, cv; int ksh = 0, ksv = 0; size_t toff = 0, woff = 0; };
    std::vector<Plan> plan((size_t)n);
    const CropSpec& spec = r->model->crop();
    const int OW = spec.out_w, OH = spec.out_h;   // outputs per row / column of the pre-processed image
    size_t off = align_up(sizeof(ReidCrop) * (size_t)nb, 256);
    for (int i = 0; i < n; ++i) {
        Plan& p = plan[i];
        p.f = box_frame ? box_frame[i] : 0;
        if (p.f < 0 || p.f >= n_frames) return fail(OPD_EINVAL, "opd_reid_extract: box " + std::to_string(i) + " names frame " + std::to_string(p.f));
        const int H = frame_hw[2 * p.f], W = frame_hw[2 * p.f + 1];
        if (H < 1 || W < 1 || !frames[p.f]) return fail(OPD_EINVAL, "opd_reid_extract: frame " + std::to_string(p.f) + " has no pixels");
        crop_geometry(spec, boxes[4 * i], boxes[4 * i + 1], boxes[4 * i + 2], boxes[4 * i + 3], H, W, &p.g);
        if (p.g.zero) continue;
        crop_axis_tables(spec, p.g, true, &p.bx, &p.ch, &p.ksh);
        crop_axis_tables(spec, p.g, false, &p.by, &p.cv, &p.ksv);
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
    ReidCrop* rec = reinterpret_cast<ReidCrop*>(r->up.host);
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
        int32_t* t = reinterpret_cast<int32_t*>(r->up.host + p.toff);
        memcpy(t, p.bx.data(), 4 * 2 * (size_t)OW);
        memcpy(t + 2 * OW, p.by.data(), 4 * 2 * (size_t)OH);
        memcpy(t + 2 * OW + 2 * OH, p.ch.data(), 4 * (size_t)OW * p.ksh);
        memcpy(t + 2 * OW + 2 * OH + (size_t)OW * p.ksh, p.cv.data(), 4 * (size_t)OH * p.ksv);
        const size_t fstart = ((size_t)p.g.wy0 * W + p.g.wx0) * 3;
        if (mem_kind == OPD_MEM_HOST) {
            const size_t rowb = (size_t)(p.g.wx1 - p.g.wx0) * 3;
            for (int y = p.g.wy0; y < p.g.wy1; ++y)
                memcpy(r->up.host + p.woff + (size_t)(y - p.g.wy0) * rowb, frames[p.f] + fstart + (size_t)(y - p.g.wy0) * W * 3, rowb);
            c.src = r->up.dev + p.woff;
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
    if (r->launch.stream) (void)hipStreamSynchronize(r->launch.stream);
    destroy_graphs(r);
    r->launch.timer.release();
    for (hipEvent_t e : {r->ev_planned, r->ev_done})
        if (e) (void)hipEventDestroy(e);
    r->up.release();
    if (r->ws) (void)hipFree(r->ws);
    if (r->wmem) (void)hipFree(r->wmem);
    if (r->launch.stream) (void)hipStreamDestroy(r->launch.stream);
    delete r;
}

struct ReidDeleter {
    void operator()(opd_reid* r) const { destroy_impl(r); }
};

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
    std::unique_ptr<ReidModel> model;   // the schema is settled before the device is touched
    RCCHK(cfg->model == OPD_REID_MODEL_OSNET ? osnet_create(sd, &model) : clip_create(sd, weights_path, &model));
    std::unique_ptr<opd_reid, ReidDeleter> r(new opd_reid);   // a failure below releases whatever was already made
    r->cfg = *cfg;
    r->device = device;
    r->model = std::move(model);
    for (int b = 8; b < cfg->max_crops; b *= 2) r->buckets.push_back(b);
    r->buckets.push_back(cfg->max_crops);
    std::vector<uint16_t> h16;
    std::vector<float> h32;
    r->model->pack(sd, &h16, &h32);
    sd.clear();
    RCCHK(use_device("opd_reid_create", device));
    HIPCHK(hipStreamCreateWithFlags(&r->launch.stream, hipStreamNonBlocking));
    HIPCHK(hipEventCreateWithFlags(&r->ev_planned, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&r->ev_done, hipEventDisableTiming));
    const size_t b16 = align_up(h16.size() * 2, 256), b32 = h32.size() * 4;
    r->wbytes = b16 + b32;
    HIPCHK(hipMalloc(&r->wmem, r->wbytes));
    unsigned char* wb = static_cast<unsigned char*>(r->wmem);
    HIPCHK(hipMemcpy(wb, h16.data(), h16.size() * 2, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(wb + b16, h32.data(), b32, hipMemcpyHostToDevice));
    r->model->bind(reinterpret_cast<const f16_t*>(wb), reinterpret_cast<const float*>(wb + b16));
    r->wsbytes = r->model->workspace(cfg->max_crops, nullptr);
    HIPCHK(hipMalloc(&r->ws, r->wsbytes));
    r->model->workspace(cfg->max_crops, static_cast<unsigned char*>(r->ws));
    const size_t C = (size_t)cfg->max_crops, outs = r->model->crop().out_h + r->model->crop().out_w;
    RCCHK(ensure_upload(r.get(), align_up(sizeof(ReidCrop) * C, 256) + C * 4 * outs * 8));   // 8 taps per output; stage() grows it
    *out = r.release();
    ++g_handle_epoch;
    return OPD_OK;
}

}  // namespace

namespace opd {

// ---- the Re-ID half of the fused detect call (opd_api.cpp: opd_detr_detect_frames_reid) ------------------------------------------------
// Staging layout of a fused call: [ReidCrop x max_crops | slot[max_crops], rec[max_crops], n_person | tables: one fixed stride per crop]
static size_t fused_sel_off(const opd_reid* r) { return align_up(sizeof(ReidCrop) * (size_t)r->cfg.max_crops, 256); }
static size_t fused_tables_off(const opd_reid* r) { return fused_sel_off(r) + align_up(4 * (2 * (size_t)r->cfg.max_crops + 1), 256); }

int reid_fused_check(const opd_reid* r, int device, int slots, const char* who) {
    if (!r) return fail(OPD_EINVAL, std::string(who) + ": null Re-ID handle");
    if (slots < 1 || slots > r->cfg.max_crops)
        return fail(OPD_EINVAL, std::string(who) + ": slots = " + std::to_string(slots) + " outside 1 .. max_crops = " + std::to_string(r->cfg.max_crops));
    if (r->device != device)
        return fail(OPD_EINVAL, std::string(who) + ": the detector is on device " + std::to_string(device) + ", the Re-ID model on device " + std::to_string(r->device));
    return OPD_OK;
}

int reid_feature_dim(const opd_reid* r) { return r->model->feature_dim(); }

ReidFusedCall::ReidFusedCall(opd_reid* r_) : r(r_), lk(r_->call_mu, std::defer_lock) {
    ApiUnlocked waiting;
    lk.lock();
}

int ReidFusedCall::enqueue(hipStream_t s, const RecordView& v, const uint8_t* frames, int h, int w, int label, int slots_, int32_t* geom) {
    slots = slots_;
    const int C = r->cfg.max_crops, E = r->model->feature_dim();
    const CropSpec& spec = r->model->crop();
    const CropSlots cs = crop_slots(spec, h, w);
    const size_t out_bytes = (size_t)slots * E * 4 + 4 * (2 * (size_t)C + 1);   // what comes back through the pinned side
    RCCHK(ensure_upload(r, std::max(fused_tables_off(r) + (size_t)C * cs.stride, out_bytes)));   // (drops the graphs only when it had to grow: a larger frame size)
    const int nb = bucket_of(r, slots);
    int32_t* sel = reinterpret_cast<int32_t*>(r->up.dev + fused_sel_off(r));
    CropSelectParams sp{};
    sp.view = v; sp.label = label; sp.slots = slots;
    sp.slot = sel; sp.rec = sel + C; sp.n_person = sel + 2 * C;
    HIPCHK(opd_launch_crop_select(sp, s));
    CropPlanParams pp{};
    pp.spec = spec;
    pp.view = v; pp.rec = sp.rec; pp.n_person = sp.n_person;
    pp.frames = frames; pp.h = h; pp.w = w; pp.slots = slots; pp.geom = geom;
    pp.base = r->up.dev; pp.tables_off = fused_tables_off(r); pp.stride = cs.stride;
    pp.ksh_max = cs.ksh_max; pp.ksv_max = cs.ksv_max;
    HIPCHK(opd_launch_crop_plan(pp, nb, s));
    HIPCHK(hipEventRecord(r->ev_planned, s));
    HIPCHK(hipStreamWaitEvent(r->launch.stream, r->ev_planned, 0));
    RCCHK(run_forward(r, nb));
    HIPCHK(hipEventRecord(r->ev_done, r->launch.stream));
    HIPCHK(hipStreamWaitEvent(s, r->ev_done, 0));
    return OPD_OK;
}

int ReidFusedCall::copy_back(hipStream_t s) {
    const int C = r->cfg.max_crops, E = r->model->feature_dim();
    const size_t fb = (size_t)slots * E * 4;
    if (with_rows) HIPCHK(hipMemcpyAsync(r->up.host, r->model->features(), fb, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(r->up.host + fb, r->up.dev + fused_sel_off(r), 4 * (2 * (size_t)C + 1), hipMemcpyDeviceToHost, s));
    return OPD_OK;
}

void ReidFusedCall::deliver(float* features, int32_t* slot_map, int32_t* n_person) const {
    const int C = r->cfg.max_crops, E = r->model->feature_dim();
    const int32_t* sel = reinterpret_cast<const int32_t*>(r->up.host + (size_t)slots * E * 4);
    const int np = sel[2 * C], n = std::min(np, slots);
    *n_person = np;
    if (features && with_rows) memcpy(features, r->up.host, (size_t)n * E * 4);
    memcpy(slot_map, sel, (size_t)n * 4);
}

const float* ReidFusedCall::dev_rows() const { return r->model->features(); }
const int32_t* ReidFusedCall::dev_slot_map() const { return reinterpret_cast<const int32_t*>(r->up.dev + fused_sel_off(r)); }
const int32_t* ReidFusedCall::dev_rec() const { return dev_slot_map() + (size_t)r->cfg.max_crops; }
const int32_t* ReidFusedCall::dev_n_person() const { return dev_slot_map() + 2 * (size_t)r->cfg.max_crops; }

void ReidFusedCall::slots_per_frame(int B, int Q, int32_t* out) const {
    const int C = r->cfg.max_crops, E = r->model->feature_dim();
    const int32_t* sel = reinterpret_cast<const int32_t*>(r->up.host + (size_t)slots * E * 4);
    const int n = std::min(sel[2 * C], slots);
    for (int b = 0; b < B; ++b) out[b] = 0;
    for (int k = 0; k < n; ++k) {
        const int f = sel[C + k] / Q;   // (rec[k] = frame * Q + record index)
        if (f >= 0 && f < B) ++out[f];
    }
}

// test hook body (opd_reid_test_api.cpp): stage + pre-process only, the model's image of each crop back to the host
int reid_test_pixels(opd_reid* r, const uint8_t* const* frames, const int32_t* frame_hw, int n_frames, int mem_kind, const float* boxes,
                     const int32_t* box_frame, int n, uint16_t* out) {
    ApiScope api_scope;
    RCCHK(check_extract_args(r, frames, frame_hw, n_frames, mem_kind, boxes, n, out));
    if (n > r->cfg.max_crops) return fail(OPD_EINVAL, "reid_test_pixels: more boxes than max_crops");
    if (n == 0) return OPD_OK;
    CallLock one_call(r);
    HIPCHK(hipSetDevice(r->device));
    size_t used = 0;
    RCCHK(stage(r, frames, frame_hw, n_frames, mem_kind, boxes, box_frame, n, n, &used));
    HIPCHK(hipMemcpyAsync(r->up.dev, r->up.host, used, hipMemcpyHostToDevice, r->launch.stream));
    HIPCHK(r->model->preprocess(n, reinterpret_cast<const ReidCrop*>(r->up.dev), r->up.dev, r->launch.stream));
    HIPCHK(hipMemcpyAsync(out, r->model->image(), (size_t)n * r->model->image_bytes(), hipMemcpyDeviceToHost, r->launch.stream));
    HIPCHK(hipStreamSynchronize(r->launch.stream));
    return OPD_OK;
}

int reid_test_kernel_table(opd_reid* r, const uint8_t* const* frames, const int32_t* frame_hw, int n_frames, const float* boxes,
                           const int32_t* box_frame, int n, int iters, opd_kernel_stat* out, int capacity, int* count) {
    ApiScope api_scope;
    RCCHK(check_extract_args(r, frames, frame_hw, n_frames, OPD_MEM_HOST, boxes, n, out));
    if (n < 1 || n > r->cfg.max_crops || iters < 1 || !count) return fail(OPD_EINVAL, "reid_test_kernel_table: bad arguments");
    CallLock one_call(r);
    HIPCHK(hipSetDevice(r->device));
    const int nb = bucket_of(r, n);
    size_t used = 0;
    RCCHK(stage(r, frames, frame_hw, n_frames, OPD_MEM_HOST, boxes, box_frame, n, nb, &used));
    HIPCHK(hipMemcpyAsync(r->up.dev, r->up.host, used, hipMemcpyHostToDevice, r->launch.stream));
    static const char* const unnamed[1] = {"(unnamed)"};   // (LCHK times every launch as class 0)
    std::vector<KernelRow> rows;   // first-seen order, summed over the iterations
    r->launch.prof = true;
    int rc = OPD_OK;
    for (int it = 0; it < iters && rc == OPD_OK; ++it) {
        r->launch.timer.reset();
        rc = enqueue_forward(r, nb);
        if (rc == OPD_OK && hipStreamSynchronize(r->launch.stream) != hipSuccess) rc = fail(OPD_EHIP, "hipStreamSynchronize failed");
        if (rc == OPD_OK && r->launch.timer.fold(&rows, unnamed)) rc = fail(OPD_EHIP, "hipEventElapsedTime failed");
    }
    r->launch.prof = false;
    r->launch.timer.reset();
    RCCHK(rc);
    *count = (int)rows.size();
    for (int i = 0; i < (int)rows.size() && i < capacity; ++i) {
        memset(&out[i], 0, sizeof out[i]);
        snprintf(out[i].name, sizeof out[i].name, "%s", rows[i].name.c_str());
        out[i].launches = rows[i].launches; out[i].ms = rows[i].ms; out[i].flops = rows[i].flops;
    }
    return OPD_OK;
}

}  // namespace opd

extern "C" {

int opd_reid_create(const opd_reid_config* cfg, const char* weights_path, int device_ordinal, opd_reid** out) {
    return api_call("opd_reid_create", [&] { return create_impl(cfg, weights_path, device_ordinal, out); }, API_CREATE);
}

void opd_reid_destroy(opd_reid* r) { (void)api_call("opd_reid_destroy", [&]() -> int {
    if (!r) return OPD_OK;
    destroy_impl(r);
    ++g_handle_epoch;
    return OPD_OK;
}); }

int opd_reid_info(const opd_reid* r, opd_reid_model_info* info) { return api_call_unlocked("opd_reid_info", [&]() -> int {
    if (!r || !info) return fail(OPD_EINVAL, "opd_reid_info: null argument");
    memset(info, 0, sizeof *info);
    r->model->fill_info(info);
    info->max_crops = r->cfg.max_crops;
    info->device_ordinal = r->device;
    info->weight_bytes_device = (int64_t)r->wbytes;
    info->workspace_bytes_device = (int64_t)(r->wsbytes + r->up.dev_cap);
    return OPD_OK;
}); }

int opd_reid_extract(opd_reid* r, const uint8_t* const* frames, const int32_t* frame_hw, int n_frames, int mem_kind, const float* boxes_xywh,
                     const int32_t* box_frame, int n_boxes, float* out) { return api_call("opd_reid_extract", [&]() -> int {
    RCCHK(check_extract_args(r, frames, frame_hw, n_frames, mem_kind, boxes_xywh, n_boxes, out));
    if (n_boxes == 0) return OPD_OK;
    CallLock one_call(r);
    HIPCHK(hipSetDevice(r->device));
    const int E = r->model->feature_dim();
    const float* feat = r->model->features();
    for (int c0 = 0; c0 < n_boxes; c0 += r->cfg.max_crops) {   // more boxes than max_crops: chunks of max_crops
        const int n = std::min(r->cfg.max_crops, n_boxes - c0);
        const int nb = bucket_of(r, n);
        size_t used = 0;
        RCCHK(stage(r, frames, frame_hw, n_frames, mem_kind, boxes_xywh + 4 * (size_t)c0, box_frame ? box_frame + c0 : nullptr, n, nb, &used));
        HIPCHK(hipMemcpyAsync(r->up.dev, r->up.host, used, hipMemcpyHostToDevice, r->launch.stream));
        RCCHK(run_forward(r, nb));
        HIPCHK(hipMemcpyAsync(out + (size_t)c0 * E, feat, (size_t)n * E * 4, hipMemcpyDeviceToHost, r->launch.stream));
        HIPCHK(hipStreamSynchronize(r->launch.stream));   // (the pinned staging image is rewritten by the next chunk)
    }
    return OPD_OK;
}); }

}  // extern "C"
