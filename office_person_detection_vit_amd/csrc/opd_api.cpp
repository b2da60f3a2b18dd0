// opd_api.cpp — the C-ABI of include/opd_detr.h for the detector: handle creation / cloning / destruction, the argument checks of every
// entry point, and the ONE detect pipeline behind them (frame source -> device pixels -> forward -> the sink's stages -> one fetch; opd_model.h).
// The model itself is opd_weights.cpp (the weights) and opd_model.cpp (workspace, plans, the forward and its graph cache).
#include <algorithm>
#include <new>
#include <optional>
#include <stdexcept>

#include "opd_floor.h"
#include "opd_lwt.h"
#include "opd_model.h"
#include "opd_nms.h"
#include "opd_reid.h"
#include "opd_tile.h"
#include "opd_track.h"

namespace opd {

// mem_kind: where the pixels come from / where the outputs go
static inline bool pixels_on_device(int mem_kind) { return mem_kind == OPD_MEM_DEVICE; }
static inline bool outputs_on_device(int mem_kind) { return mem_kind != OPD_MEM_HOST; }

static int check_device_outputs(int mem_kind, const void* out, const void* counts, const char* who) {
    if (!outputs_on_device(mem_kind)) return OPD_OK;
    if (!device_accessible(out) || !device_accessible(counts))
        return fail(OPD_EINVAL, std::string(who) + ": this mem_kind takes DEVICE output pointers; the ones given are not device-accessible memory");
    return OPD_OK;
}

int check_shape(opd_detr* m, const void* pixels, int pixel_format, int mem_kind, int B, int H, int W) {
    if (!m) return fail(OPD_EINVAL, "null model handle");
    if (!pixels) return fail(OPD_EINVAL, "null pixel buffer");
    if (pixel_format != OPD_PIXELS_U8_BGR_HWC && pixel_format != OPD_PIXELS_F32_NCHW) return fail(OPD_EINVAL, "unknown pixel_format");
    if (mem_kind != OPD_MEM_HOST && mem_kind != OPD_MEM_DEVICE && mem_kind != OPD_MEM_HOST_PIXELS_DEVICE_OUT)
        return fail(OPD_EINVAL, "unknown mem_kind");
    if (pixels_on_device(mem_kind) && !device_accessible(pixels))
        return fail(OPD_EINVAL, "OPD_MEM_DEVICE: the pixel pointer is not device-accessible memory");
    const int edge = std::max(m->cfg.max_height, m->cfg.max_width);   // either orientation: see build_workspace
    if (B < 1 || B > m->cfg.max_batch || H < 32 || W < 32 || H > edge || W > edge ||
        (size_t)H * W > (size_t)m->cfg.max_height * m->cfg.max_width)
        return fail(OPD_EINVAL, "frame batch [" + std::to_string(B) + "," + std::to_string(H) + "," + std::to_string(W) +
                                    "] outside the configured maximum [" + std::to_string(m->cfg.max_batch) + "," +
                                    std::to_string(m->cfg.max_height) + "," + std::to_string(m->cfg.max_width) + "] (either orientation)");
    return OPD_OK;
}

static int stage_pixels(opd_detr* m, const void* pixels, int pixel_format, int mem_kind, int B, int H, int W, const void** d_pixels) {
    if (pixels_on_device(mem_kind)) { *d_pixels = pixels; return OPD_OK; }
    const bool u8 = pixel_format == OPD_PIXELS_U8_BGR_HWC;
    void* dst = u8 ? static_cast<void*>(m->d_u8) : m->d_pv;
    HIPCHK(hipMemcpyAsync(dst, pixels, (size_t)B * H * W * 3 * (u8 ? 1 : 4), hipMemcpyHostToDevice, m->stream));
    *d_pixels = dst;
    return OPD_OK;
}

// The handle's coefficient tables of a h x w -> oh x ow resize (opd_resize_coeffs), built and uploaded by the first call that needs them
static int resize_tab(opd_detr* m, int h, int w, int oh, int ow, const opd_detr::ResizeTab** out) {
    for (const auto& t : m->resize_tabs)
        if (t.h == h && t.w == w && t.oh == oh && t.ow == ow) { *out = &t; return OPD_OK; }
    std::vector<int32_t> bh, kh, bv, kv;
    opd_detr::ResizeTab t{h, w, oh, ow, 0, 0, nullptr, nullptr, nullptr, nullptr};
    opd_resize_coeffs(w, ow, &bh, &kh, &t.ksh);
    opd_resize_coeffs(h, oh, &bv, &kv, &t.ksv);
    auto up = [&](const std::vector<int32_t>& v, int32_t** d) -> int {
        RCCHK(dalloc(m, d, v.size(), false));
        HIPCHK(hipMemcpy(*d, v.data(), v.size() * 4, hipMemcpyHostToDevice));
        return OPD_OK;
    };
    RCCHK(up(bh, &t.bh)); RCCHK(up(kh, &t.kh)); RCCHK(up(bv, &t.bv)); RCCHK(up(kv, &t.kv));
    m->resize_tabs.push_back(t);
    *out = &m->resize_tabs.back();
    return OPD_OK;
}

// A camera frame of h x w: what the resize tables and the byte counts of the source step are sized for (each entry words its own refusal)
static inline bool frame_size_ok(int h, int w) { return h >= 1 && w >= 1 && (size_t)h * w <= (size_t)1 << 26; }

// Host camera frames -> m->src, one behind the other: ONE block, or (`list` != null) one host pointer per frame
static int upload_camera_frames(opd_detr* m, const uint8_t* block, const uint8_t* const* list, int n, int h, int w) {
    const size_t n1 = (size_t)h * w * 3;
    RCCHK(m->src.reserve("source frames", 0, n * n1, m->stream));
    if (!list) HIPCHK(hipMemcpyAsync(m->src.dev, block, n * n1, hipMemcpyHostToDevice, m->stream));
    else for (int b = 0; b < n; ++b) HIPCHK(hipMemcpyAsync(m->src.dev + b * n1, list[b], n1, hipMemcpyHostToDevice, m->stream));
    return OPD_OK;
}

// Frames at camera resolution -> m->d_u8 at model resolution (Pillow-exact bilinear, kernels_untyped.hip).
// (`list` != null: one host pointer per frame instead of the contiguous block `frames`)
static int enqueue_resize(opd_detr* m, const uint8_t* frames, int mem_kind, int B, int h, int w, int oh, int ow, const uint8_t* const* list = nullptr) {
    if (!frame_size_ok(h, w)) return fail(OPD_EINVAL, "source frame size out of range");
    const uint8_t* d_in = frames;
    if (!pixels_on_device(mem_kind)) {
        RCCHK(upload_camera_frames(m, frames, list, B, h, w));
        d_in = m->src.dev;
    }
    const opd_detr::ResizeTab* tab = nullptr;
    RCCHK(resize_tab(m, h, w, oh, ow, &tab));
    HIPCHK(opd_launch_resize_u8(d_in, m->d_u8, B, h, w, oh, ow, tab->bh, tab->kh, tab->ksh, tab->bv, tab->kv, tab->ksv, m->stream));
    return OPD_OK;
}

// A small host table that rarely changes from call to call (the frame sizes, the tile windows of a video): uploaded only when it does
static int upload_if_changed(opd_detr* m, const std::vector<int32_t>& now, std::vector<int32_t>* kept, int32_t* dev) {
    if (now == *kept) return OPD_OK;
    HIPCHK(hipStreamSynchronize(m->stream));   // (an earlier asynchronous copy may still be reading the old host vector)
    *kept = now;                               // member: must outlive the async copy
    HIPCHK(hipMemcpyAsync(dev, kept->data(), kept->size() * 4, hipMemcpyHostToDevice, m->stream));
    return OPD_OK;
}

// SRC_TILES: every frame once, whole, into m->src; its windows, from where it lies, -> the stem's input block (kernels_tile.hip)
static int enqueue_tiles(opd_detr* m, const FrameSource& src, int H, int W) {
    RCCHK(upload_camera_frames(m, nullptr, static_cast<const uint8_t* const*>(src.frames), src.n_frames, src.h, src.w));
    if (!m->d_tiles) RCCHK(dalloc(m, &m->d_tiles, (size_t)m->cfg.max_batch * 4, false));
    RCCHK(upload_if_changed(m, std::vector<int32_t>(src.tiles, src.tiles + (size_t)src.n_tiles * 4), &m->h_tiles, m->d_tiles));
    if (src.tile_HW) {   // tiles of several sizes: a descriptor per tile, with the tables of its own (th, tw, oh, ow); the canvas of a ragged batch
        std::vector<int32_t> desc((size_t)src.n_tiles * (sizeof(TileRaggedDesc) / 4));
        for (int t = 0; t < src.n_tiles; ++t) {
            const int32_t* g = src.tiles + 4 * t;
            const opd_detr::ResizeTab* tab = nullptr;
            RCCHK(resize_tab(m, g[2], g[3], src.tile_HW[2 * t], src.tile_HW[2 * t + 1], &tab));
            // (copied out at once: the next tile's lookup may grow the vector `tab` points into)
            const TileRaggedDesc d{g[0], g[1], g[2], g[3], tab->oh, tab->ow, tab->ksh, tab->ksv, tab->bh, tab->kh, tab->bv, tab->kv};
            memcpy(desc.data() + (size_t)t * (sizeof d / 4), &d, sizeof d);
        }
        if (!m->d_tile_desc) RCCHK(dalloc(m, &m->d_tile_desc, (size_t)m->cfg.max_batch * (sizeof(TileRaggedDesc) / 4), false));
        RCCHK(upload_if_changed(m, desc, &m->h_tile_desc, m->d_tile_desc));
        TileRaggedParams rp{m->src.dev, m->d_u8, reinterpret_cast<const TileRaggedDesc*>(m->d_tile_desc), src.n_frames, src.n_tiles, src.h, src.w, H, W};
        return launch(m, m->stream, CLS_OTHER, 0.0, [&] { return opd_launch_tile_resize_ragged_u8(rp, m->stream); });
    }
    const int th = src.box_h(), tw = src.box_w();
    const opd_detr::ResizeTab* tab = nullptr;
    RCCHK(resize_tab(m, th, tw, H, W, &tab));
    TileResizeParams rp{m->src.dev, m->d_u8, m->d_tiles, src.n_frames, src.n_tiles, src.h, src.w, th, tw, H, W, tab->bh, tab->kh, tab->bv, tab->kv, tab->ksh, tab->ksv};
    return launch(m, m->stream, CLS_OTHER, 0.0, [&] { return opd_launch_tile_resize_u8(rp, m->stream); });
}

// The source step of every detect / forward entry point: the frames of `src` -> `*d_pixels`, device pixels at model resolution H x W.
// `*d_camera`: where the camera-resolution frames now lie on the device (d_src, or the caller's block, when they were resized; d_u8 when not).
static int stage_frames(opd_detr* m, const FrameSource& src, int B, int H, int W, const void** d_pixels, const uint8_t** d_camera) {
    if (src.kind == SRC_PIXELS) return stage_pixels(m, src.frames, src.pixel_format, src.mem_kind, B, H, W, d_pixels);
    *d_pixels = *d_camera = m->d_u8;
    if (src.kind == SRC_TILES) {
        RCCHK(enqueue_tiles(m, src, H, W));
        *d_camera = m->src.dev;   // (whole frames; read AFTER the upload, which is what allocates or grows the staging buffer)
        return OPD_OK;
    }
    const uint8_t* block = src.kind == SRC_BLOCK ? static_cast<const uint8_t*>(src.frames) : nullptr;
    const uint8_t* const* list = src.kind == SRC_LIST ? static_cast<const uint8_t* const*>(src.frames) : nullptr;
    if (list && src.h == H && src.w == W) {
        const size_t n1 = (size_t)H * W * 3;
        for (int b = 0; b < B; ++b) HIPCHK(hipMemcpyAsync(m->d_u8 + b * n1, list[b], n1, hipMemcpyHostToDevice, m->stream));
        return OPD_OK;
    }
    RCCHK(enqueue_resize(m, block, src.mem_kind, B, src.h, src.w, H, W, list));
    *d_camera = pixels_on_device(src.mem_kind) ? block : m->src.dev;
    return OPD_OK;
}

// ---- buffers of the optional stages: allocated by the first call of the stage that uses them (a page-locked twin of the same size with some) ----
template <typename T>
static int ensure(opd_detr* m, T** dev, size_t count, void** pinned = nullptr) {
    if (*dev) return OPD_OK;
    RCCHK(dalloc(m, dev, count, false));
    if (pinned) HIPCHK(hipHostMalloc(pinned, count * sizeof(T), hipHostMallocDefault));
    return OPD_OK;
}
static size_t slots_of(const opd_detr* m) { return (size_t)m->cfg.max_batch * m->arch.queries; }   // record slots of a full batch
static int ensure_nms_flag(opd_detr* m) {
    if (m->d_nms_flag) return OPD_OK;
    RCCHK(ensure(m, &m->d_nms_flag, 1));
    HIPCHK(hipMemsetAsync(m->d_nms_flag, 0, 4, m->stream));
    return OPD_OK;
}
// The merged records of a tiled call lie as [counts of max_batch frames | records]
static size_t tile_out_off(const opd_detr* m) { return align_up((size_t)m->cfg.max_batch * 4, 64); }   // where the records begin
static int ensure_tile_out(opd_detr* m) { return ensure(m, &m->d_tile_out, tile_out_off(m) + slots_of(m) * sizeof(opd_tile_det), &m->tile_pinned); }
// ... and are what the feature, floor and track stages of a tiled call read, where tile_merge_kernel left them: [n_frames][S], S = n_tiles x queries, rows by position
static const int32_t* merged_counts(const opd_detr* m) { return reinterpret_cast<const int32_t*>(m->d_tile_out); }
static const opd_tile_det* merged_records(const opd_detr* m) { return reinterpret_cast<const opd_tile_det*>(m->d_tile_out + tile_out_off(m)); }
// The records leave the device as ONE block, the d_records allocation as it lies: [records of max_batch frames | counts | feature rows]
static size_t rec_bytes(const opd_detr* m) { return slots_of(m) * sizeof(opd_det); }   // = offset of the counts
static size_t feat_off(const opd_detr* m) { return reinterpret_cast<const char*>(m->d_feat_all) - reinterpret_cast<const char*>(m->d_records); }
static size_t feat_row(const opd_detr* m) { return (size_t)m->arch.queries * m->arch.d_model * 4; }   // a frame's feature rows
static int ensure_sync_pinned(opd_detr* m) {
    if (!m->sync_pinned) HIPCHK(hipHostMalloc(&m->sync_pinned, feat_off(m) + m->cfg.max_batch * feat_row(m), hipHostMallocDefault));
    return OPD_OK;
}

// ---- the stages of the sink, in the order deliver_records runs them ----------------------------------------------------------------------
// Person filter + greedy IoU-NMS in place on device records (kernels_nms.hip), through the launch helper like the post-process before it
static int enqueue_nms(opd_detr* m, opd_det* dets, int32_t* counts, int n_frames, int stride, int label, float threshold) {
    RCCHK(ensure_nms_flag(m));
    NmsParams np{dets, counts, m->d_nms_flag, n_frames, stride, label, threshold};
    return launch(m, m->stream, CLS_OTHER, 0.0, [&] { return opd_launch_person_nms(np, m->stream); });
}

// `orig_hw` (nullable): the frame sizes the boxes are scaled to, else h x w for every frame.  `dev_out` / `dev_counts` (nullable): device buffers of the
// caller; the kernel then writes there directly instead of the library's own record buffers (no device-to-device copies afterwards).
// `nms_label`, `nms_threshold`: the suppression behind it (off while the threshold is negative)
static int enqueue_postprocess(opd_detr* m, float threshold, const int32_t* orig_hw, int h, int w, opd_det* dev_out, int32_t* dev_counts, int nms_label,
                               float nms_threshold) {
    const int B = m->last_B;
    std::vector<int32_t> hw((size_t)B * 2);
    for (int b = 0; b < B; ++b) {
        hw[2 * b] = orig_hw ? orig_hw[2 * b] : h;
        hw[2 * b + 1] = orig_hw ? orig_hw[2 * b + 1] : w;
    }
    RCCHK(upload_if_changed(m, hw, &m->h_orig_hw, m->d_orig_hw));
    PostParams pp{};
    pp.logits = m->d_logits; pp.boxes = m->d_boxes; pp.orig_hw = m->d_orig_hw;
    pp.records = dev_out ? dev_out : m->d_records;
    pp.counts = dev_counts ? dev_counts : m->d_counts;
    pp.B = B; pp.Q = m->arch.queries; pp.ncls = m->arch.ncls; pp.threshold = threshold;
    RCCHK(launch(m, m->stream, CLS_OTHER, 0.0, [&] { return opd_launch_postprocess(pp, m->stream); }));
    if (nms_threshold >= 0.f)   // the stages behind, and the caller, see final records in score order (in front of mark 8: the kernel's time is part of stage_ms[7])
        RCCHK(enqueue_nms(m, static_cast<opd_det*>(pp.records), pp.counts, B, pp.Q, nms_label, nms_threshold));
    MARK(8);
    return OPD_OK;
}

// What the seam merge takes from the caller's parameter block and sizes (the tile stage here, merge_tiles on host records)
static void fill_tile_merge(TileMergeParams* mp, const opd_tile_params* p, int n_frames, int n_tiles, int stride, int h, int w) {
    mp->n_frames = n_frames; mp->n_tiles = n_tiles; mp->stride = stride; mp->frame_h = h; mp->frame_w = w;
    mp->merge_nms_threshold = p->merge_nms_threshold; mp->merge_threshold = p->merge_threshold; mp->edge_tolerance = p->edge_tolerance;
}
// The tile stage: the records of every frame's tiles (tile pixels, suppressed per tile) -> frame pixels, merged across the seams (kernels_tile.hip)
static int enqueue_tile_merge(opd_detr* m, const TileStage& t) {
    RCCHK(ensure_tile_out(m));
    RCCHK(ensure_nms_flag(m));
    TileMergeParams mp{};
    mp.recs = m->d_records; mp.tile_counts = m->d_counts; mp.tiles_yxhw = m->d_tiles;
    mp.counts = reinterpret_cast<int32_t*>(m->d_tile_out); mp.out = reinterpret_cast<opd_tile_det*>(m->d_tile_out + tile_out_off(m)); mp.flag = m->d_nms_flag;
    fill_tile_merge(&mp, t.params, t.n_frames, t.n_tiles, m->arch.queries, t.frame_h, t.frame_w);
    return launch(m, m->stream, CLS_OTHER, 0.0, [&] { return opd_launch_tile_merge(mp, m->stream); });
}

// The records of a call behind the tile merge, said once for the stages below.  `view` (opd_records.h): where they lie on the device, d_records / d_counts
// [B][Q], or (a tiled call) the merged records [n_frames][n_tiles x Q].  `any_label`: the colour and floor stages take every record of a tiled call, not
// only those labelled s.label.  The rest describes the copy the call delivers to the host, for finish_trackers: record i of frame f has its confidence
// at score[(f * view.stride + i) * score_stride] (floats), frame f has counts[f] records; `entry`: the entry point's name, for errors.
struct CallRecords {
    RecordView view;
    int any_label;
    const float* score;
    int score_stride;
    const int32_t* counts;
    const char* entry;
};
static CallRecords call_records(const opd_detr* m, const RecordSink& s, bool tiled) {
    if (tiled)
        return {RecordView{nullptr, merged_records(m), merged_counts(m), s.tile.n_frames, s.tile.n_tiles * m->arch.queries}, 1,
                s.tile.out ? &s.tile.out->score : nullptr, (int)(sizeof(opd_tile_det) / sizeof(float)), s.tile.counts, s.tile.entry};
    return {RecordView{m->d_records, nullptr, m->d_counts, m->last_B, m->arch.queries}, 0,
            s.out ? &s.out->score : nullptr, (int)(sizeof(opd_det) / sizeof(float)), s.counts, "opd_detr_detect_frames_track"};
}

// The feature stage, on the records of the call.  (h, w): the camera resolution of the frames at d_camera (FEAT_COLOR, FEAT_REID; a tiled call: the WHOLE frames).
// Returns in *rows what a tracker behind it may read: nothing, a row per key in d_feat_all, or a row per slot of the Re-ID call.  `reid` is
// the caller's: the call holds the Re-ID handle's lock and must outlive the wait.
static int enqueue_features(opd_detr* m, const RecordSink& s, const CallRecords& c, int h, int w, const uint8_t* d_camera, std::optional<ReidFusedCall>* reid,
                            TrackFeatureSource* rows) {
    const FeatureStage& f = s.feature;
    *rows = TrackFeatureSource{};
    if (f.kind == FEAT_NONE) return OPD_OK;
    if (f.kind == FEAT_REID) {   // select, plan and the Re-ID forward behind the records; the rows come back behind the records, before the one wait
        reid->emplace(f.reid);
        RCCHK((*reid)->enqueue(m->stream, c.view, d_camera, h, w, s.label, f.slots));
        // (the rows come back only where the caller takes them: a tracker reads them where the forward left them, and the slot list alone comes back)
        // (this rests on the entries: opd_detr_detect_frames_reid refuses a null `features`, detect_track never sets it, the tiled entry passes the caller's)
        (*reid)->with_rows = f.features != nullptr;
        *rows = {TRACK_ROWS_BY_SLOT, reid_feature_dim(f.reid), (*reid)->dev_rows(), (*reid)->dev_slot_map(), (*reid)->dev_n_person(), f.slots};
        return OPD_OK;
    }
    if (f.kind == FEAT_ROI)   // (no tiled entry asks for it: the pooled map is a tile's)
        HIPCHK(opd_launch_roi_features_records(m->d_x32, m->d_records, m->d_counts, m->d_orig_hw, s.label, m->d_feat_all, m->last_B, m->arch.queries, m->last_fh, m->last_fw, m->stream));
    if (f.kind == FEAT_COLOR) {   // the histogram kernels read the CAMERA-resolution frames under the boxes of the records
        RCCHK(ensure(m, &m->d_color_acc, slots_of(m) * OPD_COLOR_ACC_WORDS));
        ColorParams cp{};
        cp.view = c.view; cp.frames = d_camera; cp.acc = m->d_color_acc; cp.out = m->d_feat_all;
        cp.fh = h; cp.fw = w; cp.label = s.label; cp.any_label = c.any_label; cp.n = c.view.n_frames * c.view.stride;
        HIPCHK(opd_launch_color_features(cp, std::min(64, (h + 15) / 16), m->stream));
    }
    rows->rows_kind = TRACK_ROWS_BY_KEY; rows->D = m->arch.d_model; rows->rows = m->d_feat_all;
    return OPD_OK;
}

// The floor stage: the floor record of every record the stage takes, from the box the Python shim derives, while the records are on the device
static int enqueue_floor(opd_detr* m, const RecordSink& s, const CallRecords& c) {
    RCCHK(ensure(m, &m->d_floor, slots_of(m), (void**)&m->h_floor));
    FloorParams fp{};
    fp.m = s.floor.fmap->model; fp.mode = FLOOR_IN_RECORDS; fp.n = c.view.n_frames * c.view.stride;
    fp.view = c.view; fp.label = s.label; fp.any_label = c.any_label; fp.out = m->d_floor;
    HIPCHK(opd_launch_floor(fp, m->stream));
    return OPD_OK;
}

// The tracker half of a fused detect-and-track call (opd_track.h), around the one wait of fetch_records.  Before it: every tracker's ingest and
// predict / cost launches on m->stream, behind the feature stage.  After it: association and commit per tracker; a tracker out of slots does not
// keep the others from being committed, and its error is the call's.
static int enqueue_trackers(opd_detr* m, const RecordSink& s, const CallRecords& c, const TrackFeatureSource& src) {
    const TrackStage& t = s.track;
    if (t.cams) return track_streams_enqueue(t.cams, t.n_cams, t.camera_of, m->stream, c.view.records, c.view.counts, c.view.stride, c.view.n_frames, src, "opd_detr_detect_streams_track");
    if (t.seq) return track_sequence_enqueue(t.seq, m->stream, c.view.records, c.view.counts, c.view.stride, c.view.n_frames, src, "opd_detr_detect_sequence_track");
    for (int f = 0; f < c.view.n_frames; ++f) RCCHK(track_fused_enqueue(t.trackers[f], m->stream, record_frame(c.view, f), f, src));
    return OPD_OK;
}
static int finish_trackers(opd_detr* m, const RecordSink& s, const CallRecords& c, bool with_features) {
    const TrackStage& t = s.track;
    const int frames = c.view.n_frames, stride = c.view.stride;
    if (t.cams) return track_streams_finish(t.cams, t.n_cams, t.camera_of, c.counts, stride, frames, t.track_ids, t.frames_done, "opd_detr_detect_streams_track");
    if (t.seq) return track_sequence_finish(t.seq, c.counts, stride, frames, t.track_ids, t.frames_done, "opd_detr_detect_sequence_track");
    int rc = OPD_OK;
    std::string first;
    for (int b = 0; b < frames; ++b) {
        const int n = std::max(0, std::min(c.counts[b], stride));
        const int one = track_fused_finish(t.trackers[b], c.score + (size_t)b * stride * c.score_stride, c.score_stride, n, with_features, t.track_ids + (size_t)b * stride, c.entry);
        if (one != OPD_OK && rc == OPD_OK) { rc = one; first = g_err; }
    }
    return rc == OPD_OK ? OPD_OK : fail(rc, first);
}

// The hybrid-tracker half of a fused detect call (opd_lwt.h), around the one wait of fetch_records like the track stage.  Before it, per tracker on
// m->stream: ingest of the frame's kept records through the call's view (a tiled call: the merged records), gray + pyramid of its camera-resolution
// frame of h x w where the source step left it (a tiled call: the WHOLE frame), the update with the count read on the device.  After it: adoption
// per tracker with the counts the call delivers; a tracker whose new tracks did not fit keeps its state and reference frame, gets -1 for every id
// and does not keep the others from being committed; its error is the call's.
static int enqueue_hybrid(opd_detr* m, const RecordSink& s, const CallRecords& c, int h, int w, const uint8_t* d_camera) {
    if (s.hybrid.seq) return lwt_sequence_enqueue(s.hybrid.seq, m->stream, *s.hybrid.call, &c.view, d_camera, s.hybrid.entry);
    for (int f = 0; f < c.view.n_frames; ++f)
        RCCHK(lwt_fused_enqueue(s.hybrid.trackers[f], m->stream, record_frame(c.view, f), d_camera + (size_t)f * h * w * 3, h, w, s.hybrid.entry));
    return OPD_OK;
}
static int finish_hybrid(const RecordSink& s, const CallRecords& c) {
    const int frames = c.view.n_frames, stride = c.view.stride;
    const HybridStage& y = s.hybrid;
    if (y.seq) return lwt_sequence_finish(y.seq, *y.call, c.counts, y.track_ids, y.recs_out, y.capacity, y.rec_counts, y.frames_done, y.entry);
    int rc = OPD_OK;
    std::string first;
    for (int b = 0; b < frames; ++b) {
        const int one = lwt_fused_finish(y.trackers[b], std::max(0, std::min(c.counts[b], stride)), y.track_ids + (size_t)b * stride, y.entry);
        if (one != OPD_OK && rc == OPD_OK) { rc = one; first = g_err; }
    }
    return rc == OPD_OK ? OPD_OK : fail(rc, first);
}

// A page-locked copy of the record block is taken apart into the caller's arrays here (deliver_records, opd_detr_wait)
static void unpack_records(const opd_detr* m, const void* pinned, int B, opd_det* out, int32_t* counts, float* features = nullptr) {
    const char* p = static_cast<const char*>(pinned);
    memcpy(out, p, (size_t)B * m->arch.queries * sizeof(opd_det));
    memcpy(counts, p + rec_bytes(m), (size_t)B * 4);
    if (features) memcpy(features, p + feat_off(m), (size_t)B * feat_row(m));
}
// The per-query feature rows that travel with the records (the Re-ID call brings its rows back itself, by slot)
static float* query_rows_out(const RecordSink& s) { return s.feature.kind == FEAT_REID ? nullptr : s.feature.features; }

// The one fetch of a blocking call: what the sink's parts ask for comes back into page-locked memory (a copy into the caller's pageable arrays is staged by
// the runtime anyway, once per call), then the call's ONE wait.  A tiled call: [counts | merged records], and of its stages the rows by position (unless
// a tracker alone reads them), the floor rows, the Re-ID call's slot list (with its rows when the caller takes them), and what the hybrid stage brings
// back (below).  Host outputs: [records of max_batch frames |
// counts (| per-query feature rows)] in one copy, the floor rows, the Re-ID call's slot list (and rows, unless a tracker reads them in place).  Device
// outputs were written in place by the post-process kernel.
static int fetch_records(opd_detr* m, const RecordSink& s, const CallRecords& c, ReidFusedCall* reid) {
    const int B = m->last_B, frames = c.view.n_frames, stride = c.view.stride;   // (B x Q = frames x stride record slots either way)
    const bool tiled = s.tile.params != nullptr;
    if (tiled || !outputs_on_device(s.mem_kind)) {
        if (tiled) {
            HIPCHK(hipMemcpyAsync(m->tile_pinned, m->d_tile_out, tile_out_off(m) + (size_t)frames * stride * sizeof(opd_tile_det), hipMemcpyDeviceToHost, m->stream));
            if (query_rows_out(s)) {   // the rows by position, where the per-query rows of a frame-list call travel
                RCCHK(ensure_sync_pinned(m));
                HIPCHK(hipMemcpyAsync(static_cast<char*>(m->sync_pinned) + feat_off(m), m->d_feat_all, B * feat_row(m), hipMemcpyDeviceToHost, m->stream));
            }
        } else {
            RCCHK(ensure_sync_pinned(m));
            HIPCHK(hipMemcpyAsync(m->sync_pinned, m->d_records, query_rows_out(s) ? feat_off(m) + B * feat_row(m) : rec_bytes(m) + (size_t)B * 4, hipMemcpyDeviceToHost, m->stream));
        }
        if (s.floor.fmap) HIPCHK(hipMemcpyAsync(m->h_floor, m->d_floor, (size_t)frames * stride * sizeof(opd_floor_rec), hipMemcpyDeviceToHost, m->stream));
        if (reid) RCCHK(reid->copy_back(m->stream));   // the slot list (and the rows by slot, when the caller takes them)
        if (s.hybrid.seq) RCCHK(lwt_sequence_fetch(s.hybrid.seq, m->stream, s.hybrid.call->F));   // a slot per frame: [head | ids] or [head | records]
        else if (s.hybrid.on())   // every tracker's [head | ids], an id per record slot of its frame
            for (int f = 0; f < frames; ++f) RCCHK(lwt_fused_fetch(s.hybrid.trackers[f], m->stream, stride));
    }
    HIPCHK(hipStreamSynchronize(m->stream));
    if (m->profiling) {
        for (int i = 0; i < 8; ++i) {
            float ms = 0.f;
            // (mode 2: marks 0 .. 7 are nodes of the replayed graph, mark 8 is recorded eagerly behind the post-process launch: events of the
            //  two kinds do not subtract meaningfully, so the last stage runs from the eager mark 9 behind the graph launch)
            hipEvent_t from = (i == 7 && m->profiling == 2 && m->graph_marks) ? m->ev[9] : m->ev[i];
            if (hipEventElapsedTime(&ms, from, m->ev[i + 1]) == hipSuccess) m->stage_ms[i] = ms;
            else (void)hipGetLastError();   // (a mark that was never recorded: not this call's error)
        }
        if (m->profiling == 1) timed_collect(m);
    }
    return OPD_OK;
}

// WAIT_TICKET: the records go to async slot s.ticket behind an event of its own; opd_detr_wait delivers them
static int hand_to_ticket(opd_detr* m, const RecordSink& s) {
    opd_detr::AsyncHost& slot = m->async_host[s.ticket];
    slot.out = nullptr;
    if (!outputs_on_device(s.mem_kind)) {   // host outputs: pinned staging so that the copy stays asynchronous
        if (!slot.pinned) HIPCHK(hipHostMalloc(&slot.pinned, rec_bytes(m) + (size_t)m->cfg.max_batch * 4, hipHostMallocDefault));
        HIPCHK(hipMemcpyAsync(slot.pinned, m->d_records, rec_bytes(m) + (size_t)m->last_B * 4, hipMemcpyDeviceToHost, m->stream));   // (records | counts: one copy)
        slot.out = s.out; slot.counts = s.counts; slot.B = m->last_B;
    }
    HIPCHK(hipEventRecord(m->ev_async[s.ticket], m->stream));
    m->async_pending[s.ticket] = true;
    ++m->async_next;
    return OPD_OK;
}

// The back half, on the outputs of the last forward (opd_detr_postprocess enters here): the stages of the sink in their one order, each skipped when its
// part is absent.  (h, w): the size the boxes are scaled to (0: the model resolution); d_camera: the source's frames on the device at camera resolution.
// The feature, floor, track and hybrid stages read the records of the call through ONE view (call_records): in a tiled call the MERGED records, not d_records.
// The feature, floor, track and tile parts deliver to the host after the call's own wait: setting one with WAIT_TICKET or WAIT_NONE, or with device
// outputs, is a programming error (no entry point does).
static int deliver_records(opd_detr* m, const RecordSink& s, int h, int w, const uint8_t* d_camera) {
    const int B = m->last_B;
    const bool dev = outputs_on_device(s.mem_kind), tiled = s.tile.params != nullptr, tracked = s.track.on();
    RCCHK(enqueue_postprocess(m, s.threshold, s.orig_hw, h ? h : m->last_H, h ? w : m->last_W, dev ? s.out : nullptr, dev ? s.counts : nullptr,
                              tiled ? s.tile.params->person_label : m->nms_label, tiled ? s.tile.params->tile_nms_threshold : m->nms_threshold));
    if (tiled) RCCHK(enqueue_tile_merge(m, s.tile));
    std::optional<ReidFusedCall> reid;   // (lives until the rows are delivered)
    TrackFeatureSource rows;
    const CallRecords recs = call_records(m, s, tiled);
    RCCHK(enqueue_features(m, s, recs, tiled ? s.tile.frame_h : h, tiled ? s.tile.frame_w : w, d_camera, &reid, &rows));
    if (s.floor.fmap) RCCHK(enqueue_floor(m, s, recs));
    if (tracked) RCCHK(enqueue_trackers(m, s, recs, rows));
    if (s.hybrid.on()) RCCHK(enqueue_hybrid(m, s, recs, tiled ? s.tile.frame_h : h, tiled ? s.tile.frame_w : w, d_camera));
    if (s.wait == WAIT_NONE) return OPD_OK;
    if (s.wait == WAIT_TICKET) return hand_to_ticket(m, s);
    RCCHK(fetch_records(m, s, recs, reid ? &*reid : nullptr));
    // behind the wait: into the caller's arrays, the stages' rows over the frames and the record slots per frame of the call's view
    const int frames = recs.view.n_frames, stride = recs.view.stride;
    if (tiled) {
        memcpy(s.tile.counts, m->tile_pinned, (size_t)frames * 4);
        memcpy(s.tile.out, static_cast<const char*>(m->tile_pinned) + tile_out_off(m), (size_t)frames * stride * sizeof(opd_tile_det));
        if (query_rows_out(s)) memcpy(query_rows_out(s), static_cast<const char*>(m->sync_pinned) + feat_off(m), B * feat_row(m));
    } else if (!dev) unpack_records(m, m->sync_pinned, B, s.out, s.counts, query_rows_out(s));
    // the Re-ID rows by slot and the slot list (a tiled call: slot_map[k] = f * S + position), where the caller takes the list: a frame-list call that
    // hands the rows to a tracker leaves it null
    if (reid && s.feature.slot_map) reid->deliver(s.feature.features, s.feature.slot_map, s.feature.n_person);
    for (int f = 0; f < frames && s.floor.fmap; ++f) {
        const int n = std::max(0, std::min(recs.counts[f], stride));
        const size_t at = (size_t)f * stride;
        if (tiled) {   // by position: row f * S + k of merged record k of frame f
            memcpy(s.floor.out + at, m->h_floor + at, (size_t)n * sizeof(opd_floor_rec));
            continue;
        }
        for (int i = 0; i < n; ++i) {   // by query, and only rows of records of the class are handed on
            const opd_det& r = s.out[at + i];
            if (r.label == s.label && (unsigned)r.query_index < (unsigned)stride) s.floor.out[at + r.query_index] = m->h_floor[at + r.query_index];
        }
    }
    if (s.hybrid.on()) return finish_hybrid(s, recs);   // (adoption by the counts the call delivers; no entry sets both tracker stages)
    if (!tracked) return OPD_OK;
    const bool featured = rows.rows_kind != TRACK_ROWS_NONE;
    if (reid) reid->slots_per_frame(frames, stride, s.track.n_featured);   // a frame's featured records are those that got a slot
    else for (int f = 0; f < frames; ++f) s.track.n_featured[f] = featured ? std::max(0, std::min(recs.counts[f], stride)) : 0;
    return finish_trackers(m, s, recs, featured);
}

// The front half: the source step and the forward.  The launch timer starts anew here, once per call: the source's launches, the forward's and the
// sink's behind it make up the call's kernel table (profiling mode 1; with profiling off no launch leaves a mark and this empties an empty list).
static int forward_frames(opd_detr* m, const FrameSource& src, int B, int H, int W, const int32_t* valid_hw, const uint8_t** d_camera) {
    const void* d_pixels = nullptr;
    m->timer.reset();
    RCCHK(stage_frames(m, src, B, H, W, &d_pixels, d_camera));
    return run_forward(m, d_pixels, src.pixel_format, B, H, W, valid_hw);
}

int detect_pipeline(opd_detr* m, const FrameSource& src, int B, int H, int W, const int32_t* valid_hw, const RecordSink& sink) {
    const uint8_t* d_camera = nullptr;
    RCCHK(forward_frames(m, src, B, H, W, valid_hw, &d_camera));
    return deliver_records(m, sink, src.box_h(), src.box_w(), d_camera);
}

// The front half alone (opd_detr_forward*): the raw outputs go to host or device memory according to src.mem_kind
static int forward_device(opd_detr* m, const FrameSource& src, int B, int H, int W, const int32_t* valid_hw, float* logits, float* boxes,
                          float* enc_features) {
    const uint8_t* d_camera = nullptr;
    RCCHK(forward_frames(m, src, B, H, W, valid_hw, &d_camera));
    const hipMemcpyKind kind = outputs_on_device(src.mem_kind) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    const size_t Md = (size_t)B * m->arch.queries;
    if (logits) HIPCHK(hipMemcpyAsync(logits, m->d_logits, Md * m->arch.ncls * 4, kind, m->stream));
    if (boxes) HIPCHK(hipMemcpyAsync(boxes, m->d_boxes, Md * 4 * 4, kind, m->stream));
    if (enc_features)
        HIPCHK(hipMemcpyAsync(enc_features, m->d_x32, (size_t)B * m->last_fh * m->last_fw * m->arch.d_model * 4, kind, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    if (m->profiling == 1) timed_collect(m);
    return OPD_OK;
}

// ---- tiled detection ----------------------------------------------------------------------------------------------------
// What the two tiled entries check alike, before any device call: the parameter block and the windows ([n_tiles][4] = y0, x0, th, tw) on an h x w frame
static int check_tiles(const std::string& who, const opd_tile_params* p, const int32_t* tiles, int n_tiles, int h, int w, bool one_size) {
    if (!p || !tiles) return fail(OPD_EINVAL, who + ": null argument");
    if (p->struct_size != (int32_t)sizeof(opd_tile_params)) return fail(OPD_EINVAL, who + ": opd_tile_params.struct_size mismatch");
    if (n_tiles < 1) return fail(OPD_EINVAL, who + ": n_tiles < 1");
    if (!frame_size_ok(h, w)) return fail(OPD_EINVAL, who + ": frame size " + std::to_string(h) + " x " + std::to_string(w) + " out of range");
    for (int t = 0; t < n_tiles; ++t) {
        const int32_t* g = tiles + 4 * t;
        if (g[0] < 0 || g[1] < 0 || g[2] < 1 || g[3] < 1 || (long long)g[0] + g[2] > h || (long long)g[1] + g[3] > w)
            return fail(OPD_EINVAL, who + ": tile " + std::to_string(t) + " (y0 " + std::to_string(g[0]) + ", x0 " + std::to_string(g[1]) + ", " + std::to_string(g[2]) + " x " +
                                        std::to_string(g[3]) + ") lies outside the " + std::to_string(h) + " x " + std::to_string(w) + " frame");
        if (one_size && (g[2] != tiles[2] || g[3] != tiles[3]))
            return fail(OPD_EINVAL, who + ": tiles of more than one size (" + std::to_string(tiles[2]) + " x " + std::to_string(tiles[3]) + " and " + std::to_string(g[2]) + " x " +
                                        std::to_string(g[3]) + "): one forward has one model size");
    }
    return OPD_OK;
}

// The merge kernel on host records of the caller: temporaries of the call, blocking
static int merge_tiles(opd_detr* m, const opd_det* recs, const int32_t* tile_counts, int n_frames, int n_tiles, int stride, const int32_t* tiles, int h, int w,
                       const opd_tile_params* p, opd_tile_det* out, int32_t* counts) {
    const size_t nt = (size_t)n_frames * n_tiles, nr = nt * stride;
    DevMem tmp;
    TileMergeParams mp{};
    mp.recs = tmp.up(recs, nr); mp.tile_counts = tmp.up(tile_counts, nt); mp.tiles_yxhw = tmp.up(tiles, (size_t)n_tiles * 4);
    mp.out = tmp.alloc<opd_tile_det>(nr); mp.counts = tmp.alloc<int32_t>((size_t)n_frames);
    const int32_t zero = 0;
    mp.flag = tmp.up(&zero, 1);
    if (!tmp.ok) return fail(OPD_ENOMEM, "opd_detr_merge_tiles: device allocation failed");
    fill_tile_merge(&mp, p, n_frames, n_tiles, stride, h, w);
    if (m->profiling == 1) m->timer.reset();
    RCCHK(launch(m, m->stream, CLS_OTHER, 0.0, [&] { return opd_launch_tile_merge(mp, m->stream); }));
    HIPCHK(hipStreamSynchronize(m->stream));
    int32_t over = 0;
    HIPCHK(hipMemcpy(counts, mp.counts, (size_t)n_frames * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out, mp.out, nr * sizeof(opd_tile_det), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&over, mp.flag, 4, hipMemcpyDeviceToHost));
    if (m->profiling == 1) timed_collect(m);
    if (over) return fail(OPD_EINVAL, "opd_detr_merge_tiles: a tile holds more records than its slots (its frame comes back empty)");
    return OPD_OK;
}

}  // namespace opd

// =====================================================================================================================
// C-ABI
// =====================================================================================================================
static void drop_streams(opd_detr* m) {
    if (m->ev_fork) (void)hipEventDestroy(m->ev_fork);
    if (m->ev_join) (void)hipEventDestroy(m->ev_join);
    if (m->stream2) (void)hipStreamDestroy(m->stream2);
    if (m->stream) (void)hipStreamDestroy(m->stream);
    m->ev_fork = m->ev_join = nullptr; m->stream2 = m->stream = nullptr;
}

// The forward-plan switches: defaults, overridden by environment variables (A/B switches for benchmarking and ablations)
Switches opd::read_switches(int flags) {
    Switches sw;
    auto env = [](const char* name, int* v) { if (const char* e = getenv(name)) *v = atoi(e); };
    env("OPD_DUAL_OVER_TAIL", &sw.dual_over_tail);
    env("OPD_SC2_TAIL", &sw.sc2_tail);
    env("OPD_TAIL_REV", &sw.tail_rev);
    env("OPD_TAIL3", &sw.tail3);
    env("OPD_TAIL_RC", &sw.tail_rc);
    sw.tail_rc = sw.tail_rc != 0;
    env("OPD_WPREFETCH", &sw.wprefetch);
    env("OPD_W8", &sw.w8);
    if (sw.w8 < 0) sw.w8 = (flags & OPD_FLAG_MULTI_STREAM) ? 1 : 0;
    env("OPD_SMALL_SPLITK", &sw.small_splitk);
    env("OPD_SMALL_ENC", &sw.small_enc);
    env("OPD_Y_STRIDE2", &sw.y_stride2);
    env("OPD_RES_DMA128", &sw.res_dma128);
    env("OPD_STEM_REDUCE", &sw.stem_reduce);
    env("OPD_TAIL3_SPLIT", &sw.tail3_split);
    env("OPD_FUSE_PREP", &sw.fuse_prep);
    env("OPD_POS_SHADOW", &sw.pos_shadow);
    env("OPD_DEEP_FC2", &sw.deep_fc2);
    env("OPD_WROUND", &sw.wround);
    env("OPD_FUSED_DEC", &sw.fused_dec);
    env("OPD_FUSED_ENC_FFN", &sw.fused_enc_ffn);
    env("OPD_ENC_TAIL", &sw.enc_tail);
    env("OPD_ENC_FRONT", &sw.enc_front);
    env("OPD_HEADS2", &sw.heads2);
    env("OPD_DBG_DEC_LAYERS", &sw.dbg_dec_layers);   // timing ablation (tools/dec_cost.sh): results are wrong
    env("OPD_DBG_BTAIL", &sw.dbg_btail);             // timing ablations of the whole forward: BtailParams::dbg / ConvGemmParams::dbg
    env("OPD_DBG_SKIP", &sw.dbg_skip);               // bit i: no kernel launches in segment i of stage_ms (stem, stages 1-4, encoder, decoder, post-process)
    env("OPD_DBG_GEMM", &sw.dbg_gemm);               // of every fused tail / implicit-GEMM launch (results are wrong)
    return sw;
}

// What creation and cloning share: the handle's streams, workspace and events (creation: its weights from `sd` too; a clone shares its source's)
static int open_handle(std::unique_ptr<opd_detr> m, const StateDict* sd, opd_detr** out) {
    auto cleanup = [&](int code) {
        for (void* p : m->allocs) (void)hipFree(p);
        drop_streams(m.get());
        return code;
    };
    hipError_t he = hipSetDevice(m->device);
    if (he == hipSuccess) he = hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking);
    // second branch of the forward (stage-3 frame split): a stream and two untimed events per handle
    if (he == hipSuccess) he = hipStreamCreateWithFlags(&m->stream2, hipStreamNonBlocking);
    if (he == hipSuccess) he = hipEventCreateWithFlags(&m->ev_fork, hipEventDisableTiming);
    if (he == hipSuccess) he = hipEventCreateWithFlags(&m->ev_join, hipEventDisableTiming);
    if (he != hipSuccess) { drop_streams(m.get()); return fail(OPD_EHIP, std::string("device/stream setup failed: ") + hipGetErrorString(he)); }
    int rc;
    if (sd) {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, m->device) == hipSuccess && cus > 0) m->num_cus = cus;
        m->weights = std::make_shared<WeightSet>();
        m->weights->device = m->device;
        if ((rc = build_weights(m.get(), *sd))) return cleanup(rc);
    }
    m->weights_sealed = true;
    if ((rc = build_workspace(m.get()))) return cleanup(rc);
    for (auto& e : m->ev)
        if (hipEventCreate(&e) != hipSuccess) return cleanup(fail(OPD_EHIP, "hipEventCreate failed"));
    *out = m.release();
    ++g_handle_epoch;
    return OPD_OK;
}

static int create_impl(const opd_config* cfg, const char* weights_path, int device_ordinal, opd_detr** out) {
    if (!cfg || !weights_path || !out) return fail(OPD_EINVAL, "opd_detr_create: null argument");
    if (cfg->struct_size != (int32_t)sizeof(opd_config)) return fail(OPD_EINVAL, "opd_config.struct_size mismatch");
    if (cfg->max_batch < 1 || cfg->max_height < 32 || cfg->max_width < 32) return fail(OPD_EINVAL, "opd_config maxima must be >= 1 x 32 x 32");
    StateDict sd;
    std::string err;
    int rc = load_safetensors(weights_path, &sd, &err);
    if (rc) return fail(rc, err);
    std::unique_ptr<opd_detr> m(new opd_detr());
    rc = infer_arch(sd, &m->arch, &err);
    if (rc) return fail(rc, err);
    m->cfg = *cfg;
    m->dtype = (cfg->flags & OPD_FLAG_BF16) ? OPD_DT_BF16 : OPD_DT_F16;
    m->sw = read_switches(cfg->flags);
    m->device = device_ordinal;
    RCCHK(use_device("opd_detr_create", device_ordinal, "device_ordinal out of range"));
    return open_handle(std::move(m), &sd, out);
}

static int clone_impl(const opd_detr* src, opd_detr** out) {
    if (!src || !out) return fail(OPD_EINVAL, "opd_detr_clone: null argument");
    std::unique_ptr<opd_detr> m(new opd_detr());
    static_cast<DetrWeights&>(*m) = *src;   // everything build_weights produced, whole
    m->weights = src->weights;
    m->arch = src->arch; m->cfg = src->cfg; m->device = src->device; m->dtype = src->dtype;
    m->sw = src->sw; m->num_cus = src->num_cus;
    return open_handle(std::move(m), nullptr, out);
}

extern "C" {

const char* opd_version(void) {
    const char* text = "";
    (void)api_call_unlocked("opd_version", [&] { text = "opd_hip 0.2 gfx950 (fp16 MFMA operands, fp32 accumulate; OPD_FLAG_BF16: bf16 operands)"; return OPD_OK; });
    return text;
}

int opd_detr_create(const opd_config* cfg, const char* weights_path, int device_ordinal, opd_detr** out) { return api_call("opd_detr_create", [&] {
    if (out) *out = nullptr;
    return create_impl(cfg, weights_path, device_ordinal, out);
}, API_CREATE); }
int opd_detr_clone(const opd_detr* src, opd_detr** out) { return api_call("opd_detr_clone", [&] {
    if (out) *out = nullptr;
    return clone_impl(src, out);
}); }
void opd_detr_destroy(opd_detr* m) { (void)api_call("opd_detr_destroy", [&]() -> int {
    if (!m) return OPD_OK;
    (void)hipSetDevice(m->device);
    if (m->stream) (void)hipStreamSynchronize(m->stream);
    comm_detach_all(m);   // communicator lanes bound to this handle refuse work from here on (their own destroy still frees them)
    for (void* p : m->allocs) (void)hipFree(p);
    m->src.release();
    for (auto& e : m->ev_async)
        if (e) (void)hipEventDestroy(e);
    for (auto& a : m->async_host)
        if (a.pinned) (void)hipHostFree(a.pinned);
    if (m->sync_pinned) { (void)hipHostFree(m->sync_pinned); m->sync_pinned = nullptr; }
    if (m->tile_pinned) { (void)hipHostFree(m->tile_pinned); m->tile_pinned = nullptr; }
    if (m->h_floor) { (void)hipHostFree(m->h_floor); m->h_floor = nullptr; }
    for (auto& e : m->ev)
        if (e) (void)hipEventDestroy(e);
    m->timer.release();
    drop_graphs(m);
    drop_streams(m);
    delete m;
    ++g_handle_epoch;
    return OPD_OK;
}); }

int opd_detr_info(const opd_detr* m, opd_model_info* info) { return api_call_unlocked("opd_detr_info", [&]() -> int {
    if (!m || !info) return fail(OPD_EINVAL, "opd_detr_info: null argument");
    for (int i = 0; i < 4; ++i) info->depths[i] = m->arch.depths[i];
    info->d_model = m->arch.d_model; info->heads = m->arch.heads; info->ffn_dim = m->arch.ffn;
    info->encoder_layers = m->arch.enc_layers; info->decoder_layers = m->arch.dec_layers;
    info->num_queries = m->arch.queries; info->num_classes_plus1 = m->arch.ncls;
    info->max_batch = m->cfg.max_batch; info->max_height = m->cfg.max_height; info->max_width = m->cfg.max_width;
    info->device_ordinal = m->device;
    info->weight_bytes_device = m->weight_bytes; info->workspace_bytes_device = m->workspace_bytes;
    return OPD_OK;
}); }

int opd_detr_forward(opd_detr* m, const void* pixels, int pixel_format, int mem_kind, int B, int H, int W, float* logits,
                     float* boxes, float* enc_features) { return api_call("opd_detr_forward", [&]() -> int {
    return opd_detr_forward_ragged(m, pixels, pixel_format, mem_kind, B, H, W, nullptr, logits, boxes, enc_features);
}); }
int opd_detr_forward_ragged(opd_detr* m, const void* pixels, int pixel_format, int mem_kind, int B, int H, int W,
                            const int32_t* valid_hw, float* logits, float* boxes, float* enc_features) { return api_call("opd_detr_forward_ragged", [&]() -> int {
    RCCHK(check_shape(m, pixels, pixel_format, mem_kind, B, H, W));
    HIPCHK(hipSetDevice(m->device));
    return forward_device(m, {SRC_PIXELS, pixels, pixel_format, mem_kind, 0, 0}, B, H, W, valid_hw, logits, boxes, enc_features);
}); }
int opd_detr_postprocess(opd_detr* m, float threshold, const int32_t* orig_hw, opd_det* out, int32_t* counts) { return api_call("opd_detr_postprocess", [&]() -> int {
    if (!m || !out || !counts) return fail(OPD_EINVAL, "opd_detr_postprocess: null argument");
    if (m->last_B == 0) return fail(OPD_ESTATE, "opd_detr_postprocess called before any forward");
    HIPCHK(hipSetDevice(m->device));
    return deliver_records(m, RecordSink(threshold, orig_hw, out, counts, OPD_MEM_HOST), 0, 0, nullptr);
}); }
int opd_detr_set_nms(opd_detr* m, int person_label, float nms_threshold) { return api_call_unlocked("opd_detr_set_nms", [&]() -> int {
    if (!m) return fail(OPD_EINVAL, "null model handle");
    if (nms_threshold != nms_threshold) return fail(OPD_EINVAL, "opd_detr_set_nms: the threshold is NaN");
    m->nms_label = person_label;
    m->nms_threshold = nms_threshold < 0.f ? -1.0f : nms_threshold;
    return OPD_OK;
}); }
int opd_detr_nms_records(opd_detr* m, opd_det* dets, int32_t* counts, int n_frames, int stride, int person_label, float nms_threshold) { return api_call("opd_detr_nms_records", [&]() -> int {
    if (!m) return fail(OPD_EINVAL, "null model handle");
    if (n_frames < 0 || stride < 1 || stride > OPD_NMS_MAX) return fail(OPD_EINVAL, "opd_detr_nms_records: n_frames < 0, or a stride outside [1, 128]");
    if (nms_threshold != nms_threshold) return fail(OPD_EINVAL, "opd_detr_nms_records: the threshold is NaN");
    if (n_frames == 0) return OPD_OK;
    HIPCHK(hipSetDevice(m->device));
    if (!device_accessible(dets) || !device_accessible(counts))
        return fail(OPD_EINVAL, "opd_detr_nms_records: records and counts must be device-accessible memory");
    int32_t over = 0;
    RCCHK(enqueue_nms(m, dets, counts, n_frames, stride, person_label, nms_threshold));
    HIPCHK(hipMemcpyAsync(&over, m->d_nms_flag, 4, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    if (m->profiling == 1) timed_collect(m);   // (the launch's event pair: this call's row of opd_detr_kernel_table)
    if (over) {
        HIPCHK(hipMemsetAsync(m->d_nms_flag, 0, 4, m->stream));
        return fail(OPD_EINVAL, "opd_detr_nms_records: a frame holds more records than its slots (left as it was)");
    }
    return OPD_OK;
}); }
// A run of frames without a key frame (both sequence-hybrid entries, behind their checks): no forward; the run on the tracker's own stream, which is
// opd_lwt_interpolate_sequence
static int sequence_without_keys(opd_lwt* t, const LwtSeqCall& call, opd_lwt_rec* recs_out, int capacity, int32_t* rec_counts, int32_t* frames_done, const std::string& me) {
    HIPCHK(hipSetDevice(t->device));
    RCCHK(lwt_sequence_enqueue(t, t->stream(), call, nullptr, nullptr, me.c_str()));
    RCCHK(lwt_sequence_fetch(t, t->stream(), call.F));
    HIPCHK(hipStreamSynchronize(t->stream()));
    t->last_waits = 1;
    return lwt_sequence_finish(t, call, nullptr, nullptr, recs_out, capacity, rec_counts, frames_done, me);
}
// What both sequence-hybrid entries refuse first, without a handle: the F range, the capacity, the null lists; then the key frames of the run into *keys,
// and a null output among those their number asks for (`key_outputs`: out, counts and track_ids are there; `between_outputs`: recs_out and rec_counts)
static int sequence_keys(const std::string& me, const uint8_t* const* frames, const uint8_t* is_key, int F, int capacity, const int32_t* frames_done, bool key_outputs,
                         bool between_outputs, std::vector<const uint8_t*>* keys) {
    if (F < 1 || F > LWT_MAX_SEQUENCE) return fail(OPD_EINVAL, me + ": " + std::to_string(F) + " frames, a call takes 1 .. " + std::to_string(LWT_MAX_SEQUENCE));
    if (capacity < 1) return fail(OPD_EINVAL, me + ": capacity " + std::to_string(capacity) + " is below the tracker's max_tracks");
    if (!frames || !is_key || !frames_done) return fail(OPD_EINVAL, me + ": null argument (frame list, key flags or frames_done)");
    for (int f = 0; f < F; ++f)
        if (is_key[f]) keys->push_back(frames[f]);
    const int K = (int)keys->size();
    if (K > 0 && !key_outputs) return fail(OPD_EINVAL, me + ": null output of the key frames");
    if (K < F && !between_outputs) return fail(OPD_EINVAL, me + ": null output of the in-between frames");
    return OPD_OK;
}
// A tracker inside a frame-list call takes the records the suppression on the device has kept, of the label it keeps
static int check_device_nms(const opd_detr* m, int label, const std::string& me) {
    if (m->nms_threshold < 0.f)
        return fail(OPD_EINVAL, me + ": opd_detr_set_nms is off on this handle; a tracker takes the kept records of a frame, which only the suppression on the device leaves there");
    if (m->nms_label != label)
        return fail(OPD_EINVAL, me + ": opd_detr_set_nms keeps label " + std::to_string(m->nms_label) + ", the call asks for label " + std::to_string(label));
    return OPD_OK;
}
// Tiled detection: every refusal comes before the first device call (check_tiles; check_shape makes none for host pixels).  `st` (null: opd_detr_detect_tiled
// itself): the feature, floor and track parts of the sink, which then read the merged records where the merge left them, rows by position.  `rs`
// (opd_detr_detect_tiled_reid; `st` is then null): the same with the Re-ID rows as the feature kind, rows by slot, a slot naming a position.
// `mixed` (opd_detr_detect_tiled_ragged): the windows may differ in size, `tile_HW` [n_tiles][2] is the model size of each and H x W, not read as given, the
// canvas that holds them all; windows of one size with one model size take the path of the other entries, launch for launch.  `hyb` (the hybrid entries;
// `st` then carries their floor part alone): the hybrid stage of the sink, a tracker per frame or `seq` with the run `hyb_call`, whose Q becomes S here
static int detect_tiled(const std::string& me, opd_detr* m, const uint8_t* const* frames, int n_frames, int h, int w, const int32_t* tiles_yxhw, int n_tiles, int H, int W,
                        const int32_t* tile_HW, bool mixed, float threshold, const opd_tile_params* p, const opd_tile_stages* st, const opd_tile_reid_stages* rs, opd_tile_det* out, int32_t* counts,
                        const HybridStage* hyb = nullptr, LwtSeqCall* hyb_call = nullptr) {
    if (!frames || !out || !counts) return fail(OPD_EINVAL, me + ": null argument");
    opd_tile_stages of_reid{};   // the floor and track parts of the Re-ID entry's block, as the checks below read them
    if (rs) {   // (opd_detr_detect_tiled_reid: `st` is null)
        if (rs->struct_size != (int32_t)sizeof(opd_tile_reid_stages)) return fail(OPD_EINVAL, me + ": opd_tile_reid_stages.struct_size mismatch");
        if (!rs->reid) return fail(OPD_EINVAL, me + ": null Re-ID handle");
        if (!rs->slot_map || !rs->n_person) return fail(OPD_EINVAL, me + ": slot_map or n_person is null");
        if (!rs->features && !rs->trackers) return fail(OPD_EINVAL, me + ": features is null while no trackers are given (the rows would go nowhere)");
        of_reid = opd_tile_stages{(int32_t)sizeof(opd_tile_stages), OPD_TRACK_FEAT_REID, rs->features, rs->floor, rs->floor_out, rs->trackers, rs->track_ids, rs->n_featured};
        st = &of_reid;
    }
    const bool color = st && st->feature_kind == OPD_TRACK_FEAT_COLOR;
    if (st) {   // what needs neither the handle nor the windows
        if (st->struct_size != (int32_t)sizeof(opd_tile_stages)) return fail(OPD_EINVAL, me + ": opd_tile_stages.struct_size mismatch");
        if (st->feature_kind != OPD_TRACK_FEAT_NONE && !color && !rs)
            return fail(OPD_EINVAL, me + ": feature_kind " + std::to_string(st->feature_kind) + "; a tiled call takes OPD_TRACK_FEAT_NONE or OPD_TRACK_FEAT_COLOR (a box merged from two "
                                         "tiles' maps has no encoder row, and Re-ID is a call of its own)");
        if (st->features && !color && !rs) return fail(OPD_EINVAL, me + ": features given with feature_kind OPD_TRACK_FEAT_NONE");
        if (st->floor && !st->floor_out) return fail(OPD_EINVAL, me + ": floor_out is null while a floor-map handle is given");
        if (st->trackers && (!st->track_ids || !st->n_featured)) return fail(OPD_EINVAL, me + ": track_ids or n_featured is null while trackers are given");
    }
    RCCHK(check_tiles(me, p, tiles_yxhw, n_tiles, h, w, !mixed));
    if (!(p->tile_nms_threshold >= 0.f)) return fail(OPD_EINVAL, me + ": tile_nms_threshold is negative or NaN");
    bool one_size = true;   // one window size and one model size: the canvas is every tile's
    if (mixed) {
        if (!tile_HW) return fail(OPD_EINVAL, me + ": null argument (tile_HW)");
        H = W = 0;
        for (int t = 0; t < n_tiles; ++t) {
            if (tile_HW[2 * t] < 1 || tile_HW[2 * t + 1] < 1)
                return fail(OPD_EINVAL, me + ": tile " + std::to_string(t) + " has the model size " + std::to_string(tile_HW[2 * t]) + " x " + std::to_string(tile_HW[2 * t + 1]) + ", below 1");
            H = std::max(H, (int)tile_HW[2 * t]); W = std::max(W, (int)tile_HW[2 * t + 1]);
            one_size = one_size && tile_HW[2 * t] == tile_HW[0] && tile_HW[2 * t + 1] == tile_HW[1] && tiles_yxhw[4 * t + 2] == tiles_yxhw[2] && tiles_yxhw[4 * t + 3] == tiles_yxhw[3];
        }
    }
    if (color && (h > OPD_COLOR_MAX_EDGE || w > OPD_COLOR_MAX_EDGE))
        return fail(OPD_EINVAL, me + ": feature_kind OPD_TRACK_FEAT_COLOR on frames of " + std::to_string(h) + " x " + std::to_string(w) +
                                     ", outside the 4096 x 4096 the exact integer sums of the colour histogram are sized for");
    if (!m) return fail(OPD_EINVAL, "null model handle");
    if ((long long)n_tiles * m->arch.queries > OPD_TILE_MAX_CAND)
        return fail(OPD_EINVAL, me + ": " + std::to_string(n_tiles) + " tiles x " + std::to_string(m->arch.queries) + " queries exceed the 1024 candidates a frame's merge holds");
    if (n_frames < 1 || (long long)n_frames * n_tiles > m->cfg.max_batch)
        return fail(OPD_EINVAL, me + ": " + std::to_string(n_frames) + " frames x " + std::to_string(n_tiles) + " tiles outside [1, max_batch = " + std::to_string(m->cfg.max_batch) + "]");
    for (int f = 0; f < n_frames; ++f)
        if (!frames[f]) return fail(OPD_EINVAL, me + ": null frame pointer");
    RCCHK(check_shape(m, frames, OPD_PIXELS_U8_BGR_HWC, OPD_MEM_HOST, n_frames * n_tiles, H, W));
    FrameSource src{SRC_TILES, frames, OPD_PIXELS_U8_BGR_HWC, OPD_MEM_HOST, h, w};
    src.n_frames = n_frames; src.n_tiles = n_tiles; src.tiles = tiles_yxhw;
    std::vector<int32_t> valid_hw, window_hw;   // tiles of several sizes, [B][2]: image b's model size inside the canvas; its window, which its boxes are scaled to
    if (!one_size) {
        src.tile_HW = tile_HW;
        for (int b = 0; b < n_frames * n_tiles; ++b) {
            const int t = b % n_tiles;
            valid_hw.insert(valid_hw.end(), {tile_HW[2 * t], tile_HW[2 * t + 1]});
            window_hw.insert(window_hw.end(), {tiles_yxhw[4 * t + 2], tiles_yxhw[4 * t + 3]});
        }
    }
    RecordSink sink(threshold, one_size ? nullptr : window_hw.data(), nullptr, nullptr, OPD_MEM_HOST);   // (boxes in TILE pixels; the merge puts them on the frame)
    sink.tile.params = p; sink.tile.n_frames = n_frames; sink.tile.n_tiles = n_tiles; sink.tile.frame_h = h; sink.tile.frame_w = w;
    sink.tile.out = out; sink.tile.counts = counts; sink.tile.entry = me.c_str();
    if (st) {   // the stages' own refusals that need the handle, then their parts of the sink
        const int S = n_tiles * m->arch.queries;
        if (rs) RCCHK(reid_fused_check(rs->reid, m->device, rs->slots, me.c_str()));
        const int reid_dim = rs ? reid_feature_dim(rs->reid) : 0;
        if (color && m->arch.d_model != OPD_COLOR_DIM) return fail(OPD_EINVAL, me + ": feature_kind OPD_TRACK_FEAT_COLOR: the feature area of the handle is sized for d_model = 256");
        if (st->floor && st->floor->device != m->device)
            return fail(OPD_EINVAL, me + ": the detector is on device " + std::to_string(m->device) + ", the floor map `floor` on device " + std::to_string(st->floor->device));
        for (int f = 0; st->trackers && f < n_frames; ++f) {
            const opd_track* t = st->trackers[f];
            const std::string who = me + ": trackers[" + std::to_string(f) + "] ";
            if (!t) return fail(OPD_EINVAL, who + "is null");
            if (t->device != m->device) return fail(OPD_EINVAL, who + "is on device " + std::to_string(t->device) + ", the detector on device " + std::to_string(m->device));
            if (t->NM < S)
                return fail(OPD_EINVAL, who + "was made for max_dets = " + std::to_string(t->NM) + ", a tiled frame can keep n_tiles x num_queries = " + std::to_string(S) + " records");
            if (color && t->D != OPD_COLOR_DIM)
                return fail(OPD_EINVAL, who + "was made for feature_dim = " + std::to_string(t->D) + ", the rows of feature_kind OPD_TRACK_FEAT_COLOR have 256 numbers");
            if (rs && t->D != reid_dim)
                return fail(OPD_EINVAL, who + "was made for feature_dim = " + std::to_string(t->D) + ", the rows of the Re-ID model have " + std::to_string(reid_dim) + " numbers");
            for (int a = 0; a < f; ++a)
                if (st->trackers[a] == t) return fail(OPD_EINVAL, who + "is trackers[" + std::to_string(a) + "] too; a tracker takes one frame per call");
        }
        sink.label = p->person_label;
        sink.feature.kind = color ? FEAT_COLOR : rs ? FEAT_REID : FEAT_NONE; sink.feature.features = st->features;
        if (rs) { sink.feature.reid = rs->reid; sink.feature.slots = rs->slots; sink.feature.slot_map = rs->slot_map; sink.feature.n_person = rs->n_person; }
        sink.floor.fmap = st->floor; sink.floor.out = st->floor_out;
        sink.track.trackers = st->trackers; sink.track.track_ids = st->track_ids; sink.track.n_featured = st->n_featured;
    }
    if (hyb) {   // a merged frame enters a hybrid tracker with up to S records and its WHOLE frame of h x w
        const int S = n_tiles * m->arch.queries;
        if (hyb_call) {   // (a null tracker is lwt_fused_check's to refuse, inside)
            hyb_call->Q = S;
            RCCHK(lwt_sequence_check(hyb->seq, *hyb_call, hyb->capacity, m->device, me));
            *hyb->frames_done = 0;
        } else for (int f = 0; f < n_frames; ++f) {
            RCCHK(lwt_fused_check(hyb->trackers[f], m->device, S, h, w, me + ": trackers[" + std::to_string(f) + "]"));
            for (int a = 0; a < f; ++a)
                if (hyb->trackers[a] == hyb->trackers[f])
                    return fail(OPD_EINVAL, me + ": frames " + std::to_string(a) + " and " + std::to_string(f) + " name the same tracker; a tracker takes one frame per call");
        }
        sink.hybrid = *hyb;
        sink.hybrid.entry = sink.tile.entry;
        sink.label = p->person_label;
    }
    HIPCHK(hipSetDevice(m->device));
    return detect_pipeline(m, src, n_frames * n_tiles, H, W, one_size ? nullptr : valid_hw.data(), sink);
}
int opd_detr_detect_tiled(opd_detr* m, const uint8_t* const* frames, int n_frames, int h, int w, const int32_t* tiles_yxhw, int n_tiles, int H, int W, float threshold,
                          const opd_tile_params* p, opd_tile_det* out, int32_t* counts) { return api_call("opd_detr_detect_tiled", [&]() -> int {
    return detect_tiled("opd_detr_detect_tiled", m, frames, n_frames, h, w, tiles_yxhw, n_tiles, H, W, nullptr, false, threshold, p, nullptr, nullptr, out, counts);
}); }
// ... with the feature, floor and track stages on the merged records, in front of the same one wait
int opd_detr_detect_tiled_stages(opd_detr* m, const uint8_t* const* frames, int n_frames, int h, int w, const int32_t* tiles_yxhw, int n_tiles, int H, int W, float threshold,
                                 const opd_tile_params* p, const opd_tile_stages* stages, opd_tile_det* out, int32_t* counts) { return api_call("opd_detr_detect_tiled_stages", [&]() -> int {
    if (!stages) return fail(OPD_EINVAL, "opd_detr_detect_tiled_stages: null argument (stages)");
    return detect_tiled("opd_detr_detect_tiled_stages", m, frames, n_frames, h, w, tiles_yxhw, n_tiles, H, W, nullptr, false, threshold, p, stages, nullptr, out, counts);
}); }
// ... with the Re-ID rows of the merged records instead: crops planned on the device from the merged records, cut from the whole frames in m->src, the
// forward on the Re-ID handle's stream between two events, rows by slot into the caller's array and / or the trackers
int opd_detr_detect_tiled_reid(opd_detr* m, const uint8_t* const* frames, int n_frames, int h, int w, const int32_t* tiles_yxhw, int n_tiles, int H, int W, float threshold,
                               const opd_tile_params* p, const opd_tile_reid_stages* stages, opd_tile_det* out, int32_t* counts) { return api_call("opd_detr_detect_tiled_reid", [&]() -> int {
    if (!stages) return fail(OPD_EINVAL, "opd_detr_detect_tiled_reid: null argument (stages)");
    return detect_tiled("opd_detr_detect_tiled_reid", m, frames, n_frames, h, w, tiles_yxhw, n_tiles, H, W, nullptr, false, threshold, p, nullptr, stages, out, counts);
}); }
// ... for a grid whose tiles differ in size: every tile at the model size of its own inside one canvas, a ragged batch; `stages` as in
// opd_detr_detect_tiled_stages, or null
int opd_detr_detect_tiled_ragged(opd_detr* m, const uint8_t* const* frames, int n_frames, int h, int w, const int32_t* tiles_yxhw, int n_tiles, const int32_t* tile_HW,
                                 float threshold, const opd_tile_params* p, const opd_tile_stages* stages, opd_tile_det* out, int32_t* counts) { return api_call("opd_detr_detect_tiled_ragged", [&]() -> int {
    return detect_tiled("opd_detr_detect_tiled_ragged", m, frames, n_frames, h, w, tiles_yxhw, n_tiles, 0, 0, tile_HW, true, threshold, p, stages, nullptr, out, counts);
}); }
// ... with the Re-ID rows on such a grid: opd_detr_detect_tiled_reid's stages behind the ragged forward (windows of one size with one model size: that entry's path)
int opd_detr_detect_tiled_ragged_reid(opd_detr* m, const uint8_t* const* frames, int n_frames, int h, int w, const int32_t* tiles_yxhw, int n_tiles, const int32_t* tile_HW,
                                      float threshold, const opd_tile_params* p, const opd_tile_reid_stages* stages, opd_tile_det* out, int32_t* counts) { return api_call("opd_detr_detect_tiled_ragged_reid", [&]() -> int {
    if (!stages) return fail(OPD_EINVAL, "opd_detr_detect_tiled_ragged_reid: null argument (stages)");
    return detect_tiled("opd_detr_detect_tiled_ragged_reid", m, frames, n_frames, h, w, tiles_yxhw, n_tiles, 0, 0, tile_HW, true, threshold, p, nullptr, stages, out, counts);
}); }
// ... with a detection frame of the hybrid tracker on the merged records: frame f's merged records and its WHOLE frame, where the tiled source
// left it, enter hybrid tracker f in front of the same one wait.  `tile_HW` null: one size H x W; else the ragged form
int opd_detr_detect_tiled_hybrid(opd_detr* m, const uint8_t* const* frames, int n_frames, int h, int w, const int32_t* tiles_yxhw, int n_tiles, int H, int W,
                                 const int32_t* tile_HW, float threshold, const opd_tile_params* p, const opd_tile_hybrid* hy, opd_tile_det* out, int32_t* counts) { return api_call("opd_detr_detect_tiled_hybrid", [&]() -> int {
    const std::string me = "opd_detr_detect_tiled_hybrid";
    if (!hy) return fail(OPD_EINVAL, me + ": null argument (hy)");
    if (hy->struct_size != (int32_t)sizeof(opd_tile_hybrid)) return fail(OPD_EINVAL, me + ": opd_tile_hybrid.struct_size mismatch");
    if (!hy->trackers || !hy->track_ids) return fail(OPD_EINVAL, me + ": trackers or track_ids is null");
    opd_tile_stages floor_part{};   // (floor_out without floor, a floor map on another device: detect_tiled's refusals)
    floor_part.struct_size = (int32_t)sizeof(opd_tile_stages); floor_part.feature_kind = OPD_TRACK_FEAT_NONE; floor_part.floor = hy->floor; floor_part.floor_out = hy->floor_out;
    HybridStage stage;
    stage.trackers = hy->trackers; stage.track_ids = hy->track_ids;
    return detect_tiled(me, m, frames, n_frames, h, w, tiles_yxhw, n_tiles, H, W, tile_HW, tile_HW != nullptr, threshold, p, &floor_part, nullptr, out, counts, &stage);
}); }
// The sequence twin on tiled frames: opd_detr_detect_sequence_hybrid whose K key frames go through ONE tiled forward, suppression and seam merge; a key
// frame's merged records (up to S = n_tiles x num_queries) and its whole frame enter the tracker in frame order, the in-between frames around them
int opd_detr_detect_tiled_sequence_hybrid(opd_detr* m, opd_lwt* t, const uint8_t* const* frames, const uint8_t* is_key, int F, int h, int w, const int32_t* tiles_yxhw,
                                          int n_tiles, int H, int W, const int32_t* tile_HW, float threshold, const opd_tile_params* p, opd_tile_det* out, int32_t* counts,
                                          int32_t* track_ids, opd_lwt_rec* recs_out, int capacity, int32_t* rec_counts, int32_t* frames_done) { return api_call("opd_detr_detect_tiled_sequence_hybrid", [&]() -> int {
    const std::string me = "opd_detr_detect_tiled_sequence_hybrid";
    std::vector<const uint8_t*> keys;
    RCCHK(sequence_keys(me, frames, is_key, F, capacity, frames_done, out && counts && track_ids, recs_out && rec_counts, &keys));
    const int K = (int)keys.size();
    LwtSeqCall call{frames, is_key, F, h, w, 0};
    if (K == 0) {   // no forward and no tiles: opd_lwt_interpolate_sequence, as in the frame-list entry
        if (!frame_size_ok(h, w)) return fail(OPD_EINVAL, me + ": source frame size " + std::to_string(h) + " x " + std::to_string(w) + " out of range");
        if (!m) return fail(OPD_EINVAL, "null model handle");
        if (n_tiles < 1 || (long long)n_tiles * m->arch.queries > OPD_TILE_MAX_CAND)
            return fail(OPD_EINVAL, me + ": " + std::to_string(n_tiles) + " tiles x " + std::to_string(m->arch.queries) + " queries outside the 1024 candidates a frame's merge holds");
        call.Q = n_tiles * m->arch.queries;
        RCCHK(lwt_sequence_check(t, call, capacity, m->device, me));
        *frames_done = 0;
        return sequence_without_keys(t, call, recs_out, capacity, rec_counts, frames_done, me);
    }
    HybridStage stage;
    stage.seq = t; stage.call = &call; stage.track_ids = track_ids;
    stage.recs_out = recs_out; stage.capacity = capacity; stage.rec_counts = rec_counts; stage.frames_done = frames_done;
    return detect_tiled(me, m, keys.data(), K, h, w, tiles_yxhw, n_tiles, H, W, tile_HW, tile_HW != nullptr, threshold, p, nullptr, nullptr, out, counts, &stage, &call);
}); }
int opd_detr_merge_tiles(opd_detr* m, const opd_det* recs, const int32_t* tile_counts, int n_frames, int n_tiles, int stride, const int32_t* tiles_yxhw, int h, int w,
                         const opd_tile_params* p, opd_tile_det* out, int32_t* counts) { return api_call("opd_detr_merge_tiles", [&]() -> int {
    RCCHK(check_tiles("opd_detr_merge_tiles", p, tiles_yxhw, n_tiles, h, w, false));
    if (n_frames < 0 || stride < 1 || (long long)n_tiles * stride > OPD_TILE_MAX_CAND)
        return fail(OPD_EINVAL, "opd_detr_merge_tiles: n_frames < 0, stride < 1, or n_tiles x stride above the 1024 candidates a frame's merge holds");
    if (!m) return fail(OPD_EINVAL, "null model handle");
    if (n_frames == 0) return OPD_OK;
    if (!recs || !tile_counts || !out || !counts) return fail(OPD_EINVAL, "opd_detr_merge_tiles: null argument");
    HIPCHK(hipSetDevice(m->device));
    return merge_tiles(m, recs, tile_counts, n_frames, n_tiles, stride, tiles_yxhw, h, w, p, out, counts);
}); }
int opd_detr_resize_u8(opd_detr* m, const uint8_t* frames, int B, int h, int w, int out_h, int out_w, uint8_t* out) { return api_call("opd_detr_resize_u8", [&]() -> int {
    if (!m) return fail(OPD_EINVAL, "null model handle");
    if (!frames || !out) return fail(OPD_EINVAL, "opd_detr_resize_u8: null buffer");
    uint8_t dummy = 0;
    RCCHK(check_shape(m, &dummy, OPD_PIXELS_U8_BGR_HWC, OPD_MEM_HOST, B, out_h, out_w));
    HIPCHK(hipSetDevice(m->device));
    RCCHK(enqueue_resize(m, frames, OPD_MEM_HOST, B, h, w, out_h, out_w));
    HIPCHK(hipMemcpyAsync(out, m->d_u8, (size_t)B * out_h * out_w * 3, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    return OPD_OK;
}); }
int opd_detr_forward_resized(opd_detr* m, const uint8_t* frames, int mem_kind, int B, int h, int w, int H, int W, float* logits,
                             float* boxes, float* enc_features) { return api_call("opd_detr_forward_resized", [&]() -> int {
    RCCHK(check_shape(m, frames, OPD_PIXELS_U8_BGR_HWC, mem_kind, B, H, W));
    HIPCHK(hipSetDevice(m->device));
    return forward_device(m, {SRC_BLOCK, frames, OPD_PIXELS_U8_BGR_HWC, mem_kind, h, w}, B, H, W, nullptr, logits, boxes, enc_features);
}); }
int opd_detr_detect(opd_detr* m, const void* pixels, int pixel_format, int mem_kind, int B, int H, int W, float threshold,
                    const int32_t* orig_hw, opd_det* out, int32_t* counts) { return api_call("opd_detr_detect", [&]() -> int {
    return opd_detr_detect_ragged(m, pixels, pixel_format, mem_kind, B, H, W, nullptr, threshold, orig_hw, out, counts);
}); }
int opd_detr_detect_ragged(opd_detr* m, const void* pixels, int pixel_format, int mem_kind, int B, int H, int W,
                           const int32_t* valid_hw, float threshold, const int32_t* orig_hw, opd_det* out, int32_t* counts) { return api_call("opd_detr_detect_ragged", [&]() -> int {
    RCCHK(check_shape(m, pixels, pixel_format, mem_kind, B, H, W));
    if (!out || !counts) return fail(OPD_EINVAL, "opd_detr_detect: null output buffer");
    RCCHK(check_device_outputs(mem_kind, out, counts, "opd_detr_detect"));
    HIPCHK(hipSetDevice(m->device));
    return detect_pipeline(m, {SRC_PIXELS, pixels, pixel_format, mem_kind, 0, 0}, B, H, W, valid_hw, RecordSink(threshold, orig_hw, out, counts, mem_kind));
}); }
int opd_detr_detect_async(opd_detr* m, const void* pixels, int pixel_format, int mem_kind, int B, int H, int W, float threshold,
                          const int32_t* orig_hw, opd_det* out, int32_t* counts, int* ticket) { return api_call("opd_detr_detect_async", [&]() -> int {
    RCCHK(check_shape(m, pixels, pixel_format, mem_kind, B, H, W));
    if (!out || !counts || !ticket) return fail(OPD_EINVAL, "opd_detr_detect_async: null argument");
    RCCHK(check_device_outputs(mem_kind, out, counts, "opd_detr_detect_async"));
    if (m->profiling) return fail(OPD_ESTATE, "opd_detr_detect_async is not available in profiling mode");
    HIPCHK(hipSetDevice(m->device));
    const int t = (int)(m->async_next & 3u);
    if (m->async_pending[t])
        return fail(OPD_ESTATE, "opd_detr_detect_async: 4 submissions are outstanding on this handle; opd_detr_wait the oldest ticket first");
    if (!m->ev_async[t]) HIPCHK(hipEventCreateWithFlags(&m->ev_async[t], hipEventDisableTiming));
    RCCHK(detect_pipeline(m, {SRC_PIXELS, pixels, pixel_format, mem_kind, 0, 0}, B, H, W, nullptr, RecordSink(threshold, orig_hw, out, counts, mem_kind, WAIT_TICKET, t)));
    *ticket = t;
    return OPD_OK;
}); }
int opd_detr_wait(opd_detr* m, int ticket) { return api_call("opd_detr_wait", [&]() -> int {
    if (!m || ticket < 0 || ticket > 3 || !m->ev_async[ticket]) return fail(OPD_EINVAL, "opd_detr_wait: bad handle or ticket");
    if (!m->async_pending[ticket]) return fail(OPD_ESTATE, "opd_detr_wait: this ticket is not outstanding (already waited for?)");
    HIPCHK(hipSetDevice(m->device));
    HIPCHK(hipEventSynchronize(m->ev_async[ticket]));
    opd_detr::AsyncHost& slot = m->async_host[ticket];
    if (slot.out) {
        unpack_records(m, slot.pinned, slot.B, slot.out, slot.counts);
        slot.out = nullptr;
    }
    m->async_pending[ticket] = false;
    return OPD_OK;
}); }
int opd_detr_detect_resized(opd_detr* m, const uint8_t* frames, int mem_kind, int B, int h, int w, int H, int W, float threshold,
                            opd_det* out, int32_t* counts) { return api_call("opd_detr_detect_resized", [&]() -> int {
    RCCHK(check_shape(m, frames, OPD_PIXELS_U8_BGR_HWC, mem_kind, B, H, W));
    if (!out || !counts) return fail(OPD_EINVAL, "opd_detr_detect_resized: null output buffer");
    RCCHK(check_device_outputs(mem_kind, out, counts, "opd_detr_detect_resized"));
    HIPCHK(hipSetDevice(m->device));
    return detect_pipeline(m, {SRC_BLOCK, frames, OPD_PIXELS_U8_BGR_HWC, mem_kind, h, w}, B, H, W, nullptr, RecordSink(threshold, nullptr, out, counts, mem_kind));
}); }

// The frame-list entries with a stage behind the records (host frames, host outputs, blocking): the base of their sink, and its feature stage ...
static RecordSink host_sink(float threshold, int label, opd_det* out, int32_t* counts, int feature = FEAT_NONE, float* features = nullptr) {
    RecordSink s(threshold, nullptr, out, counts, OPD_MEM_HOST);
    s.label = label; s.feature.kind = feature; s.feature.features = features;
    return s;
}
// ... their one call of the pipeline, behind the last refusal ...
static int detect_frames(opd_detr* m, const uint8_t* const* frames, int mem_kind, int B, int h, int w, int H, int W, const RecordSink& sink) {
    HIPCHK(hipSetDevice(m->device));
    return detect_pipeline(m, {SRC_LIST, frames, OPD_PIXELS_U8_BGR_HWC, mem_kind, h, w}, B, H, W, nullptr, sink);
}
// ... and the argument checks they share, worded with the entry's own name
static int check_frame_list(opd_detr* m, const uint8_t* const* frames, int mem_kind, int B, int H, int W, bool have_outputs, const std::string& who) {
    RCCHK(check_shape(m, frames, OPD_PIXELS_U8_BGR_HWC, mem_kind, B, H, W));
    for (int b = 0; b < B; ++b)
        if (!frames[b]) return fail(OPD_EINVAL, who + ": null frame pointer");
    if (!have_outputs) return fail(OPD_EINVAL, who + ": null output buffer");
    return OPD_OK;
}
int opd_detr_detect_frames(opd_detr* m, const uint8_t* const* frames, int mem_kind, int B, int h, int w, int H, int W, float threshold,
                           opd_det* out, int32_t* counts) { return api_call("opd_detr_detect_frames", [&]() -> int {
    if (!m) return fail(OPD_EINVAL, "null model handle");
    if (mem_kind != OPD_MEM_HOST && mem_kind != OPD_MEM_HOST_PIXELS_DEVICE_OUT) return fail(OPD_EINVAL, "opd_detr_detect_frames takes host frames");
    RCCHK(check_frame_list(m, frames, mem_kind, B, H, W, out && counts, "opd_detr_detect_frames"));
    RCCHK(check_device_outputs(mem_kind, out, counts, "opd_detr_detect_frames"));
    return detect_frames(m, frames, mem_kind, B, h, w, H, W, RecordSink(threshold, nullptr, out, counts, mem_kind));
}); }

int opd_detr_detect_frames_features(opd_detr* m, const uint8_t* const* frames, int B, int h, int w, int H, int W, float threshold, int label,
                                    opd_det* out, int32_t* counts, float* features) { return api_call("opd_detr_detect_frames_features", [&]() -> int {
    RCCHK(check_frame_list(m, frames, OPD_MEM_HOST, B, H, W, out && counts && features, "opd_detr_detect_frames_features"));
    if (m->arch.d_model != 256) return fail(OPD_EINVAL, "opd_detr_detect_frames_features: the pooling kernel is built for d_model = 256");
    return detect_frames(m, frames, OPD_MEM_HOST, B, h, w, H, W, host_sink(threshold, label, out, counts, FEAT_ROI, features));
}); }

// The colour-histogram twin: the feature stage reads the CAMERA-resolution frames the source step has just put on the device
int opd_detr_detect_frames_color(opd_detr* m, const uint8_t* const* frames, int B, int h, int w, int H, int W, float threshold, int label,
                                 opd_det* out, int32_t* counts, float* features) { return api_call("opd_detr_detect_frames_color", [&]() -> int {
    RCCHK(check_frame_list(m, frames, OPD_MEM_HOST, B, H, W, out && counts && features, "opd_detr_detect_frames_color"));
    if (m->arch.d_model != OPD_COLOR_DIM) return fail(OPD_EINVAL, "opd_detr_detect_frames_color: the feature area of the handle is sized for d_model = 256");
    if (h < 1 || w < 1 || h > OPD_COLOR_MAX_EDGE || w > OPD_COLOR_MAX_EDGE)
        return fail(OPD_EINVAL, "opd_detr_detect_frames_color: frames of " + std::to_string(h) + " x " + std::to_string(w) +
                                    " are outside the 4096 x 4096 the exact integer sums are sized for");
    return detect_frames(m, frames, OPD_MEM_HOST, B, h, w, H, W, host_sink(threshold, label, out, counts, FEAT_COLOR, features));
}); }

// The floor-map twin: the floor stage maps the foot point of every record of the class with `f`'s model (read-only device tables: any stream may read them)
int opd_detr_detect_frames_floor(opd_detr* m, opd_floor* f, const uint8_t* const* frames, int B, int h, int w, int H, int W, float threshold,
                                 int label, opd_det* out, int32_t* counts, opd_floor_rec* floor) { return api_call("opd_detr_detect_frames_floor", [&]() -> int {
    if (!f) return fail(OPD_EINVAL, "opd_detr_detect_frames_floor: null floor-map handle");
    RCCHK(check_frame_list(m, frames, OPD_MEM_HOST, B, H, W, out && counts && floor, "opd_detr_detect_frames_floor"));
    if (f->device != m->device)
        return fail(OPD_EINVAL, "opd_detr_detect_frames_floor: the detector is on device " + std::to_string(m->device) + ", the floor map on device " + std::to_string(f->device));
    RecordSink sink = host_sink(threshold, label, out, counts);
    sink.floor.fmap = f; sink.floor.out = floor;
    return detect_frames(m, frames, OPD_MEM_HOST, B, h, w, H, W, sink);
}); }

// The Re-ID twin: the feature stage is `r`'s fused call (opd_reid.h), crops read in place from the CAMERA-resolution frames, its forward on its own stream
int opd_detr_detect_frames_reid(opd_detr* m, opd_reid* r, const uint8_t* const* frames, int B, int h, int w, int H, int W, float threshold, int label,
                                int slots, opd_det* out, int32_t* counts, float* features, int32_t* slot_map, int32_t* n_person) { return api_call("opd_detr_detect_frames_reid", [&]() -> int {
    if (!r) return fail(OPD_EINVAL, "opd_detr_detect_frames_reid: null Re-ID handle");
    RCCHK(check_frame_list(m, frames, OPD_MEM_HOST, B, H, W, out && counts && features && slot_map && n_person, "opd_detr_detect_frames_reid"));
    RCCHK(reid_fused_check(r, m->device, slots, "opd_detr_detect_frames_reid"));
    if (!frame_size_ok(h, w))
        return fail(OPD_EINVAL, "opd_detr_detect_frames_reid: source frame size " + std::to_string(h) + " x " + std::to_string(w) + " out of range");
    RecordSink sink = host_sink(threshold, label, out, counts, FEAT_REID, features);
    sink.feature.reid = r; sink.feature.slots = slots; sink.feature.slot_map = slot_map; sink.feature.n_person = n_person;
    return detect_frames(m, frames, OPD_MEM_HOST, B, h, w, H, W, sink);
}); }

// The tracking twins, behind their own null-argument check: the refusals they share, in this order, and the sink they build alike -- the
// track stage `track` (a tracker per frame, or `seq` for all of them) behind the suppression and the feature stage of `feature_kind`
static int detect_track(const std::string& me, opd_detr* m, opd_reid* r, const TrackStage& track, const uint8_t* const* frames, int B, int h, int w, int H, int W,
                        float threshold, int label, int feature_kind, int slots, opd_det* out, int32_t* counts) {
    if (feature_kind != OPD_TRACK_FEAT_NONE && feature_kind != OPD_TRACK_FEAT_ENCODER && feature_kind != OPD_TRACK_FEAT_COLOR && feature_kind != OPD_TRACK_FEAT_REID)
        return fail(OPD_EINVAL, me + ": unknown feature_kind " + std::to_string(feature_kind));
    if (feature_kind == OPD_TRACK_FEAT_REID && !r) return fail(OPD_EINVAL, me + ": feature_kind OPD_TRACK_FEAT_REID with a null Re-ID handle");
    if (!frame_size_ok(h, w)) return fail(OPD_EINVAL, me + ": source frame size " + std::to_string(h) + " x " + std::to_string(w) + " out of range");
    if (feature_kind == OPD_TRACK_FEAT_COLOR && (h > OPD_COLOR_MAX_EDGE || w > OPD_COLOR_MAX_EDGE))
        return fail(OPD_EINVAL, me + ": frames of " + std::to_string(h) + " x " + std::to_string(w) + " are outside the 4096 x 4096 the exact integer sums of the colour histogram are sized for");
    RCCHK(check_frame_list(m, frames, OPD_MEM_HOST, B, H, W, true, me));
    RCCHK(check_device_nms(m, label, me));
    RecordSink sink = host_sink(threshold, label, out, counts);
    sink.track = track;
    int dim = 0;   // the width of a feature row of the kind
    if (feature_kind == OPD_TRACK_FEAT_REID) {
        RCCHK(reid_fused_check(r, m->device, slots, me.c_str()));
        dim = reid_feature_dim(r);
        sink.feature.kind = FEAT_REID; sink.feature.reid = r; sink.feature.slots = slots;
    } else if (feature_kind != OPD_TRACK_FEAT_NONE) {
        if (m->arch.d_model != OPD_COLOR_DIM) return fail(OPD_EINVAL, me + ": the feature area of the handle and both kernels that fill it are sized for d_model = 256");
        dim = OPD_COLOR_DIM;
        sink.feature.kind = feature_kind == OPD_TRACK_FEAT_ENCODER ? FEAT_ROI : FEAT_COLOR;
    }
    if (track.cams) {   // (every tracker of the list by the same checks, then the list against camera_of)
        for (int c = 0; c < track.n_cams; ++c) RCCHK(track_fused_check(track.cams[c], m->device, m->arch.queries, dim, me.c_str()));
        RCCHK(track_streams_check(track.cams, track.n_cams, track.camera_of, B, me.c_str()));
    }
    for (int b = 0; b < (track.trackers ? B : 1) && !track.cams; ++b) {   // (a null tracker, `seq` too, is track_fused_check's to refuse)
        RCCHK(track_fused_check(track.trackers ? track.trackers[b] : track.seq, m->device, m->arch.queries, dim, me.c_str()));
        for (int a = 0; a < b; ++a)
            if (track.trackers[a] == track.trackers[b])
                return fail(OPD_EINVAL, me + ": frames " + std::to_string(a) + " and " + std::to_string(b) + " name the same tracker; a tracker takes one frame per call");
    }
    return detect_frames(m, frames, OPD_MEM_HOST, B, h, w, H, W, sink);
}
// (both: what needs no handle first, so that a null handle is the last thing reported without one)
int opd_detr_detect_frames_track(opd_detr* m, opd_reid* r, opd_track* const* trackers, const uint8_t* const* frames, int B, int h, int w, int H, int W,
                                 float threshold, int label, int feature_kind, int slots, opd_det* out, int32_t* counts, int32_t* track_ids,
                                 int32_t* n_featured) { return api_call("opd_detr_detect_frames_track", [&]() -> int {
    const std::string me = "opd_detr_detect_frames_track";
    if (!trackers || !frames || !out || !counts || !track_ids || !n_featured) return fail(OPD_EINVAL, me + ": null argument (tracker list, frame list or an output)");
    TrackStage track;
    track.trackers = trackers; track.track_ids = track_ids; track.n_featured = n_featured;
    return detect_track(me, m, r, track, frames, B, h, w, H, W, threshold, label, feature_kind, slots, out, counts);
}); }
// The sequence twin: B consecutive frames of ONE camera into ONE tracker, the association on the device between them
int opd_detr_detect_sequence_track(opd_detr* m, opd_reid* r, opd_track* t, const uint8_t* const* frames, int B, int h, int w, int H, int W, float threshold,
                                   int label, int feature_kind, int slots, opd_det* out, int32_t* counts, int32_t* track_ids, int32_t* n_featured,
                                   int32_t* frames_done) { return api_call("opd_detr_detect_sequence_track", [&]() -> int {
    const std::string me = "opd_detr_detect_sequence_track";
    if (!frames || !out || !counts || !track_ids || !n_featured || !frames_done) return fail(OPD_EINVAL, me + ": null argument (frame list or an output)");
    TrackStage track;
    track.seq = t; track.track_ids = track_ids; track.n_featured = n_featured; track.frames_done = frames_done;
    return detect_track(me, m, r, track, frames, B, h, w, H, W, threshold, label, feature_kind, slots, out, counts);
}); }

// The streams twin: K_c frames each of C cameras in one call, frame b into trackers[camera_of[b]], the cameras' steps side by side on the device
int opd_detr_detect_streams_track(opd_detr* m, opd_reid* r, opd_track* const* trackers, int C, const int32_t* camera_of, const uint8_t* const* frames, int B, int h, int w,
                                  int H, int W, float threshold, int label, int feature_kind, int slots, opd_det* out, int32_t* counts, int32_t* track_ids,
                                  int32_t* n_featured, int32_t* frames_done) { return api_call("opd_detr_detect_streams_track", [&]() -> int {
    const std::string me = "opd_detr_detect_streams_track";
    if (!trackers || !camera_of || !frames || !out || !counts || !track_ids || !n_featured || !frames_done)
        return fail(OPD_EINVAL, me + ": null argument (tracker list, camera_of, frame list or an output)");
    if (C < 1 || C > TRACK_MAX_CAMERAS) return fail(OPD_EINVAL, me + ": C = " + std::to_string(C) + " outside 1 .. " + std::to_string((int)TRACK_MAX_CAMERAS) + " trackers a call");
    TrackStage track;
    track.cams = trackers; track.n_cams = C; track.camera_of = camera_of; track.track_ids = track_ids; track.n_featured = n_featured; track.frames_done = frames_done;
    return detect_track(me, m, r, track, frames, B, h, w, H, W, threshold, label, feature_kind, slots, out, counts);
}); }

// The hybrid twin: frame b's kept records and its camera-resolution frame enter hybrid tracker b inside the call
int opd_detr_detect_frames_hybrid(opd_detr* m, opd_lwt* const* trackers, const uint8_t* const* frames, int B, int h, int w, int H, int W, float threshold,
                                  int label, opd_det* out, int32_t* counts, int32_t* track_ids) { return api_call("opd_detr_detect_frames_hybrid", [&]() -> int {
    const std::string me = "opd_detr_detect_frames_hybrid";
    if (!trackers || !frames || !out || !counts || !track_ids) return fail(OPD_EINVAL, me + ": null argument (tracker list, frame list or an output)");
    if (!frame_size_ok(h, w)) return fail(OPD_EINVAL, me + ": source frame size " + std::to_string(h) + " x " + std::to_string(w) + " out of range");
    RCCHK(check_frame_list(m, frames, OPD_MEM_HOST, B, H, W, true, me));
    RCCHK(check_device_nms(m, label, me));
    for (int b = 0; b < B; ++b) {
        RCCHK(lwt_fused_check(trackers[b], m->device, m->arch.queries, h, w, me));
        for (int a = 0; a < b; ++a)
            if (trackers[a] == trackers[b])
                return fail(OPD_EINVAL, me + ": frames " + std::to_string(a) + " and " + std::to_string(b) + " name the same tracker; a tracker takes one frame per call");
    }
    RecordSink sink = host_sink(threshold, label, out, counts);
    sink.hybrid.trackers = trackers; sink.hybrid.track_ids = track_ids;
    return detect_frames(m, frames, OPD_MEM_HOST, B, h, w, H, W, sink);
}); }

// The sequence twin: F consecutive frames of ONE camera; the key frames among them go through one batched forward, and then every frame, key or
// in-between, enters the tracker in frame order behind the one wait (opd_lwt.h: lwt_sequence_*)
int opd_detr_detect_sequence_hybrid(opd_detr* m, opd_lwt* t, const uint8_t* const* frames, const uint8_t* is_key, int F, int h, int w, int H, int W,
                                    float threshold, int label, opd_det* out, int32_t* counts, int32_t* track_ids, opd_lwt_rec* recs_out, int capacity,
                                    int32_t* rec_counts, int32_t* frames_done) { return api_call("opd_detr_detect_sequence_hybrid", [&]() -> int {
    const std::string me = "opd_detr_detect_sequence_hybrid";
    std::vector<const uint8_t*> keys;
    RCCHK(sequence_keys(me, frames, is_key, F, capacity, frames_done, out && counts && track_ids, recs_out && rec_counts, &keys));
    const int K = (int)keys.size();
    if (!frame_size_ok(h, w)) return fail(OPD_EINVAL, me + ": source frame size " + std::to_string(h) + " x " + std::to_string(w) + " out of range");
    if (!m) return fail(OPD_EINVAL, "null model handle");
    if (K > 0) {
        RCCHK(check_frame_list(m, keys.data(), OPD_MEM_HOST, K, H, W, true, me));   // (more key frames than max_batch among them)
        RCCHK(check_device_nms(m, label, me));
    }
    const LwtSeqCall call{frames, is_key, F, h, w, m->arch.queries};
    RCCHK(lwt_sequence_check(t, call, capacity, m->device, me));
    *frames_done = 0;
    if (K == 0) return sequence_without_keys(t, call, recs_out, capacity, rec_counts, frames_done, me);
    RecordSink sink = host_sink(threshold, label, out, counts);
    sink.hybrid.seq = t; sink.hybrid.call = &call; sink.hybrid.track_ids = track_ids; sink.hybrid.entry = "opd_detr_detect_sequence_hybrid";
    sink.hybrid.recs_out = recs_out; sink.hybrid.capacity = capacity; sink.hybrid.rec_counts = rec_counts; sink.hybrid.frames_done = frames_done;
    return detect_frames(m, keys.data(), OPD_MEM_HOST, K, h, w, H, W, sink);
}); }

int opd_host_alloc(size_t bytes, void** out) { return api_call("opd_host_alloc", [&]() -> int {
    if (!out || bytes == 0) return fail(OPD_EINVAL, "opd_host_alloc: null output or zero size");
    *out = nullptr;
    HIPCHK(hipHostMalloc(out, bytes, hipHostMallocDefault));
    return OPD_OK;
}); }
void opd_host_free(void* p) { (void)api_call("opd_host_free", [&]() -> int {
    if (p) (void)hipHostFree(p);
    return OPD_OK;
}); }

int opd_similarity_matrix(int device_ordinal, const float* feats1, const float* boxes1, const uint8_t* has1, int n1,
                          const float* feats2, const float* boxes2, const uint8_t* has2, int n2, int D, double appearance_weight,
                          double motion_weight, int as_distance, float* out) { return api_call("opd_similarity_matrix", [&]() -> int {
    if (n1 < 0 || n2 < 0 || D < 1) return fail(OPD_EINVAL, "opd_similarity_matrix: bad sizes");
    if (n1 == 0 || n2 == 0) return OPD_OK;
    if (!boxes1 || !boxes2 || !out) return fail(OPD_EINVAL, "opd_similarity_matrix: null boxes / output");
    if (fabs(appearance_weight + motion_weight - 1.0) > 1e-6)
        return fail(OPD_EINVAL, "appearance_weight + motion_weight must equal 1.0");
    RCCHK(use_device("opd_similarity_matrix", device_ordinal));
    DevMem tmp;
    auto up = [&](auto* h, size_t count) { return h ? tmp.up(h, count) : nullptr; };   // (features and flags are optional)
    const float *df1 = up(feats1, (size_t)n1 * D), *df2 = up(feats2, (size_t)n2 * D), *db1 = up(boxes1, (size_t)n1 * 4), *db2 = up(boxes2, (size_t)n2 * 4);
    const uint8_t *dh1 = up(has1, (size_t)n1), *dh2 = up(has2, (size_t)n2);
    float* dout = tmp.alloc<float>((size_t)n1 * n2);
    if (!tmp.ok) return fail(OPD_ENOMEM, "opd_similarity_matrix: device allocation failed");
    HIPCHK(opd_launch_similarity_matrix(df1, db1, dh1, n1, df2, db2, dh2, n2, D, appearance_weight, motion_weight, as_distance, dout, nullptr));
    HIPCHK(hipMemcpy(out, dout, (size_t)n1 * n2 * 4, hipMemcpyDeviceToHost));
    return OPD_OK;
}); }

int opd_detr_roi_features(opd_detr* m, int frame, const float* boxes_xywh, int n, int orig_h, int orig_w, float* features) { return api_call("opd_detr_roi_features", [&]() -> int {
    if (!m || (n > 0 && (!boxes_xywh || !features))) return fail(OPD_EINVAL, "opd_detr_roi_features: null argument");
    if (m->last_B == 0) return fail(OPD_ESTATE, "opd_detr_roi_features called before any forward");
    if (frame < 0 || frame >= m->last_B || n < 0 || n > 128 || orig_h <= 0 || orig_w <= 0)
        return fail(OPD_EINVAL, "opd_detr_roi_features: frame / n / image size out of range");
    if (n == 0) return OPD_OK;
    HIPCHK(hipSetDevice(m->device));
    const int h = m->last_fh, w = m->last_fw;
    std::vector<int32_t> rois(n * 4);
    for (int i = 0; i < n; ++i) {  // same int-truncation and clamping as the reference (feature_extractor.py:68-78)
        const double x = boxes_xywh[4 * i], y = boxes_xywh[4 * i + 1], bw = boxes_xywh[4 * i + 2], bh = boxes_xywh[4 * i + 3];
        int x0 = (int)((x / orig_w) * w), y0 = (int)((y / orig_h) * h);
        int x1 = (int)(((x + bw) / orig_w) * w), y1 = (int)(((y + bh) / orig_h) * h);
        x0 = std::max(0, std::min(x0, w - 1)); y0 = std::max(0, std::min(y0, h - 1));
        x1 = std::max(x0 + 1, std::min(x1, w)); y1 = std::max(y0 + 1, std::min(y1, h));
        rois[4 * i] = x0; rois[4 * i + 1] = y0; rois[4 * i + 2] = x1; rois[4 * i + 3] = y1;
    }
    HIPCHK(hipMemcpyAsync(m->d_rois, rois.data(), rois.size() * 4, hipMemcpyHostToDevice, m->stream));
    const float* enc = m->d_x32 + (size_t)frame * h * w * m->arch.d_model;
    HIPCHK(opd_launch_roi_features(enc, m->d_rois, m->d_roi_out, n, h, w, m->stream));
    HIPCHK(hipMemcpyAsync(features, m->d_roi_out, (size_t)n * m->arch.d_model * 4, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    return OPD_OK;
}); }

int opd_detr_attention_map(opd_detr* m, int frame, int layer, const int32_t* queries, int n_queries, float* out, int out_capacity) { return api_call("opd_detr_attention_map", [&]() -> int {
    if (!m || !out) return fail(OPD_EINVAL, "opd_detr_attention_map: null argument");
    if (m->last_B == 0) return fail(OPD_ESTATE, "opd_detr_attention_map called before any forward");
    const int L = m->arch.dec_layers, Q = m->arch.queries, D = m->arch.d_model;
    if (layer < 0) layer += L;
    if (frame < 0 || frame >= m->last_B || layer < 0 || layer >= L || n_queries < 0 || n_queries > Q || (n_queries > 0 && !queries))
        return fail(OPD_EINVAL, "opd_detr_attention_map: frame / layer / queries out of range");
    std::vector<int32_t> sel;
    if (n_queries == 0) { sel.resize(Q); for (int i = 0; i < Q; ++i) sel[i] = i; }
    else {
        sel.assign(queries, queries + n_queries);
        for (int q : sel) if (q < 0 || q >= Q) return fail(OPD_EINVAL, "opd_detr_attention_map: query index out of range");
    }
    HIPCHK(hipSetDevice(m->device));
    const int hw = m->last_fh * m->last_fw, NKV = L * 2 * D, Md = m->last_B * Q;
    if (out_capacity < hw)
        return fail(OPD_EINVAL, "opd_detr_attention_map: the last forward's map has " + std::to_string(m->last_fh) + " x " + std::to_string(m->last_fw) +
                                    " positions, the output buffer holds " + std::to_string(out_capacity));
    HIPCHK(hipMemcpyAsync(m->d_amap_sel, sel.data(), sel.size() * 4, hipMemcpyHostToDevice, m->stream));
    const f16_t* q = m->d_qd16 + (size_t)layer * m->cfg.max_batch * Q * D + (size_t)frame * Q * D;
    const f16_t* k = m->d_memkv16 + (size_t)frame * hw * NKV + (size_t)layer * 2 * D;
    const float scale = 1.0f / sqrtf((float)(D / m->arch.heads));
    HIPCHK(opd_launch_attention_map(q, D, k, NKV, m->d_amap_sel, (int)sel.size(), m->arch.heads, hw, scale,
                                    m->last_ragged ? m->d_key_valid + 2 * frame : nullptr, m->last_fw, m->d_amap_stat, m->d_amap, m->stream, m->dtype));
    HIPCHK(hipMemcpyAsync(out, m->d_amap, (size_t)hw * 4, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    return OPD_OK;
}); }

int opd_detr_set_profiling(opd_detr* m, int enabled) { return api_call("opd_detr_set_profiling", [&]() -> int {
    if (!m) return fail(OPD_EINVAL, "null model handle");
    const int mode = enabled == 2 ? 2 : (enabled ? 1 : 0);
    if (mode != m->profiling) {   // the stage marks of mode 2 are nodes of the captured graph: graphs of another mode do not carry them
        HIPCHK(hipSetDevice(m->device));
        HIPCHK(hipStreamSynchronize(m->stream));
        drop_graphs(m);
    }
    m->profiling = mode;
    return OPD_OK;
}); }

int opd_detr_stage_times(const opd_detr* m, float* ms8) { return api_call("opd_detr_stage_times", [&]() -> int {
    if (!m || !ms8) return fail(OPD_EINVAL, "opd_detr_stage_times: null argument");
    for (int i = 0; i < 8; ++i) ms8[i] = m->stage_ms[i];
    return OPD_OK;
}); }

int opd_detr_kernel_table(const opd_detr* m, opd_kernel_stat* out, int capacity, int* count) { return api_call("opd_detr_kernel_table", [&]() -> int {
    if (!m || !count || capacity < 0 || (capacity > 0 && !out)) return fail(OPD_EINVAL, "opd_detr_kernel_table: bad argument");
    *count = (int)m->ktable.size();
    for (int i = 0; i < capacity && i < (int)m->ktable.size(); ++i) {
        const auto& r = m->ktable[i];
        memset(&out[i], 0, sizeof out[i]);
        snprintf(out[i].name, sizeof out[i].name, "%s", r.name.c_str());
        out[i].launches = r.launches; out[i].ms = r.ms; out[i].flops = r.flops;
    }
    return OPD_OK;
}); }

int opd_detr_kernel_times(const opd_detr* m, float* ms4, int32_t* launches4, double* flops4) { return api_call("opd_detr_kernel_times", [&]() -> int {
    if (!m || !ms4 || !launches4 || !flops4) return fail(OPD_EINVAL, "opd_detr_kernel_times: null argument");
    for (int i = 0; i < 4; ++i) { ms4[i] = m->class_ms[i]; launches4[i] = m->class_launches[i]; flops4[i] = m->class_flops[i]; }
    return OPD_OK;
}); }

}  // extern "C"
