// opd_lwt.cpp — the hybrid-tracker handle of include/opd_detr.h (opd_lwt_*): the reference's `LightweightTracker` with every track number on
// the device.  `opd_lwt_update` stages the boxes, enqueues their upload, lwt_update_kernel, (with optical flow) the gray and pyramid
// launches of the new reference frame and the download of [head | ids], and waits once.  `opd_lwt_interpolate` enqueues gray + pyramid +
// LK on the points the device holds, lwt_interp_kernel on LK's results where they lie, and the download of [head | records], and waits
// once.  The host keeps three mirrors (tracks, next id, flow points) that the one wait of every call refreshes: they size the next
// call's launches and checks.  Nothing here computes on a track.
//
// Both calls are an enqueue half and an adopt half around their wait (opd_lwt.h), which three more entries share: opd_lwt_interpolate_sequence
// (F in-between frames behind one wait, here), and the hybrid parts of the detector's fused calls, opd_detr_detect_frames_hybrid,
// opd_detr_detect_sequence_hybrid and their tiled twins (opd_api.cpp), whose launches run on the detector's stream behind its suppression and whose results ride
// on the detector's one fetch (lwt_fused_*, lwt_sequence_*).
#include <string.h>

#include <algorithm>
#include <memory>
#include <string>

#include "opd_lwt.h"

using namespace opd;

// the two launches with everything a sequence call varies from frame to frame: the bank, where the result goes, the stream, the sticky word
static int launch_update(opd_lwt* t, hipStream_t s, int cur, int n, const int32_t* d_count, int32_t* d_result, int32_t* stop);
static int launch_interp(opd_lwt* t, hipStream_t s, int cur, bool with_points, int32_t* d_result, LwtRec* d_recs, const int32_t* stop);

namespace {

int write_head(opd_lwt* t) {
    const int32_t head[LWT_HEAD] = {0, 1, 0, 0};
    HIPCHK(hipSetDevice(t->device));
    HIPCHK(hipStreamSynchronize(t->stream()));
    HIPCHK(hipMemcpy(t->d_head, head, sizeof head, hipMemcpyHostToDevice));
    t->n_tracks = 0; t->next_id = 1; t->n_points = 0;
    t->last_launches = t->last_waits = 0;
    if (t->flow) t->flow->pyr[0].valid = t->flow->pyr[1].valid = false;
    return OPD_OK;
}

void read_head(opd_lwt* t, const uint8_t* host_result) {
    const int32_t* r = reinterpret_cast<const int32_t*>(host_result);
    t->n_tracks = r[LWT_HEAD_TRACKS]; t->next_id = r[LWT_HEAD_NEXT_ID]; t->n_points = r[LWT_HEAD_POINTS];
}

int check_lwt_frame(const opd_lwt* t, const char* who, const uint8_t* bgr) {
    if (t->use_flow && !bgr) return fail(OPD_EINVAL, std::string(who) + ": null frame pointer (the handle was made with use_optical_flow)");
    return OPD_OK;
}

}  // namespace

extern "C" int opd_lwt_create(const opd_lwt_config* cfg, int device_ordinal, opd_lwt** out) { return api_call("opd_lwt_create", [&]() -> int {
    const std::string me = "opd_lwt_create: ";
    if (!out) return fail(OPD_EINVAL, me + "null argument");
    *out = nullptr;
    if (!cfg) return fail(OPD_EINVAL, me + "null configuration");
    if (cfg->struct_size != (int32_t)sizeof(opd_lwt_config))
        return fail(OPD_EINVAL, me + "struct_size " + std::to_string(cfg->struct_size) + ", this library's opd_lwt_config has " + std::to_string(sizeof(opd_lwt_config)) + " bytes");
    const opd_lwt_config& c = *cfg;
    const int S = c.max_tracks ? c.max_tracks : 256, NM = c.max_dets ? c.max_dets : 256;
    if (S < 1 || S > LWT_MAX_TRACKS) return fail(OPD_EINVAL, me + "max_tracks " + std::to_string(S) + " outside 1 .. 1024");
    if (NM < 1 || NM > LWT_MAX_DETS) return fail(OPD_EINVAL, me + "max_dets " + std::to_string(NM) + " outside 1 .. 1024");
    if (c.max_age < 0) return fail(OPD_EINVAL, me + "max_age must not be negative");
    // the reference's matching loop ends when the matrix's maximum is BELOW the threshold: with a threshold <= 0 an all-zero matrix never is
    if (!(c.iou_threshold >= 0.0)) return fail(OPD_EINVAL, me + "iou_threshold " + std::to_string(c.iou_threshold) + " must be positive (0 = 0.3)");
    RCCHK(use_device("opd_lwt_create", device_ordinal));
    std::unique_ptr<opd_lwt, decltype(&opd_lwt_destroy)> t(new opd_lwt(), opd_lwt_destroy);   // a failure below releases whatever was already made
    t->device = device_ordinal;
    t->S = S; t->NM = NM;
    t->max_age = c.max_age ? c.max_age : 30;
    t->thr = c.iou_threshold != 0.0 ? c.iou_threshold : 0.3;
    t->use_flow = c.use_optical_flow != 0;
    if (t->use_flow) {
        opd_flow_config fc = c.flow;
        fc.max_points = NM;
        RCCHK(opd_flow_create(&fc, device_ordinal, &t->flow));
    } else {
        RCCHK(made("opd_lwt_create", "stream creation", hipStreamCreateWithFlags(&t->own_stream, hipStreamNonBlocking)));
    }
    size_t off = 0;
    auto place = [&](size_t bytes) { const size_t o = off; off += align_up(bytes, 256); return o; };
    size_t bx[2], bP[2], bb[2], bc[2], bm[2];
    for (int k = 0; k < 2; ++k) {
        bx[k] = place((size_t)S * 32); bP[k] = place((size_t)S * 64); bb[k] = place((size_t)S * 16); bc[k] = place((size_t)S * 16);
        bm[k] = place((size_t)S * LWT_META * 4);
    }
    const size_t s_head = place(LWT_HEAD * 4), s_ndet = place(8), s_xy = place((size_t)NM * 8), s_id = place((size_t)NM * 4), s_pos = place((size_t)NM * 4);
    const size_t s_next = place((size_t)NM * 8), s_status = place((size_t)NM), s_iou = place((size_t)S * NM * 8);
    RCCHK(made("opd_lwt_create", "state allocation", hipMalloc((void**)&t->d_state, off)));
    RCCHK(made("opd_lwt_create", "state clearing", hipMemset(t->d_state, 0, off)));
    uint8_t* d = t->d_state;
    for (int k = 0; k < 2; ++k)
        t->bank[k] = LwtBank{reinterpret_cast<double*>(d + bx[k]), reinterpret_cast<float*>(d + bP[k]), reinterpret_cast<float*>(d + bb[k]),
                             reinterpret_cast<double*>(d + bc[k]), reinterpret_cast<int32_t*>(d + bm[k])};
    t->d_head = reinterpret_cast<int32_t*>(d + s_head);
    t->d_ndet = reinterpret_cast<int32_t*>(d + s_ndet);
    t->d_stop = t->d_ndet + 1;
    t->pts = LwtPoints{reinterpret_cast<float*>(d + s_xy), reinterpret_cast<int32_t*>(d + s_id), reinterpret_cast<int32_t*>(d + s_pos)};
    t->d_next = reinterpret_cast<float*>(d + s_next);
    t->d_status = d + s_status;
    t->d_iou = reinterpret_cast<double*>(d + s_iou);
    // the staging pair: boxes up; [head | ids] or [head | records] down; the scripted hook's [next | status] up
    off = 0;
    t->o_boxes = place((size_t)NM * 16);
    t->o_result = place(LWT_HEAD * 4 + std::max((size_t)NM * 4, (size_t)S * sizeof(LwtRec)));
    t->o_script = place((size_t)NM * 9);
    RCCHK(t->io.reserve("opd_lwt_create", off, off, t->stream()));
    memset(t->io.host, 0, off);
    RCCHK(write_head(t.get()));
    ++g_handle_epoch;   // device memory changed hands: graphs captured before are captured again (opd_device.h)
    *out = t.release();
    return OPD_OK;
}); }

extern "C" void opd_lwt_destroy(opd_lwt* t) { (void)api_call("opd_lwt_destroy", [&]() -> int {
    if (!t) return OPD_OK;
    (void)hipSetDevice(t->device);
    if (t->stream()) (void)hipStreamSynchronize(t->stream());
    if (t->flow) opd_flow_destroy(t->flow);
    if (t->own_stream) (void)hipStreamDestroy(t->own_stream);
    if (t->fused_ev) (void)hipEventDestroy(t->fused_ev);
    if (t->d_state) (void)hipFree(t->d_state);
    t->io.release();
    t->seq.release();
    delete t;
    ++g_handle_epoch;
    return OPD_OK;
}); }

extern "C" int opd_lwt_reset(opd_lwt* t) { return api_call("opd_lwt_reset", [&]() -> int {
    if (!t) return fail(OPD_EINVAL, "opd_lwt_reset: null handle");
    return write_head(t);   // (a new track initialises every number of its position: nothing else needs clearing)
}); }

extern "C" int opd_lwt_info(const opd_lwt* t, opd_lwt_status* info) { return api_call_unlocked("opd_lwt_info", [&]() -> int {
    if (!t || !info) return fail(OPD_EINVAL, "opd_lwt_info: null argument");
    *info = opd_lwt_status{t->S, t->NM, t->max_age, t->use_flow, t->device, t->n_tracks, t->next_id, t->n_points, t->last_launches, t->last_waits, t->thr};
    return OPD_OK;
}); }

extern "C" int opd_lwt_update(opd_lwt* t, const uint8_t* bgr, int mem_kind, int h, int w, const float* boxes_xywh, int n, int32_t* ids_out) { return api_call("opd_lwt_update", [&]() -> int {
    const std::string me = "opd_lwt_update: ";
    if (!t) return fail(OPD_EINVAL, me + "null handle");
    if (n < 0) return fail(OPD_EINVAL, me + "negative detection count");
    if (n > t->NM) return fail(OPD_EINVAL, me + std::to_string(n) + " detections, the handle was made for max_dets = " + std::to_string(t->NM));
    if (n > 0 && (!boxes_xywh || !ids_out)) return fail(OPD_EINVAL, me + "null boxes or output");
    RCCHK(check_lwt_frame(t, "opd_lwt_update", bgr));
    HIPCHK(hipSetDevice(t->device));
    hipStream_t s = t->stream();
    uint8_t *hst = t->io.host, *dev = t->io.dev;
    t->last_launches = t->last_waits = 0;
    int which = 0;
    RCCHK(lwt_enqueue_reference(t, s, "opd_lwt_update", bgr, mem_kind, h, w, &which));   // argument errors of the frame surface before anything is enqueued
    if (n) {
        memcpy(hst + t->o_boxes, boxes_xywh, (size_t)n * 16);
        HIPCHK(hipMemcpyAsync(dev + t->o_boxes, hst + t->o_boxes, (size_t)n * 16, hipMemcpyHostToDevice, s));
    }
    RCCHK(lwt_enqueue_update(t, s, n, nullptr));
    HIPCHK(hipMemcpyAsync(hst + t->o_result, dev + t->o_result, (size_t)(LWT_HEAD + n) * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    ++t->last_waits;
    RCCHK(lwt_adopt_update(t, "opd_lwt_update", which, n));
    if (n) memcpy(ids_out, reinterpret_cast<const int32_t*>(hst + t->o_result) + LWT_HEAD, (size_t)n * 4);
    return OPD_OK;
}); }

// The new reference frame is built into the pyramid the reference does not use and becomes the reference only at the adoption: an update
// that ends before it (a refused frame, a failed HIP call, the kernel's refusal) leaves the flow handle's reference as it was.
int lwt_enqueue_reference(opd_lwt* t, hipStream_t s, const char* who, const uint8_t* bgr, int mem_kind, int h, int w, int* which) {
    *which = t->flow ? 1 - t->flow->ref : 0;
    if (!t->flow) return OPD_OK;
    RCCHK(flow_enqueue_reference(t->flow, who, bgr, mem_kind, h, w, *which, s));
    t->last_launches += 1 + t->flow->pyr[*which].top;
    return OPD_OK;
}

// lwt_update_kernel from bank[cur] into the other one, the result to d_result; `stop`: the sticky word of a sequence call
static int launch_update(opd_lwt* t, hipStream_t s, int cur, int n, const int32_t* d_count, int32_t* d_result, int32_t* stop) {
    LwtUpdateParams p{};
    p.src = t->bank[cur]; p.dst = t->bank[1 - cur];
    p.head = t->d_head;
    p.dets = reinterpret_cast<const float*>(t->io.dev + t->o_boxes);
    p.N = n; p.max_tracks = t->S; p.max_age = t->max_age; p.use_flow = t->use_flow;
    p.count = d_count;
    p.stop = stop;
    p.thr = t->thr;
    p.iou = t->d_iou;
    p.result = d_result;
    p.pts = t->pts;
    HIPCHK(opd_launch_lwt_update(p, s));
    ++t->last_launches;
    return OPD_OK;
}

int lwt_enqueue_update(opd_lwt* t, hipStream_t s, int n, const int32_t* d_count) {
    return launch_update(t, s, t->cur, n, d_count, reinterpret_cast<int32_t*>(t->io.dev + t->o_result), nullptr);
}

int lwt_adopt_update(opd_lwt* t, const std::string& who, int which, int n) {
    const int32_t* r = reinterpret_cast<const int32_t*>(t->io.host + t->o_result);
    if (r[LWT_HEAD_ERROR])   // the kernel found no room for the new tracks and wrote nothing
        return fail(OPD_EINVAL, who + ": " + std::to_string(t->n_tracks) + " live tracks and the new ones of " + std::to_string(n) + " detections exceed max_tracks = " +
                                    std::to_string(t->S) + "; nothing was changed");
    read_head(t, t->io.host + t->o_result);
    t->cur = 1 - t->cur;
    if (t->flow) flow_finish_reference(t->flow, which);
    return OPD_OK;
}

// ---- the hybrid part of a fused detect call --------------------------------------------------------------------------------------------
int lwt_fused_check(const opd_lwt* t, int device, int Q, int h, int w, const std::string& who) {
    if (!t) return fail(OPD_EINVAL, who + ": null tracker handle");
    if (t->device != device) return fail(OPD_EINVAL, who + ": the detector is on device " + std::to_string(device) + ", a tracker on device " + std::to_string(t->device));
    if (t->NM < Q)
        return fail(OPD_EINVAL, who + ": a tracker made for max_dets = " + std::to_string(t->NM) + " cannot take the " + std::to_string(Q) + " records a frame may keep");
    if (t->flow && (h < 1 || w < 1 || h > t->flow->cfg.max_h || w > t->flow->cfg.max_w))
        return fail(OPD_EINVAL, who + ": frame of " + std::to_string(h) + " x " + std::to_string(w) + " pixels, a tracker was created for up to " +
                                    std::to_string(t->flow->cfg.max_h) + " x " + std::to_string(t->flow->cfg.max_w));
    return OPD_OK;
}

// the two orderings of a call that runs on the detector's stream `s`: behind what the handle's own stream has done (it is idle: its calls
// block), and the handle's own stream behind the call, so that a per-frame call afterwards sees a complete state
static int order_behind_own_stream(opd_lwt* t, hipStream_t s) {
    if (s == t->stream()) return OPD_OK;
    if (!t->fused_ev) HIPCHK(hipEventCreateWithFlags(&t->fused_ev, hipEventDisableTiming));
    HIPCHK(hipEventRecord(t->fused_ev, t->stream()));
    HIPCHK(hipStreamWaitEvent(s, t->fused_ev, 0));
    return OPD_OK;
}
static int order_own_stream_behind(opd_lwt* t, hipStream_t s) {
    if (s == t->stream()) return OPD_OK;
    HIPCHK(hipEventRecord(t->fused_ev, s));
    HIPCHK(hipStreamWaitEvent(t->stream(), t->fused_ev, 0));
    return OPD_OK;
}

int lwt_fused_enqueue(opd_lwt* t, hipStream_t s, const RecordView& frame, const uint8_t* d_bgr, int h, int w, const char* who) {
    RCCHK(order_behind_own_stream(t, s));
    t->last_launches = t->last_waits = 0;
    LwtIngestParams ip{frame, reinterpret_cast<float*>(t->io.dev + t->o_boxes), t->d_ndet};
    HIPCHK(opd_launch_lwt_ingest(ip, s));
    ++t->last_launches;
    RCCHK(lwt_enqueue_reference(t, s, who, d_bgr, OPD_MEM_DEVICE, h, w, &t->fused_which));
    return lwt_enqueue_update(t, s, frame.stride, t->d_ndet);
}

int lwt_fused_fetch(opd_lwt* t, hipStream_t s, int Q) {
    HIPCHK(hipMemcpyAsync(t->io.host + t->o_result, t->io.dev + t->o_result, (size_t)(LWT_HEAD + Q) * 4, hipMemcpyDeviceToHost, s));
    return order_own_stream_behind(t, s);
}

int lwt_fused_finish(opd_lwt* t, int n, int32_t* ids_out, const std::string& who) {
    const int rc = lwt_adopt_update(t, who, t->fused_which, n);
    const int32_t* r = reinterpret_cast<const int32_t*>(t->io.host + t->o_result);
    for (int i = 0; i < n; ++i) ids_out[i] = rc == OPD_OK ? r[LWT_HEAD + i] : -1;
    return rc;
}

// ---- a run of frames of one camera: key frames and in-between frames behind one wait -------------------------------------------------------
static size_t seq_recs_off() { return align_up(LWT_HEAD * 4, 8); }
// a frame's slot of the sequence staging: [head | ids [max_dets]] of a key frame, [head | recs [max_tracks]] of an in-between frame
static size_t seq_slot(const opd_lwt* t) { return align_up(seq_recs_off() + std::max((size_t)t->S * sizeof(LwtRec), (size_t)t->NM * 4), 8); }
static size_t seq_bytes(const opd_lwt* t) { return LWT_MAX_SEQUENCE * seq_slot(t); }   // (covers opd_lwt_interpolate_sequence's [head | recs [F][T]])

int lwt_sequence_check(const opd_lwt* t, const LwtSeqCall& c, int capacity, int device, const std::string& who) {
    RCCHK(lwt_fused_check(t, device, c.Q, c.h, c.w, who));
    if (capacity < t->S) return fail(OPD_EINVAL, who + ": capacity " + std::to_string(capacity) + " is below the tracker's max_tracks = " + std::to_string(t->S));
    bool seen_key = false;
    for (int f = 0; f < c.F; ++f) {
        if (!c.frames[f] && (c.is_key[f] || t->use_flow)) return fail(OPD_EINVAL, who + ": null frame pointer");
        // an in-between frame in front of the first key frame follows the points held at entry from the reference held at entry
        if (!c.is_key[f] && !seen_key && t->flow && t->n_points > 0) RCCHK(flow_check_track(t->flow, who.c_str(), c.frames[f], OPD_MEM_HOST, c.h, c.w, t->n_points));
        seen_key = seen_key || c.is_key[f];
    }
    return OPD_OK;
}

int lwt_sequence_enqueue(opd_lwt* t, hipStream_t s, const LwtSeqCall& c, const RecordView* view, const uint8_t* d_camera, const char* who) {
    RCCHK(t->seq.reserve(who, seq_bytes(t), seq_bytes(t), t->stream()));
    RCCHK(order_behind_own_stream(t, s));
    t->last_launches = t->last_waits = 0;
    HIPCHK(hipMemsetAsync(t->d_stop, 0, 4, s));
    if (t->flow) { t->seq_saved[0] = t->flow->pyr[0]; t->seq_saved[1] = t->flow->pyr[1]; }
    // what the host cannot know between the frames it assumes: every key frame is accepted (banks and pyramids alternate); the sticky word
    // turns whatever follows a refusal into nothing, and lwt_sequence_finish replays only what was accepted
    int ref = t->flow ? t->flow->ref : 0, cur = t->cur, k = 0;
    bool seen_key = false;
    const bool pts_entry = t->flow && t->n_points > 0;
    const size_t slot = seq_slot(t), frame_bytes = (size_t)c.h * c.w * 3;
    for (int f = 0; f < c.F; ++f) {
        uint8_t* d_slot = t->seq.dev + (size_t)f * slot;
        if (c.is_key[f]) {
            LwtIngestParams ip{record_frame(*view, k), reinterpret_cast<float*>(t->io.dev + t->o_boxes), t->d_ndet, t->d_stop};
            HIPCHK(opd_launch_lwt_ingest(ip, s));
            ++t->last_launches;
            if (t->flow) {
                RCCHK(flow_enqueue_reference(t->flow, who, d_camera + (size_t)k * frame_bytes, OPD_MEM_DEVICE, c.h, c.w, 1 - ref, s, t->d_stop));
                t->last_launches += 1 + t->flow->pyr[1 - ref].top;
                ref = 1 - ref;
            }
            RCCHK(launch_update(t, s, cur, c.Q, t->d_ndet, reinterpret_cast<int32_t*>(d_slot), t->d_stop));
            cur = 1 - cur;
            seen_key = true;
            ++k;
        } else {
            // no points at entry and no key frame yet: no frame is read, as in the per-frame call.  Behind a key frame the host no longer
            // knows, and the frame's pyramid is built whatever the device count says (which nothing can observe: opd_lwt_interpolate_sequence)
            const bool built = t->flow && (seen_key || pts_entry);
            if (built) {
                RCCHK(flow_enqueue_track_from(t->flow, ref, c.frames[f], OPD_MEM_HOST, c.h, c.w, true, nullptr, seen_key ? c.Q : t->n_points,
                                              t->d_head + LWT_HEAD_POINTS, t->pts.xy, t->d_next, t->d_status, s, t->d_stop));
                t->last_launches += 2 + t->flow->pyr[ref].top;
                ref = 1 - ref;
            }
            RCCHK(launch_interp(t, s, cur, built, reinterpret_cast<int32_t*>(d_slot), reinterpret_cast<LwtRec*>(d_slot + seq_recs_off()), t->d_stop));
        }
    }
    return OPD_OK;
}

int lwt_sequence_fetch(opd_lwt* t, hipStream_t s, int F) {
    HIPCHK(hipMemcpyAsync(t->seq.host, t->seq.dev, (size_t)F * seq_slot(t), hipMemcpyDeviceToHost, s));
    return order_own_stream_behind(t, s);
}

int lwt_sequence_finish(opd_lwt* t, const LwtSeqCall& c, const int32_t* key_counts, int32_t* track_ids, opd_lwt_rec* recs_out, int capacity, int32_t* rec_counts,
                        int32_t* frames_done, const std::string& who) {
    // the pyramids as the call found them; a frame that was accepted puts the geometry the enqueue planned for its slot back, and its finish
    FlowPyramid planned[2];
    if (t->flow)
        for (int i = 0; i < 2; ++i) { planned[i] = t->flow->pyr[i]; t->flow->pyr[i] = t->seq_saved[i]; }
    const bool pts_entry = t->flow && t->n_points > 0;
    const size_t slot = seq_slot(t);
    bool stopped = false, seen_key = false;
    int k = 0, j = 0, rc = OPD_OK;
    *frames_done = c.F;
    for (int f = 0; f < c.F; ++f) {
        const uint8_t* h_slot = t->seq.host + (size_t)f * slot;
        const int32_t* r = reinterpret_cast<const int32_t*>(h_slot);
        if (c.is_key[f]) {
            const int n = std::max(0, std::min(key_counts[k], c.Q));
            int32_t* ids = track_ids + (size_t)k * c.Q;
            if (!stopped && r[LWT_HEAD_ERROR]) {   // the kernel found no room for the new tracks, wrote nothing and raised the sticky word
                stopped = true;
                *frames_done = f + 1;
                rc = fail(OPD_EINVAL, who + ": frame " + std::to_string(f) + ": " + std::to_string(t->n_tracks) + " live tracks and the new ones of " + std::to_string(n) +
                                          " detections exceed max_tracks = " + std::to_string(t->S) + "; the tracker is as the frame before left it");
            }
            if (stopped) {
                for (int i = 0; i < n; ++i) ids[i] = -1;
            } else {
                read_head(t, h_slot);
                t->cur = 1 - t->cur;
                if (t->flow) {
                    const int which = 1 - t->flow->ref;
                    t->flow->pyr[which] = planned[which];
                    flow_finish_reference(t->flow, which);
                }
                for (int i = 0; i < n; ++i) ids[i] = r[LWT_HEAD + i];
            }
            seen_key = true;
            ++k;
        } else {
            if (stopped) {
                rec_counts[j] = 0;
            } else {
                const int T = t->n_tracks;   // (an in-between frame neither makes nor drops a track)
                rec_counts[j] = T;
                if (T) memcpy(recs_out + (size_t)j * capacity, h_slot + seq_recs_off(), (size_t)T * sizeof(LwtRec));
                read_head(t, h_slot);
                if (t->flow && (seen_key || pts_entry)) {
                    const int which = 1 - t->flow->ref;
                    t->flow->pyr[which] = planned[which];
                    flow_finish_track(t->flow);
                }
            }
            ++j;
        }
    }
    return rc;
}

// the second half of an in-between frame: LK's results (with_points) lie at d_next / d_status, ordered on the stream before this
static int launch_interp(opd_lwt* t, hipStream_t s, int cur, bool with_points, int32_t* d_result, LwtRec* d_recs, const int32_t* stop) {
    LwtInterpParams p{};
    p.s = t->bank[cur];
    p.head = t->d_head;
    p.next = with_points ? t->d_next : nullptr;
    p.status = t->d_status;
    p.pts = t->pts;
    p.result = d_result;
    p.recs = d_recs;
    p.stop = stop;
    HIPCHK(opd_launch_lwt_interp(p, s));
    ++t->last_launches;
    return OPD_OK;
}

int lwt_enqueue_interp(opd_lwt* t, bool with_points, int32_t* d_result, LwtRec* d_recs) {
    return launch_interp(t, t->stream(), t->cur, with_points, d_result, d_recs, nullptr);
}

int lwt_interp_finish(opd_lwt* t, bool with_points, LwtRec* recs_out, int* count) {
    hipStream_t s = t->stream();
    uint8_t *hst = t->io.host, *dev = t->io.dev;
    const size_t o_recs = t->o_result + align_up(LWT_HEAD * 4, 8);
    RCCHK(lwt_enqueue_interp(t, with_points, reinterpret_cast<int32_t*>(dev + t->o_result), reinterpret_cast<LwtRec*>(dev + o_recs)));
    const int T = t->n_tracks;
    HIPCHK(hipMemcpyAsync(hst + t->o_result, dev + t->o_result, (o_recs - t->o_result) + (size_t)T * sizeof(LwtRec), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    ++t->last_waits;
    read_head(t, hst + t->o_result);
    *count = T;
    if (T) memcpy(recs_out, hst + o_recs, (size_t)T * sizeof(LwtRec));
    return OPD_OK;
}

extern "C" int opd_lwt_interpolate(opd_lwt* t, const uint8_t* bgr, int mem_kind, int h, int w, opd_lwt_rec* recs_out, int capacity, int* count) { return api_call("opd_lwt_interpolate", [&]() -> int {
    const std::string me = "opd_lwt_interpolate: ";
    if (!t || !count) return fail(OPD_EINVAL, me + "null argument");
    *count = t->n_tracks;
    if (capacity < t->n_tracks || (t->n_tracks > 0 && !recs_out))
        return fail(OPD_EINVAL, me + std::to_string(t->n_tracks) + " tracks, room for " + std::to_string(capacity < 0 || !recs_out ? 0 : capacity));
    RCCHK(check_lwt_frame(t, "opd_lwt_interpolate", bgr));
    HIPCHK(hipSetDevice(t->device));
    t->last_launches = t->last_waits = 0;
    // `OpticalFlowTracker.track` without points returns before it looks at the frame: the reference frame stays what it was
    const bool with_points = t->flow && t->n_points > 0;
    if (with_points) {
        RCCHK(flow_enqueue_track(t->flow, "opd_lwt_interpolate", bgr, mem_kind, h, w, nullptr, t->n_points, t->pts.xy, t->d_next, t->d_status));
        t->last_launches += 2 + t->flow->pyr[t->flow->ref].top;
    }
    static_assert(sizeof(LwtRec) == sizeof(opd_lwt_rec), "record layout");
    RCCHK(lwt_interp_finish(t, with_points, reinterpret_cast<LwtRec*>(recs_out), count));
    if (with_points) flow_finish_track(t->flow);
    return OPD_OK;
}); }

// F in-between frames behind one wait.  The host's mirrors are those of the entry: n_tracks holds throughout (an in-between frame neither
// makes nor drops a track), n_points only falls, so it bounds every LK launch and the device-resident count decides which waves work.
extern "C" int opd_lwt_interpolate_sequence(opd_lwt* t, const uint8_t* const* frames, int mem_kind, int F, int h, int w, opd_lwt_rec* recs_out, int capacity, int32_t* counts) { return api_call("opd_lwt_interpolate_sequence", [&]() -> int {
    const std::string me = "opd_lwt_interpolate_sequence: ";
    if (F < 1 || F > LWT_MAX_SEQUENCE) return fail(OPD_EINVAL, me + std::to_string(F) + " frames, a call takes 1 .. " + std::to_string(LWT_MAX_SEQUENCE));
    if (capacity < 1) return fail(OPD_EINVAL, me + "capacity " + std::to_string(capacity) + " is below the handle's max_tracks");
    if (!t || !counts) return fail(OPD_EINVAL, me + "null handle or counts");
    if (capacity < t->S)
        return fail(OPD_EINVAL, me + "capacity " + std::to_string(capacity) + " is below the handle's max_tracks = " + std::to_string(t->S));
    const int T = t->n_tracks;
    if (T > 0 && !recs_out) return fail(OPD_EINVAL, me + std::to_string(T) + " tracks, null records");
    if (t->use_flow) {
        if (!frames) return fail(OPD_EINVAL, me + "null frame list (the handle was made with use_optical_flow)");
        for (int f = 0; f < F; ++f) RCCHK(check_lwt_frame(t, "opd_lwt_interpolate_sequence", frames[f]));
    }
    // without points at entry no frame is looked at, as in the per-frame call: none of them can gain a point
    const bool with_points = t->flow && t->n_points > 0;
    if (with_points)
        for (int f = 0; f < F; ++f) RCCHK(flow_check_track(t->flow, "opd_lwt_interpolate_sequence", frames[f], mem_kind, h, w, t->n_points));
    HIPCHK(hipSetDevice(t->device));
    hipStream_t s = t->stream();
    static_assert(sizeof(LwtRec) == sizeof(opd_lwt_rec), "record layout");
    const size_t o_recs = seq_recs_off();
    RCCHK(t->seq.reserve("opd_lwt_interpolate_sequence", seq_bytes(t), seq_bytes(t), s));
    t->last_launches = t->last_waits = 0;
    int ref = t->flow ? t->flow->ref : 0;
    for (int f = 0; f < F; ++f) {
        if (with_points) {   // the pyramids alternate; a frame that finds no point left still builds its own, which nothing reads afterwards
            RCCHK(flow_enqueue_track_from(t->flow, ref, frames[f], mem_kind, h, w, true, nullptr, t->n_points, t->d_head + LWT_HEAD_POINTS, t->pts.xy,
                                          t->d_next, t->d_status));
            t->last_launches += 2 + t->flow->pyr[ref].top;
            ref = 1 - ref;
        }
        RCCHK(lwt_enqueue_interp(t, with_points, reinterpret_cast<int32_t*>(t->seq.dev), reinterpret_cast<LwtRec*>(t->seq.dev + o_recs) + (size_t)f * T));
    }
    HIPCHK(hipMemcpyAsync(t->seq.host, t->seq.dev, o_recs + (size_t)F * T * sizeof(LwtRec), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    ++t->last_waits;
    read_head(t, t->seq.host);   // the last frame's
    for (int f = 0; f < F; ++f) {
        counts[f] = T;
        if (T) memcpy(recs_out + (size_t)f * capacity, t->seq.host + o_recs + (size_t)f * T * sizeof(LwtRec), (size_t)T * sizeof(LwtRec));
    }
    if (with_points) flow_finish_sequence(t->flow, F);
    return OPD_OK;
}); }

extern "C" int opd_lwt_get(opd_lwt* t, opd_lwt_track* out, int capacity, int* count) { return api_call("opd_lwt_get", [&]() -> int {
    if (!t || !count) return fail(OPD_EINVAL, "opd_lwt_get: null argument");
    const int T = t->n_tracks;
    *count = T;
    if (!out && capacity == 0) return OPD_OK;
    if (!out || capacity < T) return fail(OPD_EINVAL, "opd_lwt_get: " + std::to_string(T) + " tracks, room for " + std::to_string(capacity));
    if (T == 0) return OPD_OK;
    HIPCHK(hipSetDevice(t->device));
    const LwtBank& b = t->bank[t->cur];
    std::vector<double> x((size_t)T * 4), c((size_t)T * 2);
    std::vector<float> P((size_t)T * 16), box((size_t)T * 4);
    std::vector<int32_t> m((size_t)T * LWT_META);
    hipStream_t s = t->stream();
    HIPCHK(hipMemcpyAsync(x.data(), b.x, x.size() * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(c.data(), b.center, c.size() * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(P.data(), b.P, P.size() * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(box.data(), b.bbox, box.size() * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(m.data(), b.meta, m.size() * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    for (int i = 0; i < T; ++i) {
        opd_lwt_track& o = out[i];
        const int32_t* mi = m.data() + (size_t)LWT_META * i;
        o.track_id = mi[LWT_ID]; o.age = mi[LWT_AGE]; o.hits = mi[LWT_HITS]; o.time_since_update = mi[LWT_TSU]; o.x_is_float32 = mi[LWT_F32]; o.reserved = 0;
        for (int j = 0; j < 4; ++j) { o.bbox[j] = box[4 * (size_t)i + j]; o.x[j] = x[4 * (size_t)i + j]; }
        o.center[0] = c[2 * (size_t)i]; o.center[1] = c[2 * (size_t)i + 1];
        memcpy(o.P, P.data() + 16 * (size_t)i, 64);
    }
    return OPD_OK;
}); }
