// opd_lwt.cpp — the hybrid-tracker handle of include/opd_detr.h (opd_lwt_*): the reference's `LightweightTracker` with every track number on
// the device.  `opd_lwt_update` stages the boxes, enqueues their upload, lwt_update_kernel, (with optical flow) the gray and pyramid
// launches of the new reference frame and the download of [head | ids], and waits once.  `opd_lwt_interpolate` enqueues gray + pyramid +
// LK on the points the device holds, lwt_interp_kernel on LK's results where they lie, and the download of [head | records], and waits
// once.  The host keeps three mirrors (tracks, next id, flow points) that the one wait of every call refreshes: they size the next
// call's launches and checks.  Nothing here computes on a track.
#include <string.h>

#include <algorithm>
#include <memory>
#include <string>

#include "opd_lwt.h"

using namespace opd;

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

void read_head(opd_lwt* t) {
    const int32_t* r = reinterpret_cast<const int32_t*>(t->io.host + t->o_result);
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
    const size_t s_head = place(LWT_HEAD * 4), s_xy = place((size_t)NM * 8), s_id = place((size_t)NM * 4), s_pos = place((size_t)NM * 4);
    const size_t s_next = place((size_t)NM * 8), s_status = place((size_t)NM), s_iou = place((size_t)S * NM * 8);
    RCCHK(made("opd_lwt_create", "state allocation", hipMalloc((void**)&t->d_state, off)));
    RCCHK(made("opd_lwt_create", "state clearing", hipMemset(t->d_state, 0, off)));
    uint8_t* d = t->d_state;
    for (int k = 0; k < 2; ++k)
        t->bank[k] = LwtBank{reinterpret_cast<double*>(d + bx[k]), reinterpret_cast<float*>(d + bP[k]), reinterpret_cast<float*>(d + bb[k]),
                             reinterpret_cast<double*>(d + bc[k]), reinterpret_cast<int32_t*>(d + bm[k])};
    t->d_head = reinterpret_cast<int32_t*>(d + s_head);
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
    if (t->d_state) (void)hipFree(t->d_state);
    t->io.release();
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
    // The new reference frame is built into the pyramid the reference does not use and becomes the reference only at the finish: an update
    // that ends before it (a refused frame, a failed HIP call, the kernel's refusal) leaves the flow handle's reference as it was.
    const int which = t->flow ? 1 - t->flow->ref : 0;
    if (t->flow) {   // argument errors of the frame surface before anything is enqueued
        RCCHK(flow_enqueue_reference(t->flow, "opd_lwt_update", bgr, mem_kind, h, w, which));
        t->last_launches += 1 + t->flow->pyr[which].top;
    }
    if (n) {
        memcpy(hst + t->o_boxes, boxes_xywh, (size_t)n * 16);
        HIPCHK(hipMemcpyAsync(dev + t->o_boxes, hst + t->o_boxes, (size_t)n * 16, hipMemcpyHostToDevice, s));
    }
    LwtUpdateParams p{};
    p.src = t->bank[t->cur]; p.dst = t->bank[1 - t->cur];
    p.head = t->d_head;
    p.dets = reinterpret_cast<const float*>(dev + t->o_boxes);
    p.N = n; p.max_tracks = t->S; p.max_age = t->max_age; p.use_flow = t->use_flow;
    p.thr = t->thr;
    p.iou = t->d_iou;
    p.result = reinterpret_cast<int32_t*>(dev + t->o_result);
    p.pts = t->pts;
    HIPCHK(opd_launch_lwt_update(p, s));
    ++t->last_launches;
    HIPCHK(hipMemcpyAsync(hst + t->o_result, dev + t->o_result, (size_t)(LWT_HEAD + n) * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    ++t->last_waits;
    const int32_t* r = reinterpret_cast<const int32_t*>(hst + t->o_result);
    if (r[LWT_HEAD_ERROR])   // the kernel found no room for the new tracks and wrote nothing
        return fail(OPD_EINVAL, me + std::to_string(t->n_tracks) + " live tracks and the new ones of " + std::to_string(n) + " detections exceed max_tracks = " +
                                    std::to_string(t->S) + "; nothing was changed");
    read_head(t);
    t->cur = 1 - t->cur;
    if (t->flow) flow_finish_reference(t->flow, which);
    if (n) memcpy(ids_out, r + LWT_HEAD, (size_t)n * 4);
    return OPD_OK;
}); }

// the second half of an in-between frame: LK's results (with_points) lie at d_next / d_status, ordered on the stream before this
int lwt_interp_finish(opd_lwt* t, bool with_points, LwtRec* recs_out, int* count) {
    hipStream_t s = t->stream();
    uint8_t *hst = t->io.host, *dev = t->io.dev;
    const size_t o_recs = t->o_result + align_up(LWT_HEAD * 4, 8);
    LwtInterpParams p{};
    p.s = t->bank[t->cur];
    p.head = t->d_head;
    p.next = with_points ? t->d_next : nullptr;
    p.status = t->d_status;
    p.pts = t->pts;
    p.result = reinterpret_cast<int32_t*>(dev + t->o_result);
    p.recs = reinterpret_cast<LwtRec*>(dev + o_recs);
    HIPCHK(opd_launch_lwt_interp(p, s));
    ++t->last_launches;
    const int T = t->n_tracks;
    HIPCHK(hipMemcpyAsync(hst + t->o_result, dev + t->o_result, (o_recs - t->o_result) + (size_t)T * sizeof(LwtRec), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    ++t->last_waits;
    read_head(t);
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
