// opd_flow.cpp — the optical-flow handle of include/opd_detr.h (opd_flow_*): two gray pyramids on the device that swap roles after every
// track call (`prev_gray = gray`), a stream, and one page-locked staging buffer.  A call stages the points (and a host frame) in it,
// enqueues the uploads, gray + pyramid + the one-wave-per-point LK launch of kernels_flow.hip and the download, and waits once.
#include <string.h>

#include <algorithm>
#include <memory>
#include <string>

#include "opd_flow.h"
#include "opd_kernels.h"

using namespace opd;

namespace {

// the frame size of `p` and its levels; the effective top level is the largest l <= max_level with every level 1 .. l wider and taller than the window
void plan_levels(FlowPyramid* p, int h, int w, int win, int max_level) {
    p->h = h; p->w = w;
    p->lh[0] = h; p->lw[0] = w; p->lp[0] = flow_pitch(w);
    p->top = 0;
    for (int l = 1; l <= max_level; ++l) {
        const int nh = (p->lh[l - 1] + 1) / 2, nw = (p->lw[l - 1] + 1) / 2;
        if (nh <= win || nw <= win) break;
        p->lh[l] = nh; p->lw[l] = nw; p->lp[l] = flow_pitch(nw);
        p->top = l;
    }
}

int check_frame(opd_flow* f, const char* who, const uint8_t* bgr, int mem_kind, int h, int w) {
    const std::string me(who);
    if (!f) return fail(OPD_EINVAL, me + ": null handle");
    if (!bgr) return fail(OPD_EINVAL, me + ": null frame pointer");
    if (mem_kind != OPD_MEM_HOST && mem_kind != OPD_MEM_DEVICE) return fail(OPD_EINVAL, me + ": mem_kind must be OPD_MEM_HOST or OPD_MEM_DEVICE");
    if (h < 1 || w < 1 || h > f->cfg.max_h || w > f->cfg.max_w)
        return fail(OPD_EINVAL, me + ": frame of " + std::to_string(h) + " x " + std::to_string(w) + " pixels, the handle was created for up to " +
                                    std::to_string(f->cfg.max_h) + " x " + std::to_string(f->cfg.max_w));
    if (mem_kind == OPD_MEM_DEVICE) {
        HIPCHK(hipSetDevice(f->device));
        if (!device_accessible(bgr)) return fail(OPD_EINVAL, me + ": OPD_MEM_DEVICE, but the frame is not device-accessible memory");
    }
    return OPD_OK;
}

// gray + pyramid of `bgr` into pyr[which] (whose levels are planned for h x w), enqueued on the handle's stream.  The `pts_bytes` of points the caller has put at the head of the
// staging image and a host frame (behind the points region) travel as two copies of exactly their bytes on the same stream.  `in_place`:
// the host frame is uploaded from where it lies, not through the staging image (which holds one frame: a caller that enqueues several
// frames before it waits cannot reuse it; the device side can be reused, the stream orders the upload behind the gray launch before it).
// `on`: another stream than the handle's (the detector's, in a fused detect call, which has ordered itself against the handle's).
int enqueue_pyramid(opd_flow* f, int which, const uint8_t* bgr, int mem_kind, int h, int w, size_t pts_bytes, bool in_place = false, hipStream_t on = nullptr,
                    const int32_t* stop = nullptr) {
    hipStream_t s = on ? on : f->stream;
    const uint8_t* d_bgr = bgr;
    if (pts_bytes) HIPCHK(hipMemcpyAsync(f->io.dev, f->io.host, pts_bytes, hipMemcpyHostToDevice, s));
    if (mem_kind == OPD_MEM_HOST) {
        const size_t bytes = (size_t)h * w * 3;
        if (!in_place) memcpy(f->io.host + f->frame_off, bgr, bytes);
        d_bgr = f->io.dev + f->frame_off;
        HIPCHK(hipMemcpyAsync(f->io.dev + f->frame_off, in_place ? bgr : f->io.host + f->frame_off, bytes, hipMemcpyHostToDevice, s));
    }
    const FlowPyramid& p = f->pyr[which];
    HIPCHK(opd_launch_flow_gray(d_bgr, p.base + p.off[0], h, w, p.lp[0], s, stop));
    for (int l = 1; l <= p.top; ++l)
        HIPCHK(opd_launch_flow_pyrdown(p.base + p.off[l - 1], p.lh[l - 1], p.lw[l - 1], p.lp[l - 1], p.base + p.off[l], p.lp[l], s, stop));
    return OPD_OK;
}

}  // namespace

extern "C" int opd_flow_create(const opd_flow_config* cfg, int device_ordinal, opd_flow** out) { return api_call("opd_flow_create", [&]() -> int {
    if (!cfg || !out) return fail(OPD_EINVAL, "opd_flow_create: null argument");
    *out = nullptr;
    opd_flow_config c = *cfg;
    if (c.win == 0) c.win = 21;
    if (c.max_level == 0) c.max_level = 3;
    if (c.max_iter == 0) c.max_iter = 30;
    if (c.epsilon == 0.f) c.epsilon = 0.01f;
    if (c.min_eig_threshold == 0.f) c.min_eig_threshold = 1e-4f;
    if (c.max_h < 1 || c.max_w < 1 || c.max_h > 8192 || c.max_w > 8192) return fail(OPD_EINVAL, "opd_flow_create: max_h and max_w must lie in 1 .. 8192");
    if (c.max_points < 1 || c.max_points > (1 << 20)) return fail(OPD_EINVAL, "opd_flow_create: max_points must lie in 1 .. 1048576");
    if (c.win < 3 || c.win > OPD_FLOW_MAX_WIN || c.win % 2 == 0)
        return fail(OPD_EINVAL, "opd_flow_create: win = " + std::to_string(c.win) + ", the window edge must be odd and lie in 3 .. 21");
    if (c.max_level < 0 || c.max_level >= OPD_FLOW_MAX_LEVELS) return fail(OPD_EINVAL, "opd_flow_create: max_level must lie in 0 .. 7");
    if (c.max_iter < 1 || c.max_iter > 1000) return fail(OPD_EINVAL, "opd_flow_create: max_iter must lie in 1 .. 1000");
    if (!(c.min_eig_threshold > 0.f)) return fail(OPD_EINVAL, "opd_flow_create: min_eig_threshold must be positive");
    RCCHK(use_device("opd_flow_create", device_ordinal));
    std::unique_ptr<opd_flow, decltype(&opd_flow_destroy)> f(new opd_flow(), opd_flow_destroy);   // a failure below releases whatever was already made
    f->cfg = c;
    f->device = device_ordinal;
    // the largest pyramid: level sizes fall with the frame size, so offsets planned for max_h x max_w hold every smaller frame
    int lh[OPD_FLOW_MAX_LEVELS], lw[OPD_FLOW_MAX_LEVELS], lp[OPD_FLOW_MAX_LEVELS];
    size_t bytes = 0, off[OPD_FLOW_MAX_LEVELS] = {};
    lh[0] = c.max_h; lw[0] = c.max_w;
    for (int l = 0; l <= c.max_level; ++l) {
        if (l) { lh[l] = (lh[l - 1] + 1) / 2; lw[l] = (lw[l - 1] + 1) / 2; }
        lp[l] = flow_pitch(lw[l]);
        off[l] = bytes;
        bytes += align_up((size_t)lp[l] * lh[l], 256);
    }
    f->pts_bytes = align_up((size_t)c.max_points * 8, 256);
    f->frame_off = f->pts_bytes;
    f->out_off = f->frame_off + align_up((size_t)c.max_h * c.max_w * 3, 256);
    const size_t io_bytes = f->out_off + align_up((size_t)c.max_points * 9, 256);
    RCCHK(made("opd_flow_create", "stream creation", hipStreamCreateWithFlags(&f->stream, hipStreamNonBlocking)));
    for (int k = 0; k < 2; ++k) {
        RCCHK(made("opd_flow_create", "pyramid allocation", hipMalloc((void**)&f->pyr[k].base, bytes)));
        memcpy(f->pyr[k].off, off, sizeof off);
    }
    RCCHK(f->io.reserve("opd_flow_create", io_bytes, io_bytes, f->stream));   // sized once: the handle's maxima bound every call
    *out = f.release();
    return OPD_OK;
}); }

extern "C" void opd_flow_destroy(opd_flow* f) { (void)api_call("opd_flow_destroy", [&]() -> int {
    if (!f) return OPD_OK;
    (void)hipSetDevice(f->device);
    if (f->stream) { (void)hipStreamSynchronize(f->stream); (void)hipStreamDestroy(f->stream); }
    for (int k = 0; k < 2; ++k) if (f->pyr[k].base) (void)hipFree(f->pyr[k].base);
    f->io.release();
    delete f;
    return OPD_OK;
}); }

// ---- the two entry points in halves: everything up to the wait (enqueue) and what follows it (finish).  opd_lwt.cpp puts launches of its
//      own on the handle's stream between the two and waits itself.
int opd::flow_enqueue_reference(opd_flow* f, const char* who, const uint8_t* bgr, int mem_kind, int h, int w, int which, hipStream_t on, const int32_t* stop) {
    RCCHK(check_frame(f, who, bgr, mem_kind, h, w));
    HIPCHK(hipSetDevice(f->device));
    f->pyr[which].valid = false;   // (which == ref: a failure below leaves no reference)
    plan_levels(&f->pyr[which], h, w, f->cfg.win, f->cfg.max_level);
    return enqueue_pyramid(f, which, bgr, mem_kind, h, w, 0, false, on, stop);
}

void opd::flow_finish_reference(opd_flow* f, int which) {
    f->ref = which;
    f->pyr[which].valid = true;
}

int opd::flow_check_track(opd_flow* f, const char* who, const uint8_t* bgr, int mem_kind, int h, int w, int n) {
    const std::string me(who);
    RCCHK(check_frame(f, who, bgr, mem_kind, h, w));
    if (n < 0 || n > f->cfg.max_points)
        return fail(OPD_EINVAL, me + ": " + std::to_string(n) + " points, the handle was created for up to " + std::to_string(f->cfg.max_points));
    const FlowPyramid& ref = f->pyr[f->ref];
    if (!ref.valid) return fail(OPD_ESTATE, me + ": no reference frame yet (call opd_flow_set_reference first)");
    if (h != ref.h || w != ref.w)
        return fail(OPD_EINVAL, me + ": frame of " + std::to_string(h) + " x " + std::to_string(w) + " pixels, the reference has " +
                                    std::to_string(ref.h) + " x " + std::to_string(ref.w));
    return OPD_OK;
}

int opd::flow_enqueue_track_from(opd_flow* f, int ref_slot, const uint8_t* bgr, int mem_kind, int h, int w, bool in_place, const float* host_pts, int n,
                                 const int32_t* d_count, const float* d_pts, float* d_next, uint8_t* d_status, hipStream_t on, const int32_t* stop) {
    HIPCHK(hipSetDevice(f->device));
    const FlowPyramid& ref = f->pyr[ref_slot];
    const int cur = 1 - ref_slot;
    f->pyr[cur].valid = false;
    plan_levels(&f->pyr[cur], h, w, f->cfg.win, f->cfg.max_level);   // (the reference's size: the same levels)
    const size_t pts_bytes = host_pts ? (size_t)n * 8 : 0;
    if (pts_bytes) memcpy(f->io.host, host_pts, pts_bytes);
    RCCHK(enqueue_pyramid(f, cur, bgr, mem_kind, h, w, pts_bytes, in_place, on, stop));
    if (n) {
        FlowParams p{};
        for (int l = 0; l <= ref.top; ++l)
            p.lv[l] = FlowLevel{ref.base + ref.off[l], f->pyr[cur].base + f->pyr[cur].off[l], ref.lw[l], ref.lh[l], ref.lp[l]};
        p.top = ref.top;
        p.n = n;
        p.win = f->cfg.win;
        p.max_iter = f->cfg.max_iter;
        p.eps2 = f->cfg.epsilon < 0.f ? -1.f : f->cfg.epsilon * f->cfg.epsilon;
        p.min_eig = f->cfg.min_eig_threshold;
        p.pts = d_pts;
        p.next = d_next;
        p.status = d_status;
        p.count = d_count;
        p.stop = stop;
        HIPCHK(opd_launch_flow_lk(p, on ? on : f->stream));
    }
    return OPD_OK;
}

int opd::flow_enqueue_track(opd_flow* f, const char* who, const uint8_t* bgr, int mem_kind, int h, int w, const float* host_pts, int n, const float* d_pts,
                            float* d_next, uint8_t* d_status) {
    RCCHK(flow_check_track(f, who, bgr, mem_kind, h, w, n));
    return flow_enqueue_track_from(f, f->ref, bgr, mem_kind, h, w, false, host_pts, n, nullptr, d_pts, d_next, d_status);
}

void opd::flow_finish_track(opd_flow* f) {
    f->ref = 1 - f->ref;   // the frame just seen is the reference of the next call; the old reference stays valid behind it
    f->pyr[f->ref].valid = true;
}

void opd::flow_finish_sequence(opd_flow* f, int frames) {
    f->ref = (f->ref + frames) & 1;   // the last frame is the reference; the other pyramid holds the frame before it
    f->pyr[0].valid = f->pyr[1].valid = true;
}

extern "C" int opd_flow_set_reference(opd_flow* f, const uint8_t* bgr, int mem_kind, int h, int w) { return api_call("opd_flow_set_reference", [&]() -> int {
    RCCHK(flow_enqueue_reference(f, "opd_flow_set_reference", bgr, mem_kind, h, w, f ? f->ref : 0));
    HIPCHK(hipStreamSynchronize(f->stream));
    flow_finish_reference(f, f->ref);
    return OPD_OK;
}); }

extern "C" int opd_flow_track(opd_flow* f, const uint8_t* bgr, int mem_kind, int h, int w, const float* pts_xy, int n, float* next_xy,
                              uint8_t* status) { return api_call("opd_flow_track", [&]() -> int {
    RCCHK(check_frame(f, "opd_flow_track", bgr, mem_kind, h, w));
    if (n < 0 || n > f->cfg.max_points)
        return fail(OPD_EINVAL, "opd_flow_track: " + std::to_string(n) + " points, the handle was created for up to " + std::to_string(f->cfg.max_points));
    if (n > 0 && (!pts_xy || !next_xy || !status)) return fail(OPD_EINVAL, "opd_flow_track: null point, result or status buffer");
    const size_t pts_bytes = (size_t)n * 8;
    RCCHK(flow_enqueue_track(f, "opd_flow_track", bgr, mem_kind, h, w, n ? pts_xy : nullptr, n, reinterpret_cast<const float*>(f->io.dev),
                             reinterpret_cast<float*>(f->io.dev + f->out_off), f->io.dev + f->out_off + pts_bytes));
    if (n) HIPCHK(hipMemcpyAsync(f->io.host + f->out_off, f->io.dev + f->out_off, pts_bytes + (size_t)n, hipMemcpyDeviceToHost, f->stream));
    HIPCHK(hipStreamSynchronize(f->stream));
    if (n) {
        memcpy(next_xy, f->io.host + f->out_off, pts_bytes);
        memcpy(status, f->io.host + f->out_off + pts_bytes, (size_t)n);
    }
    flow_finish_track(f);
    return OPD_OK;
}); }
