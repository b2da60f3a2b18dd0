// opd_color.cpp — opd_color_features (include/opd_detr.h): colour-histogram appearance features of boxes on frames, without a model
// handle.  The host plans one ColorCrop per box (opd_kernels.h: the reference's crop rule), uploads descriptors and -- for host frames --
// pixels in ONE transfer, and kernels_hist.hip does the rest; one host wait.  Per device: a stream and a staging pair (page-locked host
// image + device buffer) that grow on demand and live as long as the process, so a call per video frame allocates nothing.
#include <string.h>

#include <algorithm>
#include <mutex>
#include <string>
#include <vector>

#include "opd_device.h"
#include "opd_kernels.h"

using namespace opd;

namespace {

struct ColorScratch {
    std::mutex mu;   // one call at a time per device
    hipStream_t stream = nullptr;
    Staging io;      // up: [descriptors | pixels]; the device side holds the accumulators and the output behind them
};
ColorScratch g_scratch[16];   // one node: <= 16 GPUs

}  // namespace

extern "C" int opd_color_features(int device_ordinal, const uint8_t* const* frames, const int32_t* frame_hw, int n_frames, int mem_kind,
                                  const float* boxes_xywh, const int32_t* box_frame, int n_boxes, float* out) { return api_call("opd_color_features", [&]() -> int {
    if (n_boxes < 0) return fail(OPD_EINVAL, "opd_color_features: negative box count");
    if (n_boxes == 0) return OPD_OK;
    if (!frames || !frame_hw || !boxes_xywh || !out || n_frames < 1) return fail(OPD_EINVAL, "opd_color_features: null argument or no frames");
    if (mem_kind != OPD_MEM_HOST && mem_kind != OPD_MEM_DEVICE) return fail(OPD_EINVAL, "opd_color_features: mem_kind must be OPD_MEM_HOST or OPD_MEM_DEVICE");
    for (int f = 0; f < n_frames; ++f) {
        const int H = frame_hw[2 * f], W = frame_hw[2 * f + 1];
        if (!frames[f] || H < 1 || W < 1) return fail(OPD_EINVAL, "opd_color_features: frame " + std::to_string(f) + " has no pixels");
        if (H > OPD_COLOR_MAX_EDGE || W > OPD_COLOR_MAX_EDGE)
            return fail(OPD_EINVAL, "opd_color_features: frame " + std::to_string(f) + " is " + std::to_string(H) + " x " + std::to_string(W) +
                                        ", above the 4096 x 4096 the exact integer sums are sized for");
    }
    // plan: the crop of every box; which frames are named; bytes of the crops' source windows
    struct Plan { int f, x1, y1, w, h; };
    std::vector<Plan> plan((size_t)n_boxes);
    std::vector<char> named((size_t)n_frames, 0);
    size_t window_bytes = 0;
    int max_rows = 1;
    for (int i = 0; i < n_boxes; ++i) {
        Plan& p = plan[i];
        p.f = box_frame ? box_frame[i] : 0;
        if (p.f < 0 || p.f >= n_frames) return fail(OPD_EINVAL, "opd_color_features: box " + std::to_string(i) + " names frame " + std::to_string(p.f));
        int x2, y2;
        const float* b = boxes_xywh + 4 * (size_t)i;
        const bool ok = opd_color_rect(b[0], b[1], b[2], b[3], frame_hw[2 * p.f], frame_hw[2 * p.f + 1], &p.x1, &p.y1, &x2, &y2);
        p.w = ok ? x2 - p.x1 : 0;
        p.h = ok ? y2 - p.y1 : 0;
        if (!ok) continue;
        named[p.f] = 1;
        window_bytes += align_up((size_t)p.h * p.w * 3, 16);
        max_rows = std::max(max_rows, p.h);
    }
    RCCHK(use_device("opd_color_features", device_ordinal));
    if (device_ordinal >= 16) return fail(OPD_EINVAL, "opd_color_features: no device " + std::to_string(device_ordinal));   // (g_scratch)
    if (mem_kind == OPD_MEM_DEVICE)
        for (int f = 0; f < n_frames; ++f)
            if (named[f] && !device_accessible(frames[f]))
                return fail(OPD_EINVAL, "opd_color_features: OPD_MEM_DEVICE, but frame " + std::to_string(f) + " is not device-accessible memory");
    // host frames: upload the crops' windows, or the named frames whole when that is less (overlapping or frame-sized crops)
    size_t frame_bytes = 0;
    std::vector<size_t> frame_off((size_t)n_frames, 0);
    const size_t desc_bytes = align_up(sizeof(ColorCrop) * (size_t)n_boxes, 256);
    for (int f = 0; f < n_frames; ++f)
        if (named[f]) { frame_off[f] = desc_bytes + frame_bytes; frame_bytes += align_up((size_t)frame_hw[2 * f] * frame_hw[2 * f + 1] * 3, 16); }
    const bool host = mem_kind == OPD_MEM_HOST, whole = host && frame_bytes < window_bytes;
    const size_t up_bytes = desc_bytes + (host ? (whole ? frame_bytes : window_bytes) : 0);
    const size_t acc_off = align_up(up_bytes, 256), out_off = acc_off + align_up((size_t)n_boxes * OPD_COLOR_ACC_WORDS * 4, 256);
    ColorScratch& s = g_scratch[device_ordinal];
    std::lock_guard<std::mutex> guard(s.mu);
    if (!s.stream) HIPCHK(hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking));
    const size_t floor_bytes = (size_t)1 << 16;   // what the first call allocates at least
    RCCHK(s.io.reserve("opd_color_features", std::max(up_bytes, floor_bytes), std::max(out_off + (size_t)n_boxes * OPD_COLOR_DIM * 4, floor_bytes), s.stream));
    ColorCrop* desc = reinterpret_cast<ColorCrop*>(s.io.host);
    if (whole)
        for (int f = 0; f < n_frames; ++f)
            if (named[f]) memcpy(s.io.host + frame_off[f], frames[f], (size_t)frame_hw[2 * f] * frame_hw[2 * f + 1] * 3);
    size_t woff = desc_bytes;
    for (int i = 0; i < n_boxes; ++i) {
        const Plan& p = plan[i];
        ColorCrop& c = desc[i];
        c.src = s.io.dev;
        c.pitch = 0;
        c.w = p.w; c.h = p.h;
        c.row = i;
        if (p.w <= 0) continue;
        const int W = frame_hw[2 * p.f + 1];
        const size_t start = ((size_t)p.y1 * W + p.x1) * 3;
        if (!host) {
            c.src = frames[p.f] + start;
            c.pitch = 3 * W;
        } else if (whole) {
            c.src = s.io.dev + frame_off[p.f] + start;
            c.pitch = 3 * W;
        } else {
            const size_t rowb = (size_t)p.w * 3;
            for (int y = 0; y < p.h; ++y) memcpy(s.io.host + woff + (size_t)y * rowb, frames[p.f] + start + (size_t)y * W * 3, rowb);
            c.src = s.io.dev + woff;
            c.pitch = (int32_t)rowb;
            woff += align_up((size_t)p.h * rowb, 16);
        }
    }
    HIPCHK(hipMemcpyAsync(s.io.dev, s.io.host, up_bytes, hipMemcpyHostToDevice, s.stream));
    ColorParams cp{};
    cp.crops = reinterpret_cast<const ColorCrop*>(s.io.dev);
    cp.n = n_boxes;
    cp.acc = reinterpret_cast<uint32_t*>(s.io.dev + acc_off);
    cp.out = reinterpret_cast<float*>(s.io.dev + out_off);
    // row spans per crop: about 16 rows each, so that a frame-sized crop spreads over the CUs (the result does not depend on it)
    HIPCHK(opd_launch_color_features(cp, std::min(64, (max_rows + 15) / 16), s.stream));
    HIPCHK(hipMemcpyAsync(out, cp.out, (size_t)n_boxes * OPD_COLOR_DIM * 4, hipMemcpyDeviceToHost, s.stream));
    HIPCHK(hipStreamSynchronize(s.stream));
    return OPD_OK;
}); }
