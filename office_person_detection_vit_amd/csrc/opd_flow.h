// opd_flow.h — PRIVATE header of the optical-flow handle (`opd_flow`, include/opd_detr.h): the launch parameters of kernels_flow.hip and the
// handle itself.  Included by kernels_flow.hip, opd_flow.cpp and opd_flow_test_api.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "opd_device.h"

enum { OPD_FLOW_MAX_LEVELS = 8, OPD_FLOW_MAX_WIN = 21 };   // pyramid levels incl. level 0; the LK kernel's LDS and registers are sized for a 21 x 21 window

// One pyramid level: uint8 gray, rows `pitch` bytes apart (a multiple of 16; bytes behind column w - 1 are scratch, never read as pixels)
struct FlowLevel {
    const uint8_t* ref;   // the reference frame's level
    const uint8_t* cur;   // the new frame's level (same geometry)
    int32_t w, h, pitch;
};
struct FlowParams {
    FlowLevel lv[OPD_FLOW_MAX_LEVELS];
    int32_t top;          // effective top level L (levels 0 .. L exist)
    int32_t n, win, max_iter;
    float eps2, min_eig;  // epsilon^2; threshold on the smaller eigenvalue of A / win^2
    const float* pts;     // [n][2] (x, y) in the reference frame
    float* next;          // [n][2]
    uint8_t* status;      // [n]
    const int32_t* count; // null: all n points are followed.  Else the device-resident number of points (<= n, the launch's bound): the
                          // waves of the points at or beyond it leave at once
    const int32_t* stop;  // null, or the sticky word of a sequence call: while it is set every wave leaves at once
};

hipError_t opd_launch_flow_gray(const uint8_t* bgr, uint8_t* gray, int h, int w, int pitch, hipStream_t stream, const int32_t* stop = nullptr);
hipError_t opd_launch_flow_pyrdown(const uint8_t* src, int sh, int sw, int spitch, uint8_t* dst, int dpitch, hipStream_t stream, const int32_t* stop = nullptr);
hipError_t opd_launch_flow_lk(const FlowParams& p, hipStream_t stream);

inline int flow_pitch(int w) { return (w + 15) / 16 * 16; }

// One gray pyramid and the frame it holds: the geometry lives with the pixels it describes, so building into the pyramid the reference does
// not use changes nothing of the reference.
struct FlowPyramid {
    uint8_t* base = nullptr;                   // one allocation; level l at base + off[l]
    size_t off[OPD_FLOW_MAX_LEVELS] = {};
    bool valid = false;                        // holds a whole frame (false from the moment one is enqueued into it until the call's finish)
    int h = 0, w = 0, top = 0;                 // the frame, and its effective top level
    int lw[OPD_FLOW_MAX_LEVELS] = {}, lh[OPD_FLOW_MAX_LEVELS] = {}, lp[OPD_FLOW_MAX_LEVELS] = {};
};

struct opd_flow {
    opd_flow_config cfg{};                     // with the defaults filled in
    int device = 0;
    hipStream_t stream = nullptr;
    FlowPyramid pyr[2];                        // pyr[ref] is the reference (once valid); a track call builds the other one and swaps, so that
    int ref = 0;                               // pyr[1 - ref], while valid, holds the frame the reference replaced
    opd::Staging io;                           // page-locked: [points | frame] up, [next | status] down; device: [points | frame] and, behind it, [next | status]
    size_t pts_bytes = 0, frame_off = 0, out_off = 0;
};

// opd_flow_set_reference and opd_flow_track in two halves each: everything up to the wait, on the handle's stream, and the bookkeeping after
// it.  The tracker handle of opd_lwt.cpp enqueues its own launches between the two and waits once itself.  `which`: the pyramid the new
// reference is built into (f->ref for opd_flow_set_reference; 1 - f->ref keeps the old reference intact, and a caller that never reaches
// the finish has changed nothing but the contents of the pyramid the reference does not use).  The track half
// reads its points at `d_pts` on the device (`host_pts`, when given, are staged and uploaded there first: d_pts is then the head of io.dev)
// and leaves LK's results at `d_next` / `d_status` on the device.
//
// A run of track frames behind ONE wait (opd_lwt_interpolate_sequence) takes the track half in its two parts: flow_check_track is every
// refusal of flow_enqueue_track and touches nothing; flow_enqueue_track_from is its device work with the reference named by the caller
// (`ref`, which the caller alternates: no finish has run between the frames), a host frame uploaded from where it lies (the staging image
// holds one frame, and the host does not wait between two), and LK launched for the bound `n` while `d_count` on the device says how many
// points there are by then.  flow_finish_sequence is `frames` finishes at once.
namespace opd {
int flow_enqueue_reference(opd_flow* f, const char* who, const uint8_t* bgr, int mem_kind, int h, int w, int which, hipStream_t on = nullptr,
                           const int32_t* stop = nullptr);   // `on`: a stream other than f->stream; `stop`: the sticky word of a sequence call (FlowParams::stop)
void flow_finish_reference(opd_flow* f, int which);
int flow_check_track(opd_flow* f, const char* who, const uint8_t* bgr, int mem_kind, int h, int w, int n);
int flow_enqueue_track(opd_flow* f, const char* who, const uint8_t* bgr, int mem_kind, int h, int w, const float* host_pts, int n, const float* d_pts,
                       float* d_next, uint8_t* d_status);
int flow_enqueue_track_from(opd_flow* f, int ref, const uint8_t* bgr, int mem_kind, int h, int w, bool in_place, const float* host_pts, int n,
                            const int32_t* d_count, const float* d_pts, float* d_next, uint8_t* d_status, hipStream_t on = nullptr, const int32_t* stop = nullptr);
void flow_finish_track(opd_flow* f);
void flow_finish_sequence(opd_flow* f, int frames);
}  // namespace opd
