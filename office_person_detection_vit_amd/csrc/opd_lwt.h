// opd_lwt.h — PRIVATE header of the hybrid-tracker handle (`opd_lwt`, include/opd_detr.h): the per-track device state as kernels_lwt.hip
// reads and writes it, the parameters of its two launches and the handle.  Included by kernels_lwt.hip, opd_lwt.cpp and
// opd_lwt_test_api.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "opd_device.h"
#include "opd_flow.h"

enum { LWT_THREADS = 256, LWT_MAX_TRACKS = 1024, LWT_MAX_DETS = 1024 };
enum { LWT_ID = 0, LWT_AGE = 1, LWT_HITS = 2, LWT_TSU = 3, LWT_F32 = 4, LWT_META = 5 };   // columns of LwtBank::meta
enum { LWT_HEAD_TRACKS = 0, LWT_HEAD_NEXT_ID = 1, LWT_HEAD_POINTS = 2, LWT_HEAD_ERROR = 3, LWT_HEAD = 4 };

// The tracks in creation order (the reference's `self.tracks`): position i of every array is track i.  Two banks: an update reads one and
// writes the survivors, compacted, into the other, so no thread ever writes what another still has to read.
struct LwtBank {
    double* x;        // [S][4]  Kalman state; holds float32 values while meta[LWT_F32] is set (the reference's x is a float32 array until the
                      //         first update with a float64 centre, and float64 from then on)
    float* P;         // [S][16] covariance, row-major (float32 in the reference whatever x is)
    float* bbox;      // [S][4]  xywh: the last matched detection, or the box the last followed point moved it to
    double* center;   // [S][2]  `LightweightTrack.center`
    int32_t* meta;    // [S][LWT_META]
};

// The flow points `OpticalFlowTracker` would hold (`prev_points`, `prev_track_ids`), plus the position of each id's track
struct LwtPoints {
    float* xy;        // [N][2]
    int32_t* id;      // [N]
    int32_t* pos;     // [N]
};

struct LwtUpdateParams {
    LwtBank src, dst;
    int32_t* head;        // [LWT_HEAD] device-resident: tracks, next id, flow points
    const float* dets;    // [N][4] xywh
    int32_t N, max_tracks, max_age, use_flow;
    double thr;
    double* iou;          // [T][N] scratch
    int32_t* result;      // [LWT_HEAD] the head after the call (LWT_HEAD_ERROR: 1 = the new tracks did not fit, nothing was written), then ids [N]
    LwtPoints pts;
};

struct LwtRec { int32_t id, reserved; double bbox[4]; };   // = opd_lwt_rec

struct LwtInterpParams {
    LwtBank s;
    int32_t* head;
    const float* next;       // [n_points][2] where the LK launch left them; null: no flow, every track is predicted
    const uint8_t* status;   // [n_points]
    LwtPoints pts;
    int32_t* result;         // [LWT_HEAD], then (8-byte aligned) LwtRec [T]
    LwtRec* recs;
};

hipError_t opd_launch_lwt_update(const LwtUpdateParams& p, hipStream_t stream);
hipError_t opd_launch_lwt_interp(const LwtInterpParams& p, hipStream_t stream);

struct opd_lwt {
    int32_t S = 0, NM = 0, max_age = 30, use_flow = 0;
    double thr = 0.3;
    int device = 0;
    hipStream_t own_stream = nullptr;          // without optical flow; with it everything runs on the flow handle's stream
    opd_flow* flow = nullptr;
    uint8_t* d_state = nullptr;                // one allocation: two banks, head, points, LK results, IoU scratch
    LwtBank bank[2];
    int cur = 0;                               // bank[cur] holds the tracks
    int32_t* d_head = nullptr;
    LwtPoints pts{};
    float* d_next = nullptr;
    uint8_t* d_status = nullptr;
    double* d_iou = nullptr;
    opd::Staging io;                           // up: boxes [NM][4]; down: [head | ids [NM]] or [head | recs [S]]; the scripted hook's points behind
    size_t o_boxes = 0, o_result = 0, o_script = 0;
    int32_t n_tracks = 0, next_id = 1, n_points = 0;   // mirrors of the device head, refreshed by every call's one wait
    int32_t last_launches = 0, last_waits = 0;
    hipStream_t stream() const { return flow ? flow->stream : own_stream; }
};

// one in-between frame on LK results already on the device at d_next / d_status (opd_lwt.cpp; the scripted hook calls it too)
int lwt_interp_finish(opd_lwt* t, bool with_points, LwtRec* recs_out, int* count);   // recs_out holds t->n_tracks records
