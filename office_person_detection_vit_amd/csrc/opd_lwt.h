// opd_lwt.h — PRIVATE header of the hybrid-tracker handle (`opd_lwt`, include/opd_detr.h): the per-track device state as kernels_lwt.hip
// reads and writes it, the parameters of its launches, the handle, and the halves of its calls that the detector's fused entries share.
// Included by kernels_lwt.hip, opd_lwt.cpp, opd_api.cpp, opd_lwt_test_api.cpp and opd_lwt_ingest_test_api.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "opd_device.h"
#include "opd_flow.h"
#include "opd_records.h"

enum { LWT_THREADS = 256, LWT_MAX_TRACKS = 1024, LWT_MAX_DETS = 1024, LWT_MAX_SEQUENCE = 64 };
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
    const int32_t* count; // null: N detections.  Else the device-resident count (the fused detect call), of which N is the bound
    int32_t* stop;        // null, or the sticky word of a sequence call: set, the kernel leaves at once; a refusal sets it
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
    const int32_t* stop;     // null, or the sticky word of a sequence call
};

// the kept records of ONE frame (a view of n_frames = 1: post-process records [Q], or the merged records of a tiled frame [n_tiles x Q]) and their
// device-resident count -> boxes [n][4] xywh float32 and the count clamped to the view's stride (the fused detect calls)
struct LwtIngestParams {
    opd::RecordView view;
    float* boxes;
    int32_t* n_out;
    const int32_t* stop;     // null, or the sticky word of a sequence call
};

hipError_t opd_launch_lwt_ingest(const LwtIngestParams& p, hipStream_t stream);
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
    int32_t* d_ndet = nullptr;                 // the detection count of a fused detect call, left by lwt_ingest_kernel
    int32_t* d_stop = nullptr;                 // the sticky word of a sequence call, beside the head: raised by an update the kernel refuses
    LwtPoints pts{};
    float* d_next = nullptr;
    uint8_t* d_status = nullptr;
    double* d_iou = nullptr;
    opd::Staging io;                           // up: boxes [NM][4]; down: [head | ids [NM]] or [head | recs [S]]; the scripted hook's points behind
    size_t o_boxes = 0, o_result = 0, o_script = 0;
    opd::Staging seq;                          // the sequence calls', made by the first of them: [head | recs [F][n_tracks]] (opd_lwt_interpolate_sequence),
                                               // or a slot per frame, [head | ids] of a key frame, [head | recs] of an in-between frame
    FlowPyramid seq_saved[2];                  // the flow handle's pyramids (geometry, validity) as a sequence call with key frames found them
    int32_t n_tracks = 0, next_id = 1, n_points = 0;   // mirrors of the device head, refreshed by every call's one wait
    int32_t last_launches = 0, last_waits = 0;
    hipEvent_t fused_ev = nullptr;             // orders a fused detect call on the detector's stream against this handle's stream, both ways
    int fused_which = 0;                       // the pyramid the fused call in flight builds its reference frame into
    hipStream_t stream() const { return flow ? flow->stream : own_stream; }
};

// One in-between frame on LK results already on the device at d_next / d_status (opd_lwt.cpp), in two halves.  lwt_enqueue_interp launches
// lwt_interp_kernel, which leaves the head at `d_result` and the records at `d_recs`; lwt_interp_finish is that launch into the handle's
// own staging pair, the download, the one wait and the adoption of the head (the per-frame entry and the scripted hook).
int lwt_enqueue_interp(opd_lwt* t, bool with_points, int32_t* d_result, LwtRec* d_recs);
int lwt_interp_finish(opd_lwt* t, bool with_points, LwtRec* recs_out, int* count);   // recs_out holds t->n_tracks records

// A detection frame in the same two halves.  lwt_enqueue_reference: gray + pyramid of the new reference frame into the pyramid the
// reference does not use (*which; nothing without optical flow); lwt_enqueue_update: lwt_update_kernel on the boxes at io.dev + o_boxes,
// `n` of them, or with `d_count` as many as the device says, `n` at most; both on `s`.  lwt_adopt_update, behind the caller's wait on the
// [head | ids] image at io.host + o_result: OPD_EINVAL for an update the kernel refused (nothing has changed then), else the mirrors,
// the bank swap and the flow handle's finish.
int lwt_enqueue_reference(opd_lwt* t, hipStream_t s, const char* who, const uint8_t* bgr, int mem_kind, int h, int w, int* which);
int lwt_enqueue_update(opd_lwt* t, hipStream_t s, int n, const int32_t* d_count);
int lwt_adopt_update(opd_lwt* t, const std::string& who, int which, int n);

// The hybrid part of a fused detect call (opd_detr_detect_frames_hybrid, opd_api.cpp), around the detector's one wait, on the detector's
// stream `s`.  lwt_fused_check: the refusals, before any device work.  lwt_fused_enqueue: ingest of the frame's kept records (where the
// suppression left them, `d_count` of them), gray + pyramid of the camera-resolution frame at `d_bgr`, the update.  lwt_fused_fetch: the
// [head | ids] image joins the call's fetch.  lwt_fused_finish, behind the wait: adoption, and the ids of the `n` kept records (-1 each
// for an update the kernel refused, which is the return code).  `frame`: the records of the tracker's frame through the call's view
// (record_frame, opd_records.h); its stride is the Q of the other three: num_queries, or n_tiles x num_queries of a tiled call, whose
// d_bgr is the WHOLE frame.
int lwt_fused_check(const opd_lwt* t, int device, int Q, int h, int w, const std::string& who);
int lwt_fused_enqueue(opd_lwt* t, hipStream_t s, const opd::RecordView& frame, const uint8_t* d_bgr, int h, int w, const char* who);
int lwt_fused_fetch(opd_lwt* t, hipStream_t s, int Q);
int lwt_fused_finish(opd_lwt* t, int n, int32_t* ids_out, const std::string& who);

// A run of F frames of ONE camera in one call (opd_detr_detect_sequence_hybrid, opd_detr_detect_tiled_sequence_hybrid), in the same four steps.
// The K key frames (is_key[f] != 0) have gone through one batched forward: their kept records are the K frames of `view` (stride Q; null with K = 0), their camera-resolution frames lie at
// d_camera [K][h][w][3].  In frame order on `s`: a key frame runs ingest, gray + pyramid and the update; an in-between frame is uploaded
// from where it lies and runs gray + pyramid, LK and the track kernel.  Every launch carries the handle's sticky word: the update of a key
// frame whose new tracks do not fit raises it, and all launches behind leave at once, so the state and the reference frame stay those of
// the last accepted frame.  K = 0 runs on the handle's own stream (s = t->stream(), null records).
struct LwtSeqCall {
    const uint8_t* const* frames;   // [F] host
    const uint8_t* is_key;          // [F]
    int F, h, w, Q;                 // Q: the record slots of a key frame (num_queries; a tiled call: n_tiles x num_queries)
};
int lwt_sequence_check(const opd_lwt* t, const LwtSeqCall& c, int capacity, int device, const std::string& who);
int lwt_sequence_enqueue(opd_lwt* t, hipStream_t s, const LwtSeqCall& c, const opd::RecordView* view, const uint8_t* d_camera, const char* who);
int lwt_sequence_fetch(opd_lwt* t, hipStream_t s, int F);
// behind the wait.  key_counts [K] (host): the kept records of the key frames; track_ids [K][Q]; recs_out [F - K][capacity], rec_counts [F - K]
int lwt_sequence_finish(opd_lwt* t, const LwtSeqCall& c, const int32_t* key_counts, int32_t* track_ids, opd_lwt_rec* recs_out, int capacity, int32_t* rec_counts,
                        int32_t* frames_done, const std::string& who);
