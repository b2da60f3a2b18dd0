// opd_track.h — PRIVATE header of the tracker handle (`opd_track`, include/opd_detr.h): the per-slot device state as kernels_track.hip
// reads and writes it, the parameters of the three launches, the handle, and the tracker half of the fused detect-and-track call.  Included by
// kernels_track.hip, opd_track.cpp, opd_track_test_api.cpp and opd_api.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "opd_device.h"

enum { TRACK_RING = 10, TRACK_THREADS = 256, TRACK_INGEST_THREADS = 64, TRACK_MAX_TRACKS = 1024, TRACK_MAX_DETS = 1024, TRACK_MAX_DIM = 2048 };
enum { TRACK_OP_MATCHED = 0, TRACK_OP_NEW = 1 };

// Numeric state of every slot, in ONE device allocation that lives as long as the handle
struct TrackState {
    float* x;            // [S][4]   Kalman state x, y, vx, vy
    float* P;            // [S][16]  covariance, row-major
    float* last;         // [S][2]   last observation (the re-update interpolates from it)
    float* box;          // [S][4]   box of the last matched detection, xywh
    float* ring;         // [S][10][D] the last feature vectors
    int32_t* ring_meta;  // [S][2]   entries held, position of the oldest one
    float* smooth;       // [S][D]   smoothed feature of the last predict launch (what the cost rows were computed with)
};

// What both launches read of one call's detections (device staging of the handle)
struct TrackDets {
    const float* boxes;    // [N][4] xywh
    const float* foot;     // [N][2]
    const float* feat;     // [N][D]; null: no detection carries a feature
    const uint8_t* has;    // [N]
    int32_t n;
};

struct TrackPredictParams {
    TrackState s;
    TrackDets d;
    int32_t T, D;
    const int32_t* slots;      // [T] slot of row t (creation order)
    float *app, *iou, *comb;   // [T][N] each
    double aw, mw;             // appearance and motion weight
    float max_dist;            // <= 0: no gate
    const int32_t* n_dev;      // non-null: the detection count lies there (track_ingest_kernel left it), d.n is not read
};

// The ingest launch of the fused detect-and-track call: one frame's kept records, where the suppression kernel left them, -> the staging image
enum { TRACK_ROWS_NONE = 0, TRACK_ROWS_BY_QUERY = 1, TRACK_ROWS_BY_SLOT = 2 };
struct TrackIngestParams {
    const opd_det* records;    // [Q] records of the frame
    const int32_t* count;      // its kept count
    int32_t Q, D, frame;
    int32_t rows_kind;         // TRACK_ROWS_*
    const float* rows;         // BY_QUERY: [..][Q][D], row frame * Q + query_index.  BY_SLOT: [slots][D], row k of slot_map[k] = frame * Q + query_index
    const int32_t* slot_map;   // BY_SLOT: [slots], of which min(*n_person, slots) are filled
    const int32_t* n_person;
    int32_t slots;
    float* boxes; float* foot; uint8_t* has; float* feat;   // the staging regions dets_of() describes
    int32_t* n_out;            // min(count, Q), for the predict launch
};

struct TrackCommitParams {
    TrackState s;
    TrackDets d;
    int32_t M, D;
    const int32_t* ops;        // [M][4]: slot, detection, TRACK_OP_*, frames since the last update (after this frame's predict)
};

hipError_t opd_launch_track_predict_cost(const TrackPredictParams& p, hipStream_t stream);
hipError_t opd_launch_track_commit(const TrackCommitParams& p, hipStream_t stream);
hipError_t opd_launch_track_ingest(const TrackIngestParams& p, hipStream_t stream);

struct TrackEntry { int32_t slot, id, age, hits, tsu; };

struct opd_track {
    int32_t S = 0, NM = 0, D = 0;             // slots, detections per call, feature width
    int32_t max_age = 30, min_hits = 3;
    double iou_threshold = 0.3, aw = 0.7, mw = 0.3, max_dist = 150.0, high_conf = 0.5;
    int device = 0;
    hipStream_t stream = nullptr;
    uint8_t* d_state = nullptr;
    TrackState st{};
    opd::Staging io;                          // one layout on both sides, fixed at creation (offsets below)
    size_t o_slots = 0, o_boxes = 0, o_foot = 0, o_has = 0, o_feat = 0, o_ops = 0, o_app = 0, o_iou = 0, o_comb = 0, o_n = 0, io_bytes = 0;
    hipEvent_t ev_commit = nullptr;           // fused call: recorded on `stream` behind everything enqueued there, waited for by the detector's stream
    std::vector<TrackEntry> tracks;           // creation order: the reference's `self.tracks`
    std::vector<int32_t> free_slots;          // (popped from the back)
    int32_t next_id = 1;
    int32_t last_T = 0, last_N = 0, last_launches = 0, last_waits = 0;
};

namespace opd {

// The tracker half of opd_detr_detect_frames_track (opd_api.cpp runs the detector half and the one wait); opd_track_update is built from the same parts.
//   track_fused_check    the argument checks that need the handle, before any HIP call
//   track_fused_enqueue  on the detector's stream `s`, behind the feature stage and an event recorded on the tracker's own stream: the slot list, the
//                        ingest launch, the predict / cost launch when tracks are alive, the three matrices with the upper-bound size T x Q
//   track_fused_finish   after the caller's wait on `s`: association on the T x n prefix with the confidences of the returned records, ids, and the
//                        commit launch on the tracker's own stream (not waited for)
struct TrackFeatureSource {
    int rows_kind = TRACK_ROWS_NONE;   // TRACK_ROWS_*
    int D = 0;                         // width of a row
    const float* rows = nullptr;
    const int32_t* slot_map = nullptr;
    const int32_t* n_person = nullptr;
    int slots = 0;
};
int track_fused_check(const opd_track* t, int device, int Q, int feature_dim, const char* who);
int track_fused_enqueue(opd_track* t, hipStream_t s, const opd_det* records, const int32_t* count, int Q, int frame, const TrackFeatureSource& src);
int track_fused_finish(opd_track* t, const opd_det* recs, int n, int with_features, int32_t* out_ids, const char* who);

}  // namespace opd
