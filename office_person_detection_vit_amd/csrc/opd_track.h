// opd_track.h — PRIVATE header of the tracker handle (`opd_track`, include/opd_detr.h): the per-slot device state as kernels_track.hip
// reads and writes it, the parameters of the two launches and the handle.  Included by kernels_track.hip, opd_track.cpp and
// opd_track_test_api.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "opd_device.h"

enum { TRACK_RING = 10, TRACK_THREADS = 256, TRACK_MAX_TRACKS = 1024, TRACK_MAX_DETS = 1024, TRACK_MAX_DIM = 2048 };
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
};

struct TrackCommitParams {
    TrackState s;
    TrackDets d;
    int32_t M, D;
    const int32_t* ops;        // [M][4]: slot, detection, TRACK_OP_*, frames since the last update (after this frame's predict)
};

hipError_t opd_launch_track_predict_cost(const TrackPredictParams& p, hipStream_t stream);
hipError_t opd_launch_track_commit(const TrackCommitParams& p, hipStream_t stream);

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
    size_t o_slots = 0, o_boxes = 0, o_foot = 0, o_has = 0, o_feat = 0, o_ops = 0, o_app = 0, o_iou = 0, o_comb = 0, io_bytes = 0;
    std::vector<TrackEntry> tracks;           // creation order: the reference's `self.tracks`
    std::vector<int32_t> free_slots;          // (popped from the back)
    int32_t next_id = 1;
    int32_t last_T = 0, last_N = 0, last_launches = 0, last_waits = 0;
};
