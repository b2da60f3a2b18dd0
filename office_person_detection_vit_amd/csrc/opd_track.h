// opd_track.h — PRIVATE header of the tracker handle (`opd_track`, include/opd_detr.h): the per-slot device state as kernels_track.hip
// reads and writes it, the parameters of the launches, the handle, and the tracker half of the fused detect-and-track call.  Included by
// kernels_track.hip, opd_track.cpp, opd_track_test_api.cpp and opd_api.cpp.
//
// A sequence call (opd_track_update_sequence, opd_detr_detect_sequence_track) also keeps the track TABLE on the device for the length
// of the call: the header ints below, the entries in creation order and the free-slot stack.  track_assoc_kernel then does between the two launches
// what the host does in a per-frame call, so frame b + 1 needs no host wait behind frame b.  Between calls the host copy (opd_track::tracks) is
// the authoritative one: a sequence call uploads it first and adopts the downloaded table last.  A streams call (opd_track_update_streams,
// opd_detr_detect_streams_track) does the same for C trackers at once, their frames side by side: the launches read each tracker's parameter block,
// the structs below, from an array in device memory.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "opd_device.h"
#include "opd_records.h"

enum { TRACK_RING = 10, TRACK_THREADS = 256, TRACK_INGEST_THREADS = 64, TRACK_MAX_TRACKS = 1024, TRACK_MAX_DETS = 1024, TRACK_MAX_DIM = 2048 };
enum { TRACK_OP_MATCHED = 0, TRACK_OP_NEW = 1 };
enum { TRACK_ASSOC_THREADS = 64, TRACK_ASSOC_CACHE_FLOATS = 28 * 1024 };   // one wave: the solver's column scan; dynamic LDS for the block of a stage (168 x 168)
// Header of the device table (int32 each).  STOPPED: a frame ran out of slots; every later launch of the call returns at once.  FRAMES_DONE: frames
// applied so far, the out-of-slots one included.  STOP_T / STOP_NEW: the live and the new tracks of that frame, for the error text.
enum { TRACK_HDR_T = 0, TRACK_HDR_NEXT_ID, TRACK_HDR_N_FREE, TRACK_HDR_STOPPED, TRACK_HDR_M, TRACK_HDR_FRAMES_DONE, TRACK_HDR_STOP_T, TRACK_HDR_STOP_NEW, TRACK_HDR_INTS = 16 };
enum { TRACK_ENTRY_INTS = 5 };       // slot, id, age, hits, tsu: a TrackEntry
enum { TRACK_MAX_CAMERAS = 64 };     // trackers of one streams call (opd_track_update_streams, opd_detr_detect_streams_track): blockIdx.y of its launches

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
    const int32_t* hdr;        // non-null (sequence call): the device table.  T is then the grid's upper bound, the row count is hdr[TRACK_HDR_T],
    const int32_t* tab;        //   row t's slot is tab[TRACK_ENTRY_INTS * t], `slots` is not read; a set TRACK_HDR_STOPPED ends the launch at once
};

// The ingest launch of the fused detect-and-track call: one frame's kept records, where the suppression kernel left them, -> the staging image
enum { TRACK_ROWS_NONE = 0, TRACK_ROWS_BY_KEY = 1, TRACK_ROWS_BY_SLOT = 2 };
struct TrackIngestParams {
    opd::RecordView view;      // ONE frame of the call's records (opd_records.h::record_frame): [Q = view.stride] records and their kept count
    int32_t D, frame;          // `frame`: its index in the call, for the rows below
    int32_t rows_kind;         // TRACK_ROWS_*
    const float* rows;         // BY_KEY: [..][Q][D], row frame * Q + record_key.  BY_SLOT: [slots][D], row k of slot_map[k] = frame * Q + record_key
                               // (a record without a slot enters with has = 0)
    const int32_t* slot_map;   // BY_SLOT: [slots], of which min(*n_person, slots) are filled
    const int32_t* n_person;
    int32_t slots;
    float* boxes; float* foot; uint8_t* has; float* feat;   // the staging regions dets_of() describes
    int32_t* n_out;            // record_count of the frame, for the predict launch
    const int32_t* hdr;        // non-null (sequence call): a set TRACK_HDR_STOPPED ends the launch at once
};

struct TrackCommitParams {
    TrackState s;
    TrackDets d;
    int32_t M, D;
    const int32_t* ops;        // [M][4]: slot, detection, TRACK_OP_*, frames since the last update (after this frame's predict)
    const int32_t* hdr;        // non-null (sequence call): M is the grid's upper bound, the list's length is hdr[TRACK_HDR_M]; TRACK_HDR_STOPPED as above
};

// The association of one frame on the device: what associate_update and the deletion loop of enqueue_commit (opd_track.cpp) do on the host, on the
// matrices where the predict launch left them.  One workgroup of one wave.
struct TrackAssocParams {
    int32_t* hdr;              // [TRACK_HDR_INTS]
    int32_t* tab;              // [S][TRACK_ENTRY_INTS] entries in creation order
    int32_t* free_slots;       // [S] stack, handed out from the back
    const float *app, *iou, *comb;   // [T][N], row stride N
    const float* conf;         // confidence of detection j at conf[j * conf_stride]
    int32_t conf_stride;
    const int32_t* n_dev;      // non-null: N lies there; else n
    int32_t n;
    int32_t* ops;              // [S][4] out: the list of the commit launch
    int32_t* ids;              // [N] out: the id of each detection, -1 where none
    int32_t S, min_hits, max_age, frame;
    double high_conf;
    int32_t* unmatched;        // test hook only (else null): [1 + S] out, the count and the rows of the tracks no stage matched
};

hipError_t opd_launch_track_predict_cost(const TrackPredictParams& p, hipStream_t stream);
hipError_t opd_launch_track_commit(const TrackCommitParams& p, hipStream_t stream);
hipError_t opd_launch_track_ingest(const TrackIngestParams& p, hipStream_t stream);
hipError_t opd_launch_track_assoc(const TrackAssocParams& p, hipStream_t stream);
// The same four for C cameras in ONE launch each (a streams call): blockIdx.y is the camera, and every workgroup reads its camera's block, the struct
// above with `hdr` set, from `dev` [C] in device memory (64 blocks do not fit a kernel-argument block).  `host`: the same C blocks on the host, for the
// checks and the grid (blockIdx.x runs to the largest bound among them).  A block whose `hdr` is null is a camera without work in this launch.
// *launched: 0 where no camera had work and nothing was launched.
hipError_t opd_launch_track_predict_cost_multi(const TrackPredictParams* host, const TrackPredictParams* dev, int C, hipStream_t stream, int* launched);
hipError_t opd_launch_track_commit_multi(const TrackCommitParams* host, const TrackCommitParams* dev, int C, hipStream_t stream, int* launched);
hipError_t opd_launch_track_ingest_multi(const TrackIngestParams* host, const TrackIngestParams* dev, int C, hipStream_t stream, int* launched);
hipError_t opd_launch_track_assoc_multi(const TrackAssocParams* host, const TrackAssocParams* dev, int C, hipStream_t stream, int* launched);

struct TrackEntry { int32_t slot, id, age, hits, tsu; };
static_assert(sizeof(TrackEntry) == TRACK_ENTRY_INTS * 4, "the device table holds TrackEntry as it lies");

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
    opd::Staging seq;                         // sequence calls: [table | ids | the call's detections], grown lazily to the largest call so far
    opd::Staging desc;                        // streams calls, on trackers[0] alone: the parameter blocks of every step, cameras side by side
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
// `frame_view`: frame `frame` of the call's records (record_frame).  `conf`: the confidence of returned record i at conf[i * conf_stride] (floats): the
// score member of the opd_det or opd_tile_det records the call delivered
int track_fused_enqueue(opd_track* t, hipStream_t s, const RecordView& frame_view, int frame, const TrackFeatureSource& src);
int track_fused_finish(opd_track* t, const float* conf, int conf_stride, int n, int with_features, int32_t* out_ids, const char* who);

// The tracker half of opd_detr_detect_sequence_track: B consecutive frames of one camera into ONE tracker, in frame order.
//   track_sequence_enqueue  on the detector's stream `s`, behind the feature stage: the table upload, then per frame ingest -> predict / cost ->
//                           association -> commit, then the download of table and ids (all before the caller's one wait)
//   track_sequence_finish   after that wait: ids of the kept records into track_ids [B][Q], the table adopted, *frames_done; OPD_EINVAL where a
//                           frame ran out of slots
int track_sequence_enqueue(opd_track* t, hipStream_t s, const opd_det* records, const int32_t* counts, int Q, int B, const TrackFeatureSource& src, const char* who);
int track_sequence_finish(opd_track* t, const int32_t* counts, int Q, int B, int32_t* track_ids, int32_t* frames_done, const char* who);

// ---- streams calls: K_c frames each of C cameras, camera c into trackers[c], the cameras side by side ----
// The schedule: camera_of [F] names the camera of every frame of the call, in call order.  Step s holds the s-th frame of every camera that has one:
// the result is [steps][C] frame indices, -1 where a camera has no frame at that step; steps = the most frames any camera has.  (Entries outside
// 0 .. C - 1 are the caller's to refuse first.)
std::vector<std::vector<int32_t>> streams_schedule(const int32_t* camera_of, int F, int C);
// The checks of the tracker list that both streams entries make, after their own: C, camera_of, a tracker named twice or without a frame.  (Null handles
// and devices are track_fused_check's in the detect entry.)
int track_streams_check(opd_track* const* trackers, int C, const int32_t* camera_of, int F, const char* who);
// The tracker half of opd_detr_detect_streams_track, around the caller's one wait on `s` like track_sequence_*: frame b of the call is a frame of
// trackers[camera_of[b]].  frames_done [C]; OPD_EINVAL with the first stopped camera's sentence where a camera ran out of slots.
int track_streams_enqueue(opd_track* const* trackers, int C, const int32_t* camera_of, hipStream_t s, const opd_det* records, const int32_t* counts, int Q, int B,
                          const TrackFeatureSource& src, const char* who);
int track_streams_finish(opd_track* const* trackers, int C, const int32_t* camera_of, const int32_t* counts, int Q, int B, int32_t* track_ids, int32_t* frames_done,
                         const char* who);

}  // namespace opd
