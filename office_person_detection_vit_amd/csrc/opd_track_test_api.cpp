// opd_track_test_api.cpp — what the tracker computed, for tests/ and tools/ (exported from libopd_hip_test.so only): the three cost
// matrices of the last update, the device state of one track, and the ingest launch of the fused detect-and-track call on records of the caller.
#include <string.h>

#include "opd_track.h"

using namespace opd;

#define TAPI extern "C" __attribute__((visibility("default")))

// The matrices the last update's predict launch wrote, [*T][*N] each (tracks in the creation order of BEFORE that update).  Any output may
// be null; `capacity` (in elements) bounds each of them.
TAPI int opd_track_test_matrices(opd_track* t, float* app, float* iou, float* comb, int capacity, int* T, int* N) {
    if (!t) return fail(OPD_EINVAL, "opd_track_test_matrices: null handle");
    if (T) *T = t->last_T;
    if (N) *N = t->last_N;
    const size_t n = (size_t)t->last_T * t->last_N;
    if ((app || iou || comb) && (size_t)(capacity < 0 ? 0 : capacity) < n) return fail(OPD_EINVAL, "opd_track_test_matrices: the matrices have " + std::to_string(n) + " entries");
    if (app && n) memcpy(app, t->io.host + t->o_app, n * 4);
    if (iou && n) memcpy(iou, t->io.host + t->o_iou, n * 4);
    if (comb && n) memcpy(comb, t->io.host + t->o_comb, n * 4);
    return OPD_OK;
}

// Device state of live track `index` (creation order): x [4], P [16], the number of stored features and, when that is not zero, the
// smoothed feature [feature_dim] of the last predict launch.  Any output may be null.  Waits for the handle's stream.
TAPI int opd_track_test_state(opd_track* t, int index, float* x, float* P, int32_t* ring_len, float* smooth) {
    ApiScope api_scope;
    if (!t) return fail(OPD_EINVAL, "opd_track_test_state: null handle");
    if (index < 0 || index >= (int)t->tracks.size()) return fail(OPD_EINVAL, "opd_track_test_state: no track " + std::to_string(index));
    const size_t slot = (size_t)t->tracks[index].slot;
    HIPCHK(hipSetDevice(t->device));
    int32_t meta[2] = {0, 0};
    if (x) HIPCHK(hipMemcpyAsync(x, t->st.x + 4 * slot, 16, hipMemcpyDeviceToHost, t->stream));
    if (P) HIPCHK(hipMemcpyAsync(P, t->st.P + 16 * slot, 64, hipMemcpyDeviceToHost, t->stream));
    HIPCHK(hipMemcpyAsync(meta, t->st.ring_meta + 2 * slot, 8, hipMemcpyDeviceToHost, t->stream));
    if (smooth) HIPCHK(hipMemcpyAsync(smooth, t->st.smooth + slot * t->D, (size_t)t->D * 4, hipMemcpyDeviceToHost, t->stream));
    HIPCHK(hipStreamSynchronize(t->stream));
    if (ring_len) *ring_len = meta[0];
    return OPD_OK;
}

// track_ingest_kernel alone on hand-made records: records [Q] (host) of which `n` count as kept, `frame` their index in the batch; rows [n_rows][D]
// (host; TRACK_ROWS_BY_QUERY needs n_rows >= (frame + 1) * Q, TRACK_ROWS_BY_SLOT n_rows >= slots), slot_map [slots] and n_person as the crop
// selection leaves them.  boxes [Q][4], foot [Q][2], has [Q], feat [Q][D] and n_out are IN and OUT: the caller's bytes are uploaded first, so
// what the launch does not write comes back as it went in.
TAPI int opd_track_test_ingest(int device, const opd_det* records, int n, int Q, int D, int frame, int rows_kind, const float* rows, int n_rows,
                               const int32_t* slot_map, int n_person, int slots, int capacity, float* boxes, float* foot, uint8_t* has, float* feat, int32_t* n_out) {
    ApiScope api_scope;
    if (!records || !boxes || !foot || !has || !feat || !n_out) return fail(OPD_EINVAL, "opd_track_test_ingest: null argument");
    if (Q < 1 || Q > TRACK_MAX_DETS || capacity != Q || D < 1 || D > TRACK_MAX_DIM || frame < 0 || slots < 0 || n_rows < 0)
        return fail(OPD_EINVAL, "opd_track_test_ingest: size out of range");
    if (rows_kind == TRACK_ROWS_BY_QUERY && (!rows || (long long)n_rows < ((long long)frame + 1) * Q)) return fail(OPD_EINVAL, "opd_track_test_ingest: rows do not cover the frame");
    if (rows_kind == TRACK_ROWS_BY_SLOT && (!rows || !slot_map || n_rows < slots || slots < 1)) return fail(OPD_EINVAL, "opd_track_test_ingest: rows or slot map do not cover the slots");
    RCCHK(use_device("opd_track_test_ingest", device));
    DevMem tmp;
    TrackIngestParams p{};
    p.records = tmp.up(records, (size_t)Q);
    p.count = tmp.up(&n, 1);
    p.Q = Q; p.D = D; p.frame = frame; p.rows_kind = rows_kind; p.slots = slots;
    if (rows_kind != TRACK_ROWS_NONE) p.rows = tmp.up(rows, (size_t)n_rows * D);
    if (rows_kind == TRACK_ROWS_BY_SLOT) {
        p.slot_map = tmp.up(slot_map, (size_t)slots);
        p.n_person = tmp.up(&n_person, 1);
    }
    p.boxes = tmp.up(boxes, (size_t)Q * 4);
    p.foot = tmp.up(foot, (size_t)Q * 2);
    p.has = tmp.up(has, (size_t)Q);
    p.feat = tmp.up(feat, (size_t)Q * D);
    p.n_out = tmp.up(n_out, 1);
    if (!tmp.ok) return fail(OPD_ENOMEM, "opd_track_test_ingest: device allocation failed");
    HIPCHK(opd_launch_track_ingest(p, nullptr));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(boxes, p.boxes, (size_t)Q * 16, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(foot, p.foot, (size_t)Q * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(has, p.has, (size_t)Q, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(feat, p.feat, (size_t)Q * D * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(n_out, p.n_out, 4, hipMemcpyDeviceToHost));
    return OPD_OK;
}
