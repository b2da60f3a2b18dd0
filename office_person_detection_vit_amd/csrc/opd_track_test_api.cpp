// opd_track_test_api.cpp — what the tracker computed, for tests/ and tools/ (exported from libopd_hip_test.so only): the three cost
// matrices of the last update, the device state of one track, the ingest launch of the fused detect-and-track call on records of the caller, and the
// association kernel of the sequence calls next to the host's association on matrices of the caller.
#include <string.h>
#include <time.h>

#include <algorithm>

#include "opd_assoc.h"
#include "opd_track.h"
#include "opd_track_test_rig.h"

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
// (host; TRACK_ROWS_BY_KEY needs n_rows >= (frame + 1) * Q, TRACK_ROWS_BY_SLOT n_rows >= slots), slot_map [slots] and n_person as the crop
// selection leaves them.  boxes [Q][4], foot [Q][2], has [Q], feat [Q][D] and n_out are IN and OUT: the caller's bytes are uploaded first, so
// what the launch does not write comes back as it went in.
TAPI int opd_track_test_ingest(int device, const opd_det* records, int n, int Q, int D, int frame, int rows_kind, const float* rows, int n_rows,
                               const int32_t* slot_map, int n_person, int slots, int capacity, float* boxes, float* foot, uint8_t* has, float* feat, int32_t* n_out) {
    ApiScope api_scope;
    if (!records || !boxes || !foot || !has || !feat || !n_out) return fail(OPD_EINVAL, "opd_track_test_ingest: null argument");
    if (Q < 1 || Q > TRACK_MAX_DETS || capacity != Q || D < 1 || D > TRACK_MAX_DIM || frame < 0 || slots < 0 || n_rows < 0)
        return fail(OPD_EINVAL, "opd_track_test_ingest: size out of range");
    if (rows_kind == TRACK_ROWS_BY_KEY && (!rows || (long long)n_rows < ((long long)frame + 1) * Q)) return fail(OPD_EINVAL, "opd_track_test_ingest: rows do not cover the frame");
    if (rows_kind == TRACK_ROWS_BY_SLOT && (!rows || !slot_map || n_rows < slots || slots < 1)) return fail(OPD_EINVAL, "opd_track_test_ingest: rows or slot map do not cover the slots");
    RCCHK(use_device("opd_track_test_ingest", device));
    DevMem tmp;
    TrackIngestParams p{};
    p.view = RecordView{tmp.up(records, (size_t)Q), nullptr, tmp.up(&n, 1), 1, Q};
    p.D = D; p.frame = frame; p.rows_kind = rows_kind; p.slots = slots;
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

// track_assoc_kernel alone, and the host's associate() on the same inputs: app / iou / comb [T][N] (host), hits [T], conf [N]; the table the kernel sees
// has T tracks (row i in slot i) and n_free free slots.  Per side (k_*: the kernel, h_*: the host): matches [min(T, N)][2] as (track row, detection) in
// order, new detections [N], unmatched tracks [T], each with its count.  Both sides after the out-of-slots rule (more new detections than free
// slots drops matches and new detections); the unmatched tracks are what the stages left, before that rule.
TAPI int opd_track_test_assoc(int device, const float* app, const float* iou, const float* comb, int T, int N, const int32_t* hits, const float* conf, int min_hits,
                              double high_conf, int n_free, int32_t* k_matches, int32_t* k_n_matches, int32_t* k_new, int32_t* k_n_new, int32_t* k_unmatched,
                              int32_t* k_n_unmatched, int32_t* h_matches, int32_t* h_n_matches, int32_t* h_new, int32_t* h_n_new, int32_t* h_unmatched,
                              int32_t* h_n_unmatched) {
    ApiScope api_scope;
    if (T < 0 || N < 0 || n_free < 0 || T + n_free > TRACK_MAX_TRACKS || N > TRACK_MAX_DETS) return fail(OPD_EINVAL, "opd_track_test_assoc: size out of range");
    if ((T > 0 && N > 0 && (!app || !iou || !comb)) || (T > 0 && !hits) || (N > 0 && !conf)) return fail(OPD_EINVAL, "opd_track_test_assoc: null input");
    if (!k_matches || !k_n_matches || !k_new || !k_n_new || !k_unmatched || !k_n_unmatched || !h_matches || !h_n_matches || !h_new || !h_n_new || !h_unmatched || !h_n_unmatched)
        return fail(OPD_EINVAL, "opd_track_test_assoc: null output");
    // ---- the host
    AssocResult a;
    associate(app, iou, comb, T, N, hits, conf, min_hits, high_conf, &a);
    *h_n_unmatched = (int32_t)a.unmatched_tracks.size();
    for (size_t k = 0; k < a.unmatched_tracks.size(); ++k) h_unmatched[k] = a.unmatched_tracks[k];
    if (a.new_dets.size() > (size_t)n_free) { a.matches.clear(); a.new_dets.clear(); }
    *h_n_matches = (int32_t)a.matches.size();
    for (size_t k = 0; k < a.matches.size(); ++k) { h_matches[2 * k] = a.matches[k].first; h_matches[2 * k + 1] = a.matches[k].second; }
    *h_n_new = (int32_t)a.new_dets.size();
    for (size_t k = 0; k < a.new_dets.size(); ++k) h_new[k] = a.new_dets[k];
    // ---- the kernel
    RCCHK(use_device("opd_track_test_assoc", device));
    AssocRig rig;
    if (!rig.make(app, iou, comb, T, N, hits, conf, min_hits, high_conf, n_free)) return fail(OPD_ENOMEM, "opd_track_test_assoc: device allocation failed");
    const TrackAssocParams& p = rig.p;
    const int S = rig.S;
    std::vector<int32_t>& hdr = rig.hdr;
    HIPCHK(opd_launch_track_assoc(p, nullptr));
    HIPCHK(hipDeviceSynchronize());
    std::vector<int32_t> ops((size_t)S * 4), un((size_t)S + 1);
    HIPCHK(hipMemcpy(hdr.data(), p.hdr, hdr.size() * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(ops.data(), p.ops, ops.size() * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(un.data(), p.unmatched, un.size() * 4, hipMemcpyDeviceToHost));
    const int M = hdr[TRACK_HDR_M];
    if (M < 0 || M > S || un[0] < 0 || un[0] > T) return fail(OPD_EHIP, "opd_track_test_assoc: the kernel left " + std::to_string(M) + " list entries and " + std::to_string(un[0]) + " unmatched tracks");
    *k_n_matches = *k_n_new = 0;
    for (int k = 0; k < M; ++k) {
        const int32_t* op = &ops[(size_t)k * 4];
        if (op[2] == TRACK_OP_MATCHED) {
            if (*k_n_matches >= std::min(T, N)) return fail(OPD_EHIP, "opd_track_test_assoc: more matches than min(T, N)");
            k_matches[2 * *k_n_matches] = op[0]; k_matches[2 * *k_n_matches + 1] = op[1]; ++*k_n_matches;
        } else {
            if (*k_n_new >= N) return fail(OPD_EHIP, "opd_track_test_assoc: more new detections than N");
            k_new[(*k_n_new)++] = op[1];
        }
    }
    *k_n_unmatched = un[0];
    for (int k = 0; k < un[0]; ++k) k_unmatched[k] = un[1 + k];
    return OPD_OK;
}

// Time of track_assoc_kernel alone and of the host's associate() on the same inputs (tools/bench_track_sequence.py): the mean of `iters` runs each, in
// milliseconds.  The kernel between two events per launch (the table is put back before each, outside the events); the host by its own clock.
TAPI int opd_track_test_bench_assoc(int device, const float* app, const float* iou, const float* comb, int T, int N, const int32_t* hits, const float* conf, int min_hits,
                                    double high_conf, int n_free, int iters, float* kernel_ms, float* host_ms) {
    ApiScope api_scope;
    if (T < 1 || N < 1 || n_free < 0 || T + n_free > TRACK_MAX_TRACKS || N > TRACK_MAX_DETS || iters < 1) return fail(OPD_EINVAL, "opd_track_test_bench_assoc: size out of range");
    if (!app || !iou || !comb || !hits || !conf || !kernel_ms || !host_ms) return fail(OPD_EINVAL, "opd_track_test_bench_assoc: null argument");
    RCCHK(use_device("opd_track_test_bench_assoc", device));
    AssocRig rig;
    if (!rig.make(app, iou, comb, T, N, hits, conf, min_hits, high_conf, n_free)) return fail(OPD_ENOMEM, "opd_track_test_bench_assoc: device allocation failed");
    hipEvent_t e0 = nullptr, e1 = nullptr;
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    double sum = 0.0;
    int rc = OPD_OK;
    for (int k = 0; k < iters + 3 && rc == OPD_OK; ++k) {   // (three launches to warm up)
        hipError_t e = hipMemcpyAsync(rig.p.hdr, rig.hdr.data(), rig.hdr.size() * 4, hipMemcpyHostToDevice, nullptr);
        if (e == hipSuccess) e = hipMemcpyAsync(rig.p.tab, rig.tab.data(), rig.tab.size() * 4, hipMemcpyHostToDevice, nullptr);
        if (e == hipSuccess) e = hipMemcpyAsync(rig.p.free_slots, rig.stack.data(), rig.stack.size() * 4, hipMemcpyHostToDevice, nullptr);
        if (e == hipSuccess) e = hipEventRecord(e0, nullptr);
        if (e == hipSuccess) e = opd_launch_track_assoc(rig.p, nullptr);
        if (e == hipSuccess) e = hipEventRecord(e1, nullptr);
        if (e == hipSuccess) e = hipEventSynchronize(e1);
        float ms = 0.f;
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
        if (e != hipSuccess) rc = fail(OPD_EHIP, std::string("opd_track_test_bench_assoc: ") + hipGetErrorString(e));
        if (k >= 3) sum += ms;
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    RCCHK(rc);
    *kernel_ms = (float)(sum / iters);
    AssocResult a;
    timespec t0{}, t1{};
    clock_gettime(CLOCK_MONOTONIC, &t0);
    for (int k = 0; k < iters; ++k) associate(app, iou, comb, T, N, hits, conf, min_hits, high_conf, &a);
    clock_gettime(CLOCK_MONOTONIC, &t1);
    *host_ms = (float)(((double)(t1.tv_sec - t0.tv_sec) * 1e3 + (double)(t1.tv_nsec - t0.tv_nsec) * 1e-6) / iters);
    return OPD_OK;
}
