// opd_track_streams_test_api.cpp — hooks of the streams calls, for tests/ (exported from libopd_hip_test.so only): the schedule of a call as the
// host plans it, and track_assoc_multi_kernel on several cameras' matrices in ONE launch next to the host's association of each.
#include <string.h>

#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "opd_assoc.h"
#include "opd_track.h"
#include "opd_track_test_rig.h"

using namespace opd;

#define TAPI extern "C" __attribute__((visibility("default")))

// streams_schedule (opd_track.cpp) for camera_of [F] and C cameras: out [capacity] as [*steps][C] frame indices, -1 where a camera has no frame at that
// step.  Touches no device.
TAPI int opd_track_test_streams_schedule(const int32_t* camera_of, int F, int C, int32_t* out, int capacity, int32_t* steps) {
    if (!camera_of || !out || !steps || F < 0 || C < 1 || C > TRACK_MAX_CAMERAS) return fail(OPD_EINVAL, "opd_track_test_streams_schedule: null argument or size out of range");
    for (int f = 0; f < F; ++f)
        if (camera_of[f] < 0 || camera_of[f] >= C) return fail(OPD_EINVAL, "opd_track_test_streams_schedule: camera_of[" + std::to_string(f) + "] outside 0 .. C - 1");
    const std::vector<std::vector<int32_t>> s = streams_schedule(camera_of, F, C);
    *steps = (int32_t)s.size();
    if ((size_t)(capacity < 0 ? 0 : capacity) < s.size() * C) return fail(OPD_EINVAL, "opd_track_test_streams_schedule: " + std::to_string(s.size()) + " steps, the output is too small");
    for (size_t k = 0; k < s.size(); ++k) memcpy(out + k * C, s[k].data(), (size_t)C * 4);
    return OPD_OK;
}

// opd_track_test_assoc for C cameras whose association runs in ONE launch of track_assoc_multi_kernel.  T, N, n_free [C]; app / iou / comb: camera c's
// [T[c]][N[c]] matrix behind camera c - 1's; hits and conf likewise.  Outputs per side as in opd_track_test_assoc, camera c's matches at row
// sum over the cameras before it of max(min(T, N), 1), its new detections at sum of max(N, 1), its unmatched tracks at sum of max(T, 1); counts [C].
TAPI int opd_track_test_assoc_multi(int device, int C, const int32_t* T, const int32_t* N, const int32_t* n_free, const float* app, const float* iou, const float* comb,
                                    const int32_t* hits, const float* conf, int min_hits, double high_conf, int32_t* k_matches, int32_t* k_n_matches, int32_t* k_new,
                                    int32_t* k_n_new, int32_t* k_unmatched, int32_t* k_n_unmatched, int32_t* h_matches, int32_t* h_n_matches, int32_t* h_new, int32_t* h_n_new,
                                    int32_t* h_unmatched, int32_t* h_n_unmatched) {
    ApiScope api_scope;
    if (C < 1 || C > TRACK_MAX_CAMERAS || !T || !N || !n_free) return fail(OPD_EINVAL, "opd_track_test_assoc_multi: C out of range or null sizes");
    if (!k_matches || !k_n_matches || !k_new || !k_n_new || !k_unmatched || !k_n_unmatched || !h_matches || !h_n_matches || !h_new || !h_n_new || !h_unmatched || !h_n_unmatched)
        return fail(OPD_EINVAL, "opd_track_test_assoc_multi: null output");
    size_t cells = 0, rows = 0, cols = 0;
    for (int c = 0; c < C; ++c) {
        if (T[c] < 0 || N[c] < 0 || n_free[c] < 0 || T[c] + n_free[c] > TRACK_MAX_TRACKS || N[c] > TRACK_MAX_DETS) return fail(OPD_EINVAL, "opd_track_test_assoc_multi: size out of range");
        cells += (size_t)T[c] * N[c]; rows += (size_t)T[c]; cols += (size_t)N[c];
    }
    if ((cells > 0 && (!app || !iou || !comb)) || (rows > 0 && !hits) || (cols > 0 && !conf)) return fail(OPD_EINVAL, "opd_track_test_assoc_multi: null input");
    RCCHK(use_device("opd_track_test_assoc_multi", device));
    std::vector<std::unique_ptr<AssocRig>> rigs;
    std::vector<TrackAssocParams> blocks(C);
    std::vector<size_t> at_m(C), at_n(C), at_t(C);
    size_t cell = 0, row = 0, col = 0, om = 0, on = 0, ot = 0;
    for (int c = 0; c < C; ++c) {
        const float *a = app + cell, *i = iou + cell, *m = comb + cell;
        at_m[c] = om; at_n[c] = on; at_t[c] = ot;
        // ---- the host
        AssocResult r;
        associate(a, i, m, T[c], N[c], hits + row, conf + col, min_hits, high_conf, &r);
        h_n_unmatched[c] = (int32_t)r.unmatched_tracks.size();
        for (size_t k = 0; k < r.unmatched_tracks.size(); ++k) h_unmatched[ot + k] = r.unmatched_tracks[k];
        if (r.new_dets.size() > (size_t)n_free[c]) { r.matches.clear(); r.new_dets.clear(); }
        h_n_matches[c] = (int32_t)r.matches.size();
        for (size_t k = 0; k < r.matches.size(); ++k) { h_matches[2 * (om + k)] = r.matches[k].first; h_matches[2 * (om + k) + 1] = r.matches[k].second; }
        h_n_new[c] = (int32_t)r.new_dets.size();
        for (size_t k = 0; k < r.new_dets.size(); ++k) h_new[on + k] = r.new_dets[k];
        // ---- the camera's block
        rigs.emplace_back(new AssocRig());
        if (!rigs.back()->make(a, i, m, T[c], N[c], hits + row, conf + col, min_hits, high_conf, n_free[c])) return fail(OPD_ENOMEM, "opd_track_test_assoc_multi: device allocation failed");
        blocks[c] = rigs.back()->p;
        cell += (size_t)T[c] * N[c]; row += (size_t)T[c]; col += (size_t)N[c];
        om += (size_t)std::max(std::min(T[c], N[c]), 1); on += (size_t)std::max(N[c], 1); ot += (size_t)std::max(T[c], 1);
    }
    // ---- ONE launch for all of them
    DevMem tmp;
    const TrackAssocParams* dev = tmp.up(blocks.data(), blocks.size());
    if (!tmp.ok) return fail(OPD_ENOMEM, "opd_track_test_assoc_multi: device allocation failed");
    int launched = 0;
    HIPCHK(opd_launch_track_assoc_multi(blocks.data(), dev, C, nullptr, &launched));
    HIPCHK(hipDeviceSynchronize());
    if (!launched) return fail(OPD_EHIP, "opd_track_test_assoc_multi: nothing was launched");
    for (int c = 0; c < C; ++c) {
        AssocRig& rig = *rigs[c];
        const int S = rig.S;
        std::vector<int32_t> ops((size_t)S * 4), un((size_t)S + 1);
        HIPCHK(hipMemcpy(rig.hdr.data(), rig.p.hdr, rig.hdr.size() * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(ops.data(), rig.p.ops, ops.size() * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(un.data(), rig.p.unmatched, un.size() * 4, hipMemcpyDeviceToHost));
        const int M = rig.hdr[TRACK_HDR_M];
        if (M < 0 || M > S || un[0] < 0 || un[0] > T[c])
            return fail(OPD_EHIP, "opd_track_test_assoc_multi: camera " + std::to_string(c) + ": the kernel left " + std::to_string(M) + " list entries and " + std::to_string(un[0]) + " unmatched tracks");
        k_n_matches[c] = k_n_new[c] = 0;
        for (int k = 0; k < M; ++k) {
            const int32_t* op = &ops[(size_t)k * 4];
            if (op[2] == TRACK_OP_MATCHED) {
                if (k_n_matches[c] >= std::min(T[c], N[c])) return fail(OPD_EHIP, "opd_track_test_assoc_multi: more matches than min(T, N)");
                k_matches[2 * (at_m[c] + k_n_matches[c])] = op[0]; k_matches[2 * (at_m[c] + k_n_matches[c]) + 1] = op[1]; ++k_n_matches[c];
            } else {
                if (k_n_new[c] >= N[c]) return fail(OPD_EHIP, "opd_track_test_assoc_multi: more new detections than N");
                k_new[at_n[c] + k_n_new[c]++] = op[1];
            }
        }
        k_n_unmatched[c] = un[0];
        for (int k = 0; k < un[0]; ++k) k_unmatched[at_t[c] + k] = un[1 + k];
    }
    return OPD_OK;
}
