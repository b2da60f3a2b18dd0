// opd_track_test_api.cpp — what the tracker computed, for tests/ and tools/ (exported from libopd_hip_test.so only): the three cost
// matrices of the last update and the device state of one track.
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
