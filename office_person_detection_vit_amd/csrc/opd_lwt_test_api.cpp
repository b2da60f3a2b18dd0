// opd_lwt_test_api.cpp — the hybrid tracker's in-between frame on LK results the caller dictates, for tests/ (exported from
// libopd_hip_test.so only): the track logic of lwt_interp_kernel is pinned without depending on LK's numerics.
#include <string.h>

#include <string>

#include "opd_lwt.h"

using namespace opd;

#define TAPI extern "C" __attribute__((visibility("default")))

// `opd_lwt_interpolate` with next_xy [n_points][2] and status [n_points] (host) in the place of the LK launch's results; n_points is what
// opd_lwt_info reports.  No frame is read and the reference frame stays what it was.
TAPI int opd_test_lwt_interpolate_scripted(opd_lwt* t, const float* next_xy, const uint8_t* status, opd_lwt_rec* recs_out, int capacity, int* count) {
    ApiScope api_scope;
    if (!t || !count) return fail(OPD_EINVAL, "opd_test_lwt_interpolate_scripted: null argument");
    *count = t->n_tracks;
    if (capacity < t->n_tracks || (t->n_tracks > 0 && !recs_out)) return fail(OPD_EINVAL, "opd_test_lwt_interpolate_scripted: " + std::to_string(t->n_tracks) + " tracks");
    const int n = t->n_points;
    if (n > 0 && (!next_xy || !status)) return fail(OPD_EINVAL, "opd_test_lwt_interpolate_scripted: " + std::to_string(n) + " points, null results");
    HIPCHK(hipSetDevice(t->device));
    t->last_launches = t->last_waits = 0;
    if (n > 0) {
        uint8_t* h = t->io.host + t->o_script;
        memcpy(h, next_xy, (size_t)n * 8);
        memcpy(h + (size_t)n * 8, status, (size_t)n);
        HIPCHK(hipMemcpyAsync(t->d_next, h, (size_t)n * 8, hipMemcpyHostToDevice, t->stream()));
        HIPCHK(hipMemcpyAsync(t->d_status, h + (size_t)n * 8, (size_t)n, hipMemcpyHostToDevice, t->stream()));
    }
    return lwt_interp_finish(t, n > 0, reinterpret_cast<LwtRec*>(recs_out), count);
}
