// opd_flow_test_api.cpp — read-back hook of the optical-flow handle for tests/ and tools/ (exported from libopd_hip_test.so only).
#include <string>

#include "opd_flow.h"

using namespace opd;

#define TAPI extern "C" __attribute__((visibility("default")))

// Level `level` of the handle's reference pyramid (which = 0) or of the pyramid of the frame the reference replaced (which = 1; valid
// after a track call): *h x *w gray bytes into `out` (host, rows packed; null = sizes only), *levels = number of levels incl. level 0.
TAPI int opd_flow_test_level(opd_flow* f, int which, int level, uint8_t* out, int* h, int* w, int* levels) {
    ApiScope api_scope;
    if (!f || !h || !w || !levels) return fail(OPD_EINVAL, "opd_flow_test_level: null argument");
    if (which != 0 && which != 1) return fail(OPD_EINVAL, "opd_flow_test_level: which must be 0 or 1");
    const FlowPyramid& p = f->pyr[which == 0 ? f->ref : 1 - f->ref];
    if (!f->pyr[f->ref].valid || !p.valid) return fail(OPD_ESTATE, "opd_flow_test_level: that pyramid holds no frame");
    if (level < 0 || level > p.top) return fail(OPD_EINVAL, "opd_flow_test_level: no level " + std::to_string(level));
    *h = p.lh[level]; *w = p.lw[level]; *levels = p.top + 1;
    if (!out) return OPD_OK;
    HIPCHK(hipSetDevice(f->device));
    HIPCHK(hipMemcpy2D(out, (size_t)*w, p.base + p.off[level], (size_t)p.lp[level], (size_t)*w, (size_t)*h, hipMemcpyDeviceToHost));
    return OPD_OK;
}
