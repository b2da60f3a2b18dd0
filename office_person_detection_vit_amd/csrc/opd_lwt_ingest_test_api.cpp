// opd_lwt_ingest_test_api.cpp — the ingest launch of the fused hybrid detect call alone, for tests/ (exported from libopd_hip_test.so only):
// lwt_ingest_kernel on records and a count the caller dictates, against the numpy restatement in tests/lwt_ingest_common.py.
#include <string>

#include "opd_lwt.h"
#include "opd_test_util.h"

using namespace opd;

// records [Q] and the count `n` (any value: the kernel clamps it to 0 .. Q) go to the device; boxes [Q][4] arrive holding the caller's
// sentinels and come back with the first min(n, Q) rows written; *n_out: the clamped count the update kernel would read.
TAPI int opd_lwt_test_ingest(int device, const opd_det* records, int n, int Q, float* boxes, int32_t* n_out) {
    ApiScope api_scope;
    if (!records || !boxes || !n_out) return fail(OPD_EINVAL, "opd_lwt_test_ingest: null argument");
    if (Q < 1 || Q > LWT_MAX_DETS) return fail(OPD_EINVAL, "opd_lwt_test_ingest: Q outside 1 .. 1024");
    RCCHK(use_device("opd_lwt_test_ingest", device));
    DevMem tmp;
    LwtIngestParams p{};
    p.view = RecordView{tmp.up(records, (size_t)Q), nullptr, tmp.up(&n, 1), 1, Q};
    p.boxes = tmp.up(boxes, (size_t)Q * 4);
    p.n_out = tmp.up(n_out, 1);
    if (!tmp.ok) return fail(OPD_ENOMEM, "opd_lwt_test_ingest: device allocation failed");
    HIPCHK(opd_launch_lwt_ingest(p, nullptr));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(boxes, p.boxes, (size_t)Q * 16, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(n_out, p.n_out, 4, hipMemcpyDeviceToHost));
    return OPD_OK;
}
