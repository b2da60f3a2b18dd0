// opd_lwt_ingest_merged_test_api.cpp — the ingest launch of the fused hybrid TILED call alone, for tests/ (exported from libopd_hip_test.so
// only): lwt_ingest_kernel on a view of merged records and a count the caller dictates, against the numpy restatement in
// tests/tile_hybrid_common.py.
#include <string>

#include "opd_lwt.h"
#include "opd_test_util.h"

using namespace opd;

// merged [S] (host) and the count `n` (any value: the kernel clamps it to 0 .. S) go to the device; boxes [S][4] arrive holding the caller's
// sentinels and come back with the first min(n, S) rows written; *n_out: the clamped count the update kernel would read.
TAPI int opd_lwt_test_ingest_merged(int device, const opd_tile_det* merged, int n, int S, float* boxes, int32_t* n_out) {
    ApiScope api_scope;
    if (!merged || !boxes || !n_out) return fail(OPD_EINVAL, "opd_lwt_test_ingest_merged: null argument");
    if (S < 1 || S > LWT_MAX_DETS) return fail(OPD_EINVAL, "opd_lwt_test_ingest_merged: S outside 1 .. 1024");
    RCCHK(use_device("opd_lwt_test_ingest_merged", device));
    DevMem tmp;
    LwtIngestParams p{};
    p.view = RecordView{nullptr, tmp.up(merged, (size_t)S), tmp.up(&n, 1), 1, S};
    p.boxes = tmp.up(boxes, (size_t)S * 4);
    p.n_out = tmp.up(n_out, 1);
    if (!tmp.ok) return fail(OPD_ENOMEM, "opd_lwt_test_ingest_merged: device allocation failed");
    HIPCHK(opd_launch_lwt_ingest(p, nullptr));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(boxes, p.boxes, (size_t)S * 16, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(n_out, p.n_out, 4, hipMemcpyDeviceToHost));
    return OPD_OK;
}
