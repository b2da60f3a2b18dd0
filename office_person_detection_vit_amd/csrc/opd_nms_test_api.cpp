// opd_nms_test_api.cpp — hook of the device suppression for tests/ (exported from libopd_hip_test.so only):
//   opd_test_nms_plan_host   person_nms_kernel's ALGORITHM on the host (nms_plan_frame below: rank by counting, one 128-bit mask per
//                            sorted position, serial scan), with opd_person_nms_batch's arguments and conventions -- written against
//                            opd_nms.h, not against opd_person_nms, so that a machine without a GPU can hold the one to the other.
#include "opd_nms.h"
#include "opd_test_util.h"

using namespace opd;

namespace {

// One frame the kernel's way, on the host: load, filter, rank by counting, one 128-bit mask per sorted position, serial scan, compacted
// store.  Returns the kept count (dets[0 .. kept) rewritten), or -1 for n outside [0, OPD_NMS_MAX].
int nms_plan_frame(opd_det* dets, int n, int person_label, float nms_threshold) {
    if (n < 0 || n > OPD_NMS_MAX) return -1;
    opd_det rec[OPD_NMS_MAX];
    bool pass[OPD_NMS_MAX];
    int order[OPD_NMS_MAX] = {};
    uint64_t mask[OPD_NMS_MAX][2] = {};
    int m = 0;
    for (int i = 0; i < n; ++i) {
        rec[i] = dets[i];
        pass[i] = opd_nms_pass(rec[i], person_label);
        m += pass[i];
    }
    for (int i = 0; i < n; ++i) {
        if (!pass[i]) continue;
        int rank = 0;
        for (int j = 0; j < n; ++j) rank += pass[j] && opd_nms_before(rec[j].score, j, rec[i].score, i);
        order[rank] = i;
    }
    if (nms_threshold < 1.0f)
        for (int r = 0; r < m; ++r)
            for (int s = r + 1; s < m; ++s)
                if (opd_nms_iou(rec[order[s]], rec[order[r]]) > nms_threshold) mask[r][s >> 6] |= 1ull << (s & 63);
    uint64_t removed[2] = {0, 0};
    int kept = 0;
    for (int r = 0; r < m; ++r) {
        if ((removed[r >> 6] >> (r & 63)) & 1ull) continue;
        removed[0] |= mask[r][0];
        removed[1] |= mask[r][1];
        dets[kept++] = rec[order[r]];
    }
    return kept;
}

}  // namespace

TAPI int opd_test_nms_plan_host(opd_det* dets, int32_t* counts, int n_frames, int stride, int person_label, float nms_threshold) {
    if (n_frames < 0 || stride < 1 || stride > OPD_NMS_MAX || (n_frames > 0 && (!dets || !counts)))
        return fail(OPD_EINVAL, "opd_test_nms_plan_host: bad arguments");
    int rc = OPD_OK;
    for (int f = 0; f < n_frames; ++f) {
        if (counts[f] < 0) continue;
        if (counts[f] > stride) { rc = fail(OPD_EINVAL, "opd_test_nms_plan_host: a frame holds more records than its slots"); continue; }
        counts[f] = nms_plan_frame(dets + (size_t)f * stride, counts[f], person_label, nms_threshold);
    }
    return rc;
}
