// opd_nms.h — the person filter and greedy IoU suppression of the detect path, written once for the host (opd_host.cpp::opd_person_nms)
// and for the device (kernels_nms.hip::person_nms_kernel): the float32 arithmetic both evaluate, the order both produce, and the kernel's
// parameters.  Plain C++ on the host (opd_host.cpp is also built on its own by g++ for the sanitizer driver): nothing of HIP
// unless the HIP compiler reads it.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/opd_detr.h"

#if defined(__HIP__) || defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define OPD_NMS_HD __host__ __device__
#else
#define OPD_NMS_HD
#endif

enum { OPD_NMS_MAX = 128 };   // records per frame: one thread each, one bit each of a 2 x 64-bit mask

// IoU of two xyxy boxes in float32, operation for operation what opd_person_nms has always computed: widths and heights clamped at
// zero, the two areas summed and then minus the intersection, a correctly rounded divide.  No multiply-add may be fused (iw * ih - ...
// would round once instead of twice): the pragma here, -ffp-contract=off for kernels_nms.hip besides.
OPD_NMS_HD inline float opd_nms_iou(const opd_det& a, const opd_det& b) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float ix1 = fmaxf(a.x1, b.x1), iy1 = fmaxf(a.y1, b.y1), ix2 = fminf(a.x2, b.x2), iy2 = fminf(a.y2, b.y2);
    const float iw = fmaxf(0.f, ix2 - ix1), ih = fmaxf(0.f, iy2 - iy1), inter = iw * ih;
    const float ua = fmaxf(0.f, a.x2 - a.x1) * fmaxf(0.f, a.y2 - a.y1) + fmaxf(0.f, b.x2 - b.x1) * fmaxf(0.f, b.y2 - b.y1) - inter;
    return ua > 0.f ? inter / ua : 0.f;
}

OPD_NMS_HD inline bool opd_nms_pass(const opd_det& r, int person_label) { return person_label < 0 || r.label == person_label; }

// Record j stands before record i in the stable descending order by score (ties in record order).  For finite scores this is a strict
// total order, so #{j : before(j, i)} is i's position in it: exactly where the host's insertion sort (shift while the left
// neighbour's score is SMALLER) leaves i.
OPD_NMS_HD inline bool opd_nms_before(float score_j, int j, float score_i, int i) {
    return score_j > score_i || (score_j == score_i && j < i);
}

namespace opd {

struct NmsParams {
    opd_det* dets;        // [n_frames][stride], rewritten in place
    int32_t* counts;      // [n_frames]; < 0: a padding slot, left alone; > stride: left alone, *flag raised
    int32_t* flag;        // one word, set to 1 when a count exceeds the stride (never cleared by the kernel)
    int n_frames, stride;
    int person_label;     // < 0: every class
    float nms_threshold;  // >= 1: no suppression (filter and sort only)
};

#if defined(__HIP__) || defined(__HIPCC__)
// kernels_nms.hip: one workgroup of OPD_NMS_MAX threads per frame; hipErrorInvalidValue for a stride outside [1, OPD_NMS_MAX]
hipError_t opd_launch_person_nms(const NmsParams& p, hipStream_t stream);
#endif

}  // namespace opd
