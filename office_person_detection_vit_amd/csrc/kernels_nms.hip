// kernels_nms.hip — the detector's own suppression on the device: the person filter and greedy IoU-NMS of opd_person_nms, in place on the
// records and counts the post-process kernel left there (opd_detr_set_nms; opd_detr_nms_records for records of the caller).  float32,
// no fused multiply-adds (compiled with -ffp-contract=off, and the pragma in opd_nms_iou): every IoU is the host's, bit for bit.
//
//   person_nms_kernel  one workgroup of 128 threads (two waves) per frame, one thread per record slot:
//     load      all counts[f] records into LDS before anything is stored, so the rewrite in place cannot read what it has written
//     filter    label == person_label (every class when person_label < 0)
//     sort      rank by counting: thread i counts the passing records that stand before it (higher score; equal score and lower
//               index) -- its position in the host's stable descending sort -- and writes its index there
//     masks     the thread at sorted position r marks the later positions s > r whose IoU with r exceeds the threshold: 2 x 64 bits
//     scan      serial over the positions, the same in every thread (LDS broadcast reads, no divergence): a position not yet removed
//               is kept and ORs its mask into the removed set; a removed one suppresses nothing, as in the host loop, which tests a
//               candidate against KEPT records only
//     store     kept position r -> slot popcount(kept below r) of the frame; thread 0 stores the new count
//   No atomics, no traffic between workgroups; 6.5 KiB of LDS.  For NaN scores the order is unspecified (ranks may collide), but every
//   index stays in range: `order` is zeroed first and a rank is < the passing count.
#include <hip/hip_runtime.h>

#include "opd_kernels.h"
#include "opd_nms.h"

#pragma clang fp contract(off)

namespace {

using namespace opd;

__global__ __launch_bounds__(OPD_NMS_MAX) void person_nms_kernel(const NmsParams p) {
    __shared__ opd_det rec[OPD_NMS_MAX];
    __shared__ int order[OPD_NMS_MAX];
    __shared__ unsigned long long mask[OPD_NMS_MAX][2];
    __shared__ int wave_pass[2];
    const int f = blockIdx.x, tid = threadIdx.x;
    const int n = p.counts[f];
    // (both exits are uniform over the workgroup)
    if (n < 0) return;   // the padding slot of an uneven shard
    if (n > p.stride) {
        if (tid == 0) *p.flag = 1;
        return;
    }
    opd_det* dets = p.dets + (size_t)f * p.stride;
    bool pass = false;
    if (tid < n) {
        rec[tid] = dets[tid];
        pass = opd_nms_pass(rec[tid], p.person_label);
    }
    order[tid] = 0;
    mask[tid][0] = mask[tid][1] = 0ull;
    const unsigned long long ballot = __ballot(pass);
    if ((tid & 63) == 0) wave_pass[tid >> 6] = __popcll(ballot);
    __syncthreads();
    const int m = wave_pass[0] + wave_pass[1];   // records that pass the filter
    if (pass) {
        const float si = rec[tid].score;
        int rank = 0;
        for (int j = 0; j < n; ++j)
            rank += opd_nms_pass(rec[j], p.person_label) && opd_nms_before(rec[j].score, j, si, tid);
        order[rank] = tid;   // rank <= m - 1
    }
    __syncthreads();
    if (tid < m && p.nms_threshold < 1.0f) {
        const opd_det a = rec[order[tid]];
        unsigned long long lo = 0ull, hi = 0ull;
        for (int s = tid + 1; s < m; ++s) {
            if (opd_nms_iou(rec[order[s]], a) > p.nms_threshold) {
                if (s < 64) lo |= 1ull << s;
                else hi |= 1ull << (s - 64);
            }
        }
        mask[tid][0] = lo;
        mask[tid][1] = hi;
    }
    __syncthreads();
    unsigned long long removed0 = 0ull, removed1 = 0ull, kept0 = 0ull, kept1 = 0ull;
#pragma unroll 8
    for (int r = 0; r < m; ++r) {   // (the loads do not wait for the decision: unrolled, they run ahead of it)
        const unsigned long long m0 = mask[r][0], m1 = mask[r][1];
        const unsigned long long bit = 1ull << (r & 63);
        const bool alive = !((r < 64 ? removed0 : removed1) & bit);
        if (alive) {
            if (r < 64) kept0 |= bit;
            else kept1 |= bit;
            removed0 |= m0;
            removed1 |= m1;
        }
    }
    if (tid < m) {
        const unsigned long long bit = 1ull << (tid & 63);
        if ((tid < 64 ? kept0 : kept1) & bit) {
            const int pos = tid < 64 ? __popcll(kept0 & (bit - 1ull)) : __popcll(kept0) + __popcll(kept1 & (bit - 1ull));
            dets[pos] = rec[order[tid]];   // pos <= tid < m <= n <= stride
        }
    }
    if (tid == 0) p.counts[f] = __popcll(kept0) + __popcll(kept1);
}

}  // namespace

hipError_t opd::opd_launch_person_nms(const NmsParams& p, hipStream_t stream) {
    if (p.stride < 1 || p.stride > OPD_NMS_MAX || p.n_frames < 0 || !p.flag) return hipErrorInvalidValue;
    if (p.n_frames == 0) return hipSuccess;
    OPD_LAUNCH(person_nms_kernel, dim3(p.n_frames), dim3(OPD_NMS_MAX), 0, stream, p);
    return hipGetLastError();
}
