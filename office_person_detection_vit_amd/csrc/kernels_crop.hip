// kernels_crop.hip — the crops of a fused detect + Re-ID call (opd_detr_detect_frames_reid) planned on the device, from the records the
// post-process kernel left there: which records are persons, and for each of them the ReidCrop record and Pillow coefficient tables that
// opd_reid.cpp::stage builds on the host for opd_reid_extract.  float64, no fused multiply-adds (compiled with -ffp-contract=off, and the
// pragma below): every thread evaluates the shared routines of opd_crop.h, so the tables are the host's bit for bit.
//
//   crop_select_kernel  ONE workgroup of 256 walks the record slots of the view (opd_records.h) in (frame, record index) order, 256 at a time:
//                       ballot per wave, prefix counts over the lanes and the four waves.  The order of the list depends on the records alone.
//   crop_plan_kernel    one workgroup of 256 per crop slot.  Every thread repeats the box's geometry (scalar work on the same bits); thread
//                       j then evaluates output column j and output row j (at most out_w, out_h <= 256 each: a loop covers any spec), its
//                       taps summed one after the other.  The source window is the min / max over the bounds (integer atomics in LDS: the
//                       result does not depend on their order); the first taps are then made relative to it, and thread 0 stores the record.
//                       The crop is read in place from the camera-resolution frames: nothing is copied.
#include <hip/hip_runtime.h>
#include <limits.h>

#include "opd_crop.h"
#include "opd_kprims.h"

#pragma clang fp contract(off)

namespace {

using namespace opd;

__global__ __launch_bounds__(256) void crop_select_kernel(const CropSelectParams p) {
    __shared__ int wave_count[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int S = p.view.stride, n = p.view.n_frames * S;
    int seen = 0;   // persons before this round (the same in every thread)
    for (int i0 = 0; i0 < n; i0 += 256) {
        const int i = i0 + tid;
        bool keep = false;
        int target = 0;
        if (i < n) {
            const int f = i / S, q = i - f * S;
            if (q < record_count(p.view, f)) {
                const int key = record_key(p.view, i);
                keep = record_label(p.view, i) == p.label && (unsigned)key < (unsigned)S;
                target = f * S + key;
            }
        }
        const unsigned long long mask = __ballot(keep);
        if (lane == 0) wave_count[wave] = __popcll(mask);
        __syncthreads();
        int before = seen, total = 0;
        for (int v = 0; v < 4; ++v) {
            if (v < wave) before += wave_count[v];
            total += wave_count[v];
        }
        const int k = before + __popcll(mask & ((1ull << lane) - 1ull));
        if (keep && k < p.slots) {
            p.slot[k] = target;
            p.rec[k] = i;
        }
        seen += total;
        __syncthreads();   // (wave_count is rewritten by the next round)
    }
    if (tid == 0) *p.n_person = seen;
}

__device__ __forceinline__ void store_zero_crop(ReidCrop* c) {
    ReidCrop z;
    z.src = nullptr; z.tables = 0; z.pitch = 0; z.zero = 1; z.ks_h = 0; z.ks_v = 0;
    *c = z;
}

__global__ __launch_bounds__(256) void crop_plan_kernel(const CropPlanParams p) {
    __shared__ int win[4];   // wx0, wx1, wy0, wy1
    const int k = blockIdx.x, tid = threadIdx.x;
    ReidCrop* crop = reinterpret_cast<ReidCrop*>(p.base) + k;
    int32_t* geom = p.geom ? p.geom + 13 * (size_t)k : nullptr;
    // (every exit below is uniform over the workgroup)
    double bx, by, bw, bh;
    int frame = 0;
    if (p.boxes) {
        const float* b = p.boxes + 4 * (size_t)k;
        bx = b[0]; by = b[1]; bw = b[2]; bh = b[3];
    } else {
        const int np = *p.n_person;
        if (k >= (np < p.slots ? np : p.slots)) {
            if (tid == 0) store_zero_crop(crop);
            return;
        }
        const int i = p.rec[k];
        frame = i / p.view.stride;
        double box[4];   // Detection.bbox, handed on as float32
        record_box64(p.view, i, box);
        bx = (double)(float)box[0]; by = (double)(float)box[1];
        bw = (double)(float)box[2]; bh = (double)(float)box[3];
    }
    ReidGeom g;
    crop_box_geometry(p.spec, bx, by, bw, bh, p.h, p.w, &g);
    const int OW = p.spec.out_w, OH = p.spec.out_h;
    const int cw = g.x2 - g.x1, chh = g.y2 - g.y1;
    const int ksh = g.zero ? 0 : crop_ksize(cw, g.rw, p.spec.bicubic), ksv = g.zero ? 0 : crop_ksize(chh, g.rh, p.spec.bicubic);
    if (g.zero || ksh > p.ksh_max || ksv > p.ksv_max) {   // (the tap counts of a crop never exceed the stride's: opd_crop.h::crop_slots)
        if (tid == 0) {
            store_zero_crop(crop);
            if (geom) {
                const int32_t v[13] = {g.x1, g.y1, g.x2, g.y2, 1, g.rh, g.rw, g.top, g.left, 0, 0, 0, 0};
                for (int j = 0; j < 13; ++j) geom[j] = v[j];
            }
        }
        return;
    }
    if (tid == 0) { win[0] = INT_MAX; win[1] = INT_MIN; win[2] = INT_MAX; win[3] = INT_MIN; }
    __syncthreads();
    const size_t toff = p.tables_off + (size_t)k * p.stride;
    int32_t* tbx = reinterpret_cast<int32_t*>(p.base + toff);
    int32_t* tby = tbx + 2 * OW;
    int32_t* tch = tby + 2 * OH;
    int32_t* tcv = tch + (size_t)OW * ksh;
    for (int j = tid; j < OW; j += 256) {
        int32_t first, count;
        crop_coeffs_one(cw, g.rw, p.spec.bicubic, g.left + j, ksh, &first, &count, tch + (size_t)j * ksh);
        tbx[2 * j] = first;
        tbx[2 * j + 1] = count;
        atomicMin(&win[0], g.x1 + first);
        atomicMax(&win[1], g.x1 + first + count);
    }
    for (int j = tid; j < OH; j += 256) {
        int32_t first, count;
        crop_coeffs_one(chh, g.rh, p.spec.bicubic, g.top + j, ksv, &first, &count, tcv + (size_t)j * ksv);
        tby[2 * j] = first;
        tby[2 * j + 1] = count;
        atomicMin(&win[2], g.y1 + first);
        atomicMax(&win[3], g.y1 + first + count);
    }
    __syncthreads();
    g.wx0 = win[0]; g.wx1 = win[1]; g.wy0 = win[2]; g.wy1 = win[3];
    // first taps relative to the window (each thread rewrites the entries it wrote)
    for (int j = tid; j < OW; j += 256) tbx[2 * j] -= g.wx0 - g.x1;
    for (int j = tid; j < OH; j += 256) tby[2 * j] -= g.wy0 - g.y1;
    if (tid != 0) return;
    ReidCrop c;
    c.src = p.frames + ((size_t)frame * p.h * p.w + (size_t)g.wy0 * p.w + g.wx0) * 3;
    c.tables = (int64_t)toff;
    c.pitch = 3 * p.w;
    c.zero = 0;
    c.ks_h = ksh;
    c.ks_v = ksv;
    *crop = c;
    if (geom) {
        const int32_t v[13] = {g.x1, g.y1, g.x2, g.y2, g.zero, g.rh, g.rw, g.top, g.left, g.wy0, g.wx0, g.wy1, g.wx1};
        for (int j = 0; j < 13; ++j) geom[j] = v[j];
    }
}

}  // namespace

hipError_t opd::opd_launch_crop_select(const CropSelectParams& p, hipStream_t stream) {
    OPD_LAUNCH(crop_select_kernel, dim3(1), dim3(256), 0, stream, p);
    return hipGetLastError();
}

hipError_t opd::opd_launch_crop_plan(const CropPlanParams& p, int nb, hipStream_t stream) {
    if (nb <= 0) return hipSuccess;
    OPD_LAUNCH(crop_plan_kernel, dim3(nb), dim3(256), 0, stream, p);
    return hipGetLastError();
}
