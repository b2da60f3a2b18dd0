// opd_reid.h — the Re-ID handle (opd_reid.cpp) and what it asks of a model: the ReidModel interface that the CLIP tower (opd_clip.*)
// and OSNet (opd_osnet.*) implement, the launcher that every launch of a forward goes through, and the bodies of the handle's test hooks.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>
#include <vector>

#include "../../include/opd_detr.h"
#include "opd_crop.h"
#include "opd_device.h"
#include "opd_kernels.h"
#include "opd_loader.h"

namespace opd {

// The launches of one forward on `stream`, through LCHK: while `prof` is set each goes through the LaunchTimer of opd_device.h (two events,
// the kernel's name and algorithmic FLOPs; opd_test_reid_kernel_table).
struct ReidLauncher {
    hipStream_t stream = nullptr;
    bool prof = false;
    LaunchTimer timer;
};

// one launch of a forward: `expr` is a launcher call on L.stream
#define LCHK(L, expr, fl)                                            \
    do {                                                             \
        if ((L).prof) RCCHK((L).timer.begin((L).stream, 0, (fl)));   \
        HIPCHK(expr);                                                \
        if ((L).prof) RCCHK((L).timer.end((L).stream));              \
    } while (0)

// A Re-ID model behind an opd_reid handle, which owns the stream, the weight and workspace allocations and the staging of the crops.
struct ReidModel {
    virtual ~ReidModel() = default;
    virtual const CropSpec& crop() const = 0;
    virtual int feature_dim() const = 0;
    // fold and pack every weight on the host: 16-bit values into h16, fp32 into h32; bind() then resolves them on the device copies
    virtual void pack(const StateDict& sd, std::vector<uint16_t>* h16, std::vector<float>* h32) = 0;
    virtual void bind(const f16_t* w16, const float* w32) = 0;
    // workspace bytes for max_crops; with base != null the buffers are laid out from base
    virtual size_t workspace(int max_crops, unsigned char* base) = 0;
    // the pre-processing kernel alone, and the whole forward of nb staged crops (records at `crops`, tables and windows from `base`)
    virtual hipError_t preprocess(int nb, const ReidCrop* crops, const unsigned char* base, hipStream_t s) const = 0;
    virtual int enqueue(int nb, const ReidCrop* crops, const unsigned char* base, ReidLauncher& L) const = 0;
    virtual const float* features() const = 0;           // [max_crops][feature_dim], unit rows
    virtual const void* image() const = 0;               // what preprocess() writes, image_bytes() per crop
    virtual size_t image_bytes() const = 0;
    virtual void fill_info(opd_reid_model_info* info) const = 0;   // model and the architecture fields (the rest are the handle's)
};

// The Re-ID half of opd_detr_detect_frames_reid and opd_detr_detect_tiled_reid (opd_api.cpp runs the detector half and the one wait).
// reid_fused_check: the argument checks that need the handle, before any HIP call.  A ReidFusedCall holds the handle for the duration of
// the call (one call at a time: a second thread waits in the constructor):
//   enqueue    on the detector's stream `s`, behind the post-process kernel: crop_select_kernel and crop_plan_kernel (kernels_crop.hip)
//              plan the crops of the first `slots` records of the view labelled `label` into the handle's staging buffer, read in place
//              from `frames` ([B][h][w][3] on the device; a tiled call: the whole camera frames); an event; the forward of
//              bucket_of(slots) crops on the handle's own stream through its graph cache; an event back, which `s` waits for
//   copy_back  on `s`: [slots][feature_dim] rows (unless with_rows is off), the slot map and the person count into the handle's page-locked side
//   deliver    after the caller's wait on `s`: rows and slot map of k < min(n_person, slots) into the caller's arrays
int reid_fused_check(const opd_reid* r, int device, int slots, const char* who);
int reid_feature_dim(const opd_reid* r);
struct ReidFusedCall {
    opd_reid* r;
    std::unique_lock<std::mutex> lk;
    int slots = 0;
    explicit ReidFusedCall(opd_reid* r);
    // `geom` (nullable; the test hook of opd_tile_reid_test_api.cpp): device [slots][13], the plan's geometry words of every filled slot
    int enqueue(hipStream_t s, const RecordView& v, const uint8_t* frames, int h, int w, int label, int slots, int32_t* geom = nullptr);
    int copy_back(hipStream_t s);
    void deliver(float* features, int32_t* slot_map, int32_t* n_person) const;
    // the fused detect-and-track call: the rows stay on the device (copy_back then brings the slot list alone); where the rows, the slot map
    // ([slots], filled up to min(*n_person, slots)) and the person count lie there; after the wait, how many slots each of the B frames got
    bool with_rows = true;
    const float* dev_rows() const;
    const int32_t* dev_slot_map() const;
    const int32_t* dev_rec() const;
    const int32_t* dev_n_person() const;
    void slots_per_frame(int B, int Q, int32_t* out) const;
};

// Stage n <= max_crops boxes as opd_reid_extract does and run the pre-processing kernel alone: the model's image of each crop (fp16
// bits) to the host (opd_reid_test_api.cpp)
int reid_test_pixels(opd_reid* r, const uint8_t* const* frames, const int32_t* frame_hw, int n_frames, int mem_kind, const float* boxes,
                     const int32_t* box_frame, int n, uint16_t* out);

// Per-kernel table of `iters` eager forwards of n <= max_crops boxes on host frames, every launch bracketed by events (stand-alone kernel
// times, summed per kernel name, with algorithmic FLOPs): the table tools/bench_reid.py prints (opd_reid_test_api.cpp)
int reid_test_kernel_table(opd_reid* r, const uint8_t* const* frames, const int32_t* frame_hw, int n_frames, const float* boxes,
                           const int32_t* box_frame, int n, int iters, opd_kernel_stat* out, int capacity, int* count);

}  // namespace opd
