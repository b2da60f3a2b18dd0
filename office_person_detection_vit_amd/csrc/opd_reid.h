// opd_reid.h — CLIP ViT Re-ID path (opd_reid.cpp, kernels_reid.hip): launchers, the per-crop record the pre-processing kernel reads,
// and the host-side crop geometry (no HIP needed for the geometry, so CPU tests can check it against the reference's expressions).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/opd_detr.h"
#include "opd_kernels.h"

namespace opd {

constexpr int REID_IMG = 224;   // CLIPImageProcessor: shortest edge 224, centre crop 224 x 224

// One crop as the pre-processing kernel reads it.  Its Pillow coefficient tables (only the 224 output columns / rows of the centre
// window) lie at `tables` bytes from the upload base: int32 bx[224][2], by[224][2] (first tap relative to the window, tap count),
// then int32 ch[224][ks_h], cv[224][ks_v] (22-bit fixed point).
struct ReidCrop {
    const uint8_t* src;   // top-left pixel (BGR) of the crop's source window
    int64_t tables;       // byte offset of the tables from the upload base
    int32_t pitch;        // bytes per source row
    int32_t zero;         // 1: degenerate box -> 224 x 224 zero image
    int32_t ks_h, ks_v;   // taps per output column / row
};

// Geometry of one box, host-side, following the reference exactly (reid_feature_extractor.py:124-134 + CLIPImageProcessor):
//   x1 = int(max(0, x)), x2 = int(min(W, x + w)) (same for y); x2 <= x1 or y2 <= y1 -> zero image;
//   resize to shortest edge 224 (long side int(224 * long / short)), centre crop at ((rh - 224) // 2, (rw - 224) // 2);
//   the source window = Pillow bounds of the 224 x 224 centre window, in frame coordinates.
struct ReidGeom {
    int x1, y1, x2, y2;        // crop in frame pixels (x2, y2 exclusive)
    int zero;                  // degenerate
    int rh, rw;                // resized size
    int top, left;             // centre-crop offset in the resized image
    int wy0, wx0, wy1, wx1;    // source window in frame pixels (exclusive ends)
};
void reid_geometry(double x, double y, double w, double h, int H, int W, ReidGeom* g);

// Pillow bicubic (a = -0.5) coefficient tables of one axis restricted to outputs [first, first + count): bounds [count][2], coeffs
// [count][ksize] (22-bit fixed point, normalize_coeffs_8bpc).  Bounds are absolute source indices.
void reid_axis_tables(int in_size, int out_size, int first, int count, std::vector<int32_t>* bounds, std::vector<int32_t>* coeffs,
                      int* ksize);

// fp16 bits of (u8 * (1/255) - mean[c]) / std[c] in the arithmetic of HF's numpy rescale + normalize: lut[c * 256 + u8], RGB order
void reid_pixel_lut(uint16_t* lut);

// Host restatement of the pre-processing kernel for ONE crop (frame [H][W][3] BGR): fp16 patch rows [tokens][3 * P * P], row 0 zero.
void reid_preprocess_host(const uint8_t* frame, int H, int W, const ReidGeom& g, int P, const uint16_t* lut, uint16_t* out);

// Stage n <= max_crops boxes as opd_reid_extract does and run the pre-processing kernel alone: patches [n][tokens][3 P P] fp16 bits to
// the host (opd_reid_test_api.cpp)
int reid_test_pixels(opd_reid* r, const uint8_t* const* frames, const int32_t* frame_hw, int n_frames, int mem_kind, const float* boxes,
                     const int32_t* box_frame, int n, uint16_t* out);

// Per-kernel table of `iters` eager forwards of n <= max_crops boxes on host frames, every launch bracketed by events (stand-alone kernel
// times, summed per kernel name, with algorithmic FLOPs): the table tools/bench_reid.py prints (opd_reid_test_api.cpp)
int reid_test_kernel_table(opd_reid* r, const uint8_t* const* frames, const int32_t* frame_hw, int n_frames, const float* boxes,
                           const int32_t* box_frame, int n, int iters, opd_kernel_stat* out, int capacity, int* count);

}  // namespace opd

// ---- launchers (kernels_reid.hip) -----------------------------------------------------------------------------------------------------
enum { REID_EPI_F16_BIAS = 0, REID_EPI_F32_RESID = 1, REID_EPI_F16_QGELU = 2, REID_EPI_F32_PBIAS = 3 };
// out[m][n] = epi(sum_k X[m][k] W[n][k]):  F16_BIAS  fp16(acc + b[n]);  F32_RESID  out32 += acc + b[n];  F16_QGELU  fp16(qgelu(acc + b[n]));
// F32_PBIAS  out32 = acc + b[(m % period)][n] (b may be null).  K % 64 == 0, N % 64 == 0.
hipError_t opd_launch_reid_gemm(int epi, const f16_t* X, const f16_t* W, const float* bias, int period, void* out, int M, int N, int K,
                                hipStream_t stream);
// LayerNorm over H (H % 128 == 0, H <= 1024) of rows r * row_stride of x: y16[r] (compact), and y32[r * row_stride] when y32 != null
hipError_t opd_launch_reid_layernorm(const float* x, int row_stride, const float* g, const float* b, float* y32, f16_t* y16, int rows, int H,
                                     hipStream_t stream);
// softmax(q k^T) v per (crop, head), T <= 64 tokens, head_dim 64; qkv [crops * T][3H] fp16 (q pre-scaled) -> out [crops * T][H] fp16
hipError_t opd_launch_reid_attention(const f16_t* qkv, f16_t* out, int crops, int T, int H, hipStream_t stream);
// rows of y [rows][E] fp32 divided by their L2 norm
hipError_t opd_launch_reid_l2norm(float* y, int rows, int E, hipStream_t stream);
// crop + BGR->RGB + Pillow bicubic + centre crop + normalise -> patches [crops][T][3 P P] fp16 (row 0 zero)
hipError_t opd_launch_reid_preprocess(const opd::ReidCrop* crops, const unsigned char* base, const f16_t* lut, f16_t* patches, int ncrops,
                                      int P, int T, hipStream_t stream);
