// opd_clip.h — the CLIP ViT image tower of the Re-ID handle (opd_clip.cpp, kernels_reid.hip): the model behind OPD_REID_MODEL_CLIP, the
// normalisation table and host restatement of its pre-processing, and launchers.
#pragma once
#include <memory>
#include <string>

#include "opd_reid.h"

namespace opd {

constexpr int REID_IMG = CROP_CLIP.out_h;   // the processor's 224

// Infer and check the architecture of a CLIP state dict (config.json beside weights_path names the head count); OPD_ESCHEMA names a
// missing tensor or the kernel limit a shape breaks.  No device call.
int clip_create(const StateDict& sd, const std::string& weights_path, std::unique_ptr<ReidModel>* out);

// fp16 bits of (u8 * (1/255) - mean[c]) / std[c] in the arithmetic of HF's numpy rescale + normalize: lut[c * 256 + u8], RGB order
void reid_pixel_lut(uint16_t* lut);

// Host restatement of the pre-processing kernel for ONE crop (frame [H][W][3] BGR): fp16 patch rows [tokens][3 * P * P], row 0 zero.
void reid_preprocess_host(const uint8_t* frame, int W, const ReidGeom& g, int P, const uint16_t* lut, uint16_t* out);

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
