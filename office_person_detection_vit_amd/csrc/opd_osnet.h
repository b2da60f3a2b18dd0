// opd_osnet.h — the OSNet model of the Re-ID handle (opd_osnet.cpp, kernels_osnet.hip): the model behind OPD_REID_MODEL_OSNET, the
// normalisation table and host restatement of its pre-processing, and launchers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <memory>

#include "opd_reid.h"

namespace opd {

constexpr int OSNET_H = CROP_OSNET.out_h, OSNET_W = CROP_OSNET.out_w;   // 256 x 128
constexpr int OSNET_FEAT = 512;

// one 1x1-convolution launch (osnet_gemm_kernel): out[m][z o_gcol + n] = epi(sum_k [a1 | a2][m][k] W[z][n][k]) for groups z
struct OsnetGemm {
    const void* a1; int lda1, k1;   // first K segment, column z * a_gcol of group z
    const void* a2; int lda2, k2;   // optional second K segment (k2 = 0: none): the downsample's block input
    const void* w;                  // fp16 [groups][N][k1 + k2]
    const float* bias;              // [groups][N] (not read by OSNET_EPI_NONE)
    const void* res; int ldr;       // OSNET_EPI_RESID_RELU: fp16 identity [M][ldr]
    void* out; int ldo;
    int M, N;
    int a_gcol, o_gcol;
};

// Infer and check the architecture of a torchreid OSNet state dict; OPD_ESCHEMA names a missing tensor or the kernel limit a width
// breaks.  No device call.
int osnet_create(const StateDict& sd, std::unique_ptr<ReidModel>* out);

// fp16 bits of (float(u8) / 255 - mean[c]) / std[c] in torch's fp32 arithmetic (ToTensor + Normalize, ImageNet mean / std), RGB order
void osnet_pixel_lut(uint16_t* lut);
// host restatement of the pre-processing of ONE crop: [256][128][4] fp16 bits (channel 3 zero)
void osnet_preprocess_host(const uint8_t* frame, int W, const ReidGeom& g, const uint16_t* lut, uint16_t* out);

}  // namespace opd

// ---- launchers (kernels_osnet.hip) --------------------------------------------------------------------------------------------------------
enum { OSNET_EPI_NONE = 0, OSNET_EPI_RELU = 1, OSNET_EPI_RESID_RELU = 2 };
// crop + BGR->RGB + Pillow bilinear to 256 x 128 + normalise -> img [crops][256][128][4] fp16
hipError_t opd_launch_osnet_preprocess(const opd::ReidCrop* crops, const unsigned char* base, const f16_t* lut, f16_t* img, int ncrops,
                                       hipStream_t stream);
// 7x7 / 2 conv (weights [147][64] fp16, bias [64]) + ReLU: img -> out [crops][128][64][C0]
hipError_t opd_launch_osnet_stem(const f16_t* img, const f16_t* w, const float* bias, f16_t* out, int ncrops, int C0, hipStream_t stream);
hipError_t opd_launch_osnet_maxpool(const f16_t* in, f16_t* out, int ncrops, int H, int W, int C, hipStream_t stream);
// N % 16 == 0, k1 and k2 multiples of 8 (zero-padded to 32 inside)
hipError_t opd_launch_osnet_gemm(int epi, const opd::OsnetGemm& p, int groups, hipStream_t stream);
hipError_t opd_launch_osnet_dwconv(const f16_t* in, f16_t* out, const float* w, const float* bias, int ncrops, int H, int W, int ld, int c0, int nc,
                                   int ldw, hipStream_t stream);
// gates [crops][4][mid] fp32 of the four streams t [crops * HW][4 mid]
hipError_t opd_launch_osnet_gate(const f16_t* t, const float* w1, const float* b1, const float* w2, const float* b2, float* gates, int ncrops, int HW,
                                 int mid, int hid, hipStream_t stream);
hipError_t opd_launch_osnet_combine(const f16_t* t, const float* gates, f16_t* x2, int ncrops, int HW, int mid, hipStream_t stream);
hipError_t opd_launch_osnet_avgpool2(const f16_t* in, f16_t* out, int ncrops, int H, int W, int C, hipStream_t stream);
// global mean of x [crops][HW][C] -> fc (wt [C][512], b [512]) -> ReLU -> L2 normalisation -> feat [crops][512]
hipError_t opd_launch_osnet_head(const f16_t* x, const float* wt, const float* b, float* feat, int ncrops, int HW, int C, hipStream_t stream);
