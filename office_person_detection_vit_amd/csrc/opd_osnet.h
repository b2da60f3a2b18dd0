// opd_osnet.h — the OSNet model of the Re-ID handle (opd_osnet.cpp, kernels_osnet.hip): schema and width inference of a torchreid state
// dict, BN folding and packing, workspace layout, the forward's launch sequence, the crop geometry of its pre-processing, and launchers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <functional>
#include <string>
#include <vector>

#include "opd_loader.h"
#include "opd_reid.h"

namespace opd {

constexpr int OSNET_H = 256, OSNET_W = 128;   // torchvision Resize((256, 128)): no aspect ratio kept, no centre crop
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

struct OsnetArchC {
    int widths[4] = {0, 0, 0, 0};   // stem, conv2, conv3, conv4 stage widths
    int blocks[3] = {0, 0, 0};      // OSBlocks per stage
    int feat = 0;                   // fc width
};

// device pointers of one OSBlock (all weights BN-folded; 16-bit = fp16)
struct OsnetBlockW {
    int cin, cout, mid, hid;
    bool down;
    const f16_t* w1; const float* b1;       // conv1 [mid][cin]
    const f16_t* wl[4];                     // level t: [(5 - t) streams][mid][mid] (level 1: [4 mid][mid])
    const float* dw[4]; const float* dwb[4];   // level t: depthwise [9][4 mid], bias [4 mid] (streams < t - 1 unused)
    const float *g1w, *g1b, *g2w, *g2b;     // gate fc1 [hid][mid], fc2 [mid][hid]
    const f16_t* w3; const float* b3;       // [conv3 | downsample] [cout][mid (+ cin)], bias summed
};

struct OsnetModel {
    OsnetArchC a;
    // weights
    const f16_t* lut = nullptr;             // [3][256] fp16 normalisation table
    const f16_t* wstem = nullptr; const float* bstem = nullptr;   // [147][64] fp16 (channels padded to 64), bias [64]
    std::vector<OsnetBlockW> blocks;        // in forward order
    const f16_t* wtr[2] = {nullptr, nullptr}; const float* btr[2] = {nullptr, nullptr};   // transitions conv2 / conv3
    const f16_t* w5 = nullptr; const float* b5 = nullptr;
    const float* wfc = nullptr; const float* bfc = nullptr;   // fc^T [C][512] with BN1d folded
    // workspace (max_crops)
    f16_t *img = nullptr, *stem = nullptr, *act[3] = {nullptr, nullptr, nullptr}, *x1 = nullptr, *u = nullptr, *t = nullptr, *x2 = nullptr;
    float *gates = nullptr, *feat = nullptr;
};

// Infer and check the architecture of a torchreid OSNet state dict (every tensor the forward reads, with its shape).  OPD_ESCHEMA names
// a missing tensor or the kernel limit a width breaks.
int osnet_infer(const StateDict& sd, OsnetArchC* a);
// Fold BN into the convolutions and pack every weight: fp16 into h16, fp32 into h32 (offsets recorded in `offs`, resolved by osnet_bind)
struct OsnetOffsets { std::vector<size_t> o16, o32; };
void osnet_pack(const StateDict& sd, const OsnetArchC& a, std::vector<uint16_t>* h16, std::vector<float>* h32, OsnetOffsets* offs);
void osnet_bind(OsnetModel* m, const OsnetOffsets& offs, const f16_t* w16, const float* w32);
// workspace bytes for max_crops; with base != null the buffers are laid out from base
size_t osnet_workspace(OsnetModel* m, int max_crops, unsigned char* base);
// The forward of nb crops from the staged crop records; every launch goes through `launch(name_known_after, flops, fn)`.
using OsnetLaunch = std::function<int(double flops, const std::function<hipError_t()>& fn)>;
int osnet_enqueue(const OsnetModel& m, int nb, const ReidCrop* crops, const unsigned char* base, hipStream_t s, const OsnetLaunch& launch);

// crop geometry (reference reid_feature_extractor.py:295-350): x1 .. y2 as for CLIP; the resize is to 256 x 128 (rh, rw) with top = left
// = 0; the window is the Pillow bilinear bounds of all outputs
void osnet_geometry(double x, double y, double w, double h, int H, int W, ReidGeom* g);
// Pillow bilinear tables of one axis (all out_size outputs): bounds [out][2] absolute, coeffs [out][ksize] (22-bit fixed point)
void osnet_axis_tables(int in_size, int out_size, std::vector<int32_t>* bounds, std::vector<int32_t>* coeffs, int* ksize);
// fp16 bits of (float(u8) / 255 - mean[c]) / std[c] in torch's fp32 arithmetic (ToTensor + Normalize, ImageNet mean / std), RGB order
void osnet_pixel_lut(uint16_t* lut);
// host restatement of the pre-processing of ONE crop: [256][128][4] fp16 bits (channel 3 zero)
void osnet_preprocess_host(const uint8_t* frame, int H, int W, const ReidGeom& g, const uint16_t* lut, uint16_t* out);

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
