// opd_reid_test_api.cpp — kernel-level hooks of the Re-ID path for tests/ and tools/ (exported from libopd_hip_test.so only).
// Host buffers in and out; each hook allocates its device buffers, runs one launcher on the null stream and copies the result back.
#include <string.h>

#include <string>
#include <vector>

#include "opd_clip.h"
#include "opd_test_util.h"

using namespace opd;

// Host-side geometry of n boxes on an H x W frame: out[i][13] = x1 y1 x2 y2 zero rh rw top left wy0 wx0 wy1 wx1
TAPI int opd_test_reid_geometry(const float* boxes, int n, int H, int W, int32_t* out) {
    geometry_rows(CROP_CLIP, boxes, n, H, W, out);
    return OPD_OK;
}

// Pillow bicubic tables of one axis, outputs [first, first + count): bounds [count][2], coeffs [count][cap]; returns ksize or < 0
TAPI int opd_test_reid_coeffs(int in_size, int out_size, int first, int count, int32_t* bounds, int32_t* coeffs, int cap) {
    std::vector<int32_t> b, c;
    int ks = 0;
    opd_resize_coeffs_filter(in_size, out_size, CROP_CLIP.bicubic, first, count, &b, &c, &ks);
    if (ks > cap) return fail(OPD_EINVAL, "opd_test_reid_coeffs: ksize above cap");
    memcpy(bounds, b.data(), b.size() * 4);
    for (int i = 0; i < count; ++i) memcpy(coeffs + (size_t)i * cap, c.data() + (size_t)i * ks, (size_t)ks * 4);
    return ks;
}

// the normalisation table: lut[c * 256 + u8] fp16 bits
TAPI int opd_test_reid_lut(uint16_t* lut) {
    reid_pixel_lut(lut);
    return OPD_OK;
}

// host restatement of the pre-processing of n boxes on one frame: out [n][T][3 P P] fp16 bits
TAPI int opd_test_reid_pixels_host(const uint8_t* frame, int H, int W, const float* boxes, int n, int P, int T, uint16_t* out) {
    std::vector<uint16_t> lut(768);
    reid_pixel_lut(lut.data());
    const size_t per = (size_t)T * 3 * P * P;
    for (int i = 0; i < n; ++i) {
        ReidGeom g;
        crop_geometry(CROP_CLIP, boxes[4 * i], boxes[4 * i + 1], boxes[4 * i + 2], boxes[4 * i + 3], H, W, &g);
        reid_preprocess_host(frame, W, g, P, lut.data(), out + per * i);
    }
    return OPD_OK;
}

// the device pre-processing of one opd_reid_extract call (n <= max_crops): out [n][T][3 P P] fp16 bits
TAPI int opd_test_reid_pixels(opd_reid* r, const uint8_t* const* frames, const int32_t* frame_hw, int n_frames, int mem_kind, const float* boxes,
                              const int32_t* box_frame, int n, uint16_t* out) {
    return reid_test_pixels(r, frames, frame_hw, n_frames, mem_kind, boxes, box_frame, n, out);
}

// attention of `crops` crops: qkv [crops * T][3H] fp16 bits (q already scaled) -> out [crops * T][H] fp16 bits
TAPI int opd_test_reid_attention(const uint16_t* qkv, uint16_t* out, int crops, int T, int H) {
    ApiScope api_scope;
    DevMem dm;
    void* dq = dm.up_bytes(qkv, (size_t)crops * T * 3 * H * 2);
    void* dout = dm.up_bytes(nullptr, (size_t)crops * T * H * 2);
    if (!dm.ok) return fail(OPD_ENOMEM, "test alloc failed");
    HIPCHK(opd_launch_reid_attention((const f16_t*)dq, (f16_t*)dout, crops, T, H, nullptr));
    HIPCHK(hipMemcpy(out, dout, (size_t)crops * T * H * 2, hipMemcpyDeviceToHost));
    return OPD_OK;
}

// LayerNorm of rows r * row_stride of x [rows * row_stride][H] fp32: y16 [rows][H] fp16 bits; y32 (may be null) = x rewritten
TAPI int opd_test_reid_layernorm(const float* x, const float* g, const float* b, float* y32, uint16_t* y16, int rows, int row_stride, int H) {
    ApiScope api_scope;
    DevMem dm;
    const size_t xb = (size_t)rows * row_stride * H * 4;
    void* dx = dm.up_bytes(x, xb);
    void* dg = dm.up_bytes(g, (size_t)H * 4);
    void* db = dm.up_bytes(b, (size_t)H * 4);
    void* dy = dm.up_bytes(nullptr, (size_t)rows * H * 2);
    if (!dm.ok) return fail(OPD_ENOMEM, "test alloc failed");
    HIPCHK(opd_launch_reid_layernorm((const float*)dx, row_stride, (const float*)dg, (const float*)db, y32 ? (float*)dx : nullptr,
                                     (f16_t*)dy, rows, H, nullptr));
    HIPCHK(hipMemcpy(y16, dy, (size_t)rows * H * 2, hipMemcpyDeviceToHost));
    if (y32) HIPCHK(hipMemcpy(y32, dx, xb, hipMemcpyDeviceToHost));
    return OPD_OK;
}

// one linear layer: X [M][K], W [N][K] fp16 bits, bias fp32 ([N], or [period][N] for REID_EPI_F32_PBIAS), out fp16 bits or fp32
// [M][N] (for REID_EPI_F32_RESID `out` holds the residual on entry)
TAPI int opd_test_reid_gemm(int epi, const uint16_t* X, const uint16_t* W, const float* bias, int period, void* out, int M, int N, int K) {
    ApiScope api_scope;
    DevMem dm;
    void *db = nullptr;
    const bool f32 = epi == REID_EPI_F32_RESID || epi == REID_EPI_F32_PBIAS;
    const size_t ob = (size_t)M * N * (f32 ? 4 : 2);
    void* dx = dm.up_bytes(X, (size_t)M * K * 2);
    void* dw = dm.up_bytes(W, (size_t)N * K * 2);
    if (bias) db = dm.up_bytes(bias, (size_t)(epi == REID_EPI_F32_PBIAS ? period : 1) * N * 4);
    void* dout = dm.up_bytes(epi == REID_EPI_F32_RESID ? out : nullptr, ob);
    if (!dm.ok) return fail(OPD_ENOMEM, "test alloc failed");
    HIPCHK(opd_launch_reid_gemm(epi, (const f16_t*)dx, (const f16_t*)dw, (const float*)db, period, dout, M, N, K, nullptr));
    HIPCHK(hipMemcpy(out, dout, ob, hipMemcpyDeviceToHost));
    return OPD_OK;
}

// L2 normalisation of `rows` rows of y [rows][E] fp32, in place
TAPI int opd_test_reid_l2norm(float* y, int rows, int E) {
    ApiScope api_scope;
    DevMem dm;
    void* dy = dm.up_bytes(y, (size_t)rows * E * 4);
    if (!dm.ok) return fail(OPD_ENOMEM, "test alloc failed");
    HIPCHK(opd_launch_reid_l2norm((float*)dy, rows, E, nullptr));
    HIPCHK(hipMemcpy(y, dy, (size_t)rows * E * 4, hipMemcpyDeviceToHost));
    return OPD_OK;
}

// per-kernel table of `iters` eager forwards (opd_reid.cpp reid_test_kernel_table); *count = kernels seen, at most `capacity` written
TAPI int opd_test_reid_kernel_table(opd_reid* r, const uint8_t* const* frames, const int32_t* frame_hw, int n_frames, const float* boxes,
                                    const int32_t* box_frame, int n, int iters, opd_kernel_stat* out, int capacity, int* count) {
    return reid_test_kernel_table(r, frames, frame_hw, n_frames, boxes, box_frame, n, iters, out, capacity, count);
}
