// opd_osnet_test_api.cpp — kernel-level hooks of the OSNet Re-ID model for tests/ and tools/ (exported from libopd_hip_test.so only).
// Host buffers in and out; each hook allocates its device buffers, runs its launchers on the null stream and copies the result back.
#include <string.h>

#include <string>
#include <vector>

#include "opd_osnet.h"
#include "opd_test_util.h"

using namespace opd;

// the normalisation table: lut[c * 256 + u8] fp16 bits
TAPI int opd_test_osnet_lut(uint16_t* lut) {
    osnet_pixel_lut(lut);
    return OPD_OK;
}

// host restatement of the pre-processing of n boxes on one BGR frame: out [n][256][128][4] fp16 bits
TAPI int opd_test_osnet_pixels_host(const uint8_t* frame, int H, int W, const float* boxes, int n, uint16_t* out) {
    std::vector<uint16_t> lut(768);
    osnet_pixel_lut(lut.data());
    for (int i = 0; i < n; ++i) {
        ReidGeom g;
        crop_geometry(CROP_OSNET, boxes[4 * i], boxes[4 * i + 1], boxes[4 * i + 2], boxes[4 * i + 3], H, W, &g);
        osnet_preprocess_host(frame, W, g, lut.data(), out + (size_t)i * OSNET_H * OSNET_W * 4);
    }
    return OPD_OK;
}

// stem + max-pool: img [nb][256][128][4], w [147][64] fp16 bits, bias [64] -> out [nb][64][32][C0] fp16 bits
TAPI int opd_test_osnet_stem(const uint16_t* img, const uint16_t* w, const float* bias, uint16_t* out, int nb, int C0) {
    ApiScope api_scope;
    DevMem dm;
    void* di = dm.up_bytes(img, (size_t)nb * OSNET_H * OSNET_W * 4 * 2);
    void* dw = dm.up_bytes(w, 147 * 64 * 2);
    void* db = dm.up_bytes(bias, 64 * 4);
    void* ds = dm.up_bytes(nullptr, (size_t)nb * (OSNET_H / 2) * (OSNET_W / 2) * C0 * 2);
    const size_t ob = (size_t)nb * (OSNET_H / 4) * (OSNET_W / 4) * C0 * 2;
    void* dout = dm.up_bytes(nullptr, ob);
    if (!dm.ok) return fail(OPD_ENOMEM, "test alloc failed");
    HIPCHK(opd_launch_osnet_stem((const f16_t*)di, (const f16_t*)dw, (const float*)db, (f16_t*)ds, nb, C0, nullptr));
    HIPCHK(opd_launch_osnet_maxpool((const f16_t*)ds, (f16_t*)dout, nb, OSNET_H / 2, OSNET_W / 2, C0, nullptr));
    HIPCHK(hipMemcpy(out, dout, ob, hipMemcpyDeviceToHost));
    return OPD_OK;
}

// one osnet_gemm launch on host buffers: a1 [M][lda1], a2 [M][lda2] (k2 = 0: none), w [groups][N][k1 + k2] fp16 bits, bias [groups][N]
// (may be null for epi 0), res [M][ldr] (epi 2), out [M][ldo] fp16 bits (read first: columns the launch does not write keep their values)
TAPI int opd_test_osnet_gemm(int epi, const uint16_t* a1, int lda1, int k1, const uint16_t* a2, int lda2, int k2, const uint16_t* w,
                             const float* bias, const uint16_t* res, int ldr, uint16_t* out, int ldo, int M, int N, int groups, int a_gcol,
                             int o_gcol) {
    ApiScope api_scope;
    DevMem dm;
    void *da2 = nullptr, *db = nullptr, *dr = nullptr;
    void* da1 = dm.up_bytes(a1, (size_t)M * lda1 * 2);
    if (k2) da2 = dm.up_bytes(a2, (size_t)M * lda2 * 2);
    void* dw = dm.up_bytes(w, (size_t)groups * N * (k1 + k2) * 2);
    if (bias) db = dm.up_bytes(bias, (size_t)groups * N * 4);
    if (res) dr = dm.up_bytes(res, (size_t)M * ldr * 2);
    void* dout = dm.up_bytes(out, (size_t)M * ldo * 2);
    if (!dm.ok) return fail(OPD_ENOMEM, "test alloc failed");
    OsnetGemm p{};
    p.a1 = da1; p.lda1 = lda1; p.k1 = k1; p.a2 = da2; p.lda2 = lda2; p.k2 = k2; p.w = dw; p.bias = (const float*)db;
    p.res = dr; p.ldr = ldr; p.out = dout; p.ldo = ldo; p.M = M; p.N = N; p.a_gcol = a_gcol; p.o_gcol = o_gcol;
    HIPCHK(opd_launch_osnet_gemm(epi, p, groups, nullptr));
    HIPCHK(hipMemcpy(out, dout, (size_t)M * ldo * 2, hipMemcpyDeviceToHost));
    return OPD_OK;
}

// depthwise 3x3 + bias + ReLU over channels [c0, c0 + nc) of in / out [nb][H][W][ld] fp16 bits (out read first); w [9][ldw], bias [ldw]
TAPI int opd_test_osnet_dwconv(const uint16_t* in, uint16_t* out, const float* w, const float* bias, int nb, int H, int W, int ld, int c0, int nc,
                               int ldw) {
    ApiScope api_scope;
    DevMem dm;
    const size_t bytes = (size_t)nb * H * W * ld * 2;
    void* di = dm.up_bytes(in, bytes);
    void* dout = dm.up_bytes(out, bytes);
    void* dw = dm.up_bytes(w, (size_t)9 * ldw * 4);
    void* db = dm.up_bytes(bias, (size_t)ldw * 4);
    if (!dm.ok) return fail(OPD_ENOMEM, "test alloc failed");
    HIPCHK(opd_launch_osnet_dwconv((const f16_t*)di, (f16_t*)dout, (const float*)dw, (const float*)db, nb, H, W, ld, c0, nc, ldw, nullptr));
    HIPCHK(hipMemcpy(out, dout, bytes, hipMemcpyDeviceToHost));
    return OPD_OK;
}

// gate + combine of four streams t [nb * HW][4 mid] fp16 bits: gates [nb][4][mid] fp32, x2 [nb * HW][mid] fp16 bits
TAPI int opd_test_osnet_gate(const uint16_t* t, const float* w1, const float* b1, const float* w2, const float* b2, float* gates, uint16_t* x2,
                             int nb, int HW, int mid, int hid) {
    ApiScope api_scope;
    DevMem dm;
    void* dt = dm.up_bytes(t, (size_t)nb * HW * 4 * mid * 2);
    void* d1 = dm.up_bytes(w1, (size_t)hid * mid * 4);
    void* db1 = dm.up_bytes(b1, (size_t)hid * 4);
    void* d2 = dm.up_bytes(w2, (size_t)mid * hid * 4);
    void* db2 = dm.up_bytes(b2, (size_t)mid * 4);
    void* dg = dm.up_bytes(nullptr, (size_t)nb * 4 * mid * 4);
    void* dx = dm.up_bytes(nullptr, (size_t)nb * HW * mid * 2);
    if (!dm.ok) return fail(OPD_ENOMEM, "test alloc failed");
    HIPCHK(opd_launch_osnet_gate((const f16_t*)dt, (const float*)d1, (const float*)db1, (const float*)d2, (const float*)db2, (float*)dg,
                                 nb, HW, mid, hid, nullptr));
    HIPCHK(opd_launch_osnet_combine((const f16_t*)dt, (const float*)dg, (f16_t*)dx, nb, HW, mid, nullptr));
    HIPCHK(hipMemcpy(gates, dg, (size_t)nb * 4 * mid * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(x2, dx, (size_t)nb * HW * mid * 2, hipMemcpyDeviceToHost));
    return OPD_OK;
}

// 2x2 average pool [nb][H][W][C] -> [nb][H/2][W/2][C], fp16 bits
TAPI int opd_test_osnet_avgpool2(const uint16_t* in, uint16_t* out, int nb, int H, int W, int C) {
    ApiScope api_scope;
    DevMem dm;
    void* di = dm.up_bytes(in, (size_t)nb * H * W * C * 2);
    void* dout = dm.up_bytes(nullptr, (size_t)nb * H * W * C / 2);
    if (!dm.ok) return fail(OPD_ENOMEM, "test alloc failed");
    HIPCHK(opd_launch_osnet_avgpool2((const f16_t*)di, (f16_t*)dout, nb, H, W, C, nullptr));
    HIPCHK(hipMemcpy(out, dout, (size_t)nb * H * W * C / 2, hipMemcpyDeviceToHost));
    return OPD_OK;
}

// head: x [nb][HW][C] fp16 bits, wt [C][512], b [512] -> feat [nb][512] fp32
TAPI int opd_test_osnet_head(const uint16_t* x, const float* wt, const float* b, float* feat, int nb, int HW, int C) {
    ApiScope api_scope;
    DevMem dm;
    void* dx = dm.up_bytes(x, (size_t)nb * HW * C * 2);
    void* dw = dm.up_bytes(wt, (size_t)C * 512 * 4);
    void* db = dm.up_bytes(b, 512 * 4);
    void* df = dm.up_bytes(nullptr, (size_t)nb * 512 * 4);
    if (!dm.ok) return fail(OPD_ENOMEM, "test alloc failed");
    HIPCHK(opd_launch_osnet_head((const f16_t*)dx, (const float*)dw, (const float*)db, (float*)df, nb, HW, C, nullptr));
    HIPCHK(hipMemcpy(feat, df, (size_t)nb * 512 * 4, hipMemcpyDeviceToHost));
    return OPD_OK;
}
