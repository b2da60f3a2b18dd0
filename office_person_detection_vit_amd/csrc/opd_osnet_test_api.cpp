// opd_osnet_test_api.cpp — kernel-level hooks of the OSNet Re-ID model for tests/ and tools/ (exported from libopd_hip_test.so only).
// Host buffers in and out; each hook allocates its device buffers, runs its launchers on the null stream and copies the result back.
#include <string.h>

#include <string>
#include <vector>

#include "opd_osnet.h"
#include "opd_reid_test_util.h"

using namespace opd;

// the normalisation table: lut[c * 256 + u8] fp16 bits
TAPI int opd_test_osnet_lut(uint16_t* lut) {
    osnet_pixel_lut(lut);
    return OPD_OK;
}

// host geometry of n boxes: out[i][13] = x1 y1 x2 y2 zero rh rw top left wy0 wx0 wy1 wx1
TAPI int opd_test_osnet_geometry(const float* boxes, int n, int H, int W, int32_t* out) {
    geometry_rows(CROP_OSNET, boxes, n, H, W, out);
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
    DevBuf di, dw, db, ds, dout;
    RCCHK(up(di, img, (size_t)nb * OSNET_H * OSNET_W * 4 * 2));
    RCCHK(up(dw, w, 147 * 64 * 2));
    RCCHK(up(db, bias, 64 * 4));
    RCCHK(up(ds, nullptr, (size_t)nb * (OSNET_H / 2) * (OSNET_W / 2) * C0 * 2));
    const size_t ob = (size_t)nb * (OSNET_H / 4) * (OSNET_W / 4) * C0 * 2;
    RCCHK(up(dout, nullptr, ob));
    HIPCHK(opd_launch_osnet_stem((const f16_t*)di.p, (const f16_t*)dw.p, (const float*)db.p, (f16_t*)ds.p, nb, C0, nullptr));
    HIPCHK(opd_launch_osnet_maxpool((const f16_t*)ds.p, (f16_t*)dout.p, nb, OSNET_H / 2, OSNET_W / 2, C0, nullptr));
    HIPCHK(hipMemcpy(out, dout.p, ob, hipMemcpyDeviceToHost));
    return OPD_OK;
}

// one osnet_gemm launch on host buffers: a1 [M][lda1], a2 [M][lda2] (k2 = 0: none), w [groups][N][k1 + k2] fp16 bits, bias [groups][N]
// (may be null for epi 0), res [M][ldr] (epi 2), out [M][ldo] fp16 bits (read first: columns the launch does not write keep their values)
TAPI int opd_test_osnet_gemm(int epi, const uint16_t* a1, int lda1, int k1, const uint16_t* a2, int lda2, int k2, const uint16_t* w,
                             const float* bias, const uint16_t* res, int ldr, uint16_t* out, int ldo, int M, int N, int groups, int a_gcol,
                             int o_gcol) {
    ApiScope api_scope;
    DevBuf da1, da2, dw, db, dr, dout;
    RCCHK(up(da1, a1, (size_t)M * lda1 * 2));
    if (k2) RCCHK(up(da2, a2, (size_t)M * lda2 * 2));
    RCCHK(up(dw, w, (size_t)groups * N * (k1 + k2) * 2));
    if (bias) RCCHK(up(db, bias, (size_t)groups * N * 4));
    if (res) RCCHK(up(dr, res, (size_t)M * ldr * 2));
    RCCHK(up(dout, out, (size_t)M * ldo * 2));
    OsnetGemm p{};
    p.a1 = da1.p; p.lda1 = lda1; p.k1 = k1; p.a2 = da2.p; p.lda2 = lda2; p.k2 = k2; p.w = dw.p; p.bias = (const float*)db.p;
    p.res = dr.p; p.ldr = ldr; p.out = dout.p; p.ldo = ldo; p.M = M; p.N = N; p.a_gcol = a_gcol; p.o_gcol = o_gcol;
    HIPCHK(opd_launch_osnet_gemm(epi, p, groups, nullptr));
    HIPCHK(hipMemcpy(out, dout.p, (size_t)M * ldo * 2, hipMemcpyDeviceToHost));
    return OPD_OK;
}

// depthwise 3x3 + bias + ReLU over channels [c0, c0 + nc) of in / out [nb][H][W][ld] fp16 bits (out read first); w [9][ldw], bias [ldw]
TAPI int opd_test_osnet_dwconv(const uint16_t* in, uint16_t* out, const float* w, const float* bias, int nb, int H, int W, int ld, int c0, int nc,
                               int ldw) {
    ApiScope api_scope;
    DevBuf di, dout, dw, db;
    const size_t bytes = (size_t)nb * H * W * ld * 2;
    RCCHK(up(di, in, bytes));
    RCCHK(up(dout, out, bytes));
    RCCHK(up(dw, w, (size_t)9 * ldw * 4));
    RCCHK(up(db, bias, (size_t)ldw * 4));
    HIPCHK(opd_launch_osnet_dwconv((const f16_t*)di.p, (f16_t*)dout.p, (const float*)dw.p, (const float*)db.p, nb, H, W, ld, c0, nc, ldw, nullptr));
    HIPCHK(hipMemcpy(out, dout.p, bytes, hipMemcpyDeviceToHost));
    return OPD_OK;
}

// gate + combine of four streams t [nb * HW][4 mid] fp16 bits: gates [nb][4][mid] fp32, x2 [nb * HW][mid] fp16 bits
TAPI int opd_test_osnet_gate(const uint16_t* t, const float* w1, const float* b1, const float* w2, const float* b2, float* gates, uint16_t* x2,
                             int nb, int HW, int mid, int hid) {
    ApiScope api_scope;
    DevBuf dt, d1, db1, d2, db2, dg, dx;
    RCCHK(up(dt, t, (size_t)nb * HW * 4 * mid * 2));
    RCCHK(up(d1, w1, (size_t)hid * mid * 4));
    RCCHK(up(db1, b1, (size_t)hid * 4));
    RCCHK(up(d2, w2, (size_t)mid * hid * 4));
    RCCHK(up(db2, b2, (size_t)mid * 4));
    RCCHK(up(dg, nullptr, (size_t)nb * 4 * mid * 4));
    RCCHK(up(dx, nullptr, (size_t)nb * HW * mid * 2));
    HIPCHK(opd_launch_osnet_gate((const f16_t*)dt.p, (const float*)d1.p, (const float*)db1.p, (const float*)d2.p, (const float*)db2.p, (float*)dg.p,
                                 nb, HW, mid, hid, nullptr));
    HIPCHK(opd_launch_osnet_combine((const f16_t*)dt.p, (const float*)dg.p, (f16_t*)dx.p, nb, HW, mid, nullptr));
    HIPCHK(hipMemcpy(gates, dg.p, (size_t)nb * 4 * mid * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(x2, dx.p, (size_t)nb * HW * mid * 2, hipMemcpyDeviceToHost));
    return OPD_OK;
}

// 2x2 average pool [nb][H][W][C] -> [nb][H/2][W/2][C], fp16 bits
TAPI int opd_test_osnet_avgpool2(const uint16_t* in, uint16_t* out, int nb, int H, int W, int C) {
    ApiScope api_scope;
    DevBuf di, dout;
    RCCHK(up(di, in, (size_t)nb * H * W * C * 2));
    RCCHK(up(dout, nullptr, (size_t)nb * H * W * C / 2));
    HIPCHK(opd_launch_osnet_avgpool2((const f16_t*)di.p, (f16_t*)dout.p, nb, H, W, C, nullptr));
    HIPCHK(hipMemcpy(out, dout.p, (size_t)nb * H * W * C / 2, hipMemcpyDeviceToHost));
    return OPD_OK;
}

// head: x [nb][HW][C] fp16 bits, wt [C][512], b [512] -> feat [nb][512] fp32
TAPI int opd_test_osnet_head(const uint16_t* x, const float* wt, const float* b, float* feat, int nb, int HW, int C) {
    ApiScope api_scope;
    DevBuf dx, dw, db, df;
    RCCHK(up(dx, x, (size_t)nb * HW * C * 2));
    RCCHK(up(dw, wt, (size_t)C * 512 * 4));
    RCCHK(up(db, b, 512 * 4));
    RCCHK(up(df, nullptr, (size_t)nb * 512 * 4));
    HIPCHK(opd_launch_osnet_head((const f16_t*)dx.p, (const float*)dw.p, (const float*)db.p, (float*)df.p, nb, HW, C, nullptr));
    HIPCHK(hipMemcpy(feat, df.p, (size_t)nb * 512 * 4, hipMemcpyDeviceToHost));
    return OPD_OK;
}
