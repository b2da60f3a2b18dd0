// opd_crop_test_api.cpp — hooks of the device crop planner for tests/ (exported from libopd_hip_test.so only): the plan of n boxes on an
// H x W frame three ways, in ONE output format, so that the tests compare arrays:
//   opd_test_crop_plan_device   crop_plan_kernel (kernels_crop.hip) on the boxes
//   opd_test_crop_plan_host     the host instantiation of the routines the kernel evaluates (opd_crop.h)
//   opd_test_crop_plan_staged   crop_geometry + crop_axis_tables (opd_resize_coeffs_filter), as opd_reid.cpp::stage plans opd_reid_extract
// model: OPD_REID_MODEL_CLIP / OPD_REID_MODEL_OSNET picks the CropSpec.  Per box i:
//   geom[i][13]   x1 y1 x2 y2 zero rh rw top left wy0 wx0 wy1 wx1 (as opd_test_reid_geometry)
//   meta[i][4]    ks_h, ks_v, pitch, zero of the ReidCrop record
//   src_off[i]    (int64) byte offset of the record's `src` from the frame's first pixel
//   bx[i][OW][2], by[i][OH][2]   first tap relative to the source window, tap count
//   ch[i][OW][cap], cv[i][OH][cap]   22-bit coefficients, zeros behind ks_h / ks_v (OPD_EINVAL when a tap count exceeds cap)
// A degenerate box leaves zeros behind geom and meta.
#include <string.h>

#include <algorithm>
#include <vector>

#include "opd_test_util.h"

using namespace opd;

namespace {

struct PlanOut {
    int32_t *geom, *meta;
    int64_t* src_off;
    int32_t *bx, *by, *ch, *cv;
    int cap;
};

int check_args(int model, const float* boxes, int n, int H, int W, const PlanOut& o, const CropSpec** spec) {
    if (model != OPD_REID_MODEL_CLIP && model != OPD_REID_MODEL_OSNET) return fail(OPD_EINVAL, "opd_test_crop_plan: unknown model");
    if (n < 1 || H < 1 || W < 1 || o.cap < 1 || !boxes || !o.geom || !o.meta || !o.src_off || !o.bx || !o.by || !o.ch || !o.cv)
        return fail(OPD_EINVAL, "opd_test_crop_plan: bad arguments");
    static const CropSpec clip = CROP_CLIP, osnet = CROP_OSNET;
    *spec = model == OPD_REID_MODEL_OSNET ? &osnet : &clip;
    const int OW = (*spec)->out_w, OH = (*spec)->out_h;
    memset(o.geom, 0, (size_t)n * 13 * 4);
    memset(o.meta, 0, (size_t)n * 4 * 4);
    memset(o.src_off, 0, (size_t)n * 8);
    memset(o.bx, 0, (size_t)n * OW * 2 * 4);
    memset(o.by, 0, (size_t)n * OH * 2 * 4);
    memset(o.ch, 0, (size_t)n * OW * o.cap * 4);
    memset(o.cv, 0, (size_t)n * OH * o.cap * 4);
    return OPD_OK;
}

void put_geom(const PlanOut& o, int i, const ReidGeom& g) {
    const int32_t v[13] = {g.x1, g.y1, g.x2, g.y2, g.zero, g.rh, g.rw, g.top, g.left, g.wy0, g.wx0, g.wy1, g.wx1};
    memcpy(o.geom + 13 * (size_t)i, v, sizeof v);
}

// record i and its tables (bx | by | ch | cv, compact) into the output format
int put_crop(const CropSpec& spec, const PlanOut& o, int i, int ks_h, int ks_v, int pitch, int zero, int64_t src_off, const int32_t* tables) {
    const int OW = spec.out_w, OH = spec.out_h;
    const int32_t meta[4] = {ks_h, ks_v, pitch, zero};
    memcpy(o.meta + 4 * (size_t)i, meta, sizeof meta);
    o.src_off[i] = src_off;
    if (zero) return OPD_OK;
    if (ks_h > o.cap || ks_v > o.cap) return fail(OPD_EINVAL, "opd_test_crop_plan: tap count above cap");
    memcpy(o.bx + (size_t)i * OW * 2, tables, (size_t)OW * 2 * 4);
    memcpy(o.by + (size_t)i * OH * 2, tables + 2 * OW, (size_t)OH * 2 * 4);
    const int32_t* ch = tables + 2 * OW + 2 * OH;
    const int32_t* cv = ch + (size_t)OW * ks_h;
    for (int j = 0; j < OW; ++j) memcpy(o.ch + ((size_t)i * OW + j) * o.cap, ch + (size_t)j * ks_h, (size_t)ks_h * 4);
    for (int j = 0; j < OH; ++j) memcpy(o.cv + ((size_t)i * OH + j) * o.cap, cv + (size_t)j * ks_v, (size_t)ks_v * 4);
    return OPD_OK;
}

}  // namespace

TAPI int opd_test_crop_plan_device(int model, const float* boxes, int n, int H, int W, int32_t* geom, int32_t* meta, int64_t* src_off, int32_t* bx,
                                   int32_t* by, int32_t* ch, int32_t* cv, int cap) {
    ApiScope api_scope;
    const PlanOut o{geom, meta, src_off, bx, by, ch, cv, cap};
    const CropSpec* spec = nullptr;
    RCCHK(check_args(model, boxes, n, H, W, o, &spec));
    const CropSlots cs = crop_slots(*spec, H, W);
    const size_t tables_off = align_up(sizeof(ReidCrop) * (size_t)n, 256), bytes = tables_off + (size_t)n * cs.stride;
    DevMem dm;
    unsigned char* base = static_cast<unsigned char*>(dm.up_bytes(nullptr, bytes));
    uint8_t* frame = dm.alloc<uint8_t>(16);   // (the planner computes addresses in the frame and reads none of it)
    float* dboxes = dm.up(boxes, (size_t)n * 4);
    int32_t* dgeom = zeros<int32_t>(dm, (size_t)n * 13);
    if (!dm.ok) return fail(OPD_ENOMEM, "test alloc failed");
    CropPlanParams p{};
    p.spec = *spec;
    p.boxes = dboxes; p.frames = frame; p.h = H; p.w = W; p.slots = n;
    p.base = base; p.tables_off = tables_off; p.stride = cs.stride; p.ksh_max = cs.ksh_max; p.ksv_max = cs.ksv_max;
    p.geom = dgeom;
    HIPCHK(opd_launch_crop_plan(p, n, nullptr));
    HIPCHK(hipDeviceSynchronize());
    std::vector<unsigned char> host(bytes);
    RCCHK(down(host.data(), base, bytes));
    RCCHK(down(geom, dgeom, (size_t)n * 13));
    const ReidCrop* rec = reinterpret_cast<const ReidCrop*>(host.data());
    for (int i = 0; i < n; ++i) {
        const ReidCrop& c = rec[i];
        if (!c.zero && (c.tables != (int64_t)(tables_off + (size_t)i * cs.stride) || c.ks_h > cs.ksh_max || c.ks_v > cs.ksv_max))
            return fail(OPD_EINVAL, "opd_test_crop_plan_device: crop " + std::to_string(i) + " lies outside its slot");
        RCCHK(put_crop(*spec, o, i, c.ks_h, c.ks_v, c.pitch, c.zero, c.zero ? 0 : (int64_t)(c.src - frame),
                       reinterpret_cast<const int32_t*>(host.data() + (c.zero ? tables_off : (size_t)c.tables))));
    }
    return OPD_OK;
}

TAPI int opd_test_crop_plan_host(int model, const float* boxes, int n, int H, int W, int32_t* geom, int32_t* meta, int64_t* src_off, int32_t* bx,
                                 int32_t* by, int32_t* ch, int32_t* cv, int cap) {
    const PlanOut o{geom, meta, src_off, bx, by, ch, cv, cap};
    const CropSpec* spec = nullptr;
    RCCHK(check_args(model, boxes, n, H, W, o, &spec));
    const int OW = spec->out_w, OH = spec->out_h;
    std::vector<int32_t> t;
    for (int i = 0; i < n; ++i) {
        ReidGeom g;
        crop_box_geometry(*spec, boxes[4 * i], boxes[4 * i + 1], boxes[4 * i + 2], boxes[4 * i + 3], H, W, &g);
        if (g.zero) {
            put_geom(o, i, g);
            RCCHK(put_crop(*spec, o, i, 0, 0, 0, 1, 0, nullptr));
            continue;
        }
        const int cw = g.x2 - g.x1, chh = g.y2 - g.y1;
        const int ksh = crop_ksize(cw, g.rw, spec->bicubic), ksv = crop_ksize(chh, g.rh, spec->bicubic);
        t.assign((size_t)2 * OW + 2 * OH + (size_t)OW * ksh + (size_t)OH * ksv, 0);
        int32_t *tbx = t.data(), *tby = tbx + 2 * OW, *tch = tby + 2 * OH, *tcv = tch + (size_t)OW * ksh;
        for (int j = 0; j < OW; ++j) crop_coeffs_one(cw, g.rw, spec->bicubic, g.left + j, ksh, &tbx[2 * j], &tbx[2 * j + 1], tch + (size_t)j * ksh);
        for (int j = 0; j < OH; ++j) crop_coeffs_one(chh, g.rh, spec->bicubic, g.top + j, ksv, &tby[2 * j], &tby[2 * j + 1], tcv + (size_t)j * ksv);
        g.wx0 = g.x1 + tbx[0]; g.wx1 = g.x1 + tbx[0] + tbx[1];
        g.wy0 = g.y1 + tby[0]; g.wy1 = g.y1 + tby[0] + tby[1];
        for (int j = 1; j < OW; ++j) { g.wx0 = std::min(g.wx0, g.x1 + tbx[2 * j]); g.wx1 = std::max(g.wx1, g.x1 + tbx[2 * j] + tbx[2 * j + 1]); }
        for (int j = 1; j < OH; ++j) { g.wy0 = std::min(g.wy0, g.y1 + tby[2 * j]); g.wy1 = std::max(g.wy1, g.y1 + tby[2 * j] + tby[2 * j + 1]); }
        for (int j = 0; j < OW; ++j) tbx[2 * j] -= g.wx0 - g.x1;
        for (int j = 0; j < OH; ++j) tby[2 * j] -= g.wy0 - g.y1;
        put_geom(o, i, g);
        RCCHK(put_crop(*spec, o, i, ksh, ksv, 3 * W, 0, ((int64_t)g.wy0 * W + g.wx0) * 3, t.data()));
    }
    return OPD_OK;
}

TAPI int opd_test_crop_plan_staged(int model, const float* boxes, int n, int H, int W, int32_t* geom, int32_t* meta, int64_t* src_off, int32_t* bx,
                                   int32_t* by, int32_t* ch, int32_t* cv, int cap) {
    const PlanOut o{geom, meta, src_off, bx, by, ch, cv, cap};
    const CropSpec* spec = nullptr;
    RCCHK(check_args(model, boxes, n, H, W, o, &spec));
    const int OW = spec->out_w, OH = spec->out_h;
    std::vector<int32_t> t, b0, b1, c0, c1;
    for (int i = 0; i < n; ++i) {
        ReidGeom g;
        crop_geometry(*spec, boxes[4 * i], boxes[4 * i + 1], boxes[4 * i + 2], boxes[4 * i + 3], H, W, &g);
        put_geom(o, i, g);
        if (g.zero) {
            RCCHK(put_crop(*spec, o, i, 0, 0, 0, 1, 0, nullptr));
            continue;
        }
        int ksh = 0, ksv = 0;
        crop_axis_tables(*spec, g, true, &b0, &c0, &ksh);
        crop_axis_tables(*spec, g, false, &b1, &c1, &ksv);
        for (int j = 0; j < OW; ++j) b0[2 * j] -= g.wx0 - g.x1;
        for (int j = 0; j < OH; ++j) b1[2 * j] -= g.wy0 - g.y1;
        t.clear();
        t.insert(t.end(), b0.begin(), b0.end());
        t.insert(t.end(), b1.begin(), b1.end());
        t.insert(t.end(), c0.begin(), c0.end());
        t.insert(t.end(), c1.begin(), c1.end());
        RCCHK(put_crop(*spec, o, i, ksh, ksv, 3 * W, 0, ((int64_t)g.wy0 * W + g.wx0) * 3, t.data()));
    }
    return OPD_OK;
}
