// opd_crop.h — the Pillow-exact crop path both Re-ID models share (opd_crop.cpp): what a model asks of it (CropSpec), the geometry of one
// box, the coefficient tables of one axis, the host resampler, the per-output restatement of geometry and tables that the device crop
// planner (kernels_crop.hip) and the host share, and the device resampler the two pre-processing kernels call.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <vector>

#include "../../include/opd_detr.h"
#include "opd_records.h"

namespace opd {

// The image a model asks for: out_h x out_w, Pillow bicubic (a = -0.5) or bilinear; resized to shortest edge out_h (= out_w) and cut
// to the centre window, or stretched.
struct CropSpec {
    int out_h, out_w;
    bool bicubic, keep_aspect_centre_crop;
};
constexpr CropSpec CROP_CLIP{224, 224, true, true};      // CLIPImageProcessor: shortest edge 224, centre crop 224 x 224
constexpr CropSpec CROP_OSNET{256, 128, false, false};   // torchvision Resize((256, 128))

// One crop as the pre-processing kernels read it.  Its Pillow coefficient tables (only the out_w output columns / out_h rows of the
// spec's window) lie at `tables` bytes from the upload base: int32 bx[out_w][2], by[out_h][2] (first tap relative to the source
// window, tap count), then int32 ch[out_w][ks_h], cv[out_h][ks_v] (22-bit fixed point).
struct ReidCrop {
    const uint8_t* src;   // top-left pixel (BGR) of the crop's source window
    int64_t tables;       // byte offset of the tables from the upload base
    int32_t pitch;        // bytes per source row
    int32_t zero;         // 1: degenerate box -> zero image
    int32_t ks_h, ks_v;   // taps per output column / row
};

// Geometry of one box, host-side, following the reference exactly (reid_feature_extractor.py:124-134 and 295-350):
//   x1 = int(max(0, x)), x2 = int(min(W, x + w)) (same for y); x2 <= x1 or y2 <= y1 -> zero image;
//   keep_aspect_centre_crop: resized long side int(out * long / short), centre window at ((rh - out_h) // 2, (rw - out_w) // 2);
//   otherwise rh x rw = out_h x out_w and top = left = 0;
//   the source window = Pillow bounds of all outputs of the window, in frame coordinates.
struct ReidGeom {
    int x1, y1, x2, y2;        // crop in frame pixels (x2, y2 exclusive)
    int zero;                  // degenerate
    int rh, rw;                // resized size
    int top, left;             // window offset in the resized image
    int wy0, wx0, wy1, wx1;    // source window in frame pixels (exclusive ends)
};
void crop_geometry(const CropSpec& spec, double x, double y, double w, double h, int H, int W, ReidGeom* g);

// Pillow coefficient tables of the horizontal (or vertical) axis of a non-degenerate crop, restricted to the spec's window: bounds
// [out][2] (first source index relative to x1 / y1, tap count), coeffs [out][ksize] (22-bit fixed point, normalize_coeffs_8bpc).
void crop_axis_tables(const CropSpec& spec, const ReidGeom& g, bool horizontal, std::vector<int32_t>* bounds, std::vector<int32_t>* coeffs,
                      int* ksize);

// Host restatement of the device resampler for ONE crop of frame [H][W][3] BGR: uint8 RGB [out_h][out_w][3] (zeros for a degenerate box)
void crop_resample_host(const CropSpec& spec, const uint8_t* frame, int W, const ReidGeom& g, uint8_t* rgb);

// ---- shared by the host and the device crop planner (kernels_crop.hip) -----------------------------------------------------------------
// The pieces of crop_geometry and of opd_resize_coeffs_filter (opd_host.cpp) restated per box and per OUTPUT, so that one thread can
// evaluate one output column or row: the same double operations in the same order, no fused multiply-adds (the pragma in every body;
// kernels_crop.hip is compiled with -ffp-contract=off besides).  tests/test_crop_plan_cpu.py holds the host instantiation to the two
// originals bit for bit, tests/test_detect_reid_gpu.py the device instantiation to the host one.
#define OPD_HD __host__ __device__ inline

OPD_HD int crop_py_int(double v) {   // Python's int() of a finite float (truncation), saturated far outside any frame; NaN -> 0
    if (!(v == v)) return 0;
    if (v > 1e9) return 1000000000;
    if (v < -1e9) return -1000000000;
    return (int)v;
}

// crop_geometry without the source window: crop rectangle, degeneracy, resized size, window offset
OPD_HD void crop_box_geometry(const CropSpec& spec, double x, double y, double w, double h, int H, int W, ReidGeom* g) {
#pragma clang fp contract(off)
    *g = ReidGeom{};
    g->x1 = crop_py_int(fmax(0.0, x));
    g->y1 = crop_py_int(fmax(0.0, y));
    g->x2 = crop_py_int(fmin((double)W, x + w));
    g->y2 = crop_py_int(fmin((double)H, y + h));
    g->zero = g->x2 <= g->x1 || g->y2 <= g->y1;
    g->rh = spec.out_h;
    g->rw = spec.out_w;
    if (g->zero || !spec.keep_aspect_centre_crop) return;
    const int ch = g->y2 - g->y1, cw = g->x2 - g->x1;
    const int shrt = cw <= ch ? cw : ch, lng = cw <= ch ? ch : cw;
    const int nl = (int)((double)((int64_t)spec.out_h * lng) / (double)shrt);   // int(out * long / short)
    if (cw <= ch) g->rh = nl; else g->rw = nl;
    g->top = (g->rh - spec.out_h) / 2;
    g->left = (g->rw - spec.out_w) / 2;
}

// taps per output of an axis resized from in_size to out_size (precompute_coeffs' ksize)
OPD_HD int crop_ksize(int in_size, int out_size, bool bicubic) {
#pragma clang fp contract(off)
    const double scale = (double)in_size / out_size;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = (bicubic ? 2.0 : 1.0) * filterscale;
    return (int)ceil(support) * 2 + 1;
}

OPD_HD double crop_filter_weight(bool bicubic, double a) {
#pragma clang fp contract(off)
    if (a < 0.0) a = -a;
    if (bicubic)   // Pillow's bicubic_filter, a = -0.5
        return a < 1.0 ? ((-0.5 + 2.0) * a - (-0.5 + 3.0)) * a * a + 1 : a < 2.0 ? (((a - 5) * a + 8) * a - 4) * -0.5 : 0.0;
    return a < 1.0 ? 1.0 - a : 0.0;
}

// Output `xx` of that axis: first source index, tap count, and coeffs[0, ksize) (22-bit fixed point, zeros behind the taps).  The taps
// are summed one after the other, then each is evaluated again and normalised: no array of doubles, the same values.
OPD_HD void crop_coeffs_one(int in_size, int out_size, bool bicubic, int xx, int ksize, int32_t* first, int32_t* count, int32_t* coeffs) {
#pragma clang fp contract(off)
    const double scale = (double)in_size / out_size;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = (bicubic ? 2.0 : 1.0) * filterscale;
    const double center = 0.0 + (xx + 0.5) * scale;
    double ww = 0.0;
    const double ss = 1.0 / filterscale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    xmax -= xmin;
    for (int x = 0; x < xmax; ++x) ww += crop_filter_weight(bicubic, (x + xmin - center + 0.5) * ss);
    for (int x = 0; x < ksize; ++x) {
        int32_t c = 0;
        if (x < xmax) {
            double k = crop_filter_weight(bicubic, (x + xmin - center + 0.5) * ss);
            if (ww != 0.0) k /= ww;
            const double v = k * (double)(1 << 22);
            c = k < 0 ? (int)(-0.5 + v) : (int)(0.5 + v);
        }
        coeffs[x] = c;
    }
    *first = xmin;
    *count = xmax;
}

// The staging layout of a fused call (opd_detr_detect_frames_reid): every crop slot owns `stride` bytes of tables, sized for the
// largest tap counts a crop of an h x w frame can have.  An axis is never resized from more than the frame's edge to less than the
// spec's, and ksize grows with in / out, so the whole frame stretched to the output bounds it.
struct CropSlots { int ksh_max, ksv_max; size_t stride; };
inline CropSlots crop_slots(const CropSpec& spec, int h, int w) {
    CropSlots s;
    s.ksh_max = crop_ksize(w, spec.out_w, spec.bicubic);
    s.ksv_max = crop_ksize(h, spec.out_h, spec.bicubic);
    s.stride = (4 * ((size_t)2 * spec.out_w + 2 * spec.out_h + (size_t)spec.out_w * s.ksh_max + (size_t)spec.out_h * s.ksv_max) + 15) / 16 * 16;
    return s;
}

// crop_select_kernel: the records of the view (opd_records.h) that count, are labelled `label` and have a valid key, in (frame, record index) order
// -> slot[k] = frame * stride + record_key and rec[k] = frame * stride + record index for k < slots, and their number *n_person (which may exceed slots)
struct CropSelectParams {
    RecordView view;
    int label, slots;
    int32_t *slot, *rec, *n_person;
};
// crop_plan_kernel: one workgroup per crop slot k < nb writes crops[k] and its tables at base + tables_off + k * stride.  The box is the float32 box
// of record rec[k] of the view (k < min(*n_person, slots), else a zero crop) or, for the test hook, boxes[k] on frame 0.
struct CropPlanParams {
    CropSpec spec;
    RecordView view; const int32_t* rec; const int32_t* n_person;
    const float* boxes;           // non-null: [nb][4] xywh instead of the records
    const uint8_t* frames;        // [n_frames][h][w][3]
    int h, w, slots;
    unsigned char* base;          // the upload base: crops at 0
    size_t tables_off, stride;
    int ksh_max, ksv_max;
    int32_t* geom;                // nullable (test hook): [nb][13] as opd_test_reid_geometry
};
hipError_t opd_launch_crop_select(const CropSelectParams& p, hipStream_t stream);
hipError_t opd_launch_crop_plan(const CropPlanParams& p, int nb, hipStream_t stream);

// ---- device side --------------------------------------------------------------------------------------------------------------------
struct CropRgb { int c[3]; };

__device__ __forceinline__ int crop_clip8(int v) {
    v >>= 22;   // arithmetic shift, then clip to uint8 (Pillow's clip8)
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// Output pixel (xo, yo) of crop c (tables staged for an OW x OH window).  Pillow's resampler rounds the horizontal pass to uint8, then
// runs the vertical pass over those rows; a pixel depends on its own row's and column's taps only, so the window alone is exact.
__device__ __forceinline__ CropRgb crop_resample_pixel(const ReidCrop& c, const unsigned char* __restrict__ base, int xo, int yo, int OW, int OH) {
    CropRgb out{{0, 0, 0}};
    if (c.zero) return out;
    const int32_t* bx = reinterpret_cast<const int32_t*>(base + c.tables);
    const int32_t* by = bx + 2 * OW;
    const int32_t* ch = by + 2 * OH + (size_t)xo * c.ks_h;
    const int32_t* cv = by + 2 * OH + (size_t)OW * c.ks_h + (size_t)yo * c.ks_v;
    const int xmin = bx[2 * xo], xcnt = bx[2 * xo + 1];
    const int ymin = by[2 * yo], ycnt = by[2 * yo + 1];
    const int half = 1 << 21;
    int a0 = half, a1 = half, a2 = half;
    for (int j = 0; j < ycnt; ++j) {
        const uint8_t* row = c.src + (size_t)(ymin + j) * c.pitch + (size_t)xmin * 3;
        int s0 = half, s1 = half, s2 = half;
        for (int k = 0; k < xcnt; ++k) {
            const int w = ch[k];
            s0 += (int)row[3 * k] * w;
            s1 += (int)row[3 * k + 1] * w;
            s2 += (int)row[3 * k + 2] * w;
        }
        const int w = cv[j];
        a0 += crop_clip8(s0) * w; a1 += crop_clip8(s1) * w; a2 += crop_clip8(s2) * w;
    }
    out.c[0] = crop_clip8(a2);   // BGR -> RGB
    out.c[1] = crop_clip8(a1);
    out.c[2] = crop_clip8(a0);
    return out;
}

}  // namespace opd
