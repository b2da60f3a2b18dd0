// opd_crop.cpp — host side of the crop path of the Re-ID models (opd_crop.h): box geometry, Pillow coefficient tables, host resampler.
#include <math.h>
#include <string.h>

#include <algorithm>

#include "opd_crop.h"
#include "opd_host.h"

namespace opd {

static int py_int(double v) {   // Python's int() of a finite float (truncation), saturated far outside any frame
    if (!(v == v)) return 0;
    if (v > 1e9) return 1000000000;
    if (v < -1e9) return -1000000000;
    return (int)v;
}

void crop_axis_tables(const CropSpec& spec, const ReidGeom& g, bool horizontal, std::vector<int32_t>* bounds, std::vector<int32_t>* coeffs,
                      int* ksize) {
    if (horizontal) opd_resize_coeffs_filter(g.x2 - g.x1, g.rw, spec.bicubic, g.left, spec.out_w, bounds, coeffs, ksize);
    else opd_resize_coeffs_filter(g.y2 - g.y1, g.rh, spec.bicubic, g.top, spec.out_h, bounds, coeffs, ksize);
}

void crop_geometry(const CropSpec& spec, double x, double y, double w, double h, int H, int W, ReidGeom* g) {
    memset(g, 0, sizeof *g);
    // fmax / fmin return the number when the other operand is NaN, as Python's max(0, x) / min(W, x) do
    g->x1 = py_int(fmax(0.0, x));
    g->y1 = py_int(fmax(0.0, y));
    g->x2 = py_int(fmin((double)W, x + w));
    g->y2 = py_int(fmin((double)H, y + h));
    g->zero = g->x2 <= g->x1 || g->y2 <= g->y1;
    g->rh = spec.out_h;
    g->rw = spec.out_w;
    if (g->zero) return;
    if (spec.keep_aspect_centre_crop) {
        const int ch = g->y2 - g->y1, cw = g->x2 - g->x1;
        const int shrt = cw <= ch ? cw : ch, lng = cw <= ch ? ch : cw;
        const int nl = (int)((double)((int64_t)spec.out_h * lng) / (double)shrt);   // int(out * long / short)
        if (cw <= ch) g->rh = nl; else g->rw = nl;
        g->top = (g->rh - spec.out_h) / 2;
        g->left = (g->rw - spec.out_w) / 2;
    }
    std::vector<int32_t> b, c;
    int ks;
    for (int horizontal = 0; horizontal < 2; ++horizontal) {
        crop_axis_tables(spec, *g, horizontal, &b, &c, &ks);
        const int o = horizontal ? g->x1 : g->y1;
        int lo = o + b[0], hi = o + b[0] + b[1];
        for (size_t k = 2; k < b.size(); k += 2) { lo = std::min(lo, o + b[k]); hi = std::max(hi, o + b[k] + b[k + 1]); }
        (horizontal ? g->wx0 : g->wy0) = lo;
        (horizontal ? g->wx1 : g->wy1) = hi;
    }
}

void crop_resample_host(const CropSpec& spec, const uint8_t* frame, int W, const ReidGeom& g, uint8_t* rgb) {
    memset(rgb, 0, (size_t)spec.out_h * spec.out_w * 3);
    if (g.zero) return;
    std::vector<int32_t> bx, by, chh, cvv;
    int ksh = 0, ksv = 0;
    crop_axis_tables(spec, g, true, &bx, &chh, &ksh);
    crop_axis_tables(spec, g, false, &by, &cvv, &ksv);
    auto clip8 = [](int v) { v >>= 22; return v < 0 ? 0 : (v > 255 ? 255 : v); };
    for (int yo = 0; yo < spec.out_h; ++yo)
        for (int xo = 0; xo < spec.out_w; ++xo) {
            const int half = 1 << 21;
            int a[3] = {half, half, half};
            for (int j = 0; j < by[2 * yo + 1]; ++j) {
                const uint8_t* row = frame + ((size_t)(g.y1 + by[2 * yo] + j) * W + g.x1 + bx[2 * xo]) * 3;
                int s[3] = {half, half, half};
                for (int k = 0; k < bx[2 * xo + 1]; ++k)
                    for (int c = 0; c < 3; ++c) s[c] += (int)row[3 * k + c] * chh[(size_t)xo * ksh + k];
                for (int c = 0; c < 3; ++c) a[c] += clip8(s[c]) * cvv[(size_t)yo * ksv + j];
            }
            for (int c = 0; c < 3; ++c) rgb[((size_t)yo * spec.out_w + xo) * 3 + 2 - c] = (uint8_t)clip8(a[c]);   // BGR -> RGB
        }
}

}  // namespace opd
