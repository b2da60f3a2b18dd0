// opd_crop.h — the Pillow-exact crop path both Re-ID models share (opd_crop.cpp): what a model asks of it (CropSpec), the geometry of one
// box, the coefficient tables of one axis, the host resampler, and the device resampler the two pre-processing kernels call.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

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
