// opd_reid_test_util.h — test-only: what the hooks of opd_reid_test_api.cpp and opd_osnet_test_api.cpp share.
#pragma once
#include <string.h>

#include "opd_reid.h"

#define TAPI extern "C" __attribute__((visibility("default")))

namespace opd {

// Host-side geometry of n boxes on an H x W frame: out[i][13] = x1 y1 x2 y2 zero rh rw top left wy0 wx0 wy1 wx1
inline void geometry_rows(const CropSpec& spec, const float* boxes, int n, int H, int W, int32_t* out) {
    for (int i = 0; i < n; ++i) {
        ReidGeom g;
        crop_geometry(spec, boxes[4 * i], boxes[4 * i + 1], boxes[4 * i + 2], boxes[4 * i + 3], H, W, &g);
        const int32_t v[13] = {g.x1, g.y1, g.x2, g.y2, g.zero, g.rh, g.rw, g.top, g.left, g.wy0, g.wx0, g.wy1, g.wx1};
        memcpy(out + 13 * i, v, sizeof v);
    }
}

}  // namespace opd
