// opd_tile_test_api.cpp — hooks of tiled detection for tests/ (exported from libopd_hip_test.so only):
//   opd_test_tile_merge_host   opd_tile.h::opd_tile_merge_frame, the rule tile_merge_kernel runs, on the host with the serial search of the kept
//                              list: opd_detr_merge_tiles's arguments and conventions without a handle and without a HIP call, so that a
//                              machine without a GPU can hold the rule to tiling.merge_tile_detections.  (Compiled with -ffp-contract=off.)
//   opd_test_tile_resize       tile_resize_u8_kernel alone: host frames [n_frames][h][w][3] and windows of one size -> [n_frames * n_tiles][oh][ow][3]
//   opd_test_tile_resize_ragged  tile_resize_ragged_u8_kernel alone: windows of any sizes, tile t to tile_HW[t] inside an H x W canvas ->
//                              [n_frames * n_tiles][H][W][3] into the caller's array, which is uploaded first (a byte the kernel leaves out keeps its value)
#include <memory>

#include "opd_test_util.h"
#include "opd_tile.h"

using namespace opd;

namespace {

int check_windows(const char* who, const int32_t* tiles, int n_tiles, int h, int w) {
    if (!tiles || n_tiles < 1 || h < 1 || w < 1) return fail(OPD_EINVAL, std::string(who) + ": bad arguments");
    for (int t = 0; t < n_tiles; ++t) {
        const int32_t* g = tiles + 4 * t;
        if (g[0] < 0 || g[1] < 0 || g[2] < 1 || g[3] < 1 || (long long)g[0] + g[2] > h || (long long)g[1] + g[3] > w)
            return fail(OPD_EINVAL, std::string(who) + ": a tile lies outside the frame");
    }
    return OPD_OK;
}

}  // namespace

TAPI int opd_test_tile_merge_host(const opd_det* recs, const int32_t* tile_counts, int n_frames, int n_tiles, int stride, const int32_t* tiles_yxhw, int h, int w,
                                  const opd_tile_params* p, opd_tile_det* out, int32_t* counts) {
    if (!p || p->struct_size != (int32_t)sizeof(opd_tile_params)) return fail(OPD_EINVAL, "opd_test_tile_merge_host: null or mis-sized opd_tile_params");
    RCCHK(check_windows("opd_test_tile_merge_host", tiles_yxhw, n_tiles, h, w));
    if (n_frames < 0 || stride < 1 || (long long)n_tiles * stride > OPD_TILE_MAX_CAND || (n_frames > 0 && (!recs || !tile_counts || !out || !counts)))
        return fail(OPD_EINVAL, "opd_test_tile_merge_host: bad arguments");
    int32_t over = 0;
    TileMergeParams mp{recs, tile_counts, tiles_yxhw, out, counts, &over, n_frames, n_tiles, stride, h, w, p->merge_nms_threshold, p->merge_threshold, p->edge_tolerance};
    std::unique_ptr<TileWork> work(new TileWork);
    for (int f = 0; f < n_frames; ++f) opd_tile_merge_frame(mp, f, *work, TileWalkSerial{});
    return over ? fail(OPD_EINVAL, "opd_test_tile_merge_host: a tile holds more records than its slots (its frame comes back empty)") : OPD_OK;
}

TAPI int opd_test_tile_resize(const uint8_t* frames, int n_frames, int h, int w, const int32_t* tiles_yxhw, int n_tiles, int oh, int ow, uint8_t* out) {
    RCCHK(check_windows("opd_test_tile_resize", tiles_yxhw, n_tiles, h, w));
    if (!frames || !out || n_frames < 1 || oh < 1 || ow < 1) return fail(OPD_EINVAL, "opd_test_tile_resize: bad arguments");
    for (int t = 1; t < n_tiles; ++t)
        if (tiles_yxhw[4 * t + 2] != tiles_yxhw[2] || tiles_yxhw[4 * t + 3] != tiles_yxhw[3]) return fail(OPD_EINVAL, "opd_test_tile_resize: tiles of more than one size");
    const int th = tiles_yxhw[2], tw = tiles_yxhw[3];
    std::vector<int32_t> bh, kh, bv, kv;
    int ksh = 0, ksv = 0;
    opd_resize_coeffs(tw, ow, &bh, &kh, &ksh);
    opd_resize_coeffs(th, oh, &bv, &kv, &ksv);
    DevMem dm;
    const size_t n_out = (size_t)n_frames * n_tiles * oh * ow * 3;
    TileResizeParams rp{dm.up(frames, (size_t)n_frames * h * w * 3), dm.alloc<uint8_t>(n_out), dm.up(tiles_yxhw, (size_t)n_tiles * 4), n_frames, n_tiles, h, w, th, tw, oh, ow,
                        dm.up(bh.data(), bh.size()), dm.up(kh.data(), kh.size()), dm.up(bv.data(), bv.size()), dm.up(kv.data(), kv.size()), ksh, ksv};
    if (!dm.ok) return fail(OPD_ENOMEM, "opd_test_tile_resize: device allocation failed");
    HIPCHK(opd_launch_tile_resize_u8(rp, nullptr));
    HIPCHK(hipDeviceSynchronize());
    return down(out, rp.out, n_out);
}

TAPI int opd_test_tile_resize_ragged(const uint8_t* frames, int n_frames, int h, int w, const int32_t* tiles_yxhw, int n_tiles, const int32_t* tile_HW, int H, int W,
                                     uint8_t* out) {
    RCCHK(check_windows("opd_test_tile_resize_ragged", tiles_yxhw, n_tiles, h, w));
    if (!frames || !out || !tile_HW || n_frames < 1 || H < 1 || W < 1) return fail(OPD_EINVAL, "opd_test_tile_resize_ragged: bad arguments");
    for (int t = 0; t < n_tiles; ++t)
        if (tile_HW[2 * t] < 1 || tile_HW[2 * t] > H || tile_HW[2 * t + 1] < 1 || tile_HW[2 * t + 1] > W)
            return fail(OPD_EINVAL, "opd_test_tile_resize_ragged: a tile's output size lies outside the canvas");
    DevMem dm;
    std::vector<TileRaggedDesc> desc((size_t)n_tiles);
    for (int t = 0; t < n_tiles; ++t) {
        const int32_t* g = tiles_yxhw + 4 * t;
        std::vector<int32_t> bh, kh, bv, kv;
        int ksh = 0, ksv = 0;
        opd_resize_coeffs(g[3], tile_HW[2 * t + 1], &bh, &kh, &ksh);
        opd_resize_coeffs(g[2], tile_HW[2 * t], &bv, &kv, &ksv);
        desc[t] = TileRaggedDesc{g[0], g[1], g[2], g[3], tile_HW[2 * t], tile_HW[2 * t + 1], ksh, ksv,
                                 dm.up(bh.data(), bh.size()), dm.up(kh.data(), kh.size()), dm.up(bv.data(), bv.size()), dm.up(kv.data(), kv.size())};
    }
    const size_t n_out = (size_t)n_frames * n_tiles * H * W * 3;
    TileRaggedParams rp{dm.up(frames, (size_t)n_frames * h * w * 3), dm.up(out, n_out), dm.up(desc.data(), desc.size()), n_frames, n_tiles, h, w, H, W};
    if (!dm.ok) return fail(OPD_ENOMEM, "opd_test_tile_resize_ragged: device allocation failed");
    HIPCHK(opd_launch_tile_resize_ragged_u8(rp, nullptr));
    HIPCHK(hipDeviceSynchronize());
    return down(out, rp.out, n_out);
}
