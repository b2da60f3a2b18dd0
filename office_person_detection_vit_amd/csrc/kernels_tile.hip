// kernels_tile.hip — tiled detection on the device (opd_detr_detect_tiled): the tiles of a frame are resampled from windows of
// the frame where it lies, and the per-tile records are merged across the seams.  No 16-bit operands: compiled once.  float64 and integer
// arithmetic only, no fused multiply-adds (compiled with -ffp-contract=off, and the pragmas of opd_tile.h).
//
//   tile_resize_u8_kernel  resize_bilinear_u8_kernel's arithmetic (kernels_untyped.hip: Pillow's two 8-bit passes, 22-bit taps, the tables of
//                          opd_resize_coeffs, the same rounding and clipping in the same order) with another source addressing: one thread
//                          per output pixel of batch index b = frame * n_tiles + tile reads rows y0[tile] + ... and columns x0[tile] + ...
//                          of frame b / n_tiles, pitch 3 * frame_w.  Byte loads: 3 * x0 is of any alignment.
//   tile_resize_ragged_u8_kernel   the same for tiles that differ in size (opd_detr_detect_tiled_ragged): batch image b has a descriptor of its own
//                          (TileRaggedDesc: window, output size oh x ow, its coefficient tables) and writes the [H][W][3] canvas of a ragged batch,
//                          H = max oh, W = max ow: inside oh x ow the pixel of tile_resize_u8_kernel (one __device__ body for both), outside 0, 0, 0,
//                          the canvas the host path builds byte for byte.  Batch image in blockIdx.y: 32-bit index arithmetic.
//   tile_merge_kernel      tiling.merge_tile_detections for one frame per workgroup: opd_tile.h::opd_tile_merge_frame, run by ONE wave.  The
//                          kernel's own part is the search of the kept list: lane l tests kept boxes l, l + 64, ... against the candidate,
//                          64 at a time in kept order, and the first set bit of the first non-empty ballot is the first kept box that absorbs
//                          it -- what the serial loop finds, since a candidate changes the kept list only AFTER its search.  One wave, so
//                          the two syncs per candidate are waits on LDS, not workgroup barriers; no atomics, nothing between workgroups,
//                          52 KiB of LDS.  Cost: candidates x ceil(kept / 64) absorb tests in sequence (a 2 x 2 frame after per-tile
//                          suppression: some tens of candidates).
#include <hip/hip_runtime.h>

#include "opd_kernels.h"
#include "opd_tile.h"

#pragma clang fp contract(off)

namespace {

using namespace opd;

// One output pixel (yo, xo) of the resize of the window at (y0, x0) of `frame` ([frame_h][frame_w][3], pitch 3 * frame_w), the body of both resize
// kernels below: Pillow's horizontal pass on the rows the vertical taps need, each rounded and clipped to 8 bits, then the vertical pass
__device__ inline void tile_resize_pixel(const uint8_t* frame, int frame_w, int y0, int x0, int yo, int xo, const int32_t* bounds_h, const int32_t* coeff_h,
                                         int ksize_h, const int32_t* bounds_v, const int32_t* coeff_v, int ksize_v, uint8_t* o) {
    const int xmin = bounds_h[2 * xo], xcnt = bounds_h[2 * xo + 1];
    const int ymin = bounds_v[2 * yo], ycnt = bounds_v[2 * yo + 1];
    const int32_t* ckh = coeff_h + (size_t)xo * ksize_h;
    const int32_t* ckv = coeff_v + (size_t)yo * ksize_v;
    const int half = 1 << 21;
    int a0 = half, a1 = half, a2 = half;
    for (int j = 0; j < ycnt; ++j) {
        // y0 + ymin + j < y0 + th <= frame_h, x0 + xmin + k < x0 + tw <= frame_w: the tables' bounds lie inside the window, the window inside the frame
        const uint8_t* row = frame + ((size_t)(y0 + ymin + j) * frame_w + x0 + xmin) * 3;
        int s0 = half, s1 = half, s2 = half;
        for (int k = 0; k < xcnt; ++k) {
            const int c = ckh[k];
            s0 += (int)row[3 * k] * c;
            s1 += (int)row[3 * k + 1] * c;
            s2 += (int)row[3 * k + 2] * c;
        }
        s0 >>= 22; s1 >>= 22; s2 >>= 22;   // arithmetic shift, then clip8
        s0 = s0 < 0 ? 0 : (s0 > 255 ? 255 : s0);
        s1 = s1 < 0 ? 0 : (s1 > 255 ? 255 : s1);
        s2 = s2 < 0 ? 0 : (s2 > 255 ? 255 : s2);
        const int c = ckv[j];
        a0 += s0 * c; a1 += s1 * c; a2 += s2 * c;
    }
    a0 >>= 22; a1 >>= 22; a2 >>= 22;
    o[0] = (uint8_t)(a0 < 0 ? 0 : (a0 > 255 ? 255 : a0));
    o[1] = (uint8_t)(a1 < 0 ? 0 : (a1 > 255 ? 255 : a1));
    o[2] = (uint8_t)(a2 < 0 ? 0 : (a2 > 255 ? 255 : a2));
}

__global__ void tile_resize_u8_kernel(const TileResizeParams p) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)p.n_frames * p.n_tiles * p.oh * p.ow) return;
    const int xo = (int)(i % p.ow);
    const size_t t = i / p.ow;
    const int yo = (int)(t % p.oh);
    const int b = (int)(t / p.oh);
    const int frame = b / p.n_tiles, tile = b - frame * p.n_tiles;
    const int y0 = p.tiles_yxhw[4 * tile], x0 = p.tiles_yxhw[4 * tile + 1];
    tile_resize_pixel(p.frames + (size_t)frame * p.frame_h * p.frame_w * 3, p.frame_w, y0, x0, yo, xo, p.bounds_h, p.coeff_h, p.ksize_h, p.bounds_v, p.coeff_v,
                      p.ksize_v, p.out + i * 3);
}

// blockIdx.y: the batch image; blockIdx.x x 256 threads: the pixels of ITS canvas, so that the divisions are 32-bit ones (H * W fits an int: the launcher)
__global__ void tile_resize_ragged_u8_kernel(const TileRaggedParams p) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= p.H * p.W) return;
    const int b = (int)blockIdx.y;
    const int yo = i / p.W, xo = i - yo * p.W;
    const int frame = b / p.n_tiles;
    const TileRaggedDesc& d = p.desc[b - frame * p.n_tiles];
    uint8_t* o = p.out + ((size_t)b * p.H * p.W + i) * 3;
    if (yo >= d.oh || xo >= d.ow) { o[0] = 0; o[1] = 0; o[2] = 0; return; }   // the padding of the canvas, as the host writes it
    // (yo < oh and xo < ow index this tile's OWN tables, of oh and ow rows; their bounds lie inside its th x tw window, the window inside the frame)
    tile_resize_pixel(p.frames + (size_t)frame * p.frame_h * p.frame_w * 3, p.frame_w, d.y0, d.x0, yo, xo, d.bounds_h, d.coeff_h, d.ksize_h, d.bounds_v, d.coeff_v,
                      d.ksize_v, o);
}

// The wave's search of the kept list (see the head of the file)
struct TileWalkWave {
    __device__ int first(const TileWork& w, int nk, const double* c, int c_tile, bool c_cut, int stride, double nms, double mrg, int* how) const {
        const int l = (int)threadIdx.x;
        for (int base = 0; base < nk; base += 64) {   // (nk is uniform: every lane takes every ballot)
            const int k = base + l;
            int h = 0;
            if (k < nk) h = opd_tile_absorb(c, c_tile, c_cut, w.box[k], w.src[k] / stride, w.cut[k] != 0, nms, mrg);
            const unsigned long long hit = __ballot(h != 0);
            if (hit) {
                const int at = __ffsll((long long)hit) - 1;
                *how = __shfl(h, at);
                return base + at;
            }
        }
        return -1;
    }
    __device__ void sync() const { __syncthreads(); }   // a workgroup of one wave: the LDS traffic drains, no barrier is waited for
    __device__ int lane() const { return (int)threadIdx.x; }
    __device__ int lanes() const { return 64; }
};

__global__ __launch_bounds__(64) void tile_merge_kernel(const TileMergeParams p) {
    __shared__ TileWork work;
    opd_tile_merge_frame(p, (int)blockIdx.x, work, TileWalkWave{});
}

}  // namespace

hipError_t opd::opd_launch_tile_resize_u8(const TileResizeParams& p, hipStream_t stream) {
    if (p.n_frames <= 0 || p.n_tiles <= 0 || p.th <= 0 || p.tw <= 0 || p.oh <= 0 || p.ow <= 0 || p.frame_h < p.th || p.frame_w < p.tw) return hipErrorInvalidValue;
    const size_t npix = (size_t)p.n_frames * p.n_tiles * p.oh * p.ow;
    if ((npix + 255) / 256 > 0x7fffffffull) return hipErrorInvalidValue;
    OPD_LAUNCH(tile_resize_u8_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, stream, p);
    return hipGetLastError();
}

// (the descriptors lie on the device: what they hold -- windows inside the frame, oh <= H, ow <= W, tables of the right sizes -- is the caller's to check)
hipError_t opd::opd_launch_tile_resize_ragged_u8(const TileRaggedParams& p, hipStream_t stream) {
    if (p.n_frames <= 0 || p.n_tiles <= 0 || p.H <= 0 || p.W <= 0 || p.frame_h <= 0 || p.frame_w <= 0 || !p.frames || !p.out || !p.desc) return hipErrorInvalidValue;
    if ((long long)p.H * p.W > 0x7fffff00ll || (long long)p.n_frames * p.n_tiles > 65535) return hipErrorInvalidValue;
    OPD_LAUNCH(tile_resize_ragged_u8_kernel, dim3((unsigned)((p.H * p.W + 255) / 256), (unsigned)(p.n_frames * p.n_tiles)), dim3(256), 0, stream, p);
    return hipGetLastError();
}

hipError_t opd::opd_launch_tile_merge(const TileMergeParams& p, hipStream_t stream) {
    if (p.n_frames < 0 || p.n_tiles < 1 || p.stride < 1 || (long long)p.n_tiles * p.stride > OPD_TILE_MAX_CAND || !p.flag) return hipErrorInvalidValue;
    if (p.n_frames == 0) return hipSuccess;
    OPD_LAUNCH(tile_merge_kernel, dim3(p.n_frames), dim3(64), 0, stream, p);
    return hipGetLastError();
}
