// opd_test_util.h — test-only: what the hook files of libopd_hip_test.so (opd_*test*_api.cpp) share.  A hook is exported by TAPI and by
// nothing else; its device buffers live in a DevMem (opd_device.h), whose sticky `ok` flag is the ONE allocation check a hook makes.
#pragma once
#include <string.h>

#include <functional>
#include <vector>

#include "opd_crop.h"
#include "opd_device.h"
#include "opd_kernels.h"

#define TAPI extern "C" __attribute__((visibility("default")))

namespace opd {

// Launch options of the kernel hooks (test infrastructure only; the kernel tests are single-threaded): bits 8-10 = forced tile height
// (4 / 5 / 6 x 32 rows), bit 5 = flat-address tile staging (the path tensors beyond 2 GiB take), bit 13 = the L2 warm-up of the weights at
// launch start (ConvGemmParams::wprefetch, what the model's forward sets), bit 0 of the second word = k-loop gemm + LayerNorm kernel also
// for K == 256; the 16-bit operand type the hooks launch with (OPD_DT_BF16: their uint16 buffers hold bfloat16 bit patterns).
// enc_ffn_kernel's own warm-up (EncFfnParams::wprefetch), and the number of per-frame position tables of the position-shadow hooks
// (0: `pos` is one [period][256] table; B > 0: `pos` is [B][period][256] and the kernels read it through a device array of B pointers).
// Set by the opd_test_set_* hooks of opd_test_api.cpp, which defines them.
extern __attribute__((visibility("hidden"))) int g_conv_flags, g_gemm_ln_kloop, g_test_dtype, g_encffn_wprefetch, g_pos_frames, g_btail_dbg;

inline void apply_conv_flags(ConvGemmParams& p, int flags) {
    p.force_mt = (flags >> 8) & 7;
    p.flat_staging = (flags >> 5) & 1;
    p.wprefetch = (flags >> 13) & 1;
}

// `count` elements on the device with every byte set to `byte` (the bench hooks: 0x2c for activations, fp16 0x2c2c ~ 0.065, 0x1c for weights)
template <typename T>
T* filled(DevMem& dm, size_t count, int byte) {
    T* d = dm.alloc<T>(count);
    if (d && count && hipMemset(d, byte, count * sizeof(T)) != hipSuccess) { dm.ok = false; return nullptr; }
    return d;
}
template <typename T>
T* zeros(DevMem& dm, size_t count) { return filled<T>(dm, count, 0); }
inline uint16_t* filled16(DevMem& dm, size_t count, int byte) { return filled<uint16_t>(dm, count, byte); }

// host[0, count) = dev[0, count).  A hook synchronises the device ONCE before its first copy back, so that a kernel fault is that call's error.
template <typename T>
int down(T* host, const T* dev, size_t count) {
    HIPCHK(hipMemcpy(host, dev, count * sizeof(T), hipMemcpyDeviceToHost));
    return OPD_OK;
}
// an output that is fp32 or 16-bit by a flag of the hook (ConvGemmParams::out_f32)
inline void* alloc_out(DevMem& dm, size_t count, int f32) { return f32 ? (void*)dm.alloc<float>(count) : (void*)dm.alloc<uint16_t>(count); }
inline int down_out(void* host, const void* dev, size_t count, int f32) {
    return f32 ? down((float*)host, (const float*)dev, count) : down((uint16_t*)host, (const uint16_t*)dev, count);
}

// The race screen of the kernel hooks.  A kernel that orders its LDS-DMA traffic by counted waits and raw barriers can carry a wait that is one
// too permissive and still pass every reference check as long as the data happens to land in time; what shows it is the same launch many times
// under varying memory latency with bit-identical outputs required.  The hooks of those kernels in opd_test_api.cpp therefore launch through
// launch_repeated: `launch(rep)` issues the hook's launch (or launches) on the null stream, `outs` are the buffers it only writes (`fill`: the
// byte the hook initialises them with, 0xff for a buffer it merely allocates, so that a store that was skipped shows), `inplace` the buffers a
// launch both reads and overwrites.  A null or empty buffer is ignored.
//   repeat count off (the default): exactly launch(0), nothing else.
//   reps >= 2 (opd_test_set_repeat, or the `reps` argument): a pristine device copy of every in-place buffer is taken; every repetition restores
//     them, refills the outputs, starts a 256-MiB device-to-device copy on a second, non-blocking stream (so that DMA latencies vary between
//     repetitions), launches, and takes opd_launch_checksum of every buffer into a slot block of its own.  After ONE device synchronisation the
//     repetitions whose blocks differ from repetition 0's are counted; opd_test_repeat_result reports (launches, n_diff) of the last call.
// The buffers are left as the last repetition wrote them, so the hook copies back and its test compares with the reference as ever.  A buffer
// whose size is no multiple of 4 is refused under repetition: the checksum sums whole 32-bit words and would pass over its tail.
// Inside `launch`, every launcher call is written LAUNCHED(opd_launch_x(...)): a failure is then reported under that call's text, as HIPCHK
// reports it (a refused launch names its launcher in opd_last_error).
extern __attribute__((visibility("hidden"))) const char* g_launch_expr;
inline hipError_t launched(const char* expr, hipError_t e) {
    if (e != hipSuccess) g_launch_expr = expr;
    return e;
}
#define LAUNCHED(expr) opd::launched(#expr, (expr))
struct RepOut { void* ptr; size_t bytes; int fill; };
struct RepInPlace { void* ptr; size_t bytes; };
constexpr int REPEAT_DEFAULT = -1;   // `reps`: what opd_test_set_repeat set
int launch_repeated(const std::function<hipError_t(int)>& launch, const std::vector<RepOut>& outs, const std::vector<RepInPlace>& inplace = {},
                    int reps = REPEAT_DEFAULT);

// `warm` untimed launches, then `iters` launches back to back on the null stream between two events: *us = microseconds per launch.
// `launch` returns a hipError_t; the events are destroyed on every path.
template <typename F>
int time_launches(int warm, int iters, F&& launch, float* us) {
    hipEvent_t ev[2] = {nullptr, nullptr};
    auto timed = [&]() -> int {
        HIPCHK(hipEventCreate(&ev[0]));
        HIPCHK(hipEventCreate(&ev[1]));
        for (int i = 0; i < warm; ++i) HIPCHK(launch());
        HIPCHK(hipEventRecord(ev[0], nullptr));
        for (int i = 0; i < iters; ++i) HIPCHK(launch());
        HIPCHK(hipEventRecord(ev[1], nullptr));
        HIPCHK(hipEventSynchronize(ev[1]));
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, ev[0], ev[1]));
        *us = ms * 1000.f / iters;
        return OPD_OK;
    };
    const int rc = timed();
    for (hipEvent_t e : ev)
        if (e) (void)hipEventDestroy(e);
    return rc;
}

// The geometry of a convolution as an implicit GEMM: M = B * OH * OW rows, K = KH * KW * Cin (the stem and the dual-source hooks set their own K after)
inline void conv_geometry(ConvGemmParams& p, int B, int H, int W, int Cin, int OH, int OW, int N, int KH, int KW, int stride, int pad) {
    p.B = B; p.H = H; p.W = W; p.Cin = Cin; p.OH = OH; p.OW = OW; p.N = N; p.KH = KH; p.KW = KW; p.stride = stride; p.pad = pad;
    p.M = B * OH * OW; p.K = KH * KW * Cin;
}
// ... of a linear layer [M][K] x [N][K]^T: M frames of one pixel
inline void pointwise_geometry(ConvGemmParams& p, int M, int N, int K) { conv_geometry(p, M, 1, 1, K, 1, 1, N, 1, 1, 1, 0); }

// A fused bottleneck tail on x1 [B][H][W][C1] (3x3 pad 1, stride 1 or 2), and its 1x1 weights w2 [4 * C1][C1] / w3 [C3][4 * C1] (C3 > 0) from
// plain K order: the stage-3 kernel (C1 == 256) takes them K-permuted, the stage 1-2 kernel as they are
inline void btail_geometry(BtailParams& p, int B, int H, int W, int stride, int C1, int C3) {
    p.B = B; p.H = H; p.W = W; p.OH = (H - 1) / stride + 1; p.OW = (W - 1) / stride + 1; p.stride = stride;
    p.M = B * p.OH * p.OW; p.C1 = C1; p.C3 = C3;
}
inline void btail_weights(DevMem& dm, BtailParams& p, int C1, int C3, const uint16_t* w2, const uint16_t* w3) {
    const int C2 = 4 * C1;
    std::vector<uint16_t> w2p(w2, w2 + (size_t)C2 * C1), w3p;
    if (C3) w3p.assign(w3, w3 + (size_t)C3 * C2);
    if (C1 == 256) {
        opd_permute_k32(w2, w2p.data(), C2, C1);
        if (C3) opd_permute_k32(w3, w3p.data(), C3, C2);
    }
    p.w2p = dm.up(w2p.data(), w2p.size());
    p.w3p = C3 ? dm.up(w3p.data(), w3p.size()) : nullptr;
}

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
