// opd_host.h — host-only pieces of the detect path (no HIP, no device): what a CPU-only build can compile, test and run under
// AddressSanitizer / UBSan (oracle/Makefile `asan`, tests/test_host_sanitized_cpu.py): the safetensors loader (opd_loader.h),
// the Pillow coefficient tables of the device resize, the mask down-sampling, the sine position embedding, person filter + NMS; and
// the catch-all of the C-ABI, since the entry points of opd_host.cpp are defined through it like every other.
#pragma once
#include <stdint.h>

#include <exception>
#include <new>
#include <shared_mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/opd_detr.h"

namespace opd {

extern thread_local std::string g_err;   // text behind opd_last_error()
int fail(int code, const std::string& msg);

// The entry-point lock and the calling thread's hold of it (opd_device.h: ApiScope and what it is for)
extern std::shared_mutex g_api_mu;
extern thread_local std::shared_lock<std::shared_mutex>* tl_api_lock;

// No C++ exception may cross the C-ABI (it would unwind through the caller's foreign-function layer and abort the process): the body of
// EVERY function of include/opd_detr.h runs here, under the catch-all, as the one statement that does the work.  This is the lock-free
// form, for the entries that make no HIP call and must not wait behind another thread's capture (opd_version, opd_last_error, the *_info
// getters, opd_detr_set_nms, opd_person_nms*, opd_assign, opd_comm_buffers); every other entry goes through api_call (opd_device.h), which
// holds the lock around this.  `create` (API_CREATE): the body reads a weight file, whose missing tensor surfaces as std::out_of_range.
constexpr bool API_CREATE = true;
template <typename F>
int api_call_unlocked(const char* name, F&& body, bool create = false) {
    try {
        return body();
    } catch (const std::bad_alloc&) {
        return fail(OPD_ENOMEM, std::string(name) + ": out of host memory");
    } catch (const std::out_of_range& e) {
        if (create) return fail(OPD_ESCHEMA, std::string(name) + ": weight file lacks a tensor the model needs (" + e.what() + ")");
        return fail(OPD_EINVAL, std::string(name) + ": " + e.what());
    } catch (const std::exception& e) {
        return fail(OPD_EINVAL, std::string(name) + ": " + e.what());
    } catch (...) {
        return fail(OPD_EINVAL, std::string(name) + ": unknown C++ exception");
    }
}

// Valid extent of a frame on the feature map (nearest down-sampling of a top-left-rectangle pixel mask): opd_host.cpp
int valid_prefix(int valid, int in, int out);
// DetrSinePositionEmbedding for an h x w map whose valid part is the top-left vh x vw rectangle: pos [h*w][D]
void sine_pos_embed(int h, int w, int vh, int vw, int D, std::vector<float>* pos);

// fp32 -> fp16-representable fp32 for a GEMM weight matrix [rows][taps][cin] (a folded convolution kernel in the device's K order, or
// a linear layer with taps == 1), by ERROR DIFFUSION along each row's reduction instead of independent round-to-nearest: the rounding
// residual of one weight is carried into the next one of the same row, visiting the taps of one input channel first, then the next
// channel, so that the errors of neighbouring weights sum to (almost) zero.  Why: the GEMM inputs behind a ReLU are positive and
// spatially smooth, so the error of an output, sum_k dW[k] x[k], is dominated by mean(x) * sum_k dW[k] -- a random walk of K half-ulps
// under round-to-nearest, at most one half-ulp under diffusion (measured on RAW checkpoint values, tools/wround_probe.py: box drift from
// the fp16 image of the backbone kernels 7.3e-4 -> 4.6e-4, encoder map 2.5e-2 -> 1.0e-2).  Values that are fp16-exact stay untouched
// (device-exact test weights, golden vectors).  Deterministic; `taps` * `cin` entries per row.
void round_f16_diffused(float* w, size_t rows, int taps, int cin, bool bf16 = false);   // bf16: onto bfloat16 values instead

}  // namespace opd

// Pillow-exact bilinear coefficient tables (22-bit fixed point): bounds [out][2] = (first tap, taps), coeffs [out][ksize]
void opd_resize_coeffs(int in_size, int out_size, std::vector<int32_t>* bounds, std::vector<int32_t>* coeffs, int* ksize_out);
// The same tables for either Pillow filter: bilinear (= opd_resize_coeffs) or bicubic (a = -0.5, support 2; the Re-ID crops)
// restricted to the outputs [first, first + count) (tables indexed from `first`)
void opd_resize_coeffs_filter(int in_size, int out_size, bool bicubic, int first, int count, std::vector<int32_t>* bounds,
                              std::vector<int32_t>* coeffs, int* ksize_out);
