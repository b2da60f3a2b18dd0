// opd_pack.h — host-side weight packers: the layout of every pre-arranged weight of the model (opd_pack.cpp).  Plain C++ like opd_host.h (no
// HIP header, no _Float16), so tests/native/host_asan_driver.cpp runs them under AddressSanitizer; included by opd_kernels.h.
// 16-bit elements travel as raw bits (uint16_t, opd_kernels.h's f16_t).
#pragma once
#include <stddef.h>
#include <stdint.h>

// K-permutation of a [rows][K] 16-bit weight matrix (K % 32 == 0) for the 256-channel bottleneck tail (kernels_btail3.hip)
void opd_permute_k32(const uint16_t* w, uint16_t* out, int rows, int K);
// [N][K] fp32 (N % 16 == 0, K % 32 == 0) -> split fp16 pair in MFMA-fragment order, 2 * N * K halves (kernels_dec.hip)
void opd_split_f16_frag(const float* w, int N, int K, uint16_t* out);
// 1 KiB pieces per wave of the encoder FFN's weight stream (kernels_rowln.hip::enc_ffn_kernel): nch = F / 128 hidden chunks, `tail` passes, front 0 / 1
constexpr int opd_encffn_pieces(const int nch, const int tail, const int front) { return (front ? 16 : 0) + 14 + 17 * nch + (tail ? 17 * tail + 5 : 0); }
size_t opd_encffn_pack_bytes(int F, int tail, int front);
void opd_encffn_pack(const uint16_t* w1, const float* b1, const uint16_t* w2, int F, const uint16_t* wt, const float* bt, int tail, const uint16_t* wo,
                     unsigned char* out);
