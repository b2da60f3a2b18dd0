// opd_pack.cpp — host-side weight packers (opd_pack.h): they write to computed offsets in caller-owned buffers of the documented sizes.
#include "opd_pack.h"

#include <math.h>
#include <string.h>

#include "opd_loader.h"

// K-permutation of a [rows][K] fp16 weight matrix (K % 32 == 0) that makes two fp16-rounded 16x16 accumulator tiles a
// valid B operand: within each 32-block, slot 8g+e <- channel 4g+e, slot 8g+4+e <- channel 16+4g+e.
void opd_permute_k32(const uint16_t* w, uint16_t* out, int rows, int K) {
    for (int n = 0; n < rows; ++n)
        for (int b = 0; b < K; b += 32)
            for (int g = 0; g < 4; ++g)
                for (int e = 0; e < 4; ++e) {
                    out[(size_t)n * K + b + 8 * g + e] = w[(size_t)n * K + b + 4 * g + e];
                    out[(size_t)n * K + b + 8 * g + 4 + e] = w[(size_t)n * K + b + 16 + 4 * g + e];
                }
}

// host: [N][K] fp32 -> the split pair in MFMA-fragment order: for every (16-row tile nt, 32-wide k-step ks) 1 KiB of hi = fp16(w) followed by
// 1 KiB of lo = fp16((w - hi) * 2048); inside a KiB lane L = 16 g + li holds w[16 nt + li][32 ks + 8 g .. + 7].  out: 2 * N * K halves.
void opd_split_f16_frag(const float* w, int N, int K, uint16_t* out) {
    const int nks = K / 32;
    for (int nt = 0; nt < N / 16; ++nt)
        for (int ks = 0; ks < nks; ++ks) {
            uint16_t* blk = out + ((size_t)nt * nks + ks) * 1024;
            for (int L = 0; L < 64; ++L)
                for (int e = 0; e < 8; ++e) {
                    const float v = w[(size_t)(nt * 16 + (L & 15)) * K + ks * 32 + (L >> 4) * 8 + e];
                    const uint16_t h = fabsf(v) < 6.103515625e-5f ? (uint16_t)0 : opd::f32_to_f16(v);   // (no subnormal hi: see kernels_dec.hip::split1)
                    blk[L * 8 + e] = h;
                    blk[512 + L * 8 + e] = opd::f32_to_f16((v - opd::f16_to_f32(h)) * 2048.0f);
                }
        }
}

size_t opd_encffn_pack_bytes(int F, int tail, int front) { return (size_t)8 * opd_encffn_pieces(F / 128, tail, front) * 1024; }
// host: w1 [F][256], w2 [256][F] as 16-bit elements (fp16 or bf16), b1 [F] fp32 -> the eight per-wave streams of enc_ffn_kernel, in the order the
// kernel consumes them: G0(0) G1(0) G0(1) { G1(c+1) G2(c) G3(c) G0(c+2) } for c = 0 .. F/128 - 1 (zeros for fc1 chunks past the end).
//   G0(c): the bias piece (lane L = 16 g + li: b1[128 c + 16 w + 4 g .. + 3] as fp32), then k-steps 0 .. 3 of W1's tile (lane L:
//          w1[128 c + 16 w + li][32 ks + 8 g .. + 7]);  G1(c): k-steps 4 .. 7;
//   G2(c) / G3(c): W2's k-steps i = 0, 1 / 2, 3 of the chunk for the wave's tiles j = 0, 1 at 2 (i & 1) + j (lane L:
//          w2[(2 w + j) 16 + li][128 c + 32 i + 8 g .. + 7]).
// Tail (optional): wt [tail * 256][256] = the weight rows of the tail projection in PASS order, bt [tail * 256] its biases; per pass the bias piece
// (lane (g, li): bt[256 t + (2 w + (li >> 3)) 16 + 4 g .. + 3]) and 16 pieces in fc2's group format (group q: k-steps 2 q, 2 q + 1 of the wave's
// tiles 2 w, 2 w + 1 of that pass); five zero pieces at the end.
// Front (optional): wo [256][256] = the attention output projection; its 16 pieces (fc2's group format) lead every wave's stream.
void opd_encffn_pack(const uint16_t* w1, const float* b1, const uint16_t* w2, int F, const uint16_t* wt, const float* bt, int tail, const uint16_t* wo, unsigned char* out) {
    const int nch = F / 128;
    const int front = wo != nullptr;
    memset(out, 0, opd_encffn_pack_bytes(F, tail, front));
    for (int w = 0; w < 8; ++w) {
        unsigned char* o = out + (size_t)w * opd_encffn_pieces(nch, tail, front) * 1024;
        if (front)
            for (int q = 0; q < 4; ++q) {
                for (int L = 0; L < 64; ++L) {
                    const int g = L >> 4, li = L & 15;
                    for (int i = 0; i < 2; ++i)
                        for (int j = 0; j < 2; ++j)
                            memcpy(o + (2 * i + j) * 1024 + L * 16, wo + (size_t)((2 * w + j) * 16 + li) * 256 + 32 * (2 * q + i) + 8 * g, 16);
                }
                o += 4 * 1024;
            }
        auto g0 = [&](const int c) {   // 5 pieces
            if (c < nch)
                for (int L = 0; L < 64; ++L) {
                    const int g = L >> 4, li = L & 15;
                    memcpy(o + L * 16, b1 + 128 * c + 16 * w + 4 * g, 16);
                    for (int ks = 0; ks < 4; ++ks) memcpy(o + (1 + ks) * 1024 + L * 16, w1 + (size_t)(128 * c + 16 * w + li) * 256 + 32 * ks + 8 * g, 16);
                }
            o += 5 * 1024;
        };
        auto g1 = [&](const int c) {   // 4 pieces
            if (c < nch)
                for (int L = 0; L < 64; ++L) {
                    const int g = L >> 4, li = L & 15;
                    for (int ks = 4; ks < 8; ++ks) memcpy(o + (ks - 4) * 1024 + L * 16, w1 + (size_t)(128 * c + 16 * w + li) * 256 + 32 * ks + 8 * g, 16);
                }
            o += 4 * 1024;
        };
        auto g23 = [&](const int c, const int i0) {   // 4 pieces: k-steps i0, i0 + 1
            for (int L = 0; L < 64; ++L) {
                const int g = L >> 4, li = L & 15;
                for (int i = 0; i < 2; ++i)
                    for (int j = 0; j < 2; ++j)
                        memcpy(o + (2 * i + j) * 1024 + L * 16, w2 + (size_t)((2 * w + j) * 16 + li) * F + 128 * c + 32 * (i0 + i) + 8 * g, 16);
            }
            o += 4 * 1024;
        };
        g0(0); g1(0); g0(1);
        for (int c = 0; c < nch; ++c) { g1(c + 1); g23(c, 0); g23(c, 2); g0(c + 2); }
        for (int t = 0; t < tail; ++t) {
            for (int L = 0; L < 64; ++L) memcpy(o + L * 16, bt + 256 * t + (2 * w + ((L & 15) >> 3)) * 16 + 4 * (L >> 4), 16);
            o += 1024;
            for (int q = 0; q < 4; ++q) {
                for (int L = 0; L < 64; ++L) {
                    const int g = L >> 4, li = L & 15;
                    for (int i = 0; i < 2; ++i)
                        for (int j = 0; j < 2; ++j)
                            memcpy(o + (2 * i + j) * 1024 + L * 16, wt + (size_t)(t * 256 + (2 * w + j) * 16 + li) * 256 + 32 * (2 * q + i) + 8 * g, 16);
                }
                o += 4 * 1024;
            }
        }
    }
}
