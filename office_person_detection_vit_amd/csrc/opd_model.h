// opd_model.h — PRIVATE header of libopd_hip: the device model (weights, workspace, per-resolution plans, graph cache) behind the opaque
// `opd_detr` handle of include/opd_detr.h.  Included by opd_weights.cpp (build_weights), opd_model.cpp (workspace, plans, the forward), opd_api.cpp (the C-ABI and the
// detect pipeline behind it), opd_comm.cpp, and opd_test_model_api.cpp / opd_test_bench_api.cpp (the test hooks of libopd_hip_test.so that reach into a handle to flip
// its fusion switches, or plan a trunk or the transformer behind it); never installed, never seen by a caller.
#pragma once
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <initializer_list>
#include <memory>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <vector>

#include "opd_device.h"
#include "opd_kernels.h"
#include "opd_loader.h"

namespace opd {

// (g_err / fail: opd_host.cpp)

struct Conv {
    f16_t* w = nullptr;
    f16_t* wp = nullptr;  // 1x1 only: the same weights K-permuted for the fused bottleneck tail (opd_permute_k32's order)
    float* bias = nullptr;
    int Cin = 0, Cout = 0, KH = 1, KW = 1, stride = 1, pad = 0, K = 0;
    bool stem = false;
};
struct Lin {
    f16_t* w = nullptr;
    float* b = nullptr;
    int N = 0, K = 0;
};
struct LNp {
    float* g = nullptr;
    float* b = nullptr;
};
struct Block {
    Conv c0, c1, c2, sc;
    bool has_sc = false;
    float* bias2sc = nullptr;   // c2.bias + sc.bias (fp32): the fused bottleneck tail adds the shortcut GEMM into the expand's accumulators
    f16_t* w2sc = nullptr;      // [Cout][c2.K + sc.Cin] = [W2 | Wsc] per output channel: the dual-source expand GEMM of stages 3-4
};
// Which packed weight forms build_weights creates: one rule each, read by build_weights and by the planners (which must not probe pointers)
inline bool conv_has_kperm(const Conv& c) { return c.KH == 1 && c.KW == 1 && c.Cin % 32 == 0 && c.Cin <= 1024; }   // Conv::wp
inline bool block_has_bias2sc(const Block& b) { return b.has_sc && b.sc.Cout == b.c2.Cout; }                      // Block::bias2sc
inline bool block_has_w2sc(const Block& b) {                                                                       // Block::w2sc
    return block_has_bias2sc(b) && b.sc.KH == 1 && b.c2.KH == 1 && b.c2.Cout % 128 == 0 && b.c2.Cin >= 128;
}
inline bool enc_has_ffn_pack(const Arch& a) { return a.d_model == 256 && a.ffn % 128 == 0; }                      // EncLayer::ffn_pack
// Tail passes (256 output columns each) that the pack of encoder layer i carries, *pos of them on x + pos: the next layer's q | k | v, or behind
// the last layer the decoder's memory k of every layer, then v of every layer, while enc_ffn_kernel takes that many passes
inline int enc_pack_tail(const Arch& a, int i, int* pos = nullptr) {
    const bool last = i + 1 == a.enc_layers;
    const int n = !last ? 3 : 2 * a.dec_layers <= 16 ? 2 * a.dec_layers : 0;
    if (pos) *pos = !last ? 2 : n / 2;
    return n;
}
inline bool dec_has_frag_weights(const Arch& a) { return a.d_model % 32 == 0 && a.ffn % 32 == 0; }                // DecLayer::*_f
inline bool heads_have_frag_weights(const Arch& a) { return a.d_model == 256 && a.ncls <= 128; }                  // DetrWeights::wc_f, w1_f, w2_f
struct EncLayer {
    f16_t* wqkv = nullptr;  // [768][256] = [Wq; Wk; Wv]
    float* bqkv = nullptr;  // [768] = [bq; bk; bv] (pos_shadow path: plain bias vector)
    Lin o, fc1, fc2;
    LNp ln1, ln2;
    // the attention output projection, then fc1 / b1 / fc2, as the eight per-wave streams of enc_ffn_kernel (opd_encffn_pack; enc_has_ffn_pack),
    // followed by the weights of the block's TAIL projection (enc_pack_tail passes).  Where a pass stores: column tail_col[t] of rows tail_ld wide
    unsigned char* ffn_pack = nullptr;
    int tail_pos = 0, tail_ld = 0;
    int tail_col[16] = {};
};
struct DecLayer {
    f16_t* wqkv = nullptr;  // self-attention [768][256]
    f16_t* wq_c = nullptr;  // cross-attention query projection [256][256]
    Lin so, co, fc1, fc2;
    LNp ln1, ln2, ln3;
    float* rb_self = nullptr;  // [Q][768] = qpos.[Wq;Wk;0]^T + [bq;bk;bv]
    float* rb_q = nullptr;     // [Q][256] = qpos.Wq_c^T + bq_c
    // fused decoder (kernels_dec.hip): every linear layer's weights as split fp16 pairs, w = hi + lo / 2048, in MFMA-fragment order
    f16_t *wqkv_f = nullptr, *so_f = nullptr, *wqc_f = nullptr, *co_f = nullptr, *fc1_f = nullptr, *fc2_f = nullptr;
};

struct Plan {  // everything that depends on the feature-map size (h, w)
    int fh = 0, fw = 0;
    int vh = 0, vw = 0;          // valid (unpadded) rows / columns of the feature map this fold was built for (== fh, fw unless ragged)
    std::vector<float*> rb_enc;  // per encoder layer [hw][768]
    float* rb_kv = nullptr;      // [hw][dec_layers*512]
    float* d_pos = nullptr;      // [hw][256] the sine position embedding itself (pos_shadow path)
};

struct Dims {
    int B, H, W, H1, W1, H2, W2;
    int stage_h[4], stage_w[4];   // output maps of stages 1-4
};

inline int down2(int n) { return (n - 1) / 2 + 1; }

// Switches of the forward plan: read from the environment by read_switches at opd_detr_create, copied whole by opd_detr_clone, flipped
// one by one by the test hooks (opd_test_model_api.cpp).  plan_trunk and plan_transformer turn them into routes.
struct Switches {
    int small_m_gemm = 1;    // decoder linears (M = B x queries): one-shot K = 256 kernel (0: the general k-loop kernel)
    int fuse_gemm_ln = 1;    // attention output projections: Linear + residual + LayerNorm in one kernel (0: GEMM, then LN)
    int deep_fc2 = 1;        // encoder FFN-2 (K = 2048) + residual + LayerNorm as ONE row-owner launch (0: split-K slabs + reduce launch)
    int fuse_dec0 = 1;       // decoder layer 0's self-attention block from opd_detr::dec0_h (0: its four launches on the zero state like every other layer)
    int enc_front = 1;       // encoder FFN launch with the attention output projection + LayerNorm in front, from the attention output (env OPD_ENC_FRONT)
    int enc_tail = 0;        // ... with the next layer's q / k / v projection (last layer: the decoder's memory k / v) as its tail (env OPD_ENC_TAIL)
    int fused_enc_ffn = 1;   // the encoder's FFN block as one launch (kernels_rowln.hip::enc_ffn_kernel; 0: fc1 GEMM + deep-K ring launch; env OPD_FUSED_ENC_FFN)
    int fused_dec = 1;       // the decoder as five launches per layer on split fp16 operands (kernels_dec.hip; 0: the round-3 chain of nine launches
                             // per layer on single fp16 operands, also taken when the architecture does not fit: d_model != 256, heads != 8, queries % 4)
    int dec_splits = 3;      // key ranges of the fused decoder's cross-attention
    int heads2 = 1;          // the heads through kernels_dec.hip::heads2_kernel (0: kernels_untyped.hip::heads_kernel on the fp32 matrix pipe; env OPD_HEADS2)
    int fuse_btail = 1;      // stages 1-2: 3x3 -> expand + residual -> next reduce in one kernel (0: three launches)
    int fuse_shortcut = 1;   // first block of stage 1: the shortcut convolution as a second GEMM inside the fused tail (0: own launch)
    int dual_over_tail = 1;  // first block of stage 2: 3x3 + dual-source expand instead of shortcut launch + fused tail (-17 us)
    int sc2_tail = 1;        // ... and that dual-source route issued as one launch of the fused tail with the stride-2 shortcut inside
                             // (kernels_btail.hip, SC2; env OPD_SC2_TAIL, 0: three launches)
    int tail_rev = 1;        // consecutive fused tails walk their tiles in opposite directions (Infinity Cache reuse of the block output)
    int tail3 = 1;           // stage 3 (256-channel blocks) through the eight-wave fused tail (kernels_btail3.hip) where it pays (plan_trunk);
                             // 0: never (three launches per block), 2: always
    int tail3_split = 1;     // stage 3: frames beyond whole rounds of the fused tail run as a second chain on `stream2` (0: one launch per tail)
    int tail_rc = 1;         // stage 1: block 0 stores a1 instead of y; block 1 rebuilds y as its residual (kernels_btail.hip, RC; env OPD_TAIL_RC, 0 = off)
    int y_stride2 = 1;       // last tail of stage 1: y stored only where the next stage's stride-2 shortcut reads it (env OPD_Y_STRIDE2)
    int stem_reduce = 1;     // stage 1's first 1x1 reduce inside the fused stem launch (kernels_gemm.hip, StemReduce; env OPD_STEM_REDUCE, 0: own launch)
    int res_dma128 = 1;      // stage 2's 128-channel tails take their residual by LDS-DMA into one wave-private buffer (kernels_btail.hip, RB1; env
                             // OPD_RES_DMA128, 0: through register loads, BtailParams::dbg bit 16 -- identical bits)
    int wprefetch = 3;       // L2 warm-up of a launch's weights by its own workgroups: bit 0 implicit GEMM, bit 1 the encoder's FFN launch (env OPD_WPREFETCH)
    int w8 = -1;             // wide stage-4 layers through the eight-wave GEMM (kernels_w8.hip; identical bits): bit 0 3x3, bit 1 1x1 K >= 1024, bit 2 1x1 K = 512
                             // (env OPD_W8).  -1 = by the handle's flags: the 3x3 for OPD_FLAG_MULTI_STREAM handles (132 one-per-CU workgroups cost 22 % less
                             // CU time than 424 four-wave ones and leave the other CUs to the other streams: +1.1 %, 8 of 8 interleaved pairs), nothing for a
                             // single-stream handle (there half the chip would idle: stage 4 0.43 -> 0.46 ms)
    int small_splitk = 1;    // handles whose deep convolutions would fill a fraction of the CUs (small max_batch x frame): split their reduction over
                             // workgroups, fp32 slabs + reduce_act16_kernel (run_conv; env OPD_SMALL_SPLITK)
    int small_enc = 1;       // handles bounded to <= 1400 tokens: the encoder side's deep linears as split-K GEMMs + reduce / LayerNorm instead of the
                             // row-owner launches (plan_transformer; env OPD_SMALL_ENC)
    int fuse_stem_pool = 1;  // stem conv + max-pool in one kernel (0: two kernels, for cross-checking)
    int fuse_prep = 1;       // uint8 frames: pre-processing inside that kernel (0: preprocess_u8_kernel writes the padded NHWC4 image first)
    int pos_shadow = 1;      // q / k projections read a second fp16 shadow "x + position embedding" (written by the producer of x) instead
                             // of adding a row-periodic fp32 bias table W.pos + b per output tile (0: the table, the round-1 form)
    int wround = 1;          // fp16 images of the folded convolution kernels by error diffusion along the reduction (opd_host.h::round_f16_diffused;
                             // 0: round to nearest).  Identical for weights that are fp16-exact already.
    int dbg_btail = 0, dbg_gemm = 0;   // timing ablations only (OPD_DBG_BTAIL / OPD_DBG_GEMM): the kernels' dbg bits for every launch of the forward
    int dbg_dec_layers = 1 << 20;      // timing ablation only (OPD_DBG_DEC_LAYERS): run this many decoder layers
    int dbg_skip = 0;                  // timing ablation only (OPD_DBG_SKIP): bit i = segment i of stage_ms launches nothing
};

// The trunk plan: how each bottleneck block of stages 1-4 runs.
enum TrunkPath { PATH_TAIL, PATH_CONVS, PATH_DUAL };   // fused tail (kernels_btail*.hip) / 3x3 and 1x1 expand as two launches / 3x3 + dual-source expand
enum TrunkShortcut { SC_NONE, SC_TAIL, SC_EXPAND, SC_LAUNCH };   // no shortcut / a second GEMM of the fused tail / extra K of the dual expand / own launch
enum TrunkResidual { RES_NONE, RES_TRUNK, RES_SHORTCUT, RES_REBUILD };   // none (the shortcut sums into the expand) / the block input / the shortcut's
                                                                         // output / rebuilt from the previous block's a1 and input (BtailParams::rc)
enum TrunkStore { STORE_Y, STORE_A1, STORE_Y_STRIDE2 };   // block output stored whole / a1 only (the next block rebuilds y) / at even (oh, ow) only
struct TrunkStep {
    int path, sc, res, store;
    int C3;           // fused tails: channels of the next block's reduce, computed here as z (0: none)
    int rev, rev_b;   // BtailParams::rev of the launch; rev_b: of its launch in the stage-3 split's second chain
    int one_launch;   // PATH_DUAL, first block of stage 2: 3x3, dual-source expand and the next block's reduce issued as ONE launch of the fused
                      // tail with the shortcut inside (kernels_btail.hip, SC2): the dual route's arithmetic and bits, one launch instead of three
    int one_C3;       // ... channels of that reduce, computed there as z (0: the reduce keeps its launch)
    int one_rev;      // ... BtailParams::rev of that launch (it stands outside the alternation of the PATH_TAIL launches)
};
struct TrunkPlan {
    std::vector<TrunkStep> steps;   // one per block, in stage order
    int split = 0;                  // stage 3, blocks 1..: frames [0, split) on `stream`, [split, B) as a second chain on `stream2` (split == B: one chain)
};
// Pure over shapes and configuration (reads block shapes, never device pointers): called by fwd_trunk, i.e. per eager forward and per
// graph capture.  B x H2 x W2: the call's batch and stage-1 input map; `taps`, `profiling`, `has_stream2`: the handle's diagnostic modes and branch stream.
TrunkPlan plan_trunk(const Arch& a, const std::vector<Block>& blocks, const opd_config& cfg, const Switches& sw, int B, int H2, int W2, int num_cus,
                     bool taps, int profiling, bool has_stream2);

// The transformer plan: which launches run behind the trunk -- input projection, encoder layers, memory K/V, decoder, heads.
enum EncQkv { QKV_LAUNCH, QKV_PREV_TAIL };   // a layer's q | k | v: its own GEMM / written by the previous layer's FFN launch (its tail passes)
enum OutProj { OPROJ_IN_FFN, OPROJ_GEMM_LN, OPROJ_GEMM_THEN_LN };   // attention output projection + residual + LayerNorm: the front phase of the encoder's FFN
                                                                    // launch / one row-owner kernel / a GEMM, then the LayerNorm (decoder chain: split-K slabs, then reduce + LayerNorm)
enum EncFfn { FFN_ONE_LAUNCH, FFN_FC1_DEEP, FFN_FC1_SPLITK };   // enc_ffn_kernel / fc1 GEMM + deep-K ring launch / fc1 GEMM + split-K slabs + reduce-LayerNorm
enum HeadsKernel { HEADS_F32, HEADS_SPLIT16 };   // kernels_untyped.hip::heads_kernel / kernels_dec.hip::heads2_kernel
struct EncStep {
    int qkv, oproj, ffn;
    int splits;   // FFN_FC1_SPLITK: slices of fc2's reduction
    int tail;     // FFN_ONE_LAUNCH: tail passes the launch runs (0, or all of enc_pack_tail)
};
struct TransformerPlan {
    bool shadow = false;       // q / k projections read the fp16 shadow x + pos (0: x alone plus the row-periodic table W.pos + b)
    bool small_enc = false;    // handle bounded to <= 1400 tokens: no row-owner launch on the encoder side
    int enc_splits = 4;        // slices of the encoder side's split-K linears (where the k-steps divide; else 4)
    int proj_splits = 0;       // input projection: 0 = the deep-K row-owner launch, else split-K in this many slices
    std::vector<EncStep> enc;  // one per encoder layer
    bool kv_launch = true;     // memory K/V of the decoder layers: its own GEMM (false: the last encoder layer's tail passes)
    bool dec_fused = false;    // kernels_dec.hip, five launches per layer (false: the chain of nine)
    int dec_splits = 0;        // fused: key ranges of the cross-attention
    bool dec0 = false;         // chain: layer 0's self-attention block is the broadcast constant dec0_h (false: its launches on the zero state)
    bool dec_small_m = false;  // chain: linears through the one-shot K = 256 kernel (false: the general k-loop GEMM)
    int dec_oproj = OPROJ_GEMM_LN;   // chain: OPROJ_GEMM_LN or OPROJ_GEMM_THEN_LN
    int heads = HEADS_F32;
    bool heads_ln3 = false;    // the last decoder layer's FFN sum + LN3 run inside the heads kernel (the fused decoder)
    bool heads_ln = false;     // the decoder's final LayerNorm runs inside the heads kernel (false: its own launch in front)
};
// Per-frame pixel bound lvl[k] / side bound side[k] of: image, stem, pool (= stage 1), stage 2, 3, 4 -- over every H x W the handle accepts
// (H, W <= max(max_height, max_width), H * W <= max_height * max_width).  opd_detr::stage_px[s] = lvl[2 + s].
struct FrameBounds { size_t lvl[6], side[6]; };
FrameBounds frame_bounds(const opd_config& cfg);
// Pure over the architecture, configuration and switches, `stage4_px` (opd_detr::stage_px[3]) and the call's batch and feature map: reads no
// device pointer.  Called by enqueue_forward, i.e. per eager forward and per graph capture.
TransformerPlan plan_transformer(const Arch& a, const opd_config& cfg, const Switches& sw, size_t stage4_px, int B, int fh, int fw);
Switches read_switches(int flags);   // opd_api.cpp: the defaults overridden by the environment, as opd_detr_create reads them

}  // namespace opd

using namespace opd;   // (private header: every includer is library code)

// Device buffers of the folded weights: shared (read-only after opd_detr_create) by a handle and its clones, freed with the last one.
struct RedZoned { void* base; size_t bytes; int poison; };   // a poison-mode allocation: [red zone | bytes | red zone] at base
struct WeightSet {
    std::vector<void*> allocs;
    std::vector<RedZoned> zoned;
    int device = 0;
    // per-resolution bias folds (Plan): functions of the weights and the feature-map size only, so clones share them too
    std::mutex plan_mu;
    std::vector<std::unique_ptr<Plan>> plans;
    ~WeightSet() {
        (void)hipSetDevice(device);
        for (void* p : allocs) (void)hipFree(p);
    }
};

// Everything build_weights fills: device pointers into the shared WeightSet and the host copies the plans are folded from.  opd_detr_clone
// copies this struct with ONE assignment, so a new product of build_weights goes HERE and nowhere else.
struct DetrWeights {
    int64_t weight_bytes = 0;
    Conv stem;
    std::vector<Block> blocks;
    std::vector<int> stage_first;  // index of first block of each stage
    Conv proj;
    std::vector<EncLayer> enc;
    std::vector<DecLayer> dec;
    f16_t* wkv_all = nullptr;  // [dec_layers*512][256] = per layer [Wk_c; Wv_c]
    float* bkv_all = nullptr;  // [dec_layers*512] = per layer [bk_c; bv_c] (pos_shadow path)
    float* dec0_h = nullptr;   // [256]: decoder state after the self-attention block of layer 0 (input independent, see build_weights; Switches::fuse_dec0)
    f16_t* qc0 = nullptr;      // [Q][256]: layer 0's cross-attention queries (dec0_h + qpos) . Wq_c^T + bq_c: input independent as well (fp32 at load)
    LNp dec_ln;
    float *wc = nullptr, *bc = nullptr, *w1 = nullptr, *b1 = nullptr, *w2 = nullptr, *b2 = nullptr, *w3 = nullptr, *b3 = nullptr;
    f16_t *wc_f = nullptr, *w1_f = nullptr, *w2_f = nullptr;   // the heads' 256-wide layers as split fp16 pairs in fragment order (heads2_kernel)
    float* zero_bias = nullptr;  // [3072] zeros

    // host copies needed to build plans for new resolutions
    std::vector<std::vector<float>> h_enc_cat_w, h_enc_cat_b;  // per enc layer: [768*256] ([Wq;Wk;0]), [768]
    std::vector<float> h_kv_cat_w, h_kv_cat_b;                 // [L*512*256] ([Wk;0] per layer), [L*512]
};

struct opd_detr : DetrWeights {
    Arch arch;
    opd_config cfg{};
    Switches sw;                            // forward-plan switches (copied by opd_detr_clone: a clone plans like its source)
    int dtype = 0;                          // OPD_DT_F16 / OPD_DT_BF16 (cfg.flags & OPD_FLAG_BF16): the 16-bit operand type of every activation buffer and GEMM weight
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr;   // second branch of the forward (stage-3 frame split, see trunk_stage3_split); joins the capture of `stream`
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    std::vector<void*> allocs;              // this handle's own buffers: workspace, per-resolution plans
    std::vector<RedZoned> zoned;            // poison mode only: the same buffers with their red zones
    std::shared_ptr<WeightSet> weights;     // the model's weights (shared with clones)
    bool weights_sealed = false;            // set once the weights are built: later "weight" allocations (plans) are the handle's own
    int64_t workspace_bytes = 0;

    // workspace
    uint8_t* d_u8 = nullptr;
    float* d_pv = nullptr;
    f16_t *d_x4 = nullptr, *d_stem = nullptr, *d_pool = nullptr, *d_t0 = nullptr, *d_t1 = nullptr, *d_m0 = nullptr,
          *d_m1 = nullptr, *d_sc = nullptr;
    float *d_x32 = nullptr, *d_y32 = nullptr, *d_slab = nullptr;
    f16_t* d_xp16 = nullptr;   // fp16(x + position embedding): the q / k projections' input (pos_shadow)
    f16_t *d_x16 = nullptr, *d_qkv16 = nullptr, *d_attn16 = nullptr, *d_ffn16 = nullptr, *d_memkv16 = nullptr;
    float *d_h32 = nullptr, *d_yd32 = nullptr, *d_hs32 = nullptr;
    f16_t *d_h16 = nullptr, *d_qkvd16 = nullptr, *d_qd16 = nullptr, *d_attnd16 = nullptr, *d_ffnd16 = nullptr;
    // fused decoder: self-attention operands, cross-attention key-split partials, FFN partial sums
    f16_t *d_dq16 = nullptr, *d_dk16 = nullptr, *d_dvT = nullptr;
    float *d_part_o = nullptr, *d_part_ml = nullptr, *d_ffn_part = nullptr;
    float *d_logits = nullptr, *d_boxes = nullptr;
    opd_det* d_records = nullptr;
    int32_t *d_counts = nullptr, *d_orig_hw = nullptr;
    // ragged batches (frames smaller than the canvas): per-frame valid sizes and per-frame bias-fold pointers
    int32_t *d_valid_hw = nullptr, *d_key_valid = nullptr;
    const float** d_bias_ptrs = nullptr;   // [(enc_layers + 2)][max_batch]: bias folds per encoder layer, K/V fold, position embeddings
    std::vector<int32_t> h_valid_hw, h_key_valid;
    std::vector<const float*> h_bias_ptrs;
    // asynchronous submissions (opd_detr_detect_async): one completion event per in-flight ticket
    hipEvent_t ev_async[4] = {};
    unsigned async_next = 0;
    bool async_pending[4] = {};   // ticket handed out and not yet waited for: its slot (event, output pointers, staging) is in use
    // host-output submissions: the records travel device -> pinned slot (asynchronous) -> caller buffer (in opd_detr_wait)
    struct AsyncHost { void* pinned = nullptr; opd_det* out = nullptr; int32_t* counts = nullptr; int B = 0; };
    AsyncHost async_host[4];
    // allocated by the first call of the stage that uses them (opd_api.cpp: ensure_*)
    void* sync_pinned = nullptr;   // page-locked staging of the blocking entry points: [records of max_batch frames | counts | feature rows]
    uint32_t* d_color_acc = nullptr;   // [max_batch][queries][OPD_COLOR_ACC_WORDS] integer sums of the colour feature stage
    opd_floor_rec* d_floor = nullptr;   // [max_batch][queries] floor records of the floor stage, and their page-locked twin
    opd_floor_rec* h_floor = nullptr;
    float* d_feat_all = nullptr;   // [max_batch][queries][d_model] behind the counts in the d_records allocation: features of a batch's records (opd_detr_detect_frames_features)
    // device-side resize (camera resolution -> model resolution): source staging (device side only, grown on demand) and coefficient tables
    Staging src;
    struct ResizeTab { int h, w, oh, ow, ksh, ksv; int32_t *bh, *kh, *bv, *kv; };
    std::vector<ResizeTab> resize_tabs;
    float *d_amap = nullptr, *d_amap_stat = nullptr;   // opd_detr_attention_map: output [hw], row statistics
    int32_t* d_amap_sel = nullptr;
    bool last_ragged = false;
    int32_t* d_rois = nullptr;
    float* d_roi_out = nullptr;
    std::vector<int32_t> h_orig_hw;
    // device suppression (opd_detr_set_nms): off while nms_threshold < 0; the flag word of person_nms_kernel and tile_merge_kernel (ensure_nms_flag)
    int nms_label = 0;
    float nms_threshold = -1.0f;
    int32_t* d_nms_flag = nullptr;
    // tiled detection: the tile windows of the SRC_TILES source; the tile stage's [counts of max_batch frames | merged records of
    // max_batch x queries candidates] and its page-locked twin (ensure_tile_out)
    int32_t* d_tiles = nullptr;
    std::vector<int32_t> h_tiles;
    int32_t* d_tile_desc = nullptr;      // tiles of several sizes: [max_batch] TileRaggedDesc (opd_tile.h) as 16 int32 words each, and what was uploaded last
    std::vector<int32_t> h_tile_desc;
    char* d_tile_out = nullptr;
    void* tile_pinned = nullptr;

    // state of the last forward
    int last_B = 0, last_H = 0, last_W = 0, last_fh = 0, last_fw = 0;
    int profiling = 0;       // 0 off; 1 eager launches with an event pair around each (opd_detr_kernel_times) + stage marks; 2 stage marks INSIDE the replayed graph
    hipEvent_t ev[10] = {};
    bool graph_marks = false;   // profiling mode 2: the last forward was a graph replay (marks 0 .. 7 recorded by graph nodes, mark 9 eagerly behind it)
    float stage_ms[8] = {};
    size_t slab_floats = 0;  // capacity of d_slab
    size_t stage_px[4] = {}; // per-frame pixel bound of the four stages' OUTPUT maps (build_workspace): what configuration-level plans count tiles with
    int num_cus = 256;

    // hipGraph cache: the whole forward (~180 launches, many of them 5-10 us decoder kernels) replayed as one graph
    struct GraphEntry { int B, H, W, fmt, fh, fw; const void* pixels; int uses; GraphSlot slot; };
    std::vector<GraphEntry> graphs;

    // per-kernel-class timing (profiling mode 1 only): event pairs around every launch of the last forward
    LaunchTimer timer;
    std::vector<KernelRow> ktable;      // the last profiled forward by kernel (opd_detr_kernel_table), longest first
    float class_ms[4] = {};
    int class_launches[4] = {};
    double class_flops[4] = {};

    std::vector<struct opd_comm*> comms;   // communicator lanes bound to this handle (opd_comm.cpp; detached when the handle is destroyed)

    // diagnostic taps (opd_test_set_taps): a checksum launch after every launch of the forward, captured into the graph with it
    int taps = 0;
    unsigned long long* d_taps = nullptr;   // [OPD_MAX_TAPS][OPD_TAP_BLOCKS]
    int tap_next = 0;
    std::vector<std::string> tap_names;
};
enum { OPD_MAX_TAPS = 512 };
struct LwtSeqCall;   // opd_lwt.h: a run of frames of one camera (HybridStage::call)

namespace opd {

// Diagnostic allocation mode (opd_test_set_alloc_poison; -1 = off): every device buffer of handles created afterwards is filled with
// this byte and sits between two red zones of OPD_REDZONE bytes filled with it as well.  A forward that reads workspace it has not
// written, or memory next to its buffers, then gives results that depend on the byte: tests/test_detector_gpu.py runs the same
// batches through handles poisoned with 0x00 / 0xFF (fp16 and fp32 NaN patterns) and an unpoisoned one and demands identical bits.
extern std::atomic<int> g_alloc_poison;
enum : size_t { OPD_REDZONE = 256 * 1024 };

template <typename T>
inline int dalloc(opd_detr* m, T** p, size_t count, bool weight) {
    void* q = nullptr;
    const size_t bytes = count * sizeof(T);
    const int poison = g_alloc_poison.load();
    const size_t pad = poison >= 0 ? OPD_REDZONE : 0, total = (bytes ? bytes : 16) + 2 * pad;
    hipError_t e = hipMalloc(&q, total);
    if (e != hipSuccess) return fail(OPD_ENOMEM, "hipMalloc of " + std::to_string(bytes) + " bytes failed: " + hipGetErrorString(e));
    const bool to_weights = weight && !m->weights_sealed && m->weights;
    (to_weights ? m->weights->allocs : m->allocs).push_back(q);   // (the base pointer: what hipFree takes)
    if (poison >= 0) {
        HIPCHK(hipMemset(q, poison, total));
        HIPCHK(hipDeviceSynchronize());   // (the fill runs on the null stream and may return before it is done; the handle's streams do not wait for that one: a buffer
                                          //  a stage allocates in the middle of a call would else be poisoned AFTER the stage's own memset or first launch)
        (to_weights ? m->weights->zoned : m->zoned).push_back({q, bytes ? bytes : 16, poison});
    }
    (weight ? m->weight_bytes : m->workspace_bytes) += (int64_t)bytes;
    *p = reinterpret_cast<T*>(static_cast<char*>(q) + pad);
    return OPD_OK;
}

void comm_detach_all(opd_detr* m);   // opd_comm.cpp: called by opd_detr_destroy
// opd_weights.cpp: the checkpoint folded, rounded, packed and uploaded into the handle's DetrWeights; one fp32 vector as a weight allocation
int build_weights(opd_detr* m, const StateDict& sd);
int upload_f32(opd_detr* m, float** dst, const std::vector<float>& v);
// a row-bias fold *out[rows][N] = d_x[rows][K] . w[N][K]^T + b, all fp32 (the plan GEMM): the query-position folds here, a plan's position folds
int upload_fold(opd_detr* m, const float* d_x, const std::vector<float>& w, const std::vector<float>& b, int rows, int N, int K, float** out);
// opd_model.cpp, for opd_api.cpp: the rest of what a handle is made of, the forward through the graph cache, the launch helper
int fill_qc0(opd_detr* m);
int build_workspace(opd_detr* m);
int run_forward(opd_detr* m, const void* d_pixels, int pixel_format, int B, int H, int W, const int32_t* valid_hw = nullptr);
void drop_graphs(opd_detr* m);   // destroy the handle's graph executables and clear the cache: the next forwards run eagerly, then capture anew
enum { CLS_CONV = 0, CLS_GEMM = 1, CLS_ATTN = 2, CLS_OTHER = 3 };
// How a launch of the forward (and of the post-process behind it) is issued, written once: profiling mode 1's event pair (the handle's
// LaunchTimer; timing class `cls`, algorithmic `flops`) opens, `issue()` launches on stream `s`, the pair closes, and with diagnostic taps on a checksum launch follows
// for each of `taps` that has a name and a buffer.  A split-K pair is two calls, the tap on the second.
struct Tap { const char* name; const void* p; size_t bytes; };
int launch_end(opd_detr* m, hipStream_t s, std::initializer_list<Tap> taps);   // (the pair's close and the taps: nothing but launch() calls it)
template <typename F>
int launch(opd_detr* m, hipStream_t s, int cls, double flops, F&& issue, std::initializer_list<Tap> taps = {}) {
    if (m->profiling == 1) RCCHK(m->timer.begin(s, cls, flops));
    HIPCHK(issue());
    return launch_end(m, s, taps);
}
void timed_collect(opd_detr* m);
#define MARK(i)                                                   \
    do {                                                          \
        if (m->profiling) HIPCHK(hipEventRecord(m->ev[i], m->stream)); \
        opd_dbg_skip_launch = (m->sw.dbg_skip >> (i)) & 1;           \
    } while (0)

// The detect pipeline (opd_api.cpp), all enqueued on m->stream.  Every detect entry point, opd_comm_detect included, is its own argument checks
// plus ONE call of detect_pipeline:
//   source   stage_frames: the frames of a FrameSource -> device pixels at model resolution (upload, resize, or the windows of whole frames)
//   forward  run_forward, through the graph cache
//   sink     deliver_records, a straight sequence in which a stage runs when its part of the RecordSink is set: post-process with suppression ->
//            tile merge -> feature stage -> floor stage -> tracker enqueue -> hybrid-tracker enqueue -> ONE fetch (the copies back and the
//            call's one wait) -> delivery into the caller's arrays, tracker finish, hybrid-tracker finish
enum { SRC_PIXELS, SRC_BLOCK, SRC_LIST, SRC_TILES };
struct FrameSource {
    int kind;
    const void* frames;           // SRC_PIXELS: pixels of `pixel_format` at model resolution.  SRC_BLOCK: ONE block of camera frames [B][h][w][3], always resized.
                                  // SRC_LIST: const uint8_t* const*, one HOST pointer per camera frame (resized when h x w is not the model size, else uploaded as is).
                                  // SRC_TILES: such a list of n_frames whole frames; the batch is the n_tiles windows of each, resized
    int pixel_format, mem_kind;   // (where the frames lie)
    int h, w;                     // camera resolution (SRC_PIXELS: unused)
    int n_frames = 0, n_tiles = 0;    // SRC_TILES: B = n_frames x n_tiles windows `tiles` [n_tiles][4] = y0, x0, th, tw (host), all of one size unless `tile_HW` is set
    const int32_t* tiles = nullptr;
    const int32_t* tile_HW = nullptr; // SRC_TILES, nullable: [n_tiles][2] the model size of each tile inside the H x W canvas (windows and sizes may then differ: the
                                      // batch is ragged, valid_hw[b] = tile_HW[b % n_tiles], and the sink's orig_hw names each tile's window)
    // the size the post-process scales the boxes to: the camera frame, a tile's window; 0: none of its own (tiles of several sizes: the sink's orig_hw has them)
    int box_h() const { return kind == SRC_PIXELS || tile_HW ? 0 : kind == SRC_TILES ? tiles[2] : h; }
    int box_w() const { return kind == SRC_PIXELS || tile_HW ? 0 : kind == SRC_TILES ? tiles[3] : w; }
};
enum { WAIT_BLOCKING, WAIT_TICKET, WAIT_NONE };   // fetch the records and wait / hand them to async slot `ticket` (opd_detr_wait) / leave them on the stream
enum { FEAT_NONE, FEAT_ROI, FEAT_COLOR, FEAT_REID };   // nothing / ROI pooling on the records / their colour histograms / the Re-ID model's rows (opd_reid.h: ReidFusedCall)
// The optional stages of a sink, absent by default.  They work on the records labelled RecordSink::label and deliver into HOST arrays.
struct FeatureStage {
    int kind = FEAT_NONE;
    float* features = nullptr;    // rows to the caller, [B][queries][d_model] (null with a track stage: the rows stay on the device).  FEAT_REID: [slots][feature_dim],
    opd_reid* reid = nullptr;     // row k of slot_map[k] = frame * queries + query_index, k < min(*n_person, slots)
    int slots = 0;
    int32_t *slot_map = nullptr, *n_person = nullptr;
};
struct FloorStage { const opd_floor* fmap = nullptr; opd_floor_rec* out = nullptr; };   // a floor record of every record of the class -> out [B][queries]
struct TrackStage {   // the kept records and feature rows enter trackers where they lie: frame b into trackers[b], or the B frames in order into `seq`,
    struct opd_track* const* trackers = nullptr;   // or (`cams`) frame b into cams[camera_of[b]], every camera's frames in their order, the cameras side by side
    struct opd_track* seq = nullptr;
    struct opd_track* const* cams = nullptr; int n_cams = 0; const int32_t* camera_of = nullptr;
    int32_t *track_ids = nullptr, *n_featured = nullptr, *frames_done = nullptr;   // [B][queries], [B]; seq: frames applied; cams: [n_cams]
    bool on() const { return trackers || seq || cams; }
};
struct HybridStage {   // the kept records and the camera-resolution frames enter hybrid trackers (opd_lwt.h) where they lie: frame b into trackers[b], or
    struct opd_lwt* const* trackers = nullptr;   // (`seq`) as the key frames of the run of frames `call` of one camera, its in-between frames around them
    struct opd_lwt* seq = nullptr;
    const ::LwtSeqCall* call = nullptr;
    int32_t* track_ids = nullptr;   // [B][queries]; a tiled call: [n_frames][n_tiles x queries], by position in the merged records, which the stage then reads
    opd_lwt_rec* recs_out = nullptr; int capacity = 0;           // seq: the in-between frames' records [F - B][capacity], their counts, frames applied
    int32_t *rec_counts = nullptr, *frames_done = nullptr;
    const char* entry = "opd_detr_detect_frames_hybrid";         // the entry errors are worded for
    bool on() const { return trackers || seq; }
};
struct TileStage {   // a SRC_TILES batch: the records of a frame's tiles, suppressed per tile with the PARAMETERS' label and threshold, merge across the seams
    const opd_tile_params* params = nullptr;
    int n_frames = 0, n_tiles = 0, frame_h = 0, frame_w = 0;
    const char* entry = "opd_detr_detect_tiled_stages";   // the entry a tracker's error is worded for
    opd_tile_det* out = nullptr; int32_t* counts = nullptr;   // [n_frames][n_tiles x queries], [n_frames]; RecordSink::out / counts stay null: the per-tile records never leave the device
};
struct RecordSink {
    float threshold;
    const int32_t* orig_hw;       // [B][2] frame sizes of the caller; null: the source's box size, without one the model resolution
    opd_det* out; int32_t* counts;
    int mem_kind;                 // where out / counts lie: device ones are written by the post-process kernel itself, host ones filled from the library's
    int wait, ticket, label = 0;
    FeatureStage feature; FloorStage floor; TrackStage track; HybridStage hybrid; TileStage tile;
    RecordSink(float threshold, const int32_t* orig_hw, opd_det* out, int32_t* counts, int mem_kind, int wait = WAIT_BLOCKING, int ticket = 0)
        : threshold(threshold), orig_hw(orig_hw), out(out), counts(counts), mem_kind(mem_kind), wait(wait), ticket(ticket) {}
};
int check_shape(opd_detr* m, const void* pixels, int pixel_format, int mem_kind, int B, int H, int W);
int detect_pipeline(opd_detr* m, const FrameSource& src, int B, int H, int W, const int32_t* valid_hw, const RecordSink& sink);

}  // namespace opd
