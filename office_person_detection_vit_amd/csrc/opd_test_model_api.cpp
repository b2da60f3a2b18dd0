// opd_test_model_api.cpp — the test hooks that need no kernel launch of their own: host-only helpers of the loader and the planner, exported
// so that CPU tests can exercise them without a GPU, and the hooks that reach into a model handle (opd_model.h): fusion switches, poison
// allocation, graph guard, diagnostic taps.  Exported from libopd_hip_test.so only.
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "opd_model.h"
#include "opd_test_util.h"

TAPI uint16_t opd_test_f32_to_f16(float f) { return opd::f32_to_f16(f); }
TAPI float opd_test_f16_to_f32(uint16_t h) { return opd::f16_to_f32(h); }
TAPI int opd_test_normalise_key(const char* in, char* out, int cap) {
    const std::string k = opd::normalise_key(in);
    if ((int)k.size() + 1 > cap) return OPD_EINVAL;
    memcpy(out, k.c_str(), k.size() + 1);
    return OPD_OK;
}
// parse + schema-check a checkpoint on the host (no GPU needed): returns 0 and fills depths[4], enc, dec, queries, ncls
TAPI int opd_test_inspect_checkpoint(const char* path, int32_t* info8) {
    opd::StateDict sd;
    std::string err;
    int rc = opd::load_safetensors(path, &sd, &err);
    if (rc) return fail(rc, err);
    opd::Arch a;
    rc = opd::infer_arch(sd, &a, &err);
    if (rc) return fail(rc, err);
    for (int i = 0; i < 4; ++i) info8[i] = a.depths[i];
    info8[4] = a.enc_layers; info8[5] = a.dec_layers; info8[6] = a.queries; info8[7] = a.ncls;
    return OPD_OK;
}
// Pillow coefficient tables of the device resize (host only): bounds [out][2], coeffs [out][ksize]; returns ksize
TAPI int opd_test_resize_coeffs(int in_size, int out_size, int32_t* bounds, int32_t* coeffs, int coeffs_capacity) {
    std::vector<int32_t> b, k;
    int ksize = 0;
    opd_resize_coeffs(in_size, out_size, &b, &k, &ksize);
    if ((int)k.size() > coeffs_capacity) return fail(OPD_EINVAL, "coefficient buffer too small");
    memcpy(bounds, b.data(), b.size() * 4);
    memcpy(coeffs, k.data(), k.size() * 4);
    return ksize;
}
// host-only pieces of the ragged-batch path, exported for the CPU tests
TAPI int opd_test_valid_prefix(int valid, int in, int out) { return valid_prefix(valid, in, out); }
TAPI int opd_test_sine_pos_embed(int h, int w, int vh, int vw, int D, float* out) {
    if (!out || h < 1 || w < 1 || vh < 1 || vw < 1 || vh > h || vw > w || D < 2 || (D & 1)) return fail(OPD_EINVAL, "bad sine_pos_embed arguments");
    std::vector<float> pos;
    sine_pos_embed(h, w, vh, vw, D, &pos);
    memcpy(out, pos.data(), pos.size() * sizeof(float));
    return OPD_OK;
}
// the error-diffusion rounding of the weight loader (opd_host.h), in place on [rows][taps][cin]
TAPI int opd_test_round_f16_diffused(float* w, int rows, int taps, int cin) {
    if (!w || rows < 0 || taps < 1 || cin < 1) return fail(OPD_EINVAL, "opd_test_round_f16_diffused: bad arguments");
    opd::round_f16_diffused(w, (size_t)rows, taps, cin);
    return OPD_OK;
}
// plan_trunk (opd_model.cpp) for a ResNet trunk of the given stage depths with the bottleneck shapes infer_arch demands, default switches, a
// branch stream, no taps, no profiling; a batch of B frames of H x W in a handle of max_batch frames.  steps_out[block][7] = path, shortcut,
// residual, store, C3, rev, rev_b (opd_model.h); *split_out = TrunkPlan::split.  Returns the number of blocks.
static int test_trunk_plan(const int* depths, int max_batch, int flags, int B, int H, int W, int num_cus, const Switches& sw, int max_steps, TrunkPlan* out) {
    if (!depths || B < 1 || H < 1 || W < 1 || num_cus < 1) return fail(OPD_EINVAL, "bad trunk_plan arguments");
    Arch a;
    std::vector<Block> blocks;
    auto conv = [](int cin, int cout, int k, int stride) {
        Conv c;
        c.Cin = cin; c.Cout = cout; c.KH = c.KW = k; c.stride = stride; c.pad = k / 2; c.K = k * k * cin;
        return c;
    };
    for (int s = 0, cin = 64; s < 4; ++s) {
        a.depths[s] = depths[s];
        if (depths[s] < 1) return fail(OPD_EINVAL, "every stage needs a block");
        const int cout = a.hidden[s], mid = cout / 4;
        for (int l = 0; l < depths[s]; ++l) {
            const int stride = (l == 0 && s > 0) ? 2 : 1;
            Block b;
            b.has_sc = l == 0;
            if (b.has_sc) b.sc = conv(cin, cout, 1, stride);
            b.c0 = conv(cin, mid, 1, 1); b.c1 = conv(mid, mid, 3, stride); b.c2 = conv(mid, cout, 1, 1);
            blocks.push_back(b);
            cin = cout;
        }
    }
    if ((int)blocks.size() > max_steps) return fail(OPD_EINVAL, "steps_out too small");
    opd_config cfg{};
    cfg.struct_size = sizeof(opd_config); cfg.max_batch = max_batch; cfg.max_height = H; cfg.max_width = W; cfg.flags = flags;
    *out = plan_trunk(a, blocks, cfg, sw, B, down2(down2(H)), down2(down2(W)), num_cus, false, 0, true);
    return (int)blocks.size();
}
TAPI int opd_test_trunk_plan(const int* depths, int max_batch, int flags, int B, int H, int W, int num_cus, int* steps_out, int max_steps, int* split_out) {
    if (!steps_out || !split_out) return fail(OPD_EINVAL, "bad trunk_plan arguments");
    TrunkPlan plan;
    const int n = test_trunk_plan(depths, max_batch, flags, B, H, W, num_cus, Switches{}, max_steps, &plan);
    if (n < 0) return n;
    for (size_t i = 0; i < plan.steps.size(); ++i) {
        const TrunkStep& t = plan.steps[i];
        const int row[7] = {t.path, t.sc, t.res, t.store, t.C3, t.rev, t.rev_b};
        memcpy(steps_out + 7 * i, row, sizeof(row));
    }
    *split_out = plan.split;
    return n;
}
// ... with the switches as opd_detr_create reads them (defaults overridden by the environment): one_out[block][3] = one_launch, one_C3, one_rev of
// every step (opd_model.h: the dual-source route of stage 2's first block issued as one launch), steps_out as above (null: not wanted)
TAPI int opd_test_trunk_plan_one_launch(const int* depths, int max_batch, int flags, int B, int H, int W, int num_cus, int* steps_out, int* one_out, int max_steps) {
    if (!one_out) return fail(OPD_EINVAL, "bad trunk_plan arguments");
    TrunkPlan plan;
    const int n = test_trunk_plan(depths, max_batch, flags, B, H, W, num_cus, read_switches(flags), max_steps, &plan);
    if (n < 0) return n;
    for (size_t i = 0; i < plan.steps.size(); ++i) {
        const TrunkStep& t = plan.steps[i];
        const int row[7] = {t.path, t.sc, t.res, t.store, t.C3, t.rev, t.rev_b}, one[3] = {t.one_launch, t.one_C3, t.one_rev};
        if (steps_out) memcpy(steps_out + 7 * i, row, sizeof(row));
        memcpy(one_out + 3 * i, one, sizeof(one));
    }
    return n;
}
// plan_transformer (opd_model.cpp) for arch7 = d_model, heads, ffn, encoder layers, decoder layers, queries, classifier rows in a handle of
// max_batch frames of at most max_height x max_width with `flags`, for a call of B frames of H x W; the switches as opd_detr_create reads
// them (defaults overridden by the environment), the stage-4 pixel bound as build_workspace computes it.
//   head_out[14] = shadow, small_enc, enc_splits, proj_splits (0: deep row-owner), kv_launch, dec_fused, dec_splits, dec0, dec_small_m,
//                  dec_oproj, heads (HeadsKernel), heads_ln3, heads_ln, the handle's token bound max_batch x stage_px[3]
//   enc_out[layer][5] = qkv (EncQkv), oproj (OutProj), ffn (EncFfn), splits, tail
// Returns the number of encoder layers.
TAPI int opd_test_transformer_plan(const int* arch7, int max_batch, int max_height, int max_width, int flags, int B, int H, int W, int* head_out, int* enc_out,
                                   int max_layers) {
    if (!arch7 || !head_out || !enc_out || max_batch < 1 || max_height < 32 || max_width < 32 || B < 1 || H < 1 || W < 1)
        return fail(OPD_EINVAL, "bad transformer_plan arguments");
    Arch a;
    a.d_model = arch7[0]; a.heads = arch7[1]; a.ffn = arch7[2]; a.enc_layers = arch7[3]; a.dec_layers = arch7[4]; a.queries = arch7[5]; a.ncls = arch7[6];
    if (a.enc_layers < 1 || a.dec_layers < 1 || a.enc_layers > max_layers) return fail(OPD_EINVAL, "transformer_plan: layer counts");
    opd_config cfg{};
    cfg.struct_size = sizeof(opd_config); cfg.max_batch = max_batch; cfg.max_height = max_height; cfg.max_width = max_width; cfg.flags = flags;
    const size_t px = frame_bounds(cfg).lvl[5];
    int fh = H, fw = W;
    for (int k = 0; k < 5; ++k) { fh = down2(fh); fw = down2(fw); }   // stem, pool, stages 2-4
    const TransformerPlan t = plan_transformer(a, cfg, read_switches(flags), px, B, fh, fw);
    const int head[14] = {t.shadow, t.small_enc, t.enc_splits, t.proj_splits, t.kv_launch, t.dec_fused, t.dec_splits, t.dec0, t.dec_small_m,
                          t.dec_oproj, t.heads, t.heads_ln3, t.heads_ln, (int)((size_t)max_batch * px)};
    memcpy(head_out, head, sizeof(head));
    for (size_t i = 0; i < t.enc.size(); ++i) {
        const EncStep& e = t.enc[i];
        const int row[5] = {e.qkv, e.oproj, e.ffn, e.splits, e.tail};
        memcpy(enc_out + 5 * i, row, sizeof(row));
    }
    return (int)t.enc.size();
}

// ---- hooks that reach into a model handle: every switch that changes the launch sequence drops the captured graphs, which hold the old one ----
TAPI int opd_test_set_fuse_gemm_ln(opd_detr* m, int on) {
    if (!m) return fail(OPD_EINVAL, "null model handle");
    m->sw.fuse_gemm_ln = on ? 1 : 0;
    m->sw.small_m_gemm = on ? 1 : 0;   // the switch covers the transformer-side specialisations
    m->sw.deep_fc2 = on ? 1 : 0;
    m->sw.fuse_dec0 = on ? 1 : 0;
    m->sw.fused_dec = on ? 1 : 0;   // (the unfused chain is the cross-check of the fused decoder as well)
    if (fill_qc0(m) != OPD_OK) return OPD_EHIP;
    drop_graphs(m);
    return OPD_OK;
}
TAPI int opd_test_set_fuse_btail(opd_detr* m, int on) {   // bit 0: fused bottleneck tails, bit 1: the shortcut of stage 1 inside its first tail
    if (!m) return fail(OPD_EINVAL, "null model handle");
    m->sw.fuse_btail = (on & 1) ? 1 : 0;
    m->sw.fuse_shortcut = (on & 2) ? 1 : 0;
    drop_graphs(m);
    return OPD_OK;
}
TAPI int opd_test_set_pos_shadow(opd_detr* m, int on) {   // 0: row-periodic bias tables W.pos + b (round-1 form) instead of the fp16(x + pos) shadow
    if (!m) return fail(OPD_EINVAL, "null model handle");
    m->sw.pos_shadow = on ? 1 : 0;
    drop_graphs(m);
    return OPD_OK;
}
TAPI int opd_test_set_fuse_stem_pool(opd_detr* m, int on) {
    if (!m) return fail(OPD_EINVAL, "null model handle");
    m->sw.fuse_stem_pool = (on & 1) ? 1 : 0;   // bit 0: stem + pool in one kernel; bit 1: pre-processing inside it as well
    m->sw.fuse_prep = (on & 2) ? 1 : 0;
    drop_graphs(m);
    return OPD_OK;
}

TAPI int opd_test_set_alloc_poison(int byte) {   // -1: off; 0 .. 255: fill byte for the buffers and red zones of handles created from now on
    g_alloc_poison = byte < 0 ? -1 : (byte & 255);
    return OPD_OK;
}
// Scans the red zones of a poison-mode handle (its own buffers and its weight set's): returns the number of buffers with a damaged
// zone (0 = intact) and describes the first one in opd_last_error().
TAPI int opd_test_check_redzones(opd_detr* m) {
    ApiScope api_scope;
    if (!m) return fail(OPD_EINVAL, "null model handle");
    HIPCHK(hipSetDevice(m->device));
    HIPCHK(hipDeviceSynchronize());
    std::vector<unsigned char> h(OPD_REDZONE);
    int bad = 0;
    std::string first;
    auto scan = [&](const std::vector<RedZoned>& v, const char* what) -> int {
        for (size_t i = 0; i < v.size(); ++i)
            for (int side = 0; side < 2; ++side) {
                const unsigned char* z = static_cast<const unsigned char*>(v[i].base) + (side ? OPD_REDZONE + v[i].bytes : 0);
                RCCHK(down(h.data(), z, OPD_REDZONE));
                size_t lo = OPD_REDZONE, hi = 0;
                for (size_t k = 0; k < OPD_REDZONE; ++k)
                    if (h[k] != (unsigned char)v[i].poison) { lo = std::min(lo, k); hi = k; }
                if (lo <= hi) {
                    if (!bad++) first = std::string(what) + " buffer #" + std::to_string(i) + " (" + std::to_string(v[i].bytes) + " bytes): " +
                                        (side ? "zone BEHIND it" : "zone IN FRONT of it") + " overwritten at zone offsets " + std::to_string(lo) + " .. " + std::to_string(hi);
                }
            }
        return OPD_OK;
    };
    RCCHK(scan(m->zoned, "handle"));
    if (m->weights) RCCHK(scan(m->weights->zoned, "weight-set"));
    if (bad) g_err = first;
    return bad;
}
TAPI int opd_test_set_graph_guard(int on) {
    g_graph_guard = on ? 1 : 0;
    return OPD_OK;
}
// Diagnostic taps: after every launch of the forward a checksum launch of that launch's output (captured into the graph with it).
TAPI int opd_test_set_taps(opd_detr* m, int on) {
    ApiScope api_scope;
    if (!m) return fail(OPD_EINVAL, "null model handle");
    HIPCHK(hipSetDevice(m->device));
    if (on && !m->d_taps) RCCHK(dalloc(m, &m->d_taps, (size_t)OPD_MAX_TAPS * OPD_TAP_BLOCKS, false));
    m->taps = on ? 1 : 0;
    drop_graphs(m);
    return OPD_OK;
}
// sums[i] = checksum of tap i of the last forward, names = '\n'-joined tap names; returns the number of taps
TAPI int opd_test_read_taps(opd_detr* m, unsigned long long* sums, int cap, char* names, int names_cap) {
    ApiScope api_scope;
    if (!m || !sums || !m->d_taps) return fail(OPD_EINVAL, "opd_test_read_taps: taps are not enabled");
    HIPCHK(hipSetDevice(m->device));
    HIPCHK(hipStreamSynchronize(m->stream));
    const int n = std::min(cap, (int)m->tap_names.size());
    std::vector<unsigned long long> h((size_t)n * OPD_TAP_BLOCKS);
    if (n) RCCHK(down(h.data(), m->d_taps, h.size()));
    std::string all;
    for (int i = 0; i < n; ++i) {
        unsigned long long s = 0;
        for (int j = 0; j < OPD_TAP_BLOCKS; ++j) s += h[(size_t)i * OPD_TAP_BLOCKS + j];
        sums[i] = s;
        all += m->tap_names[i];
        all += '\n';
    }
    if (names && names_cap > 0) { strncpy(names, all.c_str(), (size_t)names_cap - 1); names[names_cap - 1] = 0; }
    return n;
}
