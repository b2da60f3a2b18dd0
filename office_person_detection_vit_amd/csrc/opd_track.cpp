// opd_track.cpp — the tracker handle of include/opd_detr.h (opd_track_*).  An update stages the frame's detections in page-locked memory,
// enqueues one upload, the predict / cost launch and the download of the three cost matrices on the handle's stream and waits once;
// associates on the host (opd_assoc.cpp); updates ids and counters; uploads the list of matched and new tracks and enqueues the commit
// launch without waiting for it.  The staging buffers have their full size from creation, so no call allocates.
//
// Why nothing needs a second wait: the list of the commit launch is written into its own region of the page-locked image AFTER the call's
// wait, which also covers the previous call's upload of that region; the inputs are written before the wait, and their previous upload
// was covered by the previous call's wait.
//
// The fused detect-and-track call (opd_detr_detect_frames_track, opd_api.cpp) runs the same three parts with another front: instead of the upload,
// track_ingest_kernel writes the staging image from the detector's records on the DETECTOR's stream, the predict / cost launch follows there, and
// the wait is the detect pipeline's.  An event recorded on the handle's stream orders that work behind the previous commit launch.
//
// The sequence calls (opd_track_update_sequence here, opd_detr_detect_sequence_track in opd_api.cpp) take a run of frames with ONE wait:
// the table of tracks goes to the device, track_assoc_kernel does part 2 there between the launches of every frame, and the table comes back and is
// adopted after the wait.  Between calls the host's copy stays the authoritative one, so the per-frame calls above are untouched.
//
// The streams calls (opd_track_update_streams here, opd_detr_detect_streams_track in opd_api.cpp) are sequence calls of C trackers side by side:
// step s is the s-th frame of every camera that has one, in at most four launches over C parameter blocks in device memory (StreamsDescs), one wait.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <string>

#include "opd_assoc.h"
#include "opd_track.h"

#pragma clang fp contract(off)

using namespace opd;

namespace {

TrackDets dets_of(const opd_track* t, const uint8_t* base, int n, bool with_features) {
    TrackDets d{};
    d.boxes = reinterpret_cast<const float*>(base + t->o_boxes);
    d.foot = reinterpret_cast<const float*>(base + t->o_foot);
    d.feat = with_features ? reinterpret_cast<const float*>(base + t->o_feat) : nullptr;
    d.has = base + t->o_has;
    d.n = n;
    return d;
}

void drop_all(opd_track* t) {
    t->tracks.clear();
    t->free_slots.clear();
    for (int s = t->S - 1; s >= 0; --s) t->free_slots.push_back(s);   // slot 0 is handed out first
    t->next_id = 1;
    t->last_T = t->last_N = 0;
}

// ---- the three parts of an update; opd_track_update and the fused detect-and-track call are both made of them ---------------------------------

// Part 1, before the wait, on stream `s`: the slot list (unless the caller's copy carried it), the predict / cost launch when tracks are alive, and
// the three matrices, `n_cols` columns each.  `n_dev` (nullable): where the ingest launch left the detection count; `n_cols` is then its upper bound.
int enqueue_predict(opd_track* t, hipStream_t s, int n_cols, bool with_features, const int32_t* n_dev, bool upload_slots) {
    const int T = (int)t->tracks.size();
    uint8_t* h = t->io.host;
    uint8_t* d = t->io.dev;
    if (T == 0) return OPD_OK;
    if (upload_slots) HIPCHK(hipMemcpyAsync(d + t->o_slots, h + t->o_slots, (size_t)T * 4, hipMemcpyHostToDevice, s));
    TrackPredictParams p{};
    p.s = t->st;
    p.d = dets_of(t, d, n_cols, with_features);
    p.T = T; p.D = t->D;
    p.slots = reinterpret_cast<const int32_t*>(d + t->o_slots);
    p.app = reinterpret_cast<float*>(d + t->o_app);
    p.iou = reinterpret_cast<float*>(d + t->o_iou);
    p.comb = reinterpret_cast<float*>(d + t->o_comb);
    p.aw = t->aw; p.mw = t->mw;
    p.max_dist = (float)t->max_dist;
    p.n_dev = n_dev;
    HIPCHK(opd_launch_track_predict_cost(p, s));
    ++t->last_launches;
    const size_t mat = (size_t)T * n_cols * 4;
    if (mat) {
        HIPCHK(hipMemcpyAsync(h + t->o_app, d + t->o_app, mat, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(h + t->o_iou, d + t->o_iou, mat, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(h + t->o_comb, d + t->o_comb, mat, hipMemcpyDeviceToHost, s));
    }
    return OPD_OK;
}

void fill_slots(opd_track* t) {
    int32_t* h_slots = reinterpret_cast<int32_t*>(t->io.host + t->o_slots);
    for (size_t i = 0; i < t->tracks.size(); ++i) h_slots[i] = t->tracks[i].slot;
}

// Part 2, after the wait: the association over the [T][n] matrices in the page-locked image (row stride n), ids and counters.  `conf`: the
// confidence of detection j at conf[j * conf_stride].  Leaves the list of the commit launch in the image and returns its length in *M.
int associate_update(opd_track* t, const float* conf, int conf_stride, int n, int32_t* out_ids, const std::string& who, int* M_out) {
    const int T = (int)t->tracks.size();
    uint8_t* h = t->io.host;
    t->last_T = T; t->last_N = n;
    for (TrackEntry& e : t->tracks) ++e.tsu;   // `Track.predict`
    std::vector<int32_t> hits(T);
    for (int i = 0; i < T; ++i) hits[i] = t->tracks[i].hits;
    std::vector<float> packed;
    if (conf_stride != 1) {
        packed.resize(n);
        for (int j = 0; j < n; ++j) packed[j] = conf[(size_t)j * conf_stride];
        conf = packed.data();
    }
    AssocResult a;
    associate(reinterpret_cast<const float*>(h + t->o_app), reinterpret_cast<const float*>(h + t->o_iou), reinterpret_cast<const float*>(h + t->o_comb), T, n,
              hits.data(), conf, t->min_hits, t->high_conf, &a);
    for (int j = 0; j < n; ++j) out_ids[j] = -1;
    int rc = OPD_OK;
    if (a.new_dets.size() > t->free_slots.size()) {
        rc = fail(OPD_EINVAL, who + ": " + std::to_string(T) + " live tracks and " + std::to_string(a.new_dets.size()) + " new ones exceed max_tracks = " +
                                  std::to_string(t->S) + "; the frame was counted as one without detections");
        a.matches.clear();
        a.new_dets.clear();
    }
    int32_t* ops = reinterpret_cast<int32_t*>(h + t->o_ops);
    int M = 0;
    for (const auto& m : a.matches) {
        TrackEntry& e = t->tracks[m.first];
        ops[4 * M] = e.slot; ops[4 * M + 1] = m.second; ops[4 * M + 2] = TRACK_OP_MATCHED; ops[4 * M + 3] = e.tsu;
        ++M;
        ++e.age; ++e.hits; e.tsu = 0;
        out_ids[m.second] = e.id;
    }
    for (int j : a.new_dets) {
        TrackEntry e{t->free_slots.back(), t->next_id++, 1, 1, 0};
        t->free_slots.pop_back();
        ops[4 * M] = e.slot; ops[4 * M + 1] = j; ops[4 * M + 2] = TRACK_OP_NEW; ops[4 * M + 3] = 0;
        ++M;
        t->tracks.push_back(e);
        out_ids[j] = e.id;
    }
    *M_out = M;
    return rc;
}

// Part 3: the list and the commit launch on the handle's own stream, not waited for; then the tracks that went max_age frames without a match
// leave, and their slots are free for the next frame.
int enqueue_commit(opd_track* t, int M, int n, bool with_features) {
    uint8_t* h = t->io.host;
    uint8_t* d = t->io.dev;
    if (M > 0) {
        HIPCHK(hipMemcpyAsync(d + t->o_ops, h + t->o_ops, (size_t)M * 16, hipMemcpyHostToDevice, t->stream));
        TrackCommitParams c{};
        c.s = t->st;
        c.d = dets_of(t, d, n, with_features);
        c.M = M; c.D = t->D;
        c.ops = reinterpret_cast<const int32_t*>(d + t->o_ops);
        HIPCHK(opd_launch_track_commit(c, t->stream));
        ++t->last_launches;
    }
    size_t keep = 0;
    for (size_t i = 0; i < t->tracks.size(); ++i) {
        if (t->tracks[i].tsu < t->max_age) t->tracks[keep++] = t->tracks[i];
        else t->free_slots.push_back(t->tracks[i].slot);
    }
    t->tracks.resize(keep);
    return OPD_OK;
}

int update_body(opd_track* t, const float* boxes, const float* foot, const float* conf, const float* features, const uint8_t* has, int kind, int n,
                int32_t* out_ids) {
    const int D = t->D;
    HIPCHK(hipSetDevice(t->device));
    const bool with_features = features != nullptr && n > 0;
    if (with_features && kind == OPD_MEM_DEVICE && !device_accessible(features))
        return fail(OPD_EINVAL, "opd_track_update: OPD_MEM_DEVICE, but the features are not device-accessible memory");
    uint8_t* h = t->io.host;
    uint8_t* d = t->io.dev;
    t->last_launches = t->last_waits = 0;
    // ---- upload: [slots | boxes | foot | has] in one copy (the regions are adjacent), the features in a second one
    fill_slots(t);
    if (n > 0) {
        memcpy(h + t->o_boxes, boxes, (size_t)n * 16);
        memcpy(h + t->o_foot, foot, (size_t)n * 8);
        if (with_features && has) memcpy(h + t->o_has, has, (size_t)n);
        else memset(h + t->o_has, with_features ? 1 : 0, (size_t)n);
    }
    HIPCHK(hipMemcpyAsync(d + t->o_slots, h + t->o_slots, t->o_feat - t->o_slots, hipMemcpyHostToDevice, t->stream));
    if (with_features) {
        if (kind == OPD_MEM_HOST) {
            memcpy(h + t->o_feat, features, (size_t)n * D * 4);
            HIPCHK(hipMemcpyAsync(d + t->o_feat, h + t->o_feat, (size_t)n * D * 4, hipMemcpyHostToDevice, t->stream));
        } else {
            HIPCHK(hipMemcpyAsync(d + t->o_feat, features, (size_t)n * D * 4, hipMemcpyDeviceToDevice, t->stream));
        }
    }
    // ---- launch 1 and the matrices
    RCCHK(enqueue_predict(t, t->stream, n, with_features, nullptr, false));
    HIPCHK(hipStreamSynchronize(t->stream));
    ++t->last_waits;
    int M = 0;
    const int rc = associate_update(t, conf, 1, n, out_ids, "opd_track_update", &M);
    RCCHK(enqueue_commit(t, M, n, with_features));
    return rc;
}

// ---- sequence calls: the table goes to the device once, every frame is predict / cost -> association -> commit without a wait, the table
// comes back behind the call's one wait -------------------------------------------------------------------------------------------------------------

// t->seq, the same on both sides: [header | entries [S] | free-slot stack [S] | ids [n_ids] | boxes | foot points | confidences | flags | features].  The
// part up to the ids travels both ways; the detections behind them are opd_track_update_sequence's (`rows` of them), read in place by the launches.
struct SeqLayout { size_t o_hdr, o_tab, o_free, o_ids, o_boxes, o_foot, o_conf, o_has, o_feat, bytes; };

SeqLayout seq_layout(const opd_track* t, size_t n_ids, size_t rows, bool feats) {
    SeqLayout q{};
    size_t off = 0;
    auto place = [&](size_t bytes) { const size_t o = off; off += align_up(bytes, 256); return o; };
    q.o_hdr = place(TRACK_HDR_INTS * 4); q.o_tab = place((size_t)t->S * sizeof(TrackEntry)); q.o_free = place((size_t)t->S * 4); q.o_ids = place(n_ids * 4);
    q.o_boxes = place(rows * 16); q.o_foot = place(rows * 8); q.o_conf = place(rows * 4); q.o_has = place(rows);
    q.o_feat = place(feats ? rows * t->D * 4 : 0);
    q.bytes = off;
    return q;
}

// The page-locked side of the table: the host's tracks, free slots and next id as they are, every id of the call -1
int seq_begin(opd_track* t, const SeqLayout& q, size_t n_ids, const char* who) {
    bool moved = false;
    RCCHK(t->seq.reserve(who, q.bytes, q.bytes, t->stream, &moved));
    if (moved) ++g_handle_epoch;   // device memory changed hands (opd_device.h)
    uint8_t* h = t->seq.host;
    int32_t* hdr = reinterpret_cast<int32_t*>(h + q.o_hdr);
    memset(hdr, 0, TRACK_HDR_INTS * 4);
    hdr[TRACK_HDR_T] = (int32_t)t->tracks.size();
    hdr[TRACK_HDR_NEXT_ID] = t->next_id;
    hdr[TRACK_HDR_N_FREE] = (int32_t)t->free_slots.size();
    if (!t->tracks.empty()) memcpy(h + q.o_tab, t->tracks.data(), t->tracks.size() * sizeof(TrackEntry));
    if (!t->free_slots.empty()) memcpy(h + q.o_free, t->free_slots.data(), t->free_slots.size() * 4);
    int32_t* ids = reinterpret_cast<int32_t*>(h + q.o_ids);
    for (size_t j = 0; j < n_ids; ++j) ids[j] = -1;
    t->last_launches = t->last_waits = 0;
    return OPD_OK;
}

// The parameter blocks of one frame of a sequence.  `dets`: its detections on the device, dets.n of them at most (n_dev, nullable: where the exact count lies).
// t_bound: an upper bound of the tracks alive when the frame starts; the launches take the true numbers from the table.  `predict` / `commit`: whether
// that launch has anything to do under these bounds.  seq_enqueue_frame launches them one tracker at a time, a streams call C trackers at a time.
struct SeqFrameParams { TrackPredictParams p; TrackAssocParams a; TrackCommitParams c; bool predict, commit; };

SeqFrameParams seq_frame_params(const opd_track* t, const SeqLayout& q, const TrackDets& dets, const int32_t* n_dev, const float* conf, int conf_stride, int32_t* ids_dev,
                                int frame, int t_bound) {
    uint8_t* d = t->io.dev;
    uint8_t* sq = t->seq.dev;
    int32_t* hdr = reinterpret_cast<int32_t*>(sq + q.o_hdr);
    int32_t* tab = reinterpret_cast<int32_t*>(sq + q.o_tab);
    SeqFrameParams f{};
    f.predict = t_bound > 0;
    TrackPredictParams& p = f.p;
    p.s = t->st; p.d = dets;
    p.T = t_bound; p.D = t->D;
    p.app = reinterpret_cast<float*>(d + t->o_app); p.iou = reinterpret_cast<float*>(d + t->o_iou); p.comb = reinterpret_cast<float*>(d + t->o_comb);
    p.aw = t->aw; p.mw = t->mw;
    p.max_dist = (float)t->max_dist;
    p.n_dev = n_dev; p.hdr = hdr; p.tab = tab;
    TrackAssocParams& a = f.a;
    a.hdr = hdr; a.tab = tab; a.free_slots = reinterpret_cast<int32_t*>(sq + q.o_free);
    a.app = reinterpret_cast<const float*>(d + t->o_app); a.iou = reinterpret_cast<const float*>(d + t->o_iou); a.comb = reinterpret_cast<const float*>(d + t->o_comb);
    a.conf = conf; a.conf_stride = conf_stride;
    a.n_dev = n_dev; a.n = dets.n;
    a.ops = reinterpret_cast<int32_t*>(d + t->o_ops); a.ids = ids_dev;
    a.S = t->S; a.min_hits = t->min_hits; a.max_age = t->max_age; a.frame = frame;
    a.high_conf = t->high_conf;
    const int m_bound = std::min<int>(t->S, dets.n);
    f.commit = m_bound > 0;
    TrackCommitParams& c = f.c;
    c.s = t->st; c.d = dets;
    c.M = m_bound; c.D = t->D;
    c.ops = a.ops; c.hdr = hdr;
    return f;
}

// One frame on stream `s`
int seq_enqueue_frame(opd_track* t, hipStream_t s, const SeqLayout& q, const TrackDets& dets, const int32_t* n_dev, const float* conf, int conf_stride,
                      int32_t* ids_dev, int frame, int t_bound) {
    const SeqFrameParams f = seq_frame_params(t, q, dets, n_dev, conf, conf_stride, ids_dev, frame, t_bound);
    if (f.predict) {
        HIPCHK(opd_launch_track_predict_cost(f.p, s));
        ++t->last_launches;
    }
    HIPCHK(opd_launch_track_assoc(f.a, s));
    ++t->last_launches;
    if (f.commit) {
        HIPCHK(opd_launch_track_commit(f.c, s));
        ++t->last_launches;
    }
    return OPD_OK;
}

// After the wait that covered the download of [header | entries | stack | ids]: the host's copy becomes what the device left.  *frames_done: the frames
// applied, the out-of-slots one included; that frame is the call's error, in opd_track_update's words.
int seq_adopt(opd_track* t, const SeqLayout& q, int F, int32_t* frames_done, const std::string& who) {
    const uint8_t* h = t->seq.host;
    const int32_t* hdr = reinterpret_cast<const int32_t*>(h + q.o_hdr);
    const int T = hdr[TRACK_HDR_T], n_free = hdr[TRACK_HDR_N_FREE];
    if (T < 0 || n_free < 0 || T + n_free != t->S) return fail(OPD_EHIP, who + ": the track table came back with " + std::to_string(T) + " tracks and " + std::to_string(n_free) + " free slots of " + std::to_string(t->S));
    const TrackEntry* e = reinterpret_cast<const TrackEntry*>(h + q.o_tab);
    const int32_t* fs = reinterpret_cast<const int32_t*>(h + q.o_free);
    t->tracks.assign(e, e + T);
    t->free_slots.assign(fs, fs + n_free);
    t->next_id = hdr[TRACK_HDR_NEXT_ID];
    t->last_T = t->last_N = 0;   // (no matrix came to the host)
    const bool stopped = hdr[TRACK_HDR_STOPPED] != 0;
    *frames_done = stopped ? hdr[TRACK_HDR_FRAMES_DONE] : F;
    if (stopped)
        return fail(OPD_EINVAL, who + ": " + std::to_string(hdr[TRACK_HDR_STOP_T]) + " live tracks and " + std::to_string(hdr[TRACK_HDR_STOP_NEW]) + " new ones exceed max_tracks = " +
                                    std::to_string(t->S) + "; the frame was counted as one without detections (frame " + std::to_string(hdr[TRACK_HDR_FRAMES_DONE] - 1) +
                                    " of the call; the frames after it were not applied)");
    return OPD_OK;
}

int update_sequence_body(opd_track* t, const float* boxes, const float* foot, const float* conf, const float* features, const uint8_t* has, int kind,
                         const int32_t* counts, int F, int32_t* out_ids, int32_t* frames_done) {
    const int D = t->D;
    size_t total = 0;
    for (int f = 0; f < F; ++f) total += (size_t)counts[f];
    HIPCHK(hipSetDevice(t->device));
    const bool feats = features != nullptr && total > 0;
    if (feats && kind == OPD_MEM_DEVICE && !device_accessible(features))
        return fail(OPD_EINVAL, "opd_track_update_sequence: OPD_MEM_DEVICE, but the features are not device-accessible memory");
    const SeqLayout q = seq_layout(t, total, total, feats);
    RCCHK(seq_begin(t, q, total, "opd_track_update_sequence"));
    uint8_t* h = t->seq.host;
    uint8_t* sq = t->seq.dev;
    // ---- upload: table, ids and every frame's detections in one copy, device features in a second one
    if (total > 0) {
        memcpy(h + q.o_boxes, boxes, total * 16);
        memcpy(h + q.o_foot, foot, total * 8);
        memcpy(h + q.o_conf, conf, total * 4);
        if (feats && has) memcpy(h + q.o_has, has, total);
        else memset(h + q.o_has, feats ? 1 : 0, total);
        if (feats && kind == OPD_MEM_HOST) memcpy(h + q.o_feat, features, total * D * 4);
    }
    const bool feats_by_host = feats && kind == OPD_MEM_HOST;
    HIPCHK(hipMemcpyAsync(sq, h, feats_by_host ? q.bytes : q.o_feat, hipMemcpyHostToDevice, t->stream));
    if (feats && !feats_by_host) HIPCHK(hipMemcpyAsync(sq + q.o_feat, features, total * D * 4, hipMemcpyDeviceToDevice, t->stream));
    // ---- the frames, in stream order
    size_t row = 0;
    int t_bound = (int)t->tracks.size();
    for (int f = 0; f < F; ++f) {
        const int n = counts[f];
        TrackDets d{};
        d.boxes = reinterpret_cast<const float*>(sq + q.o_boxes) + row * 4;
        d.foot = reinterpret_cast<const float*>(sq + q.o_foot) + row * 2;
        d.feat = feats && n > 0 ? reinterpret_cast<const float*>(sq + q.o_feat) + row * D : nullptr;
        d.has = sq + q.o_has + row;
        d.n = n;
        RCCHK(seq_enqueue_frame(t, t->stream, q, d, nullptr, reinterpret_cast<const float*>(sq + q.o_conf) + row, 1, reinterpret_cast<int32_t*>(sq + q.o_ids) + row, f, t_bound));
        row += (size_t)n;
        t_bound = std::min<int>(t->S, t_bound + n);
    }
    // ---- one download, one wait
    HIPCHK(hipMemcpyAsync(h, sq, q.o_ids + total * 4, hipMemcpyDeviceToHost, t->stream));
    HIPCHK(hipStreamSynchronize(t->stream));
    ++t->last_waits;
    if (total > 0) memcpy(out_ids, h + q.o_ids, total * 4);
    return seq_adopt(t, q, F, frames_done, "opd_track_update_sequence");
}

// The ingest block of frame b of a call's records into t's staging image, inside a sequence (`hdr` set)
TrackIngestParams seq_ingest_params(const opd_track* t, const SeqLayout& q, const RecordView& view, int b, const TrackFeatureSource& src) {
    uint8_t* d = t->io.dev;
    TrackIngestParams p{};
    p.view = record_frame(view, b); p.D = t->D; p.frame = b;
    p.rows_kind = src.rows_kind; p.rows = src.rows; p.slot_map = src.slot_map; p.n_person = src.n_person; p.slots = src.slots;
    p.boxes = reinterpret_cast<float*>(d + t->o_boxes);
    p.foot = reinterpret_cast<float*>(d + t->o_foot);
    p.has = d + t->o_has;
    p.feat = reinterpret_cast<float*>(d + t->o_feat);
    p.n_out = reinterpret_cast<int32_t*>(d + t->o_n);
    p.hdr = reinterpret_cast<const int32_t*>(t->seq.dev + q.o_hdr);
    return p;
}

// ---- streams calls: the sequence call's steps for C trackers side by side ------------------------------------------------------------
// The parameter blocks of every step and all four kinds, [steps][C] each, in the page-locked half of trackers[0]->desc; one copy takes them to the device
// half, and each step is at most four launches over them, whatever C is.  A zeroed block (`hdr` null) is a camera without work in that launch.
struct StreamsDescs {
    opd_track* owner = nullptr;
    int C = 0, steps = 0;
    bool ingest = false;
    size_t o_in = 0, o_p = 0, o_a = 0, o_c = 0, bytes = 0;
    int begin(opd_track* t0, int C_, int steps_, bool ingest_, const char* who) {
        owner = t0; C = C_; steps = steps_; ingest = ingest_;
        const size_t n = (size_t)steps * C;
        size_t off = 0;
        auto place = [&](size_t b) { const size_t o = off; off += align_up(b, 256); return o; };
        o_in = place(ingest ? n * sizeof(TrackIngestParams) : 0); o_p = place(n * sizeof(TrackPredictParams)); o_a = place(n * sizeof(TrackAssocParams));
        o_c = place(n * sizeof(TrackCommitParams));
        bytes = off;
        bool moved = false;
        RCCHK(t0->desc.reserve(who, bytes, bytes, t0->stream, &moved));
        if (moved) ++g_handle_epoch;   // device memory changed hands (opd_device.h)
        memset(t0->desc.host, 0, bytes);
        return OPD_OK;
    }
    template <typename P> P* at(uint8_t* base, size_t o, int s) const { return reinterpret_cast<P*>(base + o) + (size_t)s * C; }
    void set(int s, int c, const SeqFrameParams& f) {
        if (f.predict) at<TrackPredictParams>(owner->desc.host, o_p, s)[c] = f.p;
        at<TrackAssocParams>(owner->desc.host, o_a, s)[c] = f.a;
        if (f.commit) at<TrackCommitParams>(owner->desc.host, o_c, s)[c] = f.c;
    }
    void set(int s, int c, const TrackIngestParams& p) { at<TrackIngestParams>(owner->desc.host, o_in, s)[c] = p; }
    // the upload and the steps on stream `st`; *launches: the launches made
    int run(hipStream_t st, int* launches) const {
        uint8_t* h = owner->desc.host;
        uint8_t* d = owner->desc.dev;
        HIPCHK(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, st));
        *launches = 0;
        for (int s = 0; s < steps; ++s) {
            int made = 0;
            if (ingest) {
                HIPCHK(opd_launch_track_ingest_multi(at<TrackIngestParams>(h, o_in, s), at<TrackIngestParams>(d, o_in, s), C, st, &made));
                *launches += made;
            }
            HIPCHK(opd_launch_track_predict_cost_multi(at<TrackPredictParams>(h, o_p, s), at<TrackPredictParams>(d, o_p, s), C, st, &made));   // (none where no camera can have a live track)
            *launches += made;
            HIPCHK(opd_launch_track_assoc_multi(at<TrackAssocParams>(h, o_a, s), at<TrackAssocParams>(d, o_a, s), C, st, &made));
            *launches += made;
            HIPCHK(opd_launch_track_commit_multi(at<TrackCommitParams>(h, o_c, s), at<TrackCommitParams>(d, o_c, s), C, st, &made));
            *launches += made;
        }
        return OPD_OK;
    }
};

// `s` behind whatever each tracker's own stream still holds (its previous commit launch reads the staging image this call overwrites)
int streams_order(opd_track* const* trackers, int C, hipStream_t s) {
    for (int c = 0; c < C; ++c) {
        if (trackers[c]->stream == s) continue;
        HIPCHK(hipEventRecord(trackers[c]->ev_commit, trackers[c]->stream));
        HIPCHK(hipStreamWaitEvent(s, trackers[c]->ev_commit, 0));
    }
    return OPD_OK;
}

// seq_adopt per camera: every camera that ran to its end is adopted whatever another one did; the error is the lowest-numbered failing camera's,
// under a name that says which, with the list of every camera that ran out of slots behind it
int streams_adopt(opd_track* const* trackers, int C, const std::vector<SeqLayout>& q, const std::vector<int>& n_frames, int launches, int32_t* frames_done, const char* who) {
    int rc = OPD_OK;
    std::string first, stopped;
    for (int c = 0; c < C; ++c) {
        trackers[c]->last_launches = launches;
        const int one = seq_adopt(trackers[c], q[c], n_frames[c], &frames_done[c], std::string(who) + ": camera " + std::to_string(c));
        if (one != OPD_OK && rc == OPD_OK) { rc = one; first = g_err; }
        if (one == OPD_EINVAL) stopped += (stopped.empty() ? "" : ", ") + std::to_string(c);
    }
    if (rc == OPD_OK) return OPD_OK;
    return fail(rc, stopped.empty() ? first : first + "; cameras out of slots: " + stopped);
}

int update_streams_body(opd_track* const* trackers, int C, const int32_t* camera_of, int F, const float* boxes, const float* foot, const float* conf, const float* features,
                        const uint8_t* has, int kind, const int32_t* counts, int32_t* out_ids, int32_t* frames_done) {
    const char* who = "opd_track_update_streams";
    opd_track* t0 = trackers[0];
    hipStream_t s = t0->stream;
    const std::vector<std::vector<int32_t>> sched = streams_schedule(camera_of, F, C);
    const int steps = (int)sched.size();
    // where frame f lies in the packed arrays: its first detection, and its first feature float (rows as wide as its own tracker's feature_dim)
    std::vector<size_t> det_at(F + 1, 0), feat_at(F + 1, 0);
    for (int f = 0; f < F; ++f) {
        det_at[f + 1] = det_at[f] + (size_t)counts[f];
        feat_at[f + 1] = feat_at[f] + (size_t)counts[f] * trackers[camera_of[f]]->D;
    }
    std::vector<size_t> total(C, 0);
    std::vector<int> n_frames(C, 0);
    for (int f = 0; f < F; ++f) { total[camera_of[f]] += (size_t)counts[f]; ++n_frames[camera_of[f]]; }
    HIPCHK(hipSetDevice(t0->device));
    const bool any_feats = features != nullptr && det_at[F] > 0;
    if (any_feats && kind == OPD_MEM_DEVICE && !device_accessible(features))
        return fail(OPD_EINVAL, std::string(who) + ": OPD_MEM_DEVICE, but the features are not device-accessible memory");
    const bool feats_by_host = any_feats && kind == OPD_MEM_HOST;
    std::vector<SeqLayout> q(C);
    for (int c = 0; c < C; ++c) {
        q[c] = seq_layout(trackers[c], total[c], total[c], any_feats && total[c] > 0);
        RCCHK(seq_begin(trackers[c], q[c], total[c], who));
    }
    StreamsDescs descs;
    RCCHK(descs.begin(t0, C, steps, false, who));
    RCCHK(streams_order(trackers, C, s));
    // ---- per camera: its frames gathered in its own order behind its table, the blocks of its steps, one copy up (device features: a copy per frame)
    for (int c = 0; c < C; ++c) {
        opd_track* t = trackers[c];
        const bool feats = any_feats && total[c] > 0;
        const int D = t->D;
        uint8_t* h = t->seq.host;
        uint8_t* sq = t->seq.dev;
        size_t row = 0;
        int t_bound = (int)t->tracks.size();
        for (int k = 0; k < n_frames[c]; ++k) {
            const int f = sched[k][c], n = counts[f];
            if (n > 0) {
                memcpy(h + q[c].o_boxes + row * 16, boxes + det_at[f] * 4, (size_t)n * 16);
                memcpy(h + q[c].o_foot + row * 8, foot + det_at[f] * 2, (size_t)n * 8);
                memcpy(h + q[c].o_conf + row * 4, conf + det_at[f], (size_t)n * 4);
                if (feats && has) memcpy(h + q[c].o_has + row, has + det_at[f], (size_t)n);
                else memset(h + q[c].o_has + row, feats ? 1 : 0, (size_t)n);
                if (feats && feats_by_host) memcpy(h + q[c].o_feat + row * D * 4, features + feat_at[f], (size_t)n * D * 4);
                if (feats && !feats_by_host) HIPCHK(hipMemcpyAsync(sq + q[c].o_feat + row * D * 4, features + feat_at[f], (size_t)n * D * 4, hipMemcpyDeviceToDevice, s));
            }
            TrackDets d{};
            d.boxes = reinterpret_cast<const float*>(sq + q[c].o_boxes) + row * 4;
            d.foot = reinterpret_cast<const float*>(sq + q[c].o_foot) + row * 2;
            d.feat = feats && n > 0 ? reinterpret_cast<const float*>(sq + q[c].o_feat) + row * D : nullptr;
            d.has = sq + q[c].o_has + row;
            d.n = n;
            descs.set(k, c, seq_frame_params(t, q[c], d, nullptr, reinterpret_cast<const float*>(sq + q[c].o_conf) + row, 1, reinterpret_cast<int32_t*>(sq + q[c].o_ids) + row, k, t_bound));
            row += (size_t)n;
            t_bound = std::min<int>(t->S, t_bound + n);
        }
        HIPCHK(hipMemcpyAsync(sq, h, feats && feats_by_host ? q[c].bytes : q[c].o_feat, hipMemcpyHostToDevice, s));
    }
    // ---- the steps, every tracker's table back, one wait
    int launches = 0;
    RCCHK(descs.run(s, &launches));
    for (int c = 0; c < C; ++c) HIPCHK(hipMemcpyAsync(trackers[c]->seq.host, trackers[c]->seq.dev, q[c].o_ids + total[c] * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    ++t0->last_waits;
    for (int c = 0; c < C; ++c) {
        const int32_t* ids = reinterpret_cast<const int32_t*>(trackers[c]->seq.host + q[c].o_ids);
        size_t row = 0;
        for (int k = 0; k < n_frames[c]; ++k) {
            const int f = sched[k][c];
            if (counts[f] > 0) memcpy(out_ids + det_at[f], ids + row, (size_t)counts[f] * 4);
            row += (size_t)counts[f];
        }
    }
    return streams_adopt(trackers, C, q, n_frames, launches, frames_done, who);
}

}  // namespace

namespace opd {

std::vector<std::vector<int32_t>> streams_schedule(const int32_t* camera_of, int F, int C) {
    std::vector<std::vector<int32_t>> steps;
    std::vector<int> seen(C > 0 ? C : 0, 0);
    for (int f = 0; f < F; ++f) {
        const int c = camera_of[f];
        if (c < 0 || c >= C) continue;
        const int k = seen[c]++;
        if (k >= (int)steps.size()) steps.emplace_back(C, -1);
        steps[k][c] = f;
    }
    return steps;
}

int track_streams_check(opd_track* const* trackers, int C, const int32_t* camera_of, int F, const char* who) {
    const std::string me = std::string(who) + ": ";
    std::vector<int> n_frames(C, 0);
    for (int f = 0; f < F; ++f) {
        if (camera_of[f] < 0 || camera_of[f] >= C)
            return fail(OPD_EINVAL, me + "camera_of[" + std::to_string(f) + "] = " + std::to_string(camera_of[f]) + " outside 0 .. C - 1 = " + std::to_string(C - 1));
        ++n_frames[camera_of[f]];
    }
    for (int b = 0; b < C; ++b)
        for (int a = 0; a < b; ++a)
            if (trackers[a] == trackers[b])
                return fail(OPD_EINVAL, me + "cameras " + std::to_string(a) + " and " + std::to_string(b) + " name the same tracker; a tracker follows one camera");
    for (int c = 0; c < C; ++c)
        if (n_frames[c] == 0) return fail(OPD_EINVAL, me + "camera " + std::to_string(c) + " gets no frame of the call; leave its tracker out of the list");
    return OPD_OK;
}

int track_streams_enqueue(opd_track* const* trackers, int C, const int32_t* camera_of, hipStream_t s, const opd_det* records, const int32_t* counts, int Q, int B,
                          const TrackFeatureSource& src, const char* who) {
    const std::vector<std::vector<int32_t>> sched = streams_schedule(camera_of, B, C);
    const bool with_features = src.rows_kind != TRACK_ROWS_NONE;
    const RecordView view{records, nullptr, counts, B, Q};
    std::vector<SeqLayout> q(C);
    std::vector<int> n_frames(C, 0);
    for (int b = 0; b < B; ++b) ++n_frames[camera_of[b]];
    for (int c = 0; c < C; ++c) {
        q[c] = seq_layout(trackers[c], (size_t)n_frames[c] * Q, 0, false);
        RCCHK(seq_begin(trackers[c], q[c], (size_t)n_frames[c] * Q, who));
    }
    StreamsDescs descs;
    RCCHK(descs.begin(trackers[0], C, (int)sched.size(), true, who));
    RCCHK(streams_order(trackers, C, s));
    for (int c = 0; c < C; ++c) {
        opd_track* t = trackers[c];
        uint8_t* sq = t->seq.dev;
        HIPCHK(hipMemcpyAsync(sq, t->seq.host, q[c].o_ids + (size_t)n_frames[c] * Q * 4, hipMemcpyHostToDevice, s));
        int t_bound = (int)t->tracks.size();
        for (int k = 0; k < n_frames[c]; ++k) {
            const int b = sched[k][c];
            const TrackIngestParams p = seq_ingest_params(t, q[c], view, b, src);
            descs.set(k, c, p);
            descs.set(k, c, seq_frame_params(t, q[c], dets_of(t, t->io.dev, Q, with_features), p.n_out, &records[(size_t)b * Q].score, (int)(sizeof(opd_det) / sizeof(float)),
                                             reinterpret_cast<int32_t*>(sq + q[c].o_ids) + (size_t)k * Q, k, t_bound));
            t_bound = std::min<int>(t->S, t_bound + Q);
        }
    }
    int launches = 0;
    RCCHK(descs.run(s, &launches));
    for (int c = 0; c < C; ++c) {
        trackers[c]->last_launches = launches;
        HIPCHK(hipMemcpyAsync(trackers[c]->seq.host, trackers[c]->seq.dev, q[c].o_ids + (size_t)n_frames[c] * Q * 4, hipMemcpyDeviceToHost, s));
    }
    return OPD_OK;
}

int track_streams_finish(opd_track* const* trackers, int C, const int32_t* camera_of, const int32_t* counts, int Q, int B, int32_t* track_ids, int32_t* frames_done,
                         const char* who) {
    const std::vector<std::vector<int32_t>> sched = streams_schedule(camera_of, B, C);
    std::vector<SeqLayout> q(C);
    std::vector<int> n_frames(C, 0);
    for (int b = 0; b < B; ++b) ++n_frames[camera_of[b]];
    for (int c = 0; c < C; ++c) {
        q[c] = seq_layout(trackers[c], (size_t)n_frames[c] * Q, 0, false);
        const int32_t* ids = reinterpret_cast<const int32_t*>(trackers[c]->seq.host + q[c].o_ids);
        for (int k = 0; k < n_frames[c]; ++k) {
            const int b = sched[k][c], n = std::max(0, std::min(counts[b], Q));
            if (n > 0) memcpy(track_ids + (size_t)b * Q, ids + (size_t)k * Q, (size_t)n * 4);
        }
    }
    return streams_adopt(trackers, C, q, n_frames, trackers[0]->last_launches, frames_done, who);
}

int track_sequence_enqueue(opd_track* t, hipStream_t s, const opd_det* records, const int32_t* counts, int Q, int B, const TrackFeatureSource& src, const char* who) {
    const SeqLayout q = seq_layout(t, (size_t)B * Q, 0, false);
    RCCHK(seq_begin(t, q, (size_t)B * Q, who));
    uint8_t* d = t->io.dev;
    uint8_t* sq = t->seq.dev;
    // behind whatever the handle's own stream still holds (the previous commit launch reads the staging image the first ingest launch overwrites)
    HIPCHK(hipEventRecord(t->ev_commit, t->stream));
    HIPCHK(hipStreamWaitEvent(s, t->ev_commit, 0));
    HIPCHK(hipMemcpyAsync(sq, t->seq.host, q.o_ids + (size_t)B * Q * 4, hipMemcpyHostToDevice, s));
    const bool with_features = src.rows_kind != TRACK_ROWS_NONE;
    int t_bound = (int)t->tracks.size();
    for (int b = 0; b < B; ++b) {
        const TrackIngestParams p = seq_ingest_params(t, q, RecordView{records, nullptr, counts, B, Q}, b, src);
        HIPCHK(opd_launch_track_ingest(p, s));
        ++t->last_launches;
        RCCHK(seq_enqueue_frame(t, s, q, dets_of(t, d, Q, with_features), p.n_out, &records[(size_t)b * Q].score, (int)(sizeof(opd_det) / sizeof(float)),
                                reinterpret_cast<int32_t*>(sq + q.o_ids) + (size_t)b * Q, b, t_bound));
        t_bound = std::min<int>(t->S, t_bound + Q);
    }
    HIPCHK(hipMemcpyAsync(t->seq.host, sq, q.o_ids + (size_t)B * Q * 4, hipMemcpyDeviceToHost, s));
    return OPD_OK;
}

int track_sequence_finish(opd_track* t, const int32_t* counts, int Q, int B, int32_t* track_ids, int32_t* frames_done, const char* who) {
    const SeqLayout q = seq_layout(t, (size_t)B * Q, 0, false);
    const int32_t* ids = reinterpret_cast<const int32_t*>(t->seq.host + q.o_ids);
    for (int b = 0; b < B; ++b) {
        const int n = std::max(0, std::min(counts[b], Q));
        if (n > 0) memcpy(track_ids + (size_t)b * Q, ids + (size_t)b * Q, (size_t)n * 4);
    }
    return seq_adopt(t, q, B, frames_done, who);
}

int track_fused_check(const opd_track* t, int device, int Q, int feature_dim, const char* who) {
    const std::string me = std::string(who) + ": ";
    if (!t) return fail(OPD_EINVAL, me + "null tracker handle");
    if (t->device != device) return fail(OPD_EINVAL, me + "the detector is on device " + std::to_string(device) + ", a tracker on device " + std::to_string(t->device));
    if (t->NM < Q)
        return fail(OPD_EINVAL, me + "a tracker was made for max_dets = " + std::to_string(t->NM) + ", the detector can keep num_queries = " + std::to_string(Q) + " records of a frame");
    if (feature_dim > 0 && t->D != feature_dim)
        return fail(OPD_EINVAL, me + "a tracker was made for feature_dim = " + std::to_string(t->D) + ", the rows of this feature kind have " + std::to_string(feature_dim) + " numbers");
    return OPD_OK;
}

int track_fused_enqueue(opd_track* t, hipStream_t s, const RecordView& frame_view, int frame, const TrackFeatureSource& src) {
    uint8_t* d = t->io.dev;
    t->last_launches = t->last_waits = 0;
    // behind whatever the handle's own stream still holds (the previous commit launch reads the staging image the ingest launch overwrites)
    HIPCHK(hipEventRecord(t->ev_commit, t->stream));
    HIPCHK(hipStreamWaitEvent(s, t->ev_commit, 0));
    fill_slots(t);
    TrackIngestParams p{};
    p.view = frame_view; p.D = t->D; p.frame = frame;
    p.rows_kind = src.rows_kind; p.rows = src.rows; p.slot_map = src.slot_map; p.n_person = src.n_person; p.slots = src.slots;
    p.boxes = reinterpret_cast<float*>(d + t->o_boxes);
    p.foot = reinterpret_cast<float*>(d + t->o_foot);
    p.has = d + t->o_has;
    p.feat = reinterpret_cast<float*>(d + t->o_feat);
    p.n_out = reinterpret_cast<int32_t*>(d + t->o_n);
    HIPCHK(opd_launch_track_ingest(p, s));
    ++t->last_launches;
    return enqueue_predict(t, s, frame_view.stride, src.rows_kind != TRACK_ROWS_NONE, p.n_out, true);
}

int track_fused_finish(opd_track* t, const float* conf, int conf_stride, int n, int with_features, int32_t* out_ids, const char* who) {
    int M = 0;
    const int rc = associate_update(t, n > 0 ? conf : nullptr, conf_stride, n, out_ids, who, &M);
    RCCHK(enqueue_commit(t, M, n, with_features != 0));
    return rc;
}

}  // namespace opd

extern "C" int opd_track_create(const opd_track_config* cfg, int device_ordinal, opd_track** out) { return api_call("opd_track_create", [&]() -> int {
    const std::string me = "opd_track_create: ";
    if (!out) return fail(OPD_EINVAL, me + "null argument");
    *out = nullptr;
    if (!cfg) return fail(OPD_EINVAL, me + "null configuration");
    if (cfg->struct_size != (int32_t)sizeof(opd_track_config))
        return fail(OPD_EINVAL, me + "struct_size " + std::to_string(cfg->struct_size) + ", this library's opd_track_config has " + std::to_string(sizeof(opd_track_config)) + " bytes");
    const opd_track_config& c = *cfg;
    const int S = c.max_tracks ? c.max_tracks : 128, NM = c.max_dets ? c.max_dets : 128, D = c.feature_dim ? c.feature_dim : 512;
    if (S < 1 || S > TRACK_MAX_TRACKS) return fail(OPD_EINVAL, me + "max_tracks " + std::to_string(S) + " outside 1 .. 1024");
    if (NM < 1 || NM > TRACK_MAX_DETS) return fail(OPD_EINVAL, me + "max_dets " + std::to_string(NM) + " outside 1 .. 1024");
    if (D < 1 || D > TRACK_MAX_DIM) return fail(OPD_EINVAL, me + "feature_dim " + std::to_string(D) + " outside 1 .. 2048");
    if (c.max_age < 0 || c.min_hits < 0) return fail(OPD_EINVAL, me + "max_age and min_hits must not be negative");
    double aw = c.appearance_weight, mw = c.motion_weight;
    if (aw == 0.0 && mw == 0.0) { aw = 0.7; mw = 0.3; }
    if (!(aw >= 0.0) || !(mw >= 0.0) || !(fabs(aw + mw - 1.0) <= 1e-6))
        return fail(OPD_EINVAL, me + "appearance_weight (" + std::to_string(aw) + ") + motion_weight (" + std::to_string(mw) + ") must equal 1.0");
    if (!(c.high_conf_threshold == c.high_conf_threshold) || !(c.max_position_distance == c.max_position_distance))
        return fail(OPD_EINVAL, me + "a threshold is not a number");
    RCCHK(use_device("opd_track_create", device_ordinal));
    std::unique_ptr<opd_track, decltype(&opd_track_destroy)> t(new opd_track(), opd_track_destroy);   // a failure below releases whatever was already made
    t->device = device_ordinal;
    t->S = S; t->NM = NM; t->D = D;
    t->max_age = c.max_age ? c.max_age : 30;
    t->min_hits = c.min_hits ? c.min_hits : 3;
    t->iou_threshold = c.iou_threshold != 0.0 ? c.iou_threshold : 0.3;
    t->aw = aw; t->mw = mw;
    t->max_dist = c.max_position_distance == 0.0 ? 150.0 : c.max_position_distance;
    t->high_conf = c.high_conf_threshold != 0.0 ? c.high_conf_threshold : 0.5;
    RCCHK(made("opd_track_create", "stream creation", hipStreamCreateWithFlags(&t->stream, hipStreamNonBlocking)));
    RCCHK(made("opd_track_create", "event creation", hipEventCreateWithFlags(&t->ev_commit, hipEventDisableTiming)));
    // the state: one allocation, zeroed
    size_t off = 0;
    auto place = [&](size_t bytes) { const size_t o = off; off += align_up(bytes, 256); return o; };
    const size_t s_x = place((size_t)S * 16), s_P = place((size_t)S * 64), s_last = place((size_t)S * 8), s_box = place((size_t)S * 16);
    const size_t s_ring = place((size_t)S * TRACK_RING * D * 4), s_meta = place((size_t)S * 8), s_smooth = place((size_t)S * D * 4);
    RCCHK(made("opd_track_create", "state allocation", hipMalloc((void**)&t->d_state, off)));
    RCCHK(made("opd_track_create", "state clearing", hipMemset(t->d_state, 0, off)));
    t->st.x = reinterpret_cast<float*>(t->d_state + s_x);
    t->st.P = reinterpret_cast<float*>(t->d_state + s_P);
    t->st.last = reinterpret_cast<float*>(t->d_state + s_last);
    t->st.box = reinterpret_cast<float*>(t->d_state + s_box);
    t->st.ring = reinterpret_cast<float*>(t->d_state + s_ring);
    t->st.ring_meta = reinterpret_cast<int32_t*>(t->d_state + s_meta);
    t->st.smooth = reinterpret_cast<float*>(t->d_state + s_smooth);
    // the staging pair: inputs (adjacent, one copy), the commit list, the three matrices
    off = 0;
    t->o_slots = place((size_t)S * 4); t->o_boxes = place((size_t)NM * 16); t->o_foot = place((size_t)NM * 8); t->o_has = place((size_t)NM);
    t->o_feat = place((size_t)NM * D * 4); t->o_ops = place((size_t)S * 16);
    t->o_app = place((size_t)S * NM * 4); t->o_iou = place((size_t)S * NM * 4); t->o_comb = place((size_t)S * NM * 4);
    t->o_n = place(4);   // the detection count of a fused call, left by its ingest launch for its predict launch
    t->io_bytes = off;
    RCCHK(t->io.reserve("opd_track_create", off, off, t->stream));
    memset(t->io.host, 0, off);
    drop_all(t.get());
    ++g_handle_epoch;   // device memory changed hands: graphs captured before are captured again (opd_device.h)
    *out = t.release();
    return OPD_OK;
}); }

extern "C" void opd_track_destroy(opd_track* t) { (void)api_call("opd_track_destroy", [&]() -> int {
    if (!t) return OPD_OK;
    (void)hipSetDevice(t->device);
    if (t->stream) { (void)hipStreamSynchronize(t->stream); (void)hipStreamDestroy(t->stream); }
    if (t->ev_commit) (void)hipEventDestroy(t->ev_commit);
    if (t->d_state) (void)hipFree(t->d_state);
    t->io.release();
    t->seq.release();
    t->desc.release();
    delete t;
    ++g_handle_epoch;
    return OPD_OK;
}); }

extern "C" int opd_track_reset(opd_track* t) { return api_call("opd_track_reset", [&]() -> int {
    if (!t) return fail(OPD_EINVAL, "opd_track_reset: null handle");
    drop_all(t);   // (a new track initialises every number of its slot: nothing on the device needs clearing)
    return OPD_OK;
}); }

extern "C" int opd_track_info(const opd_track* t, opd_track_status* info) { return api_call_unlocked("opd_track_info", [&]() -> int {
    if (!t || !info) return fail(OPD_EINVAL, "opd_track_info: null argument");
    *info = opd_track_status{t->S, t->NM, t->D, t->max_age, t->min_hits, t->device, (int32_t)t->tracks.size(), t->next_id, t->last_launches, t->last_waits};
    return OPD_OK;
}); }

extern "C" int opd_track_update(opd_track* t, const float* boxes_xywh, const float* foot_xy, const float* confidence, const float* features,
                                const uint8_t* has_feature, int feat_mem_kind, int n, int32_t* out_ids) { return api_call("opd_track_update", [&]() -> int {
    if (!t) return fail(OPD_EINVAL, "opd_track_update: null handle");
    if (n < 0) return fail(OPD_EINVAL, "opd_track_update: negative detection count");
    if (n > t->NM) return fail(OPD_EINVAL, "opd_track_update: " + std::to_string(n) + " detections, the handle was made for max_dets = " + std::to_string(t->NM));
    if (n > 0 && (!boxes_xywh || !foot_xy || !confidence || !out_ids)) return fail(OPD_EINVAL, "opd_track_update: null boxes, foot points, confidences or output");
    if (feat_mem_kind != OPD_MEM_HOST && feat_mem_kind != OPD_MEM_DEVICE) return fail(OPD_EINVAL, "opd_track_update: feat_mem_kind must be OPD_MEM_HOST or OPD_MEM_DEVICE");
    return update_body(t, boxes_xywh, foot_xy, confidence, features, has_feature, feat_mem_kind, n, out_ids);
}); }

extern "C" int opd_track_update_sequence(opd_track* t, const float* boxes_xywh, const float* foot_xy, const float* confidence, const float* features,
                                         const uint8_t* has_feature, int feat_mem_kind, const int32_t* counts, int F, int32_t* out_ids, int32_t* frames_done) { return api_call("opd_track_update_sequence", [&]() -> int {
    const std::string me = "opd_track_update_sequence: ";
    // what needs no handle first, so that a null handle is the last thing reported without one
    if (!counts || !out_ids || !frames_done) return fail(OPD_EINVAL, me + "null argument (counts or an output)");
    if (F <= 0) return fail(OPD_EINVAL, me + "a sequence has at least one frame, got F = " + std::to_string(F));
    if (feat_mem_kind != OPD_MEM_HOST && feat_mem_kind != OPD_MEM_DEVICE) return fail(OPD_EINVAL, me + "feat_mem_kind must be OPD_MEM_HOST or OPD_MEM_DEVICE");
    size_t total = 0;
    for (int f = 0; f < F; ++f) {
        if (counts[f] < 0) return fail(OPD_EINVAL, me + "negative detection count of frame " + std::to_string(f));
        total += (size_t)counts[f];
    }
    if (total > 0 && (!boxes_xywh || !foot_xy || !confidence)) return fail(OPD_EINVAL, me + "null boxes, foot points or confidences");
    if (!t) return fail(OPD_EINVAL, me + "null handle");
    for (int f = 0; f < F; ++f)
        if (counts[f] > t->NM)
            return fail(OPD_EINVAL, me + std::to_string(counts[f]) + " detections in frame " + std::to_string(f) + ", the handle was made for max_dets = " + std::to_string(t->NM));
    return update_sequence_body(t, boxes_xywh, foot_xy, confidence, features, has_feature, feat_mem_kind, counts, F, out_ids, frames_done);
}); }

extern "C" int opd_track_update_streams(opd_track* const* trackers, int C, const int32_t* camera_of, int F, const float* boxes_xywh, const float* foot_xy,
                                        const float* confidence, const float* features, const uint8_t* has_feature, int feat_mem_kind, const int32_t* counts,
                                        int32_t* out_ids, int32_t* frames_done) { return api_call("opd_track_update_streams", [&]() -> int {
    const std::string me = "opd_track_update_streams: ";
    // what needs no handle first, as in opd_track_update_sequence
    if (!trackers || !camera_of || !counts || !out_ids || !frames_done) return fail(OPD_EINVAL, me + "null argument (tracker list, camera_of, counts or an output)");
    if (C < 1 || C > TRACK_MAX_CAMERAS) return fail(OPD_EINVAL, me + "C = " + std::to_string(C) + " outside 1 .. " + std::to_string((int)TRACK_MAX_CAMERAS) + " trackers a call");
    if (F <= 0) return fail(OPD_EINVAL, me + "a call has at least one frame, got F = " + std::to_string(F));
    if (feat_mem_kind != OPD_MEM_HOST && feat_mem_kind != OPD_MEM_DEVICE) return fail(OPD_EINVAL, me + "feat_mem_kind must be OPD_MEM_HOST or OPD_MEM_DEVICE");
    size_t total = 0;
    for (int f = 0; f < F; ++f) {
        if (counts[f] < 0) return fail(OPD_EINVAL, me + "negative detection count of frame " + std::to_string(f));
        total += (size_t)counts[f];
    }
    if (total > 0 && (!boxes_xywh || !foot_xy || !confidence)) return fail(OPD_EINVAL, me + "null boxes, foot points or confidences");
    for (int f = 0; f < F; ++f)   // (before a handle is read: an entry names the handle to read)
        if (camera_of[f] < 0 || camera_of[f] >= C) return track_streams_check(trackers, C, camera_of, F, "opd_track_update_streams");
    for (int c = 0; c < C; ++c)
        if (!trackers[c]) return fail(OPD_EINVAL, me + "null handle (camera " + std::to_string(c) + ")");
    RCCHK(track_streams_check(trackers, C, camera_of, F, "opd_track_update_streams"));
    for (int c = 1; c < C; ++c)
        if (trackers[c]->device != trackers[0]->device)
            return fail(OPD_EINVAL, me + "camera 0's tracker is on device " + std::to_string(trackers[0]->device) + ", camera " + std::to_string(c) + "'s on device " +
                                        std::to_string(trackers[c]->device) + "; the trackers of a call share one device");
    for (int f = 0; f < F; ++f)
        if (counts[f] > trackers[camera_of[f]]->NM)
            return fail(OPD_EINVAL, me + std::to_string(counts[f]) + " detections in frame " + std::to_string(f) + ", the handle of camera " + std::to_string(camera_of[f]) +
                                        " was made for max_dets = " + std::to_string(trackers[camera_of[f]]->NM));
    return update_streams_body(trackers, C, camera_of, F, boxes_xywh, foot_xy, confidence, features, has_feature, feat_mem_kind, counts, out_ids, frames_done);
}); }

extern "C" int opd_track_get(opd_track* t, opd_track_rec* out, int capacity, int* count) { return api_call("opd_track_get", [&]() -> int {
    if (!t || !count) return fail(OPD_EINVAL, "opd_track_get: null argument");
    const int T = (int)t->tracks.size();
    *count = T;
    if (!out && capacity == 0) return OPD_OK;
    if (!out || capacity < T) return fail(OPD_EINVAL, "opd_track_get: " + std::to_string(T) + " tracks, room for " + std::to_string(capacity));
    if (T == 0) return OPD_OK;
    HIPCHK(hipSetDevice(t->device));
    std::vector<float> x((size_t)t->S * 4), box((size_t)t->S * 4);
    HIPCHK(hipMemcpyAsync(x.data(), t->st.x, x.size() * 4, hipMemcpyDeviceToHost, t->stream));
    HIPCHK(hipMemcpyAsync(box.data(), t->st.box, box.size() * 4, hipMemcpyDeviceToHost, t->stream));
    HIPCHK(hipStreamSynchronize(t->stream));
    for (int i = 0; i < T; ++i) {
        const TrackEntry& e = t->tracks[i];
        out[i] = opd_track_rec{e.id, e.age, e.hits, e.tsu, {}, {}};
        memcpy(out[i].x, x.data() + 4 * (size_t)e.slot, 16);
        memcpy(out[i].box, box.data() + 4 * (size_t)e.slot, 16);
    }
    return OPD_OK;
}); }

extern "C" int opd_assign(const double* cost, int rows, int cols, int32_t* row_to_col) { return api_call_unlocked("opd_assign", [&]() -> int {
    if (rows < 0 || cols < 0) return fail(OPD_EINVAL, "opd_assign: negative size");
    if (rows > 0 && !row_to_col) return fail(OPD_EINVAL, "opd_assign: null output");
    if (rows > 0 && cols > 0 && !cost) return fail(OPD_EINVAL, "opd_assign: null cost matrix");
    assign_rect(cost, rows, cols, row_to_col);
    return OPD_OK;
}); }
