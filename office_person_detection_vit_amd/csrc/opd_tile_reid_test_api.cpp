// opd_tile_reid_test_api.cpp — the Re-ID stage of a tiled call on hand-made MERGED records, for tests/ (exported from libopd_hip_test.so only):
//   opd_test_tile_reid   crop_select_kernel and crop_plan_kernel on a view of merged records (opd_records.h), the Re-ID forward of a real handle and
//                        track_ingest_kernel with rows by slot on the same view, launched as deliver_records launches them behind tile_merge_kernel
//                        (ReidFusedCall::enqueue, then one ingest per frame), without a model handle: host frames [n_frames][h][w][3], merged
//                        [n_frames][S] and counts [n_frames] of the caller; the records labelled 1 are the persons.
#include "opd_reid.h"
#include "opd_test_util.h"
#include "opd_track.h"

using namespace opd;

namespace {
struct OwnStream {
    hipStream_t s = nullptr;
    ~OwnStream() { if (s) (void)hipStreamDestroy(s); }
};
}  // namespace

// slot_map [slots], rec [slots], n_person [1], geom [slots][13] (the words opd_test_crop_plan_device returns), rows [slots][E], boxes [n_frames][S][4],
// foot [n_frames][S][2], has [n_frames][S], feat [n_frames][S][E] and n_out [n_frames] are IN and OUT (E = the model's feature_dim): the caller's bytes
// are uploaded first, and of the slot arrays only the first min(*n_person, slots) entries are copied back, so what no launch writes comes back as it went in.
TAPI int opd_test_tile_reid(int device, opd_reid* reid, const uint8_t* frames, int n_frames, int h, int w, const opd_tile_det* merged, const int32_t* counts, int S,
                            int slots, int32_t* slot_map, int32_t* rec, int32_t* n_person, int32_t* geom, float* rows, float* boxes, float* foot, uint8_t* has,
                            float* feat, int32_t* n_out) {
    ApiScope api_scope;
    if (!reid || !frames || !merged || !counts || !slot_map || !rec || !n_person || !geom || !rows || !boxes || !foot || !has || !feat || !n_out)
        return fail(OPD_EINVAL, "opd_test_tile_reid: null argument");
    if (n_frames < 1 || S < 1 || S > TRACK_MAX_DETS || h < 1 || w < 1 || (size_t)h * w > (size_t)1 << 26) return fail(OPD_EINVAL, "opd_test_tile_reid: size out of range");
    for (int f = 0; f < n_frames; ++f)
        if (counts[f] < 0 || counts[f] > S) return fail(OPD_EINVAL, "opd_test_tile_reid: a count outside [0, S]");
    RCCHK(use_device("opd_test_tile_reid", device));
    RCCHK(reid_fused_check(reid, device, slots, "opd_test_tile_reid"));
    const size_t n = (size_t)n_frames * S, E = (size_t)reid_feature_dim(reid);
    if (E > TRACK_MAX_DIM) return fail(OPD_EINVAL, "opd_test_tile_reid: feature_dim above the tracker's maximum");
    DevMem dm;
    const opd_tile_det* d_merged = dm.up(merged, n);
    const int32_t* d_counts = dm.up(counts, (size_t)n_frames);
    const uint8_t* d_frames = dm.up(frames, (size_t)n_frames * h * w * 3);
    int32_t* d_geom = dm.up(geom, (size_t)slots * 13);
    float *d_boxes = dm.up(boxes, n * 4), *d_foot = dm.up(foot, n * 2), *d_feat = dm.up(feat, n * E);
    uint8_t* d_has = dm.up(has, n);
    int32_t* d_n = dm.up(n_out, (size_t)n_frames);
    if (!dm.ok) return fail(OPD_ENOMEM, "opd_test_tile_reid: device allocation failed");
    OwnStream own;
    HIPCHK(hipStreamCreateWithFlags(&own.s, hipStreamNonBlocking));
    {
        ReidFusedCall call(reid);
        const RecordView view{nullptr, d_merged, d_counts, n_frames, S};
        RCCHK(call.enqueue(own.s, view, d_frames, h, w, 1, slots, d_geom));
        for (int f = 0; f < n_frames; ++f) {
            TrackIngestParams p{};
            p.view = record_frame(view, f); p.D = (int)E; p.frame = f;
            p.rows_kind = TRACK_ROWS_BY_SLOT; p.rows = call.dev_rows(); p.slot_map = call.dev_slot_map(); p.n_person = call.dev_n_person(); p.slots = slots;
            p.boxes = d_boxes + (size_t)f * S * 4; p.foot = d_foot + (size_t)f * S * 2; p.has = d_has + (size_t)f * S; p.feat = d_feat + (size_t)f * S * E;
            p.n_out = d_n + f;
            HIPCHK(opd_launch_track_ingest(p, own.s));
        }
        RCCHK(call.copy_back(own.s));
        HIPCHK(hipStreamSynchronize(own.s));
        call.deliver(rows, slot_map, n_person);
        const size_t filled = (size_t)std::max(0, std::min(*n_person, slots));
        RCCHK(down(rec, call.dev_rec(), filled));
        RCCHK(down(geom, (const int32_t*)d_geom, filled * 13));
    }
    RCCHK(down(boxes, (const float*)d_boxes, n * 4));
    RCCHK(down(foot, (const float*)d_foot, n * 2));
    RCCHK(down(has, (const uint8_t*)d_has, n));
    RCCHK(down(feat, (const float*)d_feat, n * E));
    return down(n_out, (const int32_t*)d_n, (size_t)n_frames);
}
