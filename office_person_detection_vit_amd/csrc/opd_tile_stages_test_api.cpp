// opd_tile_stages_test_api.cpp — the stage kernels of a tiled call on hand-made MERGED records, for tests/ (exported from libopd_hip_test.so only):
//   opd_test_tile_stages   color_hist_kernel / color_finish_kernel, floor_kernel and track_ingest_kernel (rows by key) on a view of merged
//                          records (opd_records.h), launched as deliver_records launches them behind tile_merge_kernel, without a
//                          model handle: host frames [n_frames][h][w][3], merged [n_frames][S] and counts [n_frames] of the caller.
#include "opd_floor.h"
#include "opd_test_util.h"
#include "opd_track.h"

using namespace opd;

// color [n_frames * S][256], floor_out [n_frames * S], boxes [n_frames][S][4], foot [n_frames][S][2], has [n_frames][S], feat [n_frames][S][256] and
// n_out [n_frames] are IN and OUT: the caller's bytes are uploaded first, so what a launch does not write comes back as it went in.  `floor` may be
// null (no floor launch).  with_rows: the ingest launches take the colour rows by position; 0: motion only (TRACK_ROWS_NONE).
TAPI int opd_test_tile_stages(int device, const uint8_t* frames, int n_frames, int h, int w, const opd_tile_det* merged, const int32_t* counts, int S, const opd_floor* floor,
                              int with_rows, float* color, opd_floor_rec* floor_out, float* boxes, float* foot, uint8_t* has, float* feat, int32_t* n_out) {
    ApiScope api_scope;
    if (!frames || !merged || !counts || !color || !boxes || !foot || !has || !feat || !n_out || (floor && !floor_out)) return fail(OPD_EINVAL, "opd_test_tile_stages: null argument");
    if (n_frames < 1 || S < 1 || S > TRACK_MAX_DETS || h < 1 || w < 1 || h > OPD_COLOR_MAX_EDGE || w > OPD_COLOR_MAX_EDGE) return fail(OPD_EINVAL, "opd_test_tile_stages: size out of range");
    for (int f = 0; f < n_frames; ++f)
        if (counts[f] < 0 || counts[f] > S) return fail(OPD_EINVAL, "opd_test_tile_stages: a count outside [0, S]");
    RCCHK(use_device("opd_test_tile_stages", device));
    if (floor && floor->device != device) return fail(OPD_EINVAL, "opd_test_tile_stages: the floor map is on another device");
    const size_t n = (size_t)n_frames * S, D = OPD_COLOR_DIM;
    DevMem dm;
    const opd_tile_det* d_merged = dm.up(merged, n);
    const int32_t* d_counts = dm.up(counts, (size_t)n_frames);
    const RecordView view{nullptr, d_merged, d_counts, n_frames, S};
    ColorParams cp{};
    cp.view = view; cp.frames = dm.up(frames, (size_t)n_frames * h * w * 3);
    cp.acc = dm.alloc<uint32_t>(n * OPD_COLOR_ACC_WORDS); cp.out = dm.up(color, n * D);
    cp.fh = h; cp.fw = w; cp.label = 1; cp.any_label = 1; cp.n = (int)n;
    FloorParams fp{};
    if (floor) {
        fp.m = floor->model; fp.mode = FLOOR_IN_RECORDS; fp.n = (int)n;
        fp.view = view; fp.any_label = 1; fp.out = dm.up(floor_out, n);
    }
    float *d_boxes = dm.up(boxes, n * 4), *d_foot = dm.up(foot, n * 2), *d_feat = dm.up(feat, n * D);
    uint8_t* d_has = dm.up(has, n);
    int32_t* d_n = dm.up(n_out, (size_t)n_frames);
    if (!dm.ok) return fail(OPD_ENOMEM, "opd_test_tile_stages: device allocation failed");
    HIPCHK(opd_launch_color_features(cp, std::min(64, (h + 15) / 16), nullptr));
    if (floor) HIPCHK(opd_launch_floor(fp, nullptr));
    for (int f = 0; f < n_frames; ++f) {
        TrackIngestParams p{};
        p.view = record_frame(view, f); p.D = (int)D; p.frame = f;
        p.rows_kind = with_rows ? TRACK_ROWS_BY_KEY : TRACK_ROWS_NONE; p.rows = with_rows ? cp.out : nullptr;
        p.boxes = d_boxes + (size_t)f * S * 4; p.foot = d_foot + (size_t)f * S * 2; p.has = d_has + (size_t)f * S; p.feat = d_feat + (size_t)f * S * D;
        p.n_out = d_n + f;
        HIPCHK(opd_launch_track_ingest(p, nullptr));
    }
    HIPCHK(hipDeviceSynchronize());
    RCCHK(down(color, cp.out, n * D));
    if (floor) RCCHK(down(floor_out, fp.out, n));
    RCCHK(down(boxes, d_boxes, n * 4));
    RCCHK(down(foot, d_foot, n * 2));
    RCCHK(down(has, d_has, n));
    RCCHK(down(feat, d_feat, n * D));
    return down(n_out, d_n, (size_t)n_frames);
}
