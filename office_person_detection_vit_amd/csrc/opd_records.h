// opd_records.h — where the records of a detect call lie behind the tile merge, and how a record becomes a box and a row: said ONCE, for the host
// (opd_api.cpp builds the view of a call) and for the device (the sink stages' kernels read through it).  Plain C++ on the host (g++ compiles it for
// tests/native/records_sanitized_driver.cpp): nothing of HIP unless the HIP compiler reads it.
//
// The records have one of two forms:
//   opd_det       what the post-process kernel leaves: float32 corners x1 y1 x2 y2; a record's outputs go to the row its `query_index` names
//   opd_tile_det  what the seam merge of a tiled call leaves: float64 x y w h in frame pixels; two tiles of a frame use the same query numbers, so a
//                 record's outputs go to the row of its POSITION
// Both become the float64 box x, y, w, h that Python holds as Detection.bbox: (x1, y1, x2 - x1, y2 - y1) in Python floats, or the four doubles as they
// are.  Every value a stage uses derives from that ONE box: each of the four rounded to float32 once (np.asarray(d.bbox, np.float32): the width is not
// re-derived from rounded corners), and a foot point (x + w / 2, y + h), which the floor stage takes from the rounded floats and the track stage from
// the unrounded doubles, rounding where it stores.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/opd_detr.h"

#if defined(__HIP__) || defined(__HIPCC__)
#define OPD_REC_HD __host__ __device__
#else
#define OPD_REC_HD
#endif

namespace opd {

// [n_frames][stride] records on the device and their counts.  Exactly one of `records` and `merged` is non-null; which one is uniform over a launch.
struct RecordView {
    const opd_det* records;
    const opd_tile_det* merged;
    const int32_t* counts;    // [n_frames]
    int32_t n_frames, stride;   // slots per frame: queries, or (a tiled call) n_tiles x queries
};

// frame f alone (the trackers take one frame each); record and row indices are then relative to it
OPD_REC_HD inline RecordView record_frame(const RecordView& v, int f) {
    const size_t at = (size_t)f * v.stride;
    return RecordView{v.records ? v.records + at : nullptr, v.merged ? v.merged + at : nullptr, v.counts + f, 1, v.stride};
}

// records of frame f that count, whatever lies in counts[f]
OPD_REC_HD inline int record_count(const RecordView& v, int frame) {
    const int n = v.counts[frame];
    return n < 0 ? 0 : (n > v.stride ? v.stride : n);
}

// idx = frame * stride + position, in every accessor below
OPD_REC_HD inline int record_label(const RecordView& v, int idx) { return v.merged ? v.merged[idx].label : v.records[idx].label; }

// The row of its frame a record's outputs go by.  A post-process record's query_index is whatever lies there: test (unsigned)key < stride before use.
OPD_REC_HD inline int record_key(const RecordView& v, int idx) { return v.merged ? idx % v.stride : v.records[idx].query_index; }

// Differences of two doubles and copies: no multiply-add, so the result does not depend on -ffp-contract
OPD_REC_HD inline void record_box64(const opd_det& r, double box[4]) {
    box[0] = (double)r.x1; box[1] = (double)r.y1;
    box[2] = (double)r.x2 - (double)r.x1; box[3] = (double)r.y2 - (double)r.y1;
}
OPD_REC_HD inline void record_box64(const opd_tile_det& r, double box[4]) { box[0] = r.x; box[1] = r.y; box[2] = r.w; box[3] = r.h; }
OPD_REC_HD inline void record_box64(const RecordView& v, int idx, double box[4]) {
    if (v.merged) record_box64(v.merged[idx], box);
    else record_box64(v.records[idx], box);
}

}  // namespace opd
