// opd_assoc.h — the host half of the tracker (no HIP, no device: compiled alone under AddressSanitizer / UBSan by
// tests/test_assoc_sanitized_cpu.py): a rectangular linear-sum-assignment solver and the reference's five-stage association
// (`Tracker._associate_detections_to_tracks`, src/tracking/tracker.py) over the three cost matrices the predict launch wrote.
#pragma once
#include <stdint.h>

#include <utility>
#include <vector>

namespace opd {

// The assignment of min(rows, cols) pairs with the smallest total cost (shortest augmenting paths, Crouse 2016: what
// scipy.optimize.linear_sum_assignment computes).  cost [rows][cols] row-major; row_to_col [rows], -1 for a row left alone.
// A cost that is not finite counts as 1e9.  Which of several optimal assignments comes out is not specified.
void assign_rect(const double* cost, int rows, int cols, int32_t* row_to_col);

struct AssocResult {
    std::vector<std::pair<int, int>> matches;   // (track, detection), stage after stage
    std::vector<int> new_dets;                  // high-confidence detections no stage matched, ascending: they start tracks
    std::vector<int> unmatched_tracks;
};

// app / iou / comb: [T][N] with row stride N.  hits [T], confidence [N].  A track is confirmed when hits >= min_hits, a detection is
// high-confidence when confidence >= high_conf.
void associate(const float* app, const float* iou, const float* comb, int T, int N, const int32_t* hits, const float* confidence, int min_hits,
               double high_conf, AssocResult* out);

}  // namespace opd
