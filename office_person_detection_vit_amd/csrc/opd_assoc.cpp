// opd_assoc.cpp — see opd_assoc.h.  Indices, their order and the comparison operators follow the reference line by line: every stage
// solves the assignment over a SUB-BLOCK (remaining tracks x remaining detections, both in their current order) of one full matrix.
#include "opd_assoc.h"

#include <math.h>

#include <algorithm>
#include <limits>

namespace opd {

namespace {

// rows <= cols.  col_of [rows] out.
void solve_wide(const std::vector<double>& c, int nr, int nc, std::vector<int>& col_of) {
    const double INF = std::numeric_limits<double>::infinity();
    std::vector<double> u(nr, 0.0), v(nc, 0.0), shortest(nc);
    std::vector<int> row_of(nc, -1), path(nc), remaining(nc);
    std::vector<char> in_sr(nr), in_sc(nc);
    col_of.assign(nr, -1);
    for (int cur = 0; cur < nr; ++cur) {
        std::fill(shortest.begin(), shortest.end(), INF);
        std::fill(path.begin(), path.end(), -1);
        std::fill(in_sr.begin(), in_sr.end(), 0);
        std::fill(in_sc.begin(), in_sc.end(), 0);
        int n_rem = nc;
        for (int j = 0; j < nc; ++j) remaining[j] = nc - 1 - j;
        double min_val = 0.0;
        int i = cur, sink = -1;
        while (sink < 0) {
            in_sr[i] = 1;
            double lowest = INF;
            int index = -1;
            for (int k = 0; k < n_rem; ++k) {
                const int j = remaining[k];
                const double r = min_val + c[(size_t)i * nc + j] - u[i] - v[j];
                if (r < shortest[j]) { shortest[j] = r; path[j] = i; }
                if (shortest[j] < lowest || (shortest[j] == lowest && row_of[j] < 0)) { lowest = shortest[j]; index = k; }
            }
            if (index < 0) return;   // (cannot happen with finite costs)
            min_val = lowest;
            const int j = remaining[index];
            if (row_of[j] < 0) sink = j;
            else i = row_of[j];
            in_sc[j] = 1;
            remaining[index] = remaining[--n_rem];
        }
        u[cur] += min_val;
        for (int r = 0; r < nr; ++r)
            if (in_sr[r] && r != cur) u[r] += min_val - shortest[col_of[r]];
        for (int j = 0; j < nc; ++j)
            if (in_sc[j]) v[j] -= min_val - shortest[j];
        int j = sink;
        for (;;) {   // augment along the path back to the new row
            const int r = path[j];
            row_of[j] = r;
            std::swap(col_of[r], j);
            if (r == cur) break;
        }
    }
}

// One stage: rows `tr` x columns `dl` of `m` (row stride N); a pair is kept when its cost is < thr (inclusive: <= thr).  Matches are
// appended as (track, detection) and taken out of `dl`; `tr` becomes the tracks left over, in order.
void stage(const float* m, int N, std::vector<int>& tr, std::vector<int>& dl, double thr, bool inclusive, bool remove_dets,
           std::vector<std::pair<int, int>>& matches) {
    if (tr.empty() || dl.empty()) return;
    const int nr = (int)tr.size(), nc = (int)dl.size();
    std::vector<double> c((size_t)nr * nc);
    for (int i = 0; i < nr; ++i)
        for (int j = 0; j < nc; ++j) c[(size_t)i * nc + j] = (double)m[(size_t)tr[i] * N + dl[j]];
    std::vector<int32_t> a(nr);
    assign_rect(c.data(), nr, nc, a.data());
    std::vector<int> left;
    std::vector<char> taken(nc, 0);
    for (int i = 0; i < nr; ++i) {
        const int j = a[i];
        const double v = j >= 0 ? c[(size_t)i * nc + j] : 0.0;
        if (j >= 0 && (inclusive ? v <= thr : v < thr)) {
            matches.emplace_back(tr[i], dl[j]);
            taken[j] = 1;
        } else {
            left.push_back(tr[i]);
        }
    }
    tr.swap(left);
    if (remove_dets) {
        std::vector<int> rest;
        for (int j = 0; j < nc; ++j)
            if (!taken[j]) rest.push_back(dl[j]);
        dl.swap(rest);
    }
}

}  // namespace

void assign_rect(const double* cost, int rows, int cols, int32_t* row_to_col) {
    for (int i = 0; i < rows; ++i) row_to_col[i] = -1;
    if (rows <= 0 || cols <= 0) return;
    const bool tall = rows > cols;
    const int nr = tall ? cols : rows, nc = tall ? rows : cols;
    std::vector<double> c((size_t)nr * nc);
    for (int i = 0; i < rows; ++i)
        for (int j = 0; j < cols; ++j) {
            const double v = cost[(size_t)i * cols + j];
            c[tall ? (size_t)j * nc + i : (size_t)i * nc + j] = isfinite(v) ? v : 1e9;
        }
    std::vector<int> col_of;
    solve_wide(c, nr, nc, col_of);
    for (int i = 0; i < nr; ++i) {
        if (col_of[i] < 0) continue;
        if (tall) row_to_col[col_of[i]] = i;
        else row_to_col[i] = col_of[i];
    }
}

void associate(const float* app, const float* iou, const float* comb, int T, int N, const int32_t* hits, const float* confidence, int min_hits,
               double high_conf, AssocResult* out) {
    out->matches.clear();
    out->new_dets.clear();
    out->unmatched_tracks.clear();
    if (T <= 0) {   // no tracks: the high-confidence detections start them.  (The reference returns EVERY detection here, before it splits
                    // by confidence; low-confidence detections never start tracks in this library)
        for (int j = 0; j < N; ++j)
            if ((double)confidence[j] >= high_conf) out->new_dets.push_back(j);
        return;
    }
    if (N <= 0) {
        for (int t = 0; t < T; ++t) out->unmatched_tracks.push_back(t);
        return;
    }
    std::vector<int> high, low, confirmed, tentative;
    for (int j = 0; j < N; ++j) ((double)confidence[j] >= high_conf ? high : low).push_back(j);
    for (int t = 0; t < T; ++t) (hits[t] >= min_hits ? confirmed : tentative).push_back(t);
    std::vector<int> tracks = confirmed;
    stage(app, N, tracks, high, 0.3, true, true, out->matches);         // 1: appearance only, <= 0.3
    stage(comb, N, tracks, high, 1.0 - 0.5, false, true, out->matches);  // 2: appearance + IoU behind the distance gate
    stage(iou, N, tracks, high, 1.0 - 0.4, false, true, out->matches);   // 3: IoU only
    stage(iou, N, tracks, low, 1.0 - 0.5, false, false, out->matches);   // 4: low-confidence rescue (those detections are never removed, nor start tracks)
    stage(comb, N, tentative, high, 1.0 - 0.5, false, true, out->matches);   // tentative tracks on what is left of the high-confidence ones
    out->new_dets = high;
    out->unmatched_tracks = tracks;
    out->unmatched_tracks.insert(out->unmatched_tracks.end(), tentative.begin(), tentative.end());
}

}  // namespace opd
