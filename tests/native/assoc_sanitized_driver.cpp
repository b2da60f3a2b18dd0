// assoc_sanitized_driver.cpp — csrc/opd_assoc.cpp under AddressSanitizer + UBSan (tests/test_assoc_sanitized_cpu.py builds and runs this
// with g++ on the CPU; nothing here touches a device).  The solver on empty, single-row, single-column and rectangular matrices, checked
// against exhaustive search; the five-stage association over seeded matrices with every subset (confirmed, tentative, high-confidence,
// low-confidence, all tracks, all detections) empty in turn, checked for the invariants of a matching.
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <numeric>
#include <set>
#include <vector>

#include "opd_assoc.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static double uniform() {   // xorshift64*: seeded, the same on every machine
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return (double)((rng_state * 0x2545F4914F6CDD1Dull) >> 11) / 9007199254740992.0;
}

static int failures = 0;
#define CHECK(cond, ...)                      \
    do {                                      \
        if (!(cond)) {                        \
            ++failures;                       \
            printf("FAILED %s: ", #cond);     \
            printf(__VA_ARGS__);              \
            printf("\n");                     \
        }                                     \
    } while (0)

static double best_by_search(const std::vector<double>& c, int rows, int cols) {
    const bool tall = rows > cols;
    const int nr = tall ? cols : rows, nc = tall ? rows : cols;
    std::vector<int> perm(nc);
    std::iota(perm.begin(), perm.end(), 0);
    double best = INFINITY;
    do {
        double s = 0.0;
        for (int i = 0; i < nr; ++i) s += tall ? c[(size_t)perm[i] * cols + i] : c[(size_t)i * cols + perm[i]];
        best = std::min(best, s);
    } while (std::next_permutation(perm.begin(), perm.end()));
    return best;
}

static void solver_case(int rows, int cols, bool gated) {
    std::vector<double> c((size_t)rows * cols);
    for (double& v : c) v = gated && uniform() < 0.5 ? 1.0 : uniform() * (gated ? 1.0 : 2.0);
    std::vector<int32_t> a(rows > 0 ? rows : 1, -7);
    opd::assign_rect(c.data(), rows, cols, a.data());
    std::set<int> used;
    double total = 0.0;
    int pairs = 0;
    for (int i = 0; i < rows; ++i) {
        CHECK(a[i] >= -1 && a[i] < cols, "%d x %d: row %d -> %d", rows, cols, i, a[i]);
        if (a[i] < 0) continue;
        CHECK(used.insert(a[i]).second, "%d x %d: column %d twice", rows, cols, a[i]);
        total += c[(size_t)i * cols + a[i]];
        ++pairs;
    }
    CHECK(pairs == std::min(rows, cols), "%d x %d: %d pairs", rows, cols, pairs);
    if (rows > 0 && cols > 0 && std::max(rows, cols) <= 7) {
        const double best = best_by_search(c, rows, cols);
        CHECK(fabs(total - best) <= 1e-12, "%d x %d: total %.17g, optimum %.17g", rows, cols, total, best);
    }
}

// `empty`: 0 none, 1 no confirmed track, 2 no tentative track, 3 no high-confidence detection, 4 no low-confidence one, 5 no track, 6 no detection
static void assoc_case(int T, int N, int empty, bool features) {
    if (empty == 5) T = 0;
    if (empty == 6) N = 0;
    std::vector<float> app((size_t)T * N + 1), iou((size_t)T * N + 1), comb((size_t)T * N + 1), conf(N + 1);
    std::vector<int32_t> hits(T + 1);
    for (int t = 0; t < T; ++t) hits[t] = empty == 1 ? 1 : (empty == 2 ? 5 : (uniform() < 0.5 ? 1 : 4));
    for (int j = 0; j < N; ++j) conf[j] = (float)(empty == 3 ? 0.3 : (empty == 4 ? 0.8 : (uniform() < 0.5 ? 0.3 : 0.8)));
    for (size_t k = 0; k < (size_t)T * N; ++k) {
        app[k] = features ? (float)(uniform() < 0.3 ? uniform() * 0.3 : 0.4 + uniform()) : 1.0f;
        iou[k] = (float)(uniform() < 0.3 ? uniform() * 0.5 : 0.7 + 0.3 * uniform());
        comb[k] = uniform() < 0.2 ? 1.0f : (float)(0.7 * app[k] + 0.3 * iou[k]);
    }
    opd::AssocResult r;
    opd::associate(app.data(), iou.data(), comb.data(), T, N, hits.data(), conf.data(), 3, 0.5, &r);
    std::set<int> tr, de;
    for (const auto& m : r.matches) {
        CHECK(m.first >= 0 && m.first < T && m.second >= 0 && m.second < N, "match (%d, %d) of %d x %d", m.first, m.second, T, N);
        CHECK(tr.insert(m.first).second, "track %d matched twice", m.first);
        CHECK(de.insert(m.second).second, "detection %d matched twice", m.second);
        if (m.first < T && hits[m.first] < 3 && m.second < N) CHECK(conf[m.second] >= 0.5f, "a tentative track took a low-confidence detection");
    }
    for (int j : r.new_dets) {
        CHECK(j >= 0 && j < N && conf[j] >= 0.5f, "detection %d starts a track", j);
        CHECK(de.insert(j).second, "detection %d is matched and new", j);
    }
    CHECK(std::is_sorted(r.new_dets.begin(), r.new_dets.end()), "new detections out of order");
    for (int t : r.unmatched_tracks) CHECK(t >= 0 && t < T && tr.insert(t).second, "track %d is matched and unmatched", t);
    CHECK((int)tr.size() == T, "%d of %d tracks accounted for", (int)tr.size(), T);
    for (int j = 0; j < N; ++j)
        if (conf[j] >= 0.5f) CHECK(de.count(j) == 1, "high-confidence detection %d neither matched nor new", j);
    printf("assoc T=%d N=%d empty=%d features=%d: %zu matches, %zu new, %zu unmatched\n", T, N, empty, (int)features, r.matches.size(), r.new_dets.size(),
           r.unmatched_tracks.size());
}

int main() {
    const int shapes[][2] = {{0, 0}, {0, 5}, {5, 0}, {1, 1}, {1, 7}, {7, 1}, {5, 7}, {7, 5}, {6, 6}, {12, 16}, {16, 12}, {40, 25}};
    for (const auto& s : shapes)
        for (int rep = 0; rep < 8; ++rep) {
            solver_case(s[0], s[1], false);
            solver_case(s[0], s[1], true);
        }
    {   // costs that are not finite count as 1e9 and never hang the search
        const double c[4] = {NAN, INFINITY, 0.25, -INFINITY};
        int32_t a[2];
        opd::assign_rect(c, 2, 2, a);
        CHECK(a[0] != a[1] && a[0] >= 0 && a[1] >= 0, "non-finite costs: %d %d", a[0], a[1]);
    }
    printf("solver cases done\n");
    for (int empty = 0; empty <= 6; ++empty)
        for (int rep = 0; rep < 6; ++rep) {
            assoc_case(9, 12, empty, true);
            assoc_case(12, 5, empty, rep % 2 == 0);
            assoc_case(1, 1, empty, true);
        }
    printf("failures %d\n", failures);
    return failures ? 1 : 0;
}
