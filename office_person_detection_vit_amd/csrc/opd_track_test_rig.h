// opd_track_test_rig.h — test-only: the inputs of the association kernel as the hooks of opd_track_test_api.cpp (one tracker a launch) and of
// opd_track_streams_test_api.cpp (a camera per blockIdx.y) set them up.
#pragma once
#include <algorithm>
#include <vector>

#include "opd_track.h"

namespace opd {

// The inputs of track_assoc_kernel for the hooks: a table of T tracks (row i in slot i, hits[i] matches so far) and n_free free slots, the
// matrices and confidences of the caller on the device, room for every output
struct AssocRig {
    DevMem tmp;
    TrackAssocParams p{};
    std::vector<int32_t> hdr, tab, stack;
    int S = 1;
    bool make(const float* app, const float* iou, const float* comb, int T, int N, const int32_t* hits, const float* conf, int min_hits, double high_conf, int n_free) {
        S = std::max(1, T + n_free);
        hdr.assign(TRACK_HDR_INTS, 0); tab.assign((size_t)S * TRACK_ENTRY_INTS, 0); stack.assign(S, 0);
        hdr[TRACK_HDR_T] = T; hdr[TRACK_HDR_NEXT_ID] = T + 1; hdr[TRACK_HDR_N_FREE] = n_free;
        for (int i = 0; i < T; ++i) { int32_t* e = &tab[(size_t)i * TRACK_ENTRY_INTS]; e[0] = i; e[1] = i + 1; e[2] = 1; e[3] = hits[i]; e[4] = 0; }
        for (int k = 0; k < n_free; ++k) stack[k] = T + n_free - 1 - k;   // (slot T is handed out first)
        const size_t cells = std::max<size_t>(1, (size_t)T * N);
        p.hdr = tmp.up(hdr.data(), hdr.size());
        p.tab = tmp.up(tab.data(), tab.size());
        p.free_slots = tmp.up(stack.data(), stack.size());
        p.app = tmp.up(T > 0 && N > 0 ? app : nullptr, cells);
        p.iou = tmp.up(T > 0 && N > 0 ? iou : nullptr, cells);
        p.comb = tmp.up(T > 0 && N > 0 ? comb : nullptr, cells);
        p.conf = tmp.up(N > 0 ? conf : nullptr, (size_t)std::max(1, N));
        p.conf_stride = 1;
        p.n = N;
        p.ops = tmp.alloc<int32_t>((size_t)S * 4);
        p.ids = tmp.alloc<int32_t>((size_t)std::max(1, N));
        p.unmatched = tmp.alloc<int32_t>((size_t)S + 1);
        p.S = S; p.min_hits = min_hits; p.max_age = 1 << 30; p.frame = 0;
        p.high_conf = high_conf;
        return tmp.ok;
    }
};

}  // namespace opd
