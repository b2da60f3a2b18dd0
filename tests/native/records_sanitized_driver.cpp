// Stand-alone driver of csrc/opd_records.h on the CPU (tests/test_records_cpu.py builds it with g++ -fsanitize=address,undefined and compares what it
// prints with numpy): the file named by argv[1] holds int32 form (0: opd_det, 1: opd_tile_det), n_frames, stride, 0, then counts [n_frames], then
// (from the next multiple of 8 bytes) the records [n_frames][stride] as they lie in memory.  Printed, for the whole view and for every one-frame view:
//   count <frame> <record_count>
//   rec <idx> <record_label> <record_key> <the four doubles of record_box64 as 16 hex digits each>
#include <inttypes.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "opd_records.h"

using namespace opd;

static void dump(const char* tag, const RecordView& v) {
    for (int f = 0; f < v.n_frames; ++f) printf("%s count %d %d\n", tag, f, record_count(v, f));
    for (int idx = 0; idx < v.n_frames * v.stride; ++idx) {
        double box[4];
        uint64_t bits[4];
        record_box64(v, idx, box);
        memcpy(bits, box, sizeof bits);
        printf("%s rec %d %d %d %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64 "\n", tag, idx, record_label(v, idx), record_key(v, idx), bits[0], bits[1], bits[2],
               bits[3]);
    }
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* fp = fopen(argv[1], "rb");
    if (!fp) return 2;
    int32_t head[4];
    if (fread(head, 4, 4, fp) != 4 || head[1] < 1 || head[2] < 1) return 2;
    const int form = head[0], n_frames = head[1], stride = head[2];
    const size_t n = (size_t)n_frames * stride;
    std::vector<int32_t> counts((size_t)n_frames + (n_frames & 1));   // (padded to 8 bytes, as the file is)
    if (fread(counts.data(), 4, counts.size(), fp) != counts.size()) return 2;
    std::vector<opd_det> dets(form == 0 ? n : 0);
    std::vector<opd_tile_det> merged(form == 1 ? n : 0);
    const size_t got = form == 0 ? fread(dets.data(), sizeof(opd_det), n, fp) : fread(merged.data(), sizeof(opd_tile_det), n, fp);
    fclose(fp);
    if (got != n) return 2;
    const RecordView view{form == 0 ? dets.data() : nullptr, form == 1 ? merged.data() : nullptr, counts.data(), n_frames, stride};
    dump("all", view);
    for (int f = 0; f < n_frames; ++f) {
        char tag[32];
        snprintf(tag, sizeof tag, "frame%d", f);
        dump(tag, record_frame(view, f));
    }
    printf("records done\n");
    return 0;
}
