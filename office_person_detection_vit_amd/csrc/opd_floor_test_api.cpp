// opd_floor_test_api.cpp — the host tables of a floor-map configuration for tests/ and tools/ (exported from libopd_hip_test.so only).
#include <string.h>

#include "opd_floor.h"

using namespace opd;

#define TAPI extern "C" __attribute__((visibility("default")))

// What opd_floor_create would upload for `cfg`, without touching a device: tri [n_triangles][8] (inverse edge matrix, last vertex,
// centroid), edges [*n_edges][4] with their zones, and every zone's rank.  Any output may be null; `edge_capacity` bounds the edge arrays.
TAPI int opd_floor_test_tables(const opd_floor_config* cfg, double* tri, double* edges, int32_t* edge_zone, int edge_capacity, int32_t* zone_rank,
                               int* n_edges) {
    RCCHK(floor_check_config(cfg));
    FloorTables t;
    floor_build_tables(*cfg, &t);
    const int E = (int)t.edge_zone.size();
    if (n_edges) *n_edges = E;
    if ((edges || edge_zone) && edge_capacity < E) return fail(OPD_EINVAL, "opd_floor_test_tables: the configuration has " + std::to_string(E) + " edges");
    if (tri && !t.tri.empty()) memcpy(tri, t.tri.data(), t.tri.size() * 8);
    if (edges && E) memcpy(edges, t.edges.data(), t.edges.size() * 8);
    if (edge_zone && E) memcpy(edge_zone, t.edge_zone.data(), (size_t)E * 4);
    if (zone_rank && !t.zone_rank.empty()) memcpy(zone_rank, t.zone_rank.data(), t.zone_rank.size() * 4);
    return OPD_OK;
}
