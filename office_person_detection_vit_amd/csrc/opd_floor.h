// opd_floor.h — PRIVATE header of the floor-map handle (`opd_floor`, include/opd_detr.h): the model as kernels_floor.hip reads it, the
// launch parameters and the handle.  Included by kernels_floor.hip, opd_floor.cpp, opd_floor_test_api.cpp and opd_api.cpp (the fused call).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "opd_device.h"
#include "opd_records.h"

enum { FLOOR_TRI_LD = 8, FLOOR_AFF_LD = 6, FLOOR_EDGE_LD = 4 };

// The model: scalars by value, tables in ONE device allocation (read-only after creation, shared by every record and every stream)
struct FloorModel {
    int32_t method, n_points, n_triangles, n_zones, n_edges, has_distortion, allow_overlap;
    double H[9];
    double width, height, scale_x, scale_y;
    double fx, fy, cx, cy, ifx, ify;       // ifx = 1 / fx, as OpenCV normalises
    double k1, k2, p1, p2, k3;
    double ta[6];                          // TPS affine part: x then y
    const double* points;                  // [n_points][2]
    const double* tri;                     // [n_triangles][8]: the inverse of [[x0 - x2, x1 - x2], [y0 - y2, y1 - y2]] row-major, (x2, y2), the centroid
    const double* affine;                  // [n_triangles][6]
    const double* tps_w;                   // [n_points][2]
    const double* edges;                   // [n_edges][4]: p1x, p1y, p2x, p2y in the reference's order, zone after zone
    const int32_t* edge_zone;              // [n_edges]
    const int32_t* zone_rank;              // [n_zones]: position of the zone when sorted by (priority or +inf, index)
};

enum { FLOOR_IN_BOXES, FLOOR_IN_POINTS, FLOOR_IN_RECORDS, FLOOR_IN_FLOOR };   // what a wave starts from
struct FloorParams {
    FloorModel m;
    int32_t mode, n;
    const float* boxes;        // FLOOR_IN_BOXES: [n][4] x, y, w, h
    const double* pts;         // FLOOR_IN_POINTS: [n][2] camera pixels.  FLOOR_IN_FLOOR: [n][2] floor pixels (zones only)
    opd::RecordView view;      // FLOOR_IN_RECORDS: the n = n_frames * stride record slots of a detect call (opd_records.h); of those that count, the ones
                               // with a valid key and (unless any_label) labelled `label`: the float32 box, then the foot point of FLOOR_IN_BOXES
    int32_t label, any_label;
    opd_floor_rec* out;        // [n]; FLOOR_IN_RECORDS: row frame * stride + record_key
    uint64_t* masks;           // FLOOR_IN_FLOOR: [n]
};

hipError_t opd_launch_floor(const FloorParams& p, hipStream_t stream);

// The host tables of a checked configuration (opd_floor.cpp): what creation uploads, and what the test hook hands back
struct FloorTables {
    std::vector<double> points, tri, affine, tps_w, edges;
    std::vector<int32_t> edge_zone, zone_rank;
};
int floor_check_config(const opd_floor_config* cfg);                       // OPD_EINVAL + message, touches no device
void floor_build_tables(const opd_floor_config& cfg, FloorTables* t);      // (of a configuration that passed the check)

struct opd_floor {
    FloorModel model{};
    int device = 0;
    hipStream_t stream = nullptr;
    uint8_t* d_model = nullptr;       // the tables
    opd::Staging io;                  // [inputs | results] on the device and its page-locked image, grown on demand
};
