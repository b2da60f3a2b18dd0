// opd_floor.cpp — the floor-map handle of include/opd_detr.h (opd_floor_*): a configuration is checked and turned into the tables
// kernels_floor.hip reads (inverse edge matrices and centroids of the triangles, polygon edges in the reference's order, the zones'
// ranks) on the host, uploaded once, and never changed.  A call stages its inputs in page-locked memory, enqueues one upload, the
// one-wave-per-record launch and one download on the handle's stream, and waits once.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <numeric>
#include <string>

#include "opd_floor.h"
#include "opd_kernels.h"

#pragma clang fp contract(off)

using namespace opd;

namespace {

const size_t IN_BYTES = 16;   // per record: four float32 or two float64

// upload `in_bytes` of inputs (host; null: the kernel reads the caller's device memory), launch, download `out_bytes` per record, wait
int run(opd_floor* f, FloorParams& p, const void* host_in, size_t out_each, void* host_out) {
    const int n = p.n;
    HIPCHK(hipSetDevice(f->device));
    const size_t each = IN_BYTES + sizeof(opd_floor_rec), bytes = align_up((size_t)n, 256) * each;
    RCCHK(f->io.reserve("opd_floor", bytes, bytes, f->stream));   // whole blocks of 256 records: [inputs of 16 bytes | results]
    const size_t cap = f->io.dev_cap / each;
    uint8_t* d_out = f->io.dev + cap * IN_BYTES;
    uint8_t* h_out = f->io.host + cap * IN_BYTES;
    if (host_in) {
        memcpy(f->io.host, host_in, (size_t)n * IN_BYTES);
        HIPCHK(hipMemcpyAsync(f->io.dev, f->io.host, (size_t)n * IN_BYTES, hipMemcpyHostToDevice, f->stream));
        p.boxes = reinterpret_cast<const float*>(f->io.dev);
        p.pts = reinterpret_cast<const double*>(f->io.dev);
    }
    p.m = f->model;
    p.out = reinterpret_cast<opd_floor_rec*>(d_out);
    p.masks = reinterpret_cast<uint64_t*>(d_out);
    HIPCHK(opd_launch_floor(p, f->stream));
    HIPCHK(hipMemcpyAsync(h_out, d_out, (size_t)n * out_each, hipMemcpyDeviceToHost, f->stream));
    HIPCHK(hipStreamSynchronize(f->stream));
    memcpy(host_out, h_out, (size_t)n * out_each);
    return OPD_OK;
}

int check_call(const opd_floor* f, const char* who, const void* in, int n, const void* out) {
    const std::string me(who);
    if (!f) return fail(OPD_EINVAL, me + ": null handle");
    if (n < 0 || n > (1 << 24)) return fail(OPD_EINVAL, me + ": record count " + std::to_string(n) + " outside 0 .. 16777216");
    if (n > 0 && (!in || !out)) return fail(OPD_EINVAL, me + ": null input or output buffer");
    return OPD_OK;
}

}  // namespace

int floor_check_config(const opd_floor_config* cfg) {
    const std::string me = "opd_floor_create: ";
    if (!cfg) return fail(OPD_EINVAL, me + "null configuration");
    const opd_floor_config& c = *cfg;
    if (c.method != OPD_FLOOR_HOMOGRAPHY && c.method != OPD_FLOOR_PWA && c.method != OPD_FLOOR_TPS)
        return fail(OPD_EINVAL, me + "unknown method " + std::to_string(c.method));
    if (c.width_px < 1 || c.height_px < 1) return fail(OPD_EINVAL, me + "the floor map must be at least 1 x 1 pixels");
    if (c.method == OPD_FLOOR_HOMOGRAPHY) {
        const double* h = c.H;
        const double det = h[0] * (h[4] * h[8] - h[5] * h[7]) - h[1] * (h[3] * h[8] - h[5] * h[6]) + h[2] * (h[3] * h[7] - h[4] * h[6]);
        if (!(fabs(det) >= 1e-10)) return fail(OPD_EINVAL, me + "the homography is singular (|det| < 1e-10)");
    } else {
        if (c.n_points < 3) return fail(OPD_EINVAL, me + "at least 3 control points are needed, " + std::to_string(c.n_points) + " given");
        if (c.n_points > OPD_FLOOR_MAX_POINTS) return fail(OPD_EINVAL, me + std::to_string(c.n_points) + " control points, the limit is 256");
        if (!c.points) return fail(OPD_EINVAL, me + "null control points");
        if (c.has_distortion && (c.intrinsics[0] == 0.0 || c.intrinsics[1] == 0.0 || !(c.intrinsics[0] == c.intrinsics[0]) || !(c.intrinsics[1] == c.intrinsics[1])))
            return fail(OPD_EINVAL, me + "a distortion model needs non-zero focal lengths");
    }
    if (c.method == OPD_FLOOR_PWA) {
        if (c.n_triangles < 1) return fail(OPD_EINVAL, me + "piecewise affine needs at least one triangle");
        if (c.n_triangles > OPD_FLOOR_MAX_TRIANGLES) return fail(OPD_EINVAL, me + std::to_string(c.n_triangles) + " triangles, the limit is 512");
        if (!c.triangles || !c.affine) return fail(OPD_EINVAL, me + "null triangles or affine matrices");
        for (int i = 0; i < 3 * c.n_triangles; ++i)
            if (c.triangles[i] < 0 || c.triangles[i] >= c.n_points)
                return fail(OPD_EINVAL, me + "triangle " + std::to_string(i / 3) + " names point " + std::to_string(c.triangles[i]) + " of " + std::to_string(c.n_points));
    }
    if (c.method == OPD_FLOOR_TPS && !c.tps_weights) return fail(OPD_EINVAL, me + "null spline weights");
    if (c.n_zones < 0 || c.n_zones > OPD_FLOOR_MAX_ZONES) return fail(OPD_EINVAL, me + std::to_string(c.n_zones) + " zones, the limit is 64");
    if (c.n_zones > 0) {
        if (!c.zone_vertices || !c.zone_offsets) return fail(OPD_EINVAL, me + "null zone vertices or offsets");
        if (c.zone_offsets[0] != 0) return fail(OPD_EINVAL, me + "zone_offsets must start at 0");
        for (int z = 0; z < c.n_zones; ++z) {
            const long long nv = (long long)c.zone_offsets[z + 1] - c.zone_offsets[z];
            if (nv < 3) return fail(OPD_EINVAL, me + "the polygon of zone " + std::to_string(z) + " has " + std::to_string(nv) + " vertices, at least 3 are needed");
            if (nv > OPD_FLOOR_MAX_VERTICES) return fail(OPD_EINVAL, me + "the polygon of zone " + std::to_string(z) + " has " + std::to_string(nv) + " vertices, the limit is 64");
        }
    }
    return OPD_OK;
}

void floor_build_tables(const opd_floor_config& c, FloorTables* t) {
    *t = FloorTables();
    if (c.method != OPD_FLOOR_HOMOGRAPHY) t->points.assign(c.points, c.points + 2 * (size_t)c.n_points);
    if (c.method == OPD_FLOOR_PWA) {
        t->affine.assign(c.affine, c.affine + FLOOR_AFF_LD * (size_t)c.n_triangles);
        t->tri.resize(FLOOR_TRI_LD * (size_t)c.n_triangles);
        for (int i = 0; i < c.n_triangles; ++i) {
            const double* v0 = c.points + 2 * (size_t)c.triangles[3 * i];
            const double* v1 = c.points + 2 * (size_t)c.triangles[3 * i + 1];
            const double* v2 = c.points + 2 * (size_t)c.triangles[3 * i + 2];
            // barycentric coordinates in scipy's Delaunay.transform convention: (b0, b1) = inv([[x0 - x2, x1 - x2], [y0 - y2, y1 - y2]]) (p - v2)
            const double a = v0[0] - v2[0], b = v1[0] - v2[0], cc = v0[1] - v2[1], d = v1[1] - v2[1];
            const double det = a * d - b * cc;
            double* q = t->tri.data() + FLOOR_TRI_LD * (size_t)i;
            q[0] = d / det; q[1] = -b / det; q[2] = -cc / det; q[3] = a / det;
            q[4] = v2[0]; q[5] = v2[1];
            q[6] = ((v0[0] + v1[0]) + v2[0]) / 3.0;   // numpy's mean over the three vertices
            q[7] = ((v0[1] + v1[1]) + v2[1]) / 3.0;
        }
    }
    if (c.method == OPD_FLOOR_TPS) t->tps_w.assign(c.tps_weights, c.tps_weights + 2 * (size_t)c.n_points);
    for (int z = 0; z < c.n_zones; ++z) {   // edge i of a polygon: vertex i -> vertex (i + 1) % n, the order of the reference's loop
        const int o = c.zone_offsets[z], nv = c.zone_offsets[z + 1] - o;
        for (int i = 0; i < nv; ++i) {
            const double* p1 = c.zone_vertices + 2 * (size_t)(o + i);
            const double* p2 = c.zone_vertices + 2 * (size_t)(o + (i + 1) % nv);
            t->edges.insert(t->edges.end(), {p1[0], p1[1], p2[0], p2[1]});
            t->edge_zone.push_back(z);
        }
    }
    std::vector<int> order(c.n_zones);
    std::iota(order.begin(), order.end(), 0);
    auto prio = [&](int z) { return (c.zone_priority && c.zone_priority[z] == c.zone_priority[z]) ? c.zone_priority[z] : (double)INFINITY; };
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return prio(a) < prio(b); });
    t->zone_rank.resize(c.n_zones);
    for (int k = 0; k < c.n_zones; ++k) t->zone_rank[order[k]] = k;
}

extern "C" int opd_floor_create(const opd_floor_config* cfg, int device_ordinal, opd_floor** out) { return api_call("opd_floor_create", [&]() -> int {
    if (!out) return fail(OPD_EINVAL, "opd_floor_create: null argument");
    *out = nullptr;
    RCCHK(floor_check_config(cfg));
    const opd_floor_config& c = *cfg;
    FloorTables t;
    floor_build_tables(c, &t);
    RCCHK(use_device("opd_floor_create", device_ordinal));
    std::unique_ptr<opd_floor, decltype(&opd_floor_destroy)> f(new opd_floor(), opd_floor_destroy);   // a failure below releases whatever was already made
    f->device = device_ordinal;
    FloorModel& m = f->model;
    m.method = c.method;
    m.n_points = c.method == OPD_FLOOR_HOMOGRAPHY ? 0 : c.n_points;
    m.n_triangles = c.method == OPD_FLOOR_PWA ? c.n_triangles : 0;
    m.n_zones = c.n_zones;
    m.n_edges = (int)t.edge_zone.size();
    m.has_distortion = c.has_distortion != 0 && c.method != OPD_FLOOR_HOMOGRAPHY;
    m.allow_overlap = c.allow_overlap != 0;
    memcpy(m.H, c.H, sizeof m.H);
    m.width = (double)c.width_px; m.height = (double)c.height_px;
    m.scale_x = c.scale_x_mm_per_px; m.scale_y = c.scale_y_mm_per_px;
    m.fx = c.intrinsics[0]; m.fy = c.intrinsics[1]; m.cx = c.intrinsics[2]; m.cy = c.intrinsics[3];
    m.ifx = m.has_distortion ? 1.0 / m.fx : 0.0; m.ify = m.has_distortion ? 1.0 / m.fy : 0.0;
    m.k1 = c.distortion[0]; m.k2 = c.distortion[1]; m.p1 = c.distortion[2]; m.p2 = c.distortion[3]; m.k3 = c.distortion[4];
    memcpy(m.ta, c.tps_affine, sizeof m.ta);
    // one allocation: the double tables, then the int32 ones
    size_t off = 0;
    auto place = [&](size_t bytes) { const size_t o = off; off += align_up(bytes, 256); return o; };
    const size_t o_pts = place(t.points.size() * 8), o_tri = place(t.tri.size() * 8), o_aff = place(t.affine.size() * 8), o_w = place(t.tps_w.size() * 8);
    const size_t o_edge = place(t.edges.size() * 8), o_ez = place(t.edge_zone.size() * 4), o_rank = place(t.zone_rank.size() * 4);
    std::vector<uint8_t> image(std::max<size_t>(off, 256), 0);
    auto put = [&](size_t o, const void* src, size_t bytes) { if (bytes) memcpy(image.data() + o, src, bytes); };
    put(o_pts, t.points.data(), t.points.size() * 8); put(o_tri, t.tri.data(), t.tri.size() * 8); put(o_aff, t.affine.data(), t.affine.size() * 8);
    put(o_w, t.tps_w.data(), t.tps_w.size() * 8); put(o_edge, t.edges.data(), t.edges.size() * 8);
    put(o_ez, t.edge_zone.data(), t.edge_zone.size() * 4); put(o_rank, t.zone_rank.data(), t.zone_rank.size() * 4);
    RCCHK(made("opd_floor_create", "stream creation", hipStreamCreateWithFlags(&f->stream, hipStreamNonBlocking)));
    RCCHK(made("opd_floor_create", "model allocation", hipMalloc((void**)&f->d_model, image.size())));
    RCCHK(made("opd_floor_create", "model upload", hipMemcpy(f->d_model, image.data(), image.size(), hipMemcpyHostToDevice)));
    m.points = reinterpret_cast<const double*>(f->d_model + o_pts);
    m.tri = reinterpret_cast<const double*>(f->d_model + o_tri);
    m.affine = reinterpret_cast<const double*>(f->d_model + o_aff);
    m.tps_w = reinterpret_cast<const double*>(f->d_model + o_w);
    m.edges = reinterpret_cast<const double*>(f->d_model + o_edge);
    m.edge_zone = reinterpret_cast<const int32_t*>(f->d_model + o_ez);
    m.zone_rank = reinterpret_cast<const int32_t*>(f->d_model + o_rank);
    *out = f.release();
    return OPD_OK;
}); }

extern "C" void opd_floor_destroy(opd_floor* f) { (void)api_call("opd_floor_destroy", [&]() -> int {
    if (!f) return OPD_OK;
    (void)hipSetDevice(f->device);
    if (f->stream) { (void)hipStreamSynchronize(f->stream); (void)hipStreamDestroy(f->stream); }
    if (f->d_model) (void)hipFree(f->d_model);
    f->io.release();
    delete f;
    return OPD_OK;
}); }

extern "C" int opd_floor_info(const opd_floor* f, opd_floor_model_info* info) { return api_call_unlocked("opd_floor_info", [&]() -> int {
    if (!f || !info) return fail(OPD_EINVAL, "opd_floor_info: null argument");
    const FloorModel& m = f->model;
    *info = opd_floor_model_info{m.method, m.n_points, m.n_triangles, m.n_zones, m.n_edges, m.has_distortion, m.allow_overlap, f->device};
    return OPD_OK;
}); }

extern "C" int opd_floor_transform(opd_floor* f, const float* boxes_xywh, int n, int mem_kind, opd_floor_rec* out) { return api_call("opd_floor_transform", [&]() -> int {
    RCCHK(check_call(f, "opd_floor_transform", boxes_xywh, n, out));
    if (mem_kind != OPD_MEM_HOST && mem_kind != OPD_MEM_DEVICE) return fail(OPD_EINVAL, "opd_floor_transform: mem_kind must be OPD_MEM_HOST or OPD_MEM_DEVICE");
    if (n == 0) return OPD_OK;
    FloorParams p{};
    p.mode = FLOOR_IN_BOXES; p.n = n;
    if (mem_kind == OPD_MEM_DEVICE) {
        HIPCHK(hipSetDevice(f->device));
        if (!device_accessible(boxes_xywh)) return fail(OPD_EINVAL, "opd_floor_transform: OPD_MEM_DEVICE, but the boxes are not device-accessible memory");
        p.boxes = boxes_xywh;
    }
    return run(f, p, mem_kind == OPD_MEM_HOST ? boxes_xywh : nullptr, sizeof(opd_floor_rec), out);
}); }

extern "C" int opd_floor_transform_points(opd_floor* f, const double* pts_xy, int n, opd_floor_rec* out) { return api_call("opd_floor_transform_points", [&]() -> int {
    RCCHK(check_call(f, "opd_floor_transform_points", pts_xy, n, out));
    if (n == 0) return OPD_OK;
    FloorParams p{};
    p.mode = FLOOR_IN_POINTS; p.n = n;
    return run(f, p, pts_xy, sizeof(opd_floor_rec), out);
}); }

extern "C" int opd_floor_classify(opd_floor* f, const double* floor_xy, int n, uint64_t* masks) { return api_call("opd_floor_classify", [&]() -> int {
    RCCHK(check_call(f, "opd_floor_classify", floor_xy, n, masks));
    if (n == 0) return OPD_OK;
    FloorParams p{};
    p.mode = FLOOR_IN_FLOOR; p.n = n;
    return run(f, p, floor_xy, sizeof(uint64_t), masks);
}); }
