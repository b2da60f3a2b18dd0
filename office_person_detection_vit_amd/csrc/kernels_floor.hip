// kernels_floor.hip — camera pixels -> floor-map pixels, mm and zone membership for one record per wave (`TransformPhase.execute`,
// src/pipeline/phases/transform.py:257-330: transform_batch of the configured transformer, then ZoneClassifier.classify).  float64, and
// no fused multiply-adds (the file is compiled with -ffp-contract=off, and says so itself below): the device evaluates the operations of
// tests/floor_common.py one for one, so the only differences are the device's log and sqrt.
//
//   floor_kernel   64 threads = one wave = one record.  The point itself (foot point, undistortion, homography, the affine map) is scalar
//                  work every lane repeats on the same bits; the lanes split what is long:
//                    piecewise affine  chunks of 64 triangles in ascending order, one barycentric test per lane, ballot + first set lane:
//                                      the lowest-index triangle that holds the point, as a sequential search finds it.  None: every
//                                      lane keeps the nearest centroid of its strided triangles, then the minimum over (distance, index)
//                                      pairs across the wave: the lowest index among equal distances, as numpy's argmin.
//                    thin-plate spline lane l adds w_i U(r_i) for i = l, l + 64, ... in ascending order, then an xor butterfly adds the
//                                      64 partial sums: one fixed order that depends on the number of control points alone.
//                    zones             lane l takes edges l, l + 64, ... of all polygons; an edge the ray crosses flips its zone's bit in
//                                      the lane's 64-bit mask, and an xor over the wave gives every zone's parity at once.
//                  The model is read at addresses that do not depend on the record; lane 0 stores the 48-byte result.  Nothing is
//                  accumulated in memory, so a record's result depends on its box and the model only.
#include <float.h>
#include <hip/hip_runtime.h>
#include <limits.h>

#include "opd_floor.h"
#include "opd_kprims.h"

#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ unsigned long long wave_xor(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v ^= __shfl_xor(v, o);
    return v;
}

// OpenCV's undistortPoints with P = K: five fixed-point iterations of the k1 k2 p1 p2 k3 model on the normalised point
__device__ __forceinline__ void undistort(const FloorModel& m, double* px, double* py) {
    double x = (*px - m.cx) * m.ifx, y = (*py - m.cy) * m.ify;
    const double x0 = x, y0 = y;
    for (int j = 0; j < 5; ++j) {
        const double r2 = x * x + y * y;
        const double icdist = 1.0 / (1.0 + ((m.k3 * r2 + m.k2) * r2 + m.k1) * r2);
        if (icdist < 0.0) { x = x0; y = y0; break; }
        const double dx = 2.0 * m.p1 * x * y + m.p2 * (r2 + 2.0 * x * x);
        const double dy = m.p1 * (r2 + 2.0 * y * y) + 2.0 * m.p2 * x * y;
        x = (x0 - dx) * icdist;
        y = (y0 - dy) * icdist;
    }
    *px = x * m.fx + m.cx;
    *py = y * m.fy + m.cy;
}

__global__ __launch_bounds__(64) void floor_kernel(const FloorParams p) {
    const FloorModel& m = p.m;
    const int idx = blockIdx.x, lane = threadIdx.x;
    int row = idx;
    double x = 0.0, y = 0.0;
    if (p.mode == FLOOR_IN_BOXES) {
        const float* b = p.boxes + 4 * (size_t)idx;
        x = (double)b[0] + (double)b[2] / 2.0;
        y = (double)b[1] + (double)b[3];
    } else if (p.mode == FLOOR_IN_RECORDS) {
        const int S = p.view.stride, f = idx / S, i = idx - f * S;
        if (i >= opd::record_count(p.view, f)) return;   // (uniform over the wave, as every exit here)
        const int key = opd::record_key(p.view, idx);
        if ((!p.any_label && opd::record_label(p.view, idx) != p.label) || (unsigned)key >= (unsigned)S) return;
        double box[4];   // np.asarray(d.bbox, np.float32) of HipFloorMapper.transform_records, then the boxes mode above
        opd::record_box64(p.view, idx, box);
        x = (double)(float)box[0] + (double)(float)box[2] / 2.0;
        y = (double)(float)box[1] + (double)(float)box[3];
        row = f * S + key;
    } else {
        x = p.pts[2 * (size_t)idx];
        y = p.pts[2 * (size_t)idx + 1];
    }
    double fx = x, fy = y;
    int tri = -1;
    unsigned flags = OPD_FLOOR_VALID;
    if (p.mode != FLOOR_IN_FLOOR) {
        if (m.has_distortion && m.method != OPD_FLOOR_HOMOGRAPHY) undistort(m, &x, &y);
        if (m.method == OPD_FLOOR_HOMOGRAPHY) {
            const double u = (m.H[0] * x + m.H[1] * y) + m.H[2], v = (m.H[3] * x + m.H[4] * y) + m.H[5], w = (m.H[6] * x + m.H[7] * y) + m.H[8];
            fx = u / w;
            fy = v / w;
        } else if (m.method == OPD_FLOOR_PWA) {
            const int T = m.n_triangles;
            for (int base = 0; base < T && tri < 0; base += 64) {
                const int t = base + lane;
                bool ok = false;
                if (t < T) {
                    const double* q = m.tri + (size_t)t * FLOOR_TRI_LD;
                    const double dx = x - q[4], dy = y - q[5];
                    const double b0 = q[0] * dx + q[1] * dy, b1 = q[2] * dx + q[3] * dy, b2 = (1.0 - b0) - b1;
                    ok = b0 >= -1e-12 && b1 >= -1e-12 && b2 >= -1e-12;
                }
                const unsigned long long hit = __ballot(ok);
                if (hit) tri = base + __ffsll((long long)hit) - 1;
            }
            if (tri < 0) {
                flags |= OPD_FLOOR_EXTRAPOLATED;
                double bd = DBL_MAX;
                int bi = INT_MAX;
                for (int t = lane; t < T; t += 64) {
                    const double* q = m.tri + (size_t)t * FLOOR_TRI_LD;
                    const double dx = q[6] - x, dy = q[7] - y;
                    const double d = sqrt(dx * dx + dy * dy);
                    if (d < bd) { bd = d; bi = t; }
                }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    const double od = __shfl_xor(bd, o);
                    const int oi = __shfl_xor(bi, o);
                    if (od < bd || (od == bd && oi < bi)) { bd = od; bi = oi; }
                }
                tri = bi < T ? bi : 0;
            }
            const double* a = m.affine + (size_t)tri * FLOOR_AFF_LD;
            fx = (a[0] * x + a[1] * y) + a[2];
            fy = (a[3] * x + a[4] * y) + a[5];
        } else {
            double sx = 0.0, sy = 0.0;
            for (int i = lane; i < m.n_points; i += 64) {
                const double dx = x - m.points[2 * i], dy = y - m.points[2 * i + 1];
                const double r = sqrt(dx * dx + dy * dy);
                const double u = r > 0.0 ? r * r * log(r) : 0.0;
                sx += m.tps_w[2 * i] * u;
                sy += m.tps_w[2 * i + 1] * u;
            }
            sx = wave_sum(sx);
            sy = wave_sum(sy);
            fx = ((m.ta[0] + m.ta[1] * x) + m.ta[2] * y) + sx;
            fy = ((m.ta[3] + m.ta[4] * x) + m.ta[5] * y) + sy;
        }
        if (0.0 <= fx && fx < m.width && 0.0 <= fy && fy < m.height) flags |= OPD_FLOOR_WITHIN;
    }
    // ZoneClassifier._point_in_polygon, edge by edge: its comparisons, its one division
    unsigned long long mask = 0ull;
    for (int e = lane; e < m.n_edges; e += 64) {
        const double* q = m.edges + (size_t)e * FLOOR_EDGE_LD;
        const double p1x = q[0], p1y = q[1], p2x = q[2], p2y = q[3];
        if (fy > (p2y < p1y ? p2y : p1y) && fy <= (p2y > p1y ? p2y : p1y) && fx <= (p2x > p1x ? p2x : p1x)) {
            const double xinters = (fy - p1y) * (p2x - p1x) / (p2y - p1y) + p1x;
            if (p1x == p2x || fx <= xinters) mask ^= 1ull << m.edge_zone[e];
        }
    }
    mask = wave_xor(mask);
    if (!m.allow_overlap && mask) {   // the zone with the smallest (priority or +inf, position): its rank was sorted out on the host
        int key = (lane < m.n_zones && ((mask >> lane) & 1ull)) ? m.zone_rank[lane] : INT_MAX;
        int best = key;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) best = min(best, __shfl_xor(best, o));
        const unsigned long long who = __ballot(key == best);
        mask = 1ull << (__ffsll((long long)who) - 1);
    }
    if (lane != 0) return;
    if (p.mode == FLOOR_IN_FLOOR) {
        p.masks[idx] = mask;
        return;
    }
    opd_floor_rec r;
    r.px[0] = fx; r.px[1] = fy;
    r.mm[0] = fx * m.scale_x; r.mm[1] = fy * m.scale_y;
    r.zone_mask = mask;
    r.triangle = tri;
    r.flags = flags;
    p.out[row] = r;
}

}  // namespace

hipError_t opd_launch_floor(const FloorParams& p, hipStream_t stream) {
    if (p.n <= 0) return hipSuccess;
    OPD_LAUNCH(floor_kernel, dim3(p.n), dim3(64), 0, stream, p);
    return hipGetLastError();
}
