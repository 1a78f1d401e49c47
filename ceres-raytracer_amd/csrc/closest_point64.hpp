// closest_point64.hpp -- the arithmetic of the closest-point queries on double scenes
// (ceres_closest_points_f64*), one set of functions for the host walk (render_cpu.cpp) and the device
// walk (closest_point64.hip).
//
// closest_point.hpp with float replaced by double and the float literals by double literals, nothing
// else: the same formula, region order, clamp into the triangle's own box, selection, NaN rules and
// strict prune, so its argument holds word for word (DESIGN.md "Closest-point queries on double
// scenes") -- IEEE double + - * are monotone as the float ones are, and the answer is, bit for bit, the
// minimum over ALL triangles of near64_tri()'s d2 under near64_better()'s order.  A header of its own
// so that the float kernels compile from the text they compiled from before.
// Only IEEE operations whose result does not depend on the compiler: + - * / compare and select; every
// translation unit that includes this is built with -ffp-contract=off.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define CERES_NEAR64_FN __host__ __device__ inline
#else
#define CERES_NEAR64_FN inline
#endif

namespace ceres {

struct NearBest64 {
    double d2;       // the best squared distance so far; starts at r2max
    int32_t prim;    // its ORIGINAL triangle index, -1: none yet
    double u, v;     // the weights of p1() and p2() of its closest point
};

CERES_NEAR64_FN double near64_dot(double ax, double ay, double az, double bx, double by, double bz) { return (ax * bx + ay * by) + az * bz; }
CERES_NEAR64_FN double near64_min(double x, double y) { return x < y ? x : y; }
CERES_NEAR64_FN double near64_max(double x, double y) { return x > y ? x : y; }
CERES_NEAR64_FN double near64_clamp(double x, double lo, double hi) { return x < lo ? lo : (x > hi ? hi : x); }

// The bound of a box {xmin, xmax, ymin, ymax, zmin, zmax}: the squared distance of p to its clamp.
CERES_NEAR64_FN double near64_box(double px, double py, double pz, double xmin, double xmax, double ymin, double ymax, double zmin,
                                  double zmax) {
    const double ex = px - near64_clamp(px, xmin, xmax), ey = py - near64_clamp(py, ymin, ymax), ez = pz - near64_clamp(pz, zmin, zmax);
    return (ex * ex + ey * ey) + ez * ez;
}

// One triangle {p0, e1, e2} (p1() = p0 - e1, p2() = p0 + e2): d2 and the weights (v, w) of p1() and
// p2().  Ericson, Real-Time Collision Detection 5.1.5, his regions in his order.
CERES_NEAR64_FN double near64_tri(double px, double py, double pz, const double p0[3], const double e1[3], const double e2[3],
                                  double& v_out, double& w_out) {
    const double ax = p0[0], ay = p0[1], az = p0[2];
    const double bx = ax - e1[0], by = ay - e1[1], bz = az - e1[2];
    const double cx = ax + e2[0], cy = ay + e2[1], cz = az + e2[2];
    const double abx = -e1[0], aby = -e1[1], abz = -e1[2];
    const double acx = e2[0], acy = e2[1], acz = e2[2];
    double v, w;
    const double d1 = near64_dot(abx, aby, abz, px - ax, py - ay, pz - az), d2 = near64_dot(acx, acy, acz, px - ax, py - ay, pz - az);
    const double d3 = near64_dot(abx, aby, abz, px - bx, py - by, pz - bz), d4 = near64_dot(acx, acy, acz, px - bx, py - by, pz - bz);
    const double d5 = near64_dot(abx, aby, abz, px - cx, py - cy, pz - cz), d6 = near64_dot(acx, acy, acz, px - cx, py - cy, pz - cz);
    const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    if (d1 <= 0.0 && d2 <= 0.0) { v = 0.0; w = 0.0; }                                        // vertex a
    else if (d3 >= 0.0 && d4 <= d3) { v = 1.0; w = 0.0; }                                    // vertex b
    else if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) { v = d1 / (d1 - d3); w = 0.0; }           // edge ab
    else if (d6 >= 0.0 && d5 <= d6) { v = 0.0; w = 1.0; }                                    // vertex c
    else if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) { v = 0.0; w = d2 / (d2 - d6); }           // edge ac
    else if (va <= 0.0 && (d4 - d3) >= 0.0 && (d5 - d6) >= 0.0) {                            // edge bc
        w = (d4 - d3) / ((d4 - d3) + (d5 - d6)); v = 1.0 - w;
    } else {                                                                                 // interior
        const double denom = 1.0 / ((va + vb) + vc);
        v = vb * denom; w = vc * denom;
    }
    const double qx = near64_clamp((ax + abx * v) + acx * w, near64_min(near64_min(ax, bx), cx), near64_max(near64_max(ax, bx), cx));
    const double qy = near64_clamp((ay + aby * v) + acy * w, near64_min(near64_min(ay, by), cy), near64_max(near64_max(ay, by), cy));
    const double qz = near64_clamp((az + abz * v) + acz * w, near64_min(near64_min(az, bz), cz), near64_max(near64_max(az, bz), cz));
    const double dx = px - qx, dy = py - qy, dz = pz - qz;
    v_out = v; w_out = w;
    return (dx * dx + dy * dy) + dz * dz;
}

// The selection: a surface at exactly the best distance counts while nothing is found, equal distances
// go to the smallest original index, a NaN d2 is never taken.
CERES_NEAR64_FN bool near64_better(double d2, uint32_t orig, const NearBest64& b) {
    return d2 < b.d2 || (d2 == b.d2 && (b.prim < 0 || int32_t(orig) < b.prim));
}

}  // namespace ceres
