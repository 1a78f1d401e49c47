// closest_point.hpp -- the arithmetic of the closest-point queries (ceres_closest_points*), one set of
// functions for the host walk (render_cpu.cpp) and the device walk (closest_point.hip).
//
// The answer of a query is, bit for bit, the minimum over ALL triangles of near_tri()'s d2 under
// near_better()'s order (DESIGN.md "Closest-point queries"); the BVH only skips what cannot win or tie:
//   * near_tri clamps its closest point q into the triangle's own bounding box min/max(a, b, c), so q
//     lies in every box that contains that box;
//   * near_box is the same expression shape over e = p - clamp(p, box): per axis |e_k| <= |p_k - q_k|
//     exactly, and float subtraction, multiplication and addition are monotone, so the computed bound
//     is <= the computed d2 of every triangle below the box;
//   * a child is skipped iff its bound > best, strictly.
// Only IEEE operations whose result does not depend on the compiler: + - * / compare and select; every
// translation unit that includes this is built with -ffp-contract=off.  NaN fails every compare, so a
// NaN bound is never skipped and a NaN d2 never taken.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define CERES_NEAR_FN __host__ __device__ inline
#else
#define CERES_NEAR_FN inline
#endif

namespace ceres {

struct NearBest {
    float d2;        // the best squared distance so far; starts at r2max
    int32_t prim;    // its ORIGINAL triangle index, -1: none yet
    float u, v;      // the weights of p1() and p2() of its closest point
};

CERES_NEAR_FN float near_dot(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }
CERES_NEAR_FN float near_min(float x, float y) { return x < y ? x : y; }
CERES_NEAR_FN float near_max(float x, float y) { return x > y ? x : y; }
CERES_NEAR_FN float near_clamp(float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); }

// The bound of a box {xmin, xmax, ymin, ymax, zmin, zmax}: the squared distance of p to its clamp.
CERES_NEAR_FN float near_box(float px, float py, float pz, float xmin, float xmax, float ymin, float ymax, float zmin, float zmax) {
    const float ex = px - near_clamp(px, xmin, xmax), ey = py - near_clamp(py, ymin, ymax), ez = pz - near_clamp(pz, zmin, zmax);
    return (ex * ex + ey * ey) + ez * ez;
}

// One triangle {p0, e1, e2} (triangle.hpp:17-37: p1() = p0 - e1, p2() = p0 + e2): d2 and the weights
// (v, w) of p1() and p2().  Ericson, Real-Time Collision Detection 5.1.5, his regions in his order.
CERES_NEAR_FN float near_tri(float px, float py, float pz, const float p0[3], const float e1[3], const float e2[3], float& v_out,
                             float& w_out) {
    const float ax = p0[0], ay = p0[1], az = p0[2];
    const float bx = ax - e1[0], by = ay - e1[1], bz = az - e1[2];
    const float cx = ax + e2[0], cy = ay + e2[1], cz = az + e2[2];
    const float abx = -e1[0], aby = -e1[1], abz = -e1[2];
    const float acx = e2[0], acy = e2[1], acz = e2[2];
    float v, w;
    const float d1 = near_dot(abx, aby, abz, px - ax, py - ay, pz - az), d2 = near_dot(acx, acy, acz, px - ax, py - ay, pz - az);
    const float d3 = near_dot(abx, aby, abz, px - bx, py - by, pz - bz), d4 = near_dot(acx, acy, acz, px - bx, py - by, pz - bz);
    const float d5 = near_dot(abx, aby, abz, px - cx, py - cy, pz - cz), d6 = near_dot(acx, acy, acz, px - cx, py - cy, pz - cz);
    const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    if (d1 <= 0.f && d2 <= 0.f) { v = 0.f; w = 0.f; }                                        // vertex a
    else if (d3 >= 0.f && d4 <= d3) { v = 1.f; w = 0.f; }                                    // vertex b
    else if (vc <= 0.f && d1 >= 0.f && d3 <= 0.f) { v = d1 / (d1 - d3); w = 0.f; }           // edge ab
    else if (d6 >= 0.f && d5 <= d6) { v = 0.f; w = 1.f; }                                    // vertex c
    else if (vb <= 0.f && d2 >= 0.f && d6 <= 0.f) { v = 0.f; w = d2 / (d2 - d6); }           // edge ac
    else if (va <= 0.f && (d4 - d3) >= 0.f && (d5 - d6) >= 0.f) {                            // edge bc
        w = (d4 - d3) / ((d4 - d3) + (d5 - d6)); v = 1.f - w;
    } else {                                                                                 // interior
        const float denom = 1.f / ((va + vb) + vc);
        v = vb * denom; w = vc * denom;
    }
    const float qx = near_clamp((ax + abx * v) + acx * w, near_min(near_min(ax, bx), cx), near_max(near_max(ax, bx), cx));
    const float qy = near_clamp((ay + aby * v) + acy * w, near_min(near_min(ay, by), cy), near_max(near_max(ay, by), cy));
    const float qz = near_clamp((az + abz * v) + acz * w, near_min(near_min(az, bz), cz), near_max(near_max(az, bz), cz));
    const float dx = px - qx, dy = py - qy, dz = pz - qz;
    v_out = v; w_out = w;
    return (dx * dx + dy * dy) + dz * dz;
}

// The selection: a surface at exactly the best distance counts while nothing is found, equal distances
// go to the smallest original index, a NaN d2 is never taken.
CERES_NEAR_FN bool near_better(float d2, uint32_t orig, const NearBest& b) {
    return d2 < b.d2 || (d2 == b.d2 && (b.prim < 0 || int32_t(orig) < b.prim));
}

}  // namespace ceres
