// render64.hip -- render<double> (render.hpp:86-156 with Scalar = double; anim.cpp's -d mode,
// anim.cpp:146-155) on gfx950.
//
// The double instantiation keeps the reference's mixed precision exactly: camera basis, rays,
// BVH2 traversal (FastNodeIntersector with a true fma, node_intersectors.hpp:35-47,83-103),
// Moller-Trumbore (triangle.hpp:95-115), hit point, offset and shadow ray in double; the
// shading helpers return float (render.hpp:46-54: lambertian / blinn_phong_spec are declared
// `float`, std::pow(double, int) is a double pow narrowed to float) and smooth_shading
// accumulates `c[k] += u * clamp(...)` as float = float(double + double) (render.hpp:56-84); the
// pixel is the float colour widened to double and quantised in double (static.cpp:141-143).
//
// One kernel, one lane per pixel, 8x8 tiles per wavefront: primary closest-hit traversal in
// the reference's order, then the any-hit shadow ray over the same BVH2 (only the boolean is
// used, render.hpp:139), shading, store.  Records are double-width (112-B sibling pairs, 96-B
// triangles); the stack is u32 in LDS like the float path.  Built without FP contraction;
// IEEE double division and sqrt are correctly rounded on gfx950.
//
// CERES_MODE_FMA (kG = true, round 5): the reference's own CMake build of anim.cpp -d (g++ -O3
// -mavx2 -mfma, CMakeLists.txt:11) fuses the double hot path at the same sites as the float one
// -- GCC's widening_mul dump of the double harness lists the same (file, line, column, FMA kind)
// multiset for render()'s pixel loop, smooth_shading and blinn_phong_spec
// (oracle/contraction_sites.txt) -- so the kernel carries an explicit fma at each: dotA / dotB,
// cross with the first product fused, the primary direction dir + fma(iv, v, iu u), the hit point
// fma(n, -1e-5, fma(w, p2, fma(v, p1, u p0))), lambertian as dotA in double, and the float
// fmaf(lam, 0.5, amb) / fmaf(base, k, spec) of smooth_shading.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>
#include <type_traits>
#include <vector>

#include "ceres_render.h"
#include "ceres_types.hpp"
#include "indexed_params.hpp"
#include "pow24.hpp"
#include "query_host.hpp"

#pragma clang fp contract(off)

namespace ceres {
namespace dev64 {

#ifndef CERES64_WG
#define CERES64_WG 64            // workgroup: 64 = one 8x8 tile (a long tile pins only its own LDS), 256 = 16x16
#endif
#ifndef CERES_LANE_QUADS64
#define CERES_LANE_QUADS64 0     // lanes in Morton order over the 8x8 tile (else row-major)
#endif
constexpr int kBlock = CERES64_WG;
constexpr uint32_t kTile = kBlock == 256 ? 16u : 8u;

struct D3 { double x, y, z; };
__device__ __forceinline__ D3 operator+(D3 a, D3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ D3 operator-(D3 a, D3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ D3 operator*(D3 a, double s) { return {a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ D3 operator*(double s, D3 a) { return {s * a.x, s * a.y, s * a.z}; }
__device__ __forceinline__ double dot(D3 a, D3 b) { double s = a.x * b.x; s += a.y * b.y; s += a.z * b.z; return s; }
__device__ __forceinline__ D3 cross(D3 a, D3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ D3 normalize(D3 v) { const double inv = 1.0 / sqrt(dot(v, v)); return v * inv; }
__device__ __forceinline__ D3 d3(const double* p) { return {p[0], p[1], p[2]}; }
// GCC's contraction of vector.hpp:134-167 in the reference-flag build (kG; oracle/contraction_sites.txt)
template <bool kG> __device__ __forceinline__ double dotA(D3 a, D3 b) {
    if constexpr (kG) return fma(a.z, b.z, fma(a.x, b.x, a.y * b.y));
    else return dot(a, b);
}
template <bool kG> __device__ __forceinline__ double dotB(D3 a, D3 b) {
    if constexpr (kG) return fma(a.z, b.z, fma(a.y, b.y, a.x * b.x));
    else return dot(a, b);
}
template <bool kG> __device__ __forceinline__ D3 crossG(D3 a, D3 b) {
    if constexpr (kG) return {fma(a.y, b.z, -(a.z * b.y)), fma(a.z, b.x, -(a.x * b.z)), fma(a.x, b.y, -(a.y * b.x))};
    else return cross(a, b);
}
template <bool kG> __device__ __forceinline__ D3 normalizeG(D3 v) { const double inv = 1.0 / sqrt(dotA<kG>(v, v)); return v * inv; }

struct Cam64 { double eye[3], dir[3], iu[3], iv[3], sun[3]; };

struct KParams64 {
    Cam64 cam;
    uint32_t W, H;
    uint32_t stack_entries, root_leaf_count, root_leaf_first;
    const SiblingPair64* pairs;
    const Tri96* tris;
    const uint32_t* orig;
    const double* norms;
    double* pixels;          // 3*W*H, row 0 at the bottom (render.hpp:107)
    uint8_t* rgb8;           // PPM body, rows top-down
    Shard* shards;
    int32_t* rec_prim;       // optional per-pixel records, pixel = j*W + i
    double* rec_tuv;
    int8_t* rec_shadow;
    const uint32_t* tile_order;  // block -> tile, centre first and XCD-balanced (frame_tile_order)
    uint32_t tiles_x;
};

struct TriD { D3 p0, e1, e2, n; };
__device__ __forceinline__ TriD load_tri(const Tri96* t) {
    const double2* q = reinterpret_cast<const double2*>(t);
    const double2 a = q[0], b = q[1], c = q[2], d = q[3], e = q[4], f = q[5];
    return {{a.x, a.y, b.x}, {b.y, c.x, c.y}, {d.x, d.y, e.x}, {e.y, f.x, f.y}};
}

// Triangle<double>::intersect (triangle.hpp:95-115)
template <bool kG>
__device__ __forceinline__ bool tri_test(const TriD& tr, D3 o, D3 d, double tmin, double tmax, double& t_out, double& u_out,
                                         double& v_out) {
    const D3 c = tr.p0 - o;
    const D3 r = crossG<kG>(d, c);
    const double inv_det = 1.0 / dotA<kG>(tr.n, d);
    const double u = dotA<kG>(r, tr.e2) * inv_det;
    const double v = dotB<kG>(r, tr.e1) * inv_det;
    const double w = 1.0 - u - v;
    if (u >= 0 && v >= 0 && w >= 0) {
        const double t = dotA<kG>(tr.n, c) * inv_det;
        if (t >= tmin && t <= tmax) { t_out = t; u_out = u; v_out = v; return true; }
    }
    return false;
}

struct Hit { uint32_t slot; double t, u, v; };

// The kind of ray a walk serves (as CamRay / CallerRay of render_hip.hip):
//   CamRay64     a ray render<double>() makes itself: the window is [0, DBL_MAX] (ray.hpp:17-21),
//                two constants -- the default, so no render call site names it;
//   CallerRay64  a ray the caller supplies (ceres_trace_rays64_k): the window comes from the ray and
//                enters every box test and every triangle test.  A NaN bound fails every box and
//                triangle test of the reference (robust_max(x, NaN) is NaN, utilities.hpp:58-70;
//                fmax would drop it): the empty window [+inf, -inf] fails the same tests.
struct CamRay64 {
    __device__ __forceinline__ double tmin() const { return 0.0; }
    __device__ __forceinline__ double tmax() const { return DBL_MAX; }
};
struct CallerRay64 {
    double lo, hi;
    __device__ __forceinline__ CallerRay64(double tmin, double tmax) {
        const bool nan = isnan(tmin) || isnan(tmax);
        lo = nan ? double(INFINITY) : tmin;
        hi = nan ? -double(INFINITY) : tmax;
    }
    __device__ __forceinline__ double tmin() const { return lo; }
    __device__ __forceinline__ double tmax() const { return hi; }
};
// The reference's Statistics of one walk (single_ray_traverser.hpp:83,53): NoCount compiles to nothing.
struct NoCount {
    __device__ __forceinline__ void step() {}
    __device__ __forceinline__ void tests(uint32_t) {}
};
struct Count {
    uint32_t n_pairs = 0, n_tests = 0;
    __device__ __forceinline__ void step() { ++n_pairs; }
    __device__ __forceinline__ void tests(uint32_t n) { n_tests += n; }
};

// single_ray_traverser.hpp:68-126 in double (the float trace() of render_hip.hip: the same
// visiting order, octant-free monotone slab test, near-first ties left; any-hit returns at the
// first accepted triangle).  PT: the kernel's parameter block (scene pointers, stack bound); kS: the
// stride of the [entry][lane] stack; RK: the ray kind; Cnt: NoCount or Count.
template <bool kAnyHit, bool kG, int kS, class RK, class Cnt, class PT>
__device__ bool trace(const PT& P, D3 o, D3 d, uint32_t* stk, Hit& best, bool& overflow, RK rk, Cnt& cnt) {
    const double tmin = rk.tmin();
    double tmax = rk.tmax();
    bool have = false;
    if (P.root_leaf_count) {
        cnt.tests(P.root_leaf_count);
        for (uint32_t k = P.root_leaf_first; k < P.root_leaf_first + P.root_leaf_count; ++k) {
            double t, u, v;
            if (tri_test<kG>(load_tri(P.tris + k), o, d, tmin, tmax, t, u, v)) {
                best = {k, t, u, v}; have = true;
                if (kAnyHit) return true;
                tmax = t;
            }
        }
        return have;
    }
    auto safe_inv = [](double x) { return 1.0 / (fabs(x) < DBL_EPSILON ? copysign(DBL_EPSILON, x) : x); };   // vector.hpp:69-74
    const double ix = safe_inv(d.x), iy = safe_inv(d.y), iz = safe_inv(d.z);
    const double sx = (-o.x) * ix, sy = (-o.y) * iy, sz = (-o.z) * iz;
    uint32_t sp = 0, cur = 0;
    while (true) {
        cnt.step();
        const double2* q = reinterpret_cast<const double2*>(P.pairs + cur);
        const double2 A = q[0], B = q[1], C = q[2], D = q[3], E = q[4], F = q[5];
        const uint4 L = reinterpret_cast<const uint4*>(q)[6];
        const double l0 = fma(A.x, ix, sx), l1 = fma(A.y, ix, sx);
        const double l2 = fma(B.x, iy, sy), l3 = fma(B.y, iy, sy);
        const double l4 = fma(C.x, iz, sz), l5 = fma(C.y, iz, sz);
        const double r0 = fma(D.x, ix, sx), r1 = fma(D.y, ix, sx);
        const double r2 = fma(E.x, iy, sy), r3 = fma(E.y, iy, sy);
        const double r4 = fma(F.x, iz, sz), r5 = fma(F.y, iz, sz);
        const double le = fmax(fmin(l0, l1), fmax(fmin(l2, l3), fmax(fmin(l4, l5), tmin)));
        const double lx = fmin(fmax(l0, l1), fmin(fmax(l2, l3), fmin(fmax(l4, l5), tmax)));
        const double re = fmax(fmin(r0, r1), fmax(fmin(r2, r3), fmax(fmin(r4, r5), tmin)));
        const double rx = fmin(fmax(r0, r1), fmin(fmax(r2, r3), fmin(fmax(r4, r5), tmax)));
        const bool hit_l = le <= lx, hit_r = re <= rx;
        uint32_t k = 0, k_end = 0, k2 = 0, k2_end = 0;
        if (hit_l && L.x) { k = L.y; k_end = L.y + L.x; cnt.tests(L.x); }
        if (hit_r && L.z) { k2 = L.w; k2_end = L.w + L.z; cnt.tests(L.z); }
        while (k < k_end || k2 < k2_end) {
            const uint32_t idx = k < k_end ? k++ : k2++;
            double t, u, v;
            if (tri_test<kG>(load_tri(P.tris + idx), o, d, tmin, tmax, t, u, v)) {
                best = {idx, t, u, v}; have = true;
                if (kAnyHit) return true;
                tmax = t;
            }
        }
        const bool go_l = hit_l && !L.x, go_r = hit_r && !L.z;
        if (go_l && go_r) {
            const bool swap = le > re;
            if (sp >= P.stack_entries) { overflow = true; return have; }
            stk[sp * kS] = swap ? L.y : L.w;
            ++sp;
            cur = swap ? L.w : L.y;
        } else if (go_l || go_r) {
            cur = go_l ? L.y : L.w;
        } else {
            if (sp == 0) break;
            --sp;
            cur = stk[sp * kS];
        }
    }
    return have;
}
// render<double>()'s own rays: the default ray kind, no counters
template <bool kAnyHit, bool kG>
__device__ __forceinline__ bool trace(const KParams64& P, D3 o, D3 d, uint32_t* stk, Hit& best, bool& overflow) {
    NoCount none;
    return trace<kAnyHit, kG, kBlock>(P, o, d, stk, best, overflow, CamRay64{}, none);
}

// (float)std::pow(x, 24) for a double x: x^24 in double-double, rounded to double (the
// correctly rounded pow), then narrowed to float as blinn_phong_spec's return type does.
__device__ __forceinline__ float pow24_from_double(double x) {
    if (!(fabs(x) <= 1e12)) return isnan(x) ? float(x) : INFINITY;   // |x|^24 overflows float long before
    double h2 = x * x, l2 = fma(x, x, -h2);
    double h4, l4, h8, l8, h16, l16, h24, l24;
    dd_square(h2, l2, h4, l4);
    dd_square(h4, l4, h8, l8);
    dd_square(h8, l8, h16, l16);
    dd_mul(h16, l16, h8, l8, h24, l24);
    return float(h24 + l24);
}

// smooth_shading<double> (render.hpp:46-84): float helpers, double weights, float accumulators
template <bool kG>
__device__ __forceinline__ void shade(D3 sun_line, const double* nrm, D3 view, double u, double v, float c[3]) {
    c[0] = c[1] = c[2] = 0.0f;
    const float amb = 0.2;
    const D3 vneg = view * -1.0;
    const double w[3] = {u, v, 1 - u - v};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const D3 N{nrm[3 * k], nrm[3 * k + 1], nrm[3 * k + 2]};
        const float lam = float(fabs(kG ? dotA<true>(sun_line, N) : sun_line.x * N.x + sun_line.y * N.y + sun_line.z * N.z));   // lambertian
        const float spec = 0.8f * pow24_from_double(dotA<kG>(N, normalizeG<kG>(sun_line + vneg)));  // blinn_phong_spec
        const float base = kG ? __builtin_fmaf(lam, 0.5f, amb) : amb + 0.5f * lam;
        auto clamp01 = [](float x) { return (x < 0.f) ? 0.f : (1.f < x) ? 1.f : x; };          // std::clamp
        auto ch = [&](float k) { return kG ? __builtin_fmaf(base, k, spec) : base * k + spec; };
        c[0] = float(double(c[0]) + w[k] * double(clamp01(ch(0.5f))));
        c[1] = float(double(c[1]) + w[k] * double(clamp01(ch(0.0f))));
        c[2] = float(double(c[2]) + w[k] * double(clamp01(ch(0.8f))));
    }
}

__device__ __forceinline__ uint8_t quantize(double x) {              // static.cpp:141-143 with Scalar = double
    const double a = x * 255;
    const double m = (255.0 < a) ? 255.0 : a;
    const double q = (m < 0.0) ? 0.0 : m;
    return static_cast<uint8_t>(static_cast<int>(q));
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
    return x;
}

// 1-D grid over the frame's kTile x kTile tiles in tile_order (as the float path: expensive tiles
// first, every XCD an unbiased share); each wavefront an 8x8 tile (of its workgroup's 16x16
// pixels when kBlock = 256)
template <int kMode, bool kG>
__global__ __launch_bounds__(kBlock) void ceres_render64(const KParams64 P) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint32_t* stk = lds + tid;
    const uint32_t t = __builtin_amdgcn_readfirstlane(P.tile_order[blockIdx.x]);
    const uint32_t tby = t / P.tiles_x, tbx = t - tby * P.tiles_x;
#if CERES_LANE_QUADS64
    // lanes in Morton order over the wavefront's 8x8 tile (quads = 2x2 pixel blocks)
    const uint32_t lx = (lane & 1u) | ((lane >> 1) & 2u) | ((lane >> 2) & 4u), ly = ((lane >> 1) & 1u) | ((lane >> 2) & 2u) | ((lane >> 3) & 4u);
#else
    const uint32_t lx = lane & 7u, ly = lane >> 3;
#endif
    const uint32_t i = tbx * kTile + (kBlock == 256 ? (wave & 1u) * 8u : 0u) + lx;
    const uint32_t j = tby * kTile + (kBlock == 256 ? (wave >> 1) * 8u : 0u) + ly;
    const bool valid = i < P.W && j < P.H;
    bool overflow = false;
    uint32_t n_hit = 0, n_shadow = 0, n_occ = 0;
    if (valid) {
        const Cam64& c = P.cam;
        // render.hpp:109-113
        const double u = 2 * (double(i) + 0.5) / double(P.W) - 1.0;
        const double v = 2 * (double(j) + 0.5) / double(P.H) - 1.0;
        D3 a;
        if constexpr (kG)                                            // GCC: dir + fma(iv, v, iu u)
            a = D3{c.dir[0] + fma(c.iv[0], v, c.iu[0] * u), c.dir[1] + fma(c.iv[1], v, c.iu[1] * u),
                   c.dir[2] + fma(c.iv[2], v, c.iu[2] * u)};
        else a = d3(c.iu) * u + d3(c.iv) * v + d3(c.dir);
        const D3 view = normalizeG<kG>(a);
        Hit h{};
        const bool hit = trace<false, kG>(P, d3(c.eye), view, stk, h, overflow);
        double px[3] = {0.0, 0.0, 0.0};
        int8_t shadow_rec = -1;
        if (hit) {
            n_hit = 1;
            const TriD tri = load_tri(P.tris + h.slot);
            const D3 normal = normalizeG<kG>(tri.n);
            if (kMode == CERES_MODE_PRIMARY) {                        // render.hpp:123-125
                px[0] = fabs(normal.x); px[1] = fabs(normal.y); px[2] = fabs(normal.z);
            } else {
                const D3 p1 = tri.p0 - tri.e1, p2 = tri.p0 + tri.e2;   // p1(), p2()
                const double scale = -0.00001;
                D3 p;
                if constexpr (kG) {                                  // GCC: fma(n, scale, fma(w, p2, fma(v, p1, u p0)))
                    const double w = 1 - h.u - h.v;
                    auto cp = [&](double a0, double q1, double q2, double n) { return fma(n, scale, fma(w, q2, fma(h.v, q1, h.u * a0))); };
                    p = D3{cp(tri.p0.x, p1.x, p2.x, normal.x), cp(tri.p0.y, p1.y, p2.y, normal.y), cp(tri.p0.z, p1.z, p2.z, normal.z)};
                } else {
                    p = h.u * tri.p0 + h.v * p1 + (1 - h.u - h.v) * p2;   // render.hpp:129 (permuted weights)
                    p = p + scale * normal;
                }
                const D3 sun_line = normalizeG<kG>(d3(c.sun) - p);     // render.hpp:135
                Hit h2;
                n_shadow = 1;
                const bool blocked = trace<true, kG>(P, p, sun_line, stk, h2, overflow);
                shadow_rec = blocked ? 1 : 0;
                if (blocked) {
                    n_occ = 1;
                } else {
                    float col[3];
                    shade<kG>(sun_line, P.norms + 9 * size_t(P.orig[h.slot]), view, h.u, h.v, col);
                    px[0] = col[0]; px[1] = col[1]; px[2] = col[2];
                }
            }
        }
        const size_t pix = size_t(j) * P.W + i;
        if (P.pixels) { double* q = P.pixels + 3 * pix; q[0] = px[0]; q[1] = px[1]; q[2] = px[2]; }
        if (P.rgb8) {
            uint8_t* q = P.rgb8 + 3 * (size_t(P.H - 1 - j) * P.W + i);
            q[0] = quantize(px[0]); q[1] = quantize(px[1]); q[2] = quantize(px[2]);
        }
        if (P.rec_prim) {
            P.rec_prim[pix] = hit ? int32_t(P.orig[h.slot]) : -1;
            P.rec_tuv[3 * pix] = hit ? h.t : 0.0; P.rec_tuv[3 * pix + 1] = hit ? h.u : 0.0; P.rec_tuv[3 * pix + 2] = hit ? h.v : 0.0;
            P.rec_shadow[pix] = shadow_rec;
        }
    }
    const uint32_t wh = wave_sum(n_hit + n_occ), ws = wave_sum(n_shadow);
    const uint32_t shard = blockIdx.x * (kBlock / 64) + wave;
    if (lane == 0) {
        Shard& sh = P.shards[shard % kShards];
        if (ws) atomicAdd(&sh.queued, ws);
        if (wh) atomicAdd(&sh.hits, (unsigned long long)wh);
    }
    if (__ballot(overflow) && lane == 0) atomicOr(&P.shards[shard % kShards].error, 1u);
}

// ---------------------------------------------------------------- ray queries
// ceres_trace_rays_f64*: closest hit and occlusion for rays the CALLER supplies, on a double scene --
// SingleRayTraverser::traverse(ray, intersector) over any bvh::Ray<double> (ray.hpp:10-22,
// single_ray_traverser.hpp:68-126), the sibling of ceres_trace_rays_k (render_hip.hip).  Both queries
// are trace() above with CallerRay64: the window comes from the ray, the direction is not normalised
// (trace() divides with IEEE 1 / x for either kind of ray), and the occlusion query is the any-hit
// walk over the same BVH2 (no double BVH4 exists).  Shares the scene's buffers and nothing else.
struct RayParams64 {
    const double2* rays;                         // n_rays x ray64 = 4 x 16 B: {o.xy}, {o.z, d.x}, {d.yz}, {tmin, tmax}
    ulonglong2* hits;                            // n_rays x hit32 = 2 x 16 B: {prim | 0 << 32, t}, {u, v}; or NULL
    uint8_t* occluded;                           // n_rays x u8 or NULL
    unsigned long long* counters;                // 8 x u64 (zeroed before the launch) or NULL
    const SiblingPair64* pairs;
    const Tri96* tris;
    const uint32_t* orig;
    uint32_t n_rays;
    uint32_t stack_entries, root_leaf_count, root_leaf_first;
};
constexpr int kRayB = 64;

// One ray per lane, 64 rays of consecutive index per single-wavefront workgroup (a long ray pins only
// its own LDS and wave slot); the u32 stack in LDS [entry][lane], shared by the two queries of a ray
// (one after the other).  A ray is four aligned 16-byte loads, a hit two 16-byte stores; a tail
// wave's idle lanes run nothing, store nothing and count nothing.
// counters: {rays, hits, rays, 0, node_pairs, tri_tests, stack overflow, 0}; kStats: the Statistics
// of the closest query, summed per wave, one atomic per wave and counter.
template <bool kStats, bool kG, class PT>
__device__ __forceinline__ void trace_rays64_body(const PT& P) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const uint32_t lane = threadIdx.x;
    uint32_t* stk = lds + lane;
    const uint32_t r = lane_ray(P, blockIdx.x * uint32_t(kRayB) + lane);   // n_rays < 2^31 (host-checked)
    bool hit = false, occ = false, overflow = false;
    typename std::conditional<kStats, Count, NoCount>::type cnt;
    if (r < P.n_rays) {
        const double2* q = P.rays + 4 * size_t(r);
        const double2 a = q[0], b = q[1], c = q[2], w = q[3];
        const D3 o{a.x, a.y, b.x}, d{b.y, c.x, c.y};
        const CallerRay64 rk{w.x, w.y};
        if (P.hits) {
            Hit h{0u, 0.0, 0.0, 0.0};
            hit = trace<false, kG, kRayB>(P, o, d, stk, h, overflow, rk, cnt);
            ulonglong2 r0 = make_ulonglong2(0xffffffffull, 0ull), r1 = make_ulonglong2(0ull, 0ull);   // a miss: {-1, 0, 0.0, 0.0, 0.0}
            if (hit) {
                r0 = make_ulonglong2((unsigned long long)P.orig[h.slot], (unsigned long long)__double_as_longlong(h.t));
                r1 = make_ulonglong2((unsigned long long)__double_as_longlong(h.u), (unsigned long long)__double_as_longlong(h.v));
            }
            P.hits[2 * size_t(r)] = r0;
            P.hits[2 * size_t(r) + 1] = r1;
        }
        if (P.occluded) {
            Hit h2;
            NoCount none;                                             // the statistics count the closest query only
            occ = trace<true, kG, kRayB>(P, o, d, stk, h2, overflow, rk, none);
            P.occluded[r] = occ ? 1 : 0;
        }
    }
    if (P.counters) {                                                 // wave-uniform
        const uint32_t nh = __popcll(__ballot(P.hits ? hit : occ));
        if (lane == 0 && nh) atomicAdd(&P.counters[1], (unsigned long long)nh);
        if constexpr (kStats) {
            const uint32_t wp = wave_sum(cnt.n_pairs), wt = wave_sum(cnt.n_tests);
            if (lane == 0) {
                atomicAdd(&P.counters[4], (unsigned long long)wp);
                atomicAdd(&P.counters[5], (unsigned long long)wt);
            }
        }
        if (blockIdx.x == 0 && lane == 0) {
            atomicAdd(&P.counters[0], (unsigned long long)launch_rays(P));
            atomicAdd(&P.counters[2], (unsigned long long)launch_rays(P));
        }
        if (overflow) atomicOr(&P.counters[6], 1ull);
    }
}

// The plain launch (lane i takes ray i) and the indexed one (lane i takes ray index[i],
// indexed_params.hpp): one body, chosen by the parameter block.  Indexed launches have no stats
// instantiation (CERES_SCENE_STATS scenes refuse the indexed calls).
template <bool kStats, bool kG>
__global__ __launch_bounds__(kRayB) void ceres_trace_rays64_k(const RayParams64 P) { trace_rays64_body<kStats, kG>(P); }
template <bool kG>
__global__ __launch_bounds__(kRayB) void ceres_trace_rays64_idx_k(const Indexed<RayParams64> P) { trace_rays64_body<false, kG>(P); }

// ---------------------------------------------------------------- shaded ray queries
// ceres_shade_rays_f64*: render<double>()'s pixel for a ray the CALLER supplies -- the body of
// ceres_render64 from the primary walk on (render.hpp:114-150 with Scalar = double), with the caller's
// bvh::Ray<double> in place of Ray(eye, view) and its direction in place of `view`; the sibling of
// ceres_shade_rays_k (render_hip.hip).  One lane chains, without a queue through HBM:
//   primary   trace<false>() with CallerRay64, exactly ceres_trace_rays64_k's closest query;
//   miss      the pixel is 0, 0, 0, status 0;
//   shadow    normal = normalize(tri.n), p = the hit point with its -0.00001 offset, Ray(p, normalize(sun - p))
//             with the window [0, DBL_MAX] (CamRay64), answered any-hit over the same BVH2;
//   blocked   the pixel is 0, status 2;
//   lit       shade(sun_line, the original triangle's normals, view = the ray's direction AS GIVEN, u, v),
//             status 1: float helpers, double weights, float accumulators; the pixel is the float colour
//             widened to double, as ceres_render64 stores it.
// counters: {rays = n + primary hits, hits = primary hits + shadowed hits, primary_rays = n,
// shadow_rays = primary hits, 0, 0, stack overflow, 0} -- the pair ceres_render_f64 returns.  There is
// no stats instantiation: CERES_SCENE_STATS scenes run these kernels.
struct ShadeParams64 {
    const double2* rays;                         // n_rays x ray64
    double* pixels;                              // n_rays x 3 double or NULL
    uint8_t* rgb8;                               // n_rays x 3 bytes (quantize of the same doubles) or NULL
    ulonglong2* hits;                            // n_rays x hit32 or NULL
    uint8_t* status;                             // n_rays x u8 (0 miss, 1 lit, 2 in shadow) or NULL
    unsigned long long* counters;                // 8 x u64 (zeroed before the launch) or NULL
    const SiblingPair64* pairs;
    const Tri96* tris;
    const uint32_t* orig;
    const double* norms;
    uint32_t n_rays;
    uint32_t stack_entries, root_leaf_count, root_leaf_first;
    double sun[3];
};

// Hit point + self-intersection offset (render.hpp:127-133; p1 = p0 - e1, p2 = p0 + e2): the
// expressions of ceres_render64, which keeps its own copy so that its code does not move.
template <bool kG>
__device__ __forceinline__ D3 hit_point(const TriD& tri, D3 normal, double hu, double hv) {
    const D3 p1 = tri.p0 - tri.e1, p2 = tri.p0 + tri.e2;
    const double scale = -0.00001;
    if constexpr (kG) {                                              // GCC: fma(n, scale, fma(w, p2, fma(v, p1, u p0)))
        const double w = 1 - hu - hv;
        auto cp = [&](double a0, double q1, double q2, double n) { return fma(n, scale, fma(w, q2, fma(hv, q1, hu * a0))); };
        return D3{cp(tri.p0.x, p1.x, p2.x, normal.x), cp(tri.p0.y, p1.y, p2.y, normal.y), cp(tri.p0.z, p1.z, p2.z, normal.z)};
    } else {
        const D3 p = hu * tri.p0 + hv * p1 + (1 - hu - hv) * p2;     // render.hpp:129 (permuted weights)
        return p + scale * normal;
    }
}

// The geometry of ceres_trace_rays64_k: one ray per lane, 64 consecutive rays per single-wavefront
// workgroup, the u32 stack in LDS [entry][lane] shared by the two walks of a ray; a tail wave's idle
// lanes load, store and count nothing.  A pixel is three 8-byte stores (a 24-byte record is only
// 8-byte aligned).
template <bool kG, class PT>
__device__ __forceinline__ void shade_rays64_body(const PT& P) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const uint32_t lane = threadIdx.x;
    uint32_t* stk = lds + lane;
    const uint32_t r = lane_ray(P, blockIdx.x * uint32_t(kRayB) + lane);   // n_rays < 2^31 (host-checked)
    bool hit = false, blocked = false, overflow = false;
    if (r < P.n_rays) {
        NoCount none;
        Hit h{0u, 0.0, 0.0, 0.0};
        {
            const double2* q = P.rays + 4 * size_t(r);
            const double2 a = q[0], b = q[1], c = q[2], w = q[3];
            hit = trace<false, kG, kRayB>(P, D3{a.x, a.y, b.x}, D3{b.y, c.x, c.y}, stk, h, overflow, CallerRay64{w.x, w.y}, none);
        }
        if (P.hits) {
            ulonglong2 r0 = make_ulonglong2(0xffffffffull, 0ull), r1 = make_ulonglong2(0ull, 0ull);   // a miss: {-1, 0, 0.0, 0.0, 0.0}
            if (hit) {
                r0 = make_ulonglong2((unsigned long long)P.orig[h.slot], (unsigned long long)__double_as_longlong(h.t));
                r1 = make_ulonglong2((unsigned long long)__double_as_longlong(h.u), (unsigned long long)__double_as_longlong(h.v));
            }
            P.hits[2 * size_t(r)] = r0;
            P.hits[2 * size_t(r) + 1] = r1;
        }
        float col[3] = {0.f, 0.f, 0.f};                               // a miss: render.hpp:116-117
        if (hit) {                                                    // render.hpp:127-150
            const TriD tri = load_tri(P.tris + h.slot);
            const D3 p = hit_point<kG>(tri, normalizeG<kG>(tri.n), h.u, h.v);
            const D3 sun_line = normalizeG<kG>(d3(P.sun) - p);        // render.hpp:135
            Hit h2;
            blocked = trace<true, kG, kRayB>(P, p, sun_line, stk, h2, overflow, CamRay64{}, none);
            if (!blocked) {
                // the direction is read again from the ray record (L2-warm: this lane loaded it before
                // the walks) instead of being carried in six VGPRs across both of them
                const double2* q = P.rays + 4 * size_t(r);
                const double2 b = q[1], c = q[2];
                shade<kG>(sun_line, P.norms + 9 * size_t(P.orig[h.slot]), D3{b.y, c.x, c.y}, h.u, h.v, col);
            }
        }
        const double px[3] = {double(col[0]), double(col[1]), double(col[2])};
        if (P.pixels) {
            double* q = P.pixels + 3 * size_t(r);
            q[0] = px[0]; q[1] = px[1]; q[2] = px[2];
        }
        if (P.rgb8) {                                                 // ray order: a ray list has no rows to flip
            uint8_t* q = P.rgb8 + 3 * size_t(r);
            q[0] = quantize(px[0]); q[1] = quantize(px[1]); q[2] = quantize(px[2]);
        }
        if (P.status) P.status[r] = hit ? (blocked ? 2 : 1) : 0;
    }
    if (P.counters) {                                                 // wave-uniform
        const uint32_t nh = __popcll(__ballot(hit)), nb = __popcll(__ballot(blocked));
        if (lane == 0 && nh) {
            atomicAdd(&P.counters[0], (unsigned long long)nh);
            atomicAdd(&P.counters[1], (unsigned long long)(nh + nb));
            atomicAdd(&P.counters[3], (unsigned long long)nh);
        }
        if (blockIdx.x == 0 && lane == 0) {
            atomicAdd(&P.counters[0], (unsigned long long)launch_rays(P));
            atomicAdd(&P.counters[2], (unsigned long long)launch_rays(P));
        }
        if (overflow) atomicOr(&P.counters[6], 1ull);
    }
}

template <bool kG>
__global__ __launch_bounds__(kRayB) void ceres_shade_rays64_k(const ShadeParams64 P) { shade_rays64_body<kG>(P); }
template <bool kG>
__global__ __launch_bounds__(kRayB) void ceres_shade_rays64_idx_k(const Indexed<ShadeParams64> P) { shade_rays64_body<kG>(P); }

// ---------------------------------------------------------------- all-hits ray queries
// ceres_trace_rays_all_f64*: every hit in a caller's ray's window on a double scene -- what
// SingleRayTraverser::traverse (single_ray_traverser.hpp:68-126, Scalar = double) presents to an
// intersector whose distance() stays the ray's own tmax; the sibling of ceres_trace_all_k
// (render_hip.hip), whose comments state the semantics.  The walk is NOT trace() above with a fixed
// window: its box test picks each axis's entry / exit bound by the ray's octant, as
// NodeIntersector::intersect does (node_intersectors.hpp:35-47), instead of trace()'s min / max of
// the two fmas.  The two agree on every box with lo <= hi; an inverted box (a leaf whose triangles are
// all NaN on an axis) is a miss to the reference and to the pick and a hit to the min / max form, and
// the all-hits counters (tri_tests) are pinned to the reference's walk.  fmax / fmin nest as the
// reference's robust_max / robust_min do here: the innermost operand is the window bound, which
// CallerRay64 keeps free of NaN, so the running value never is one and a NaN slab is dropped.
//
// The kept hits of a lane are a sorted list of at most max_hits keys {t bits (64), leaf slot (32)} in
// LDS behind the stack: an 8-byte plane [entry][lane] of t, then a 4-byte plane [entry][lane] of
// slots -- 12 B per lane and entry, a wavefront's access to one entry of either plane is contiguous
// (ds_read_b64: 32 lanes x 8 B = one 256-B bank row; ds_write_b64: 16 lanes x 8 B = 32 banks; the
// dword plane likewise), so no access conflicts.  A key sorts by t (double <, so -0 == +0), equal t
// by ORIGINAL triangle index -- orig[] is read only when two t compare equal.  u and v are
// recomputed by the same tri_test when the row is written.
struct AllParams64 {
    const double2* rays;                         // n_rays x ray64
    ulonglong2* hits;                            // n_rays x max_hits hit32 (2 x 16 B each), ray-major (kKeep) or NULL
    uint32_t* counts;                            // n_rays x u32 or NULL
    unsigned long long* counters;                // 8 x u64 (zeroed before the launch) or NULL
    const SiblingPair64* pairs;
    const Tri96* tris;
    const uint32_t* orig;
    uint32_t n_rays, max_hits;
    uint32_t stack_entries, lds_entries;         // lds_entries = stack_entries + 1 stack slots, then the list
    uint32_t root_leaf_count, root_leaf_first;
};

// One lane's sorted list: entry i at t[i * kRayB] / slot[i * kRayB] (both already point at the lane's column).
struct HitList64 {
    static constexpr bool kSegments = false;     // (SegList64 below: the complete-list query's sink)
    unsigned long long* t;
    uint32_t* slot;
    uint32_t cap, n;                             // capacity (max_hits), entries held (<= cap)
    // a before b by the key; orig is read only on equal t
    __device__ __forceinline__ static bool before(double ta, uint32_t sa, double tb, uint32_t sb, const uint32_t* orig) {
        if (ta < tb) return true;
        if (ta == tb) return orig[sa] < orig[sb];
        return false;
    }
    __device__ __forceinline__ void insert(double tn, uint32_t sn, const uint32_t* orig) {
        uint32_t i = n;
        if (n == cap) {                                               // full: the last entry leaves, or the new key does
            if (!before(tn, sn, __longlong_as_double((long long)t[(cap - 1) * kRayB]), slot[(cap - 1) * kRayB], orig)) return;
            i = cap - 1;
        } else {
            ++n;
        }
        while (i > 0) {
            const unsigned long long pt = t[(i - 1) * kRayB];
            const uint32_t ps = slot[(i - 1) * kRayB];
            if (!before(tn, sn, __longlong_as_double((long long)pt), ps, orig)) break;
            t[i * kRayB] = pt;
            slot[i * kRayB] = ps;
            --i;
        }
        t[i * kRayB] = (unsigned long long)__double_as_longlong(tn);
        slot[i * kRayB] = sn;
    }
};

// One box of the fast node intersector with the bounds picked by the octant (nx / ny / nz: the
// inverse direction's sign bits; safe_inverse keeps the direction's, of +-0 too).
struct Slab64 { double ix, iy, iz, sx, sy, sz; bool nx, ny, nz; };
__device__ __forceinline__ bool box_pick(const Slab64& s, double2 X, double2 Y, double2 Z, double tmin, double tmax) {
    const double e = fmax(fma(s.nx ? X.y : X.x, s.ix, s.sx), fmax(fma(s.ny ? Y.y : Y.x, s.iy, s.sy), fmax(fma(s.nz ? Z.y : Z.x, s.iz, s.sz), tmin)));
    const double x = fmin(fma(s.nx ? X.x : X.y, s.ix, s.sx), fmin(fma(s.ny ? Y.x : Y.y, s.iy, s.sy), fmin(fma(s.nz ? Z.x : Z.y, s.iz, s.sz), tmax)));
    return e <= x;
}

// The fixed-window walk; returns the size of the hit set.  kKeep: accepted triangles enter `list`.
// With a fixed window neither the set nor the steps / tests depend on the visiting order: the walk
// goes left and pushes right.  The stack index is clamped (slot stack_entries is a spare one) with an
// overflow flag, every lane loads the next record, and that load is issued before this step's triangle
// tests (it follows from the box tests alone) -- as ceres_trace_all_k's walk.
template <bool kStats, bool kG, bool kKeep, class PT, class ListT>
__device__ __forceinline__ uint32_t trace_all(const PT& P, D3 o, D3 d, uint32_t* stk, ListT& list, uint32_t& n_pairs,
                                              uint32_t& n_tests, bool& overflow, CallerRay64 rk) {
    constexpr int kS = kRayB;
    const double tmin = rk.tmin(), tmax = rk.tmax();                  // never changed
    uint32_t count = 0;
    if (P.root_leaf_count) {                                          // root is a leaf, :72-73
        if (kStats) n_tests += P.root_leaf_count;
        for (uint32_t k = P.root_leaf_first; k < P.root_leaf_first + P.root_leaf_count; ++k) {
            double t, u, v;
            if (tri_test<kG>(load_tri(P.tris + k), o, d, tmin, tmax, t, u, v)) {
                if constexpr (ListT::kSegments) list.accept(count, t, u, v, k, P.orig);
                ++count;
                if (kKeep) list.insert(t, k, P.orig);
            }
        }
        return count;
    }
    auto safe_inv = [](double x) { return 1.0 / (fabs(x) < DBL_EPSILON ? copysign(DBL_EPSILON, x) : x); };   // vector.hpp:69-74
    Slab64 sl;
    sl.ix = safe_inv(d.x); sl.iy = safe_inv(d.y); sl.iz = safe_inv(d.z);
    sl.sx = (-o.x) * sl.ix; sl.sy = (-o.y) * sl.iy; sl.sz = (-o.z) * sl.iz;
    sl.nx = __double2hiint(sl.ix) < 0; sl.ny = __double2hiint(sl.iy) < 0; sl.nz = __double2hiint(sl.iz) < 0;
    uint32_t sp = 0;
    const double2* q = reinterpret_cast<const double2*>(P.pairs);     // pair of the root's children (:81)
    double2 A = q[0], B = q[1], C = q[2], D = q[3], E = q[4], F = q[5];
    uint4 L = reinterpret_cast<const uint4*>(q)[6];
    while (true) {                                                    // :82-123
        if (kStats) ++n_pairs;
        const uint32_t top = stk[(sp ? sp - 1 : 0) * kS];             // popped if this step descends nowhere
        const bool hit_l = box_pick(sl, A, B, C, tmin, tmax), hit_r = box_pick(sl, D, E, F, tmin, tmax);
        const bool go_l = hit_l && !L.x, go_r = hit_r && !L.z;
        const bool both = go_l && go_r, none = !go_l && !go_r;
        const bool done = none && sp == 0;                            // :118-121
        const uint32_t nxt = go_l ? L.y : (go_r ? L.w : top);         // left first, the right child waits
        overflow |= both && sp >= P.stack_entries;
        stk[(sp < P.stack_entries ? sp : P.stack_entries) * kS] = L.w;   // a free slot unless this step pushes
        sp = both ? (sp < P.stack_entries ? sp + 1 : sp) : (none ? (sp ? sp - 1 : 0) : sp);
        const uint32_t nl = hit_l ? L.x : 0u, nr = hit_r ? L.z : 0u;
        const uint32_t n_leaf = nl + nr, k2 = L.w - nl;
        if (kStats) n_tests += n_leaf;
        const double2* nq = reinterpret_cast<const double2*>(P.pairs + (done ? 0u : nxt));   // a done lane: the root's pair, cached
        const double2 nA = nq[0], nB = nq[1], nC = nq[2], nD = nq[3], nE = nq[4], nF = nq[5];
        const uint4 nL = reinterpret_cast<const uint4*>(nq)[6];
        for (uint32_t j = 0; j < n_leaf; ++j) {                       // left leaf then right leaf, one loop
            const uint32_t idx = (j < nl ? L.y : k2) + j;
            double t, u, v;
            if (tri_test<kG>(load_tri(P.tris + idx), o, d, tmin, tmax, t, u, v)) {
                if constexpr (ListT::kSegments) list.accept(count, t, u, v, idx, P.orig);
                ++count;
                if (kKeep) list.insert(t, idx, P.orig);
            }
        }
        if (done) break;
        A = nA; B = nB; C = nC; D = nD; E = nE; F = nF; L = nL;
    }
    return count;
}

// The two 16-byte halves of a hit32 record {int32 prim, uint32 0, double t, u, v}.
__device__ __forceinline__ ulonglong2 hit32_lo(uint32_t prim, unsigned long long t_bits) { return make_ulonglong2((unsigned long long)prim, t_bits); }
__device__ __forceinline__ ulonglong2 hit32_hi(double u, double v) {
    return make_ulonglong2((unsigned long long)__double_as_longlong(u), (unsigned long long)__double_as_longlong(v));
}

// ceres_trace_rays64_k's launch shape: one ray per lane, 64 consecutive rays per single-wavefront
// workgroup, idle tail lanes run nothing, the u32 stack in LDS [entry][lane].  kKeep = false is the
// count-only query: no hit buffer, no LDS beyond the stack.  kKeep = true: rows of max_hits hit32
// records, ray-major, written as 16-byte halves -- each lane its kept hits in key order, the wavefront
// together the misses {-1, 0, 0.0, 0.0, 0.0} behind them.
// counters: {rays, rays with count >= 1, rays, 0, node_pairs, tri_tests, stack overflow, 0}.
template <bool kStats, bool kG, bool kKeep, class PT>
__device__ __forceinline__ void trace_all64_body(const PT& P) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const uint32_t lane = threadIdx.x;
    uint32_t* stk = lds + lane;
    HitList64 list{nullptr, nullptr, 0u, 0u};
    if constexpr (kKeep) {                                            // lds_entries * 256 B of stack, then the two planes
        uint8_t* base = reinterpret_cast<uint8_t*>(lds) + size_t(P.lds_entries) * kRayB * 4;
        list = HitList64{reinterpret_cast<unsigned long long*>(base) + lane,
                         reinterpret_cast<uint32_t*>(base + size_t(P.max_hits) * kRayB * 8) + lane, P.max_hits, 0u};
    }
    const uint32_t r = lane_ray(P, blockIdx.x * uint32_t(kRayB) + lane);   // n_rays < 2^31 (host-checked)
    bool overflow = false;
    uint32_t n_pairs = 0, n_tests = 0, count = 0;
    if (r < P.n_rays) {
        const double2* q = P.rays + 4 * size_t(r);
        const double2 a = q[0], b = q[1], c = q[2], w = q[3];
        const D3 o{a.x, a.y, b.x}, d{b.y, c.x, c.y};
        const CallerRay64 rk{w.x, w.y};
        count = trace_all<kStats, kG, kKeep>(P, o, d, stk, list, n_pairs, n_tests, overflow, rk);
        if (P.counts) P.counts[r] = count;
        if constexpr (kKeep) {                                        // the kept hits: each lane its own, few per ray
            ulonglong2* row = P.hits + 2 * size_t(r) * P.max_hits;
            for (uint32_t i = 0; i < list.n; ++i) {
                const unsigned long long tb = list.t[i * kRayB];
                const uint32_t slot = list.slot[i * kRayB];
                double t, u, v;
                (void)tri_test<kG>(load_tri(P.tris + slot), o, d, rk.tmin(), rk.tmax(), t, u, v);
                row[2 * i] = hit32_lo(P.orig[slot], tb);
                row[2 * i + 1] = hit32_hi(u, v);
            }
            // an indexed launch's rows are wherever the list points: each lane fills the rest of its own
            if constexpr (is_indexed<PT>::value)
                for (uint32_t i = list.n; i < P.max_hits; ++i) {
                    row[2 * i] = make_ulonglong2(0xffffffffull, 0ull);
                    row[2 * i + 1] = make_ulonglong2(0ull, 0ull);
                }
        }
    }
    if constexpr (kKeep && !is_indexed<PT>::value) {
        // The miss fill, the bulk of the rows: the wavefront's 64 rows are one contiguous block of 64 x
        // max_hits records = twice as many 16-byte pieces, which the lanes fill side by side (piece j:
        // record j / 2, its first half {-1, 0 | t = 0.0} or its second {u = 0.0, v = 0.0}; ray = record /
        // max_hits, a miss where record % max_hits is past that ray's kept hits) -- 1 KB per store
        // instruction.  Every lane runs every trip (the shuffle reads other lanes' list lengths; idle
        // tail lanes hold 0 and their rows lie outside `total`).
        const uint32_t first_ray = blockIdx.x * uint32_t(kRayB);
        const uint32_t total = (P.n_rays - first_ray < uint32_t(kRayB) ? P.n_rays - first_ray : uint32_t(kRayB)) * P.max_hits * 2u;
        ulonglong2* block_rows = P.hits + 2 * size_t(first_ray) * P.max_hits;
        const float inv_k = 1.0f / float(P.max_hits);
        for (uint32_t j0 = 0; j0 < uint32_t(kRayB) * P.max_hits * 2u; j0 += kRayB) {
            const uint32_t j = j0 + lane, rec = j >> 1;
            // rec < 2048, max_hits <= 32: (rec + 0.5) / max_hits is at least 1 / 64 from an integer, far beyond the rounding
            const uint32_t ray = uint32_t((float(rec) + 0.5f) * inv_k);
            const uint32_t kept = uint32_t(__shfl(int(list.n), int(ray & (kRayB - 1)), 64));
            if (j < total && rec - ray * P.max_hits >= kept) block_rows[j] = make_ulonglong2((j & 1u) ? 0ull : 0xffffffffull, 0ull);
        }
    }
    if (P.counters) {                                                 // wave-uniform
        const uint32_t nh = __popcll(__ballot(count != 0));
        if (lane == 0 && nh) atomicAdd(&P.counters[1], (unsigned long long)nh);
        if (kStats) {
            const uint32_t wp = wave_sum(n_pairs), wt = wave_sum(n_tests);
            if (lane == 0) {
                atomicAdd(&P.counters[4], (unsigned long long)wp);
                atomicAdd(&P.counters[5], (unsigned long long)wt);
            }
        }
        if (blockIdx.x == 0 && lane == 0) {
            atomicAdd(&P.counters[0], (unsigned long long)launch_rays(P));
            atomicAdd(&P.counters[2], (unsigned long long)launch_rays(P));
        }
        if (overflow) atomicOr(&P.counters[6], 1ull);
    }
}

template <bool kStats, bool kG, bool kKeep>
__global__ __launch_bounds__(kRayB) void ceres_trace_all64_k(const AllParams64 P) { trace_all64_body<kStats, kG, kKeep>(P); }
template <bool kG, bool kKeep>
__global__ __launch_bounds__(kRayB) void ceres_trace_all64_idx_k(const Indexed<AllParams64> P) { trace_all64_body<false, kG, kKeep>(P); }

// ---------------------------------------------------------------- complete hit lists
// ceres_trace_rays_lists_f64*: the same hit sets without a cap, as a CSR pair; the sibling of
// ceres_trace_lists_k (render_hip.hip).  Every lane knows the length n_k of its segment
// [offsets[r], offsets[r + 1]) before it walks:
//   n_k = 0      no walk at all;
//   n_k <= L     HitList64 with capacity min(n_k, L) behind the stack, written out in key order;
//   n_k >  L     every accepted hit goes straight to the segment as a full hit32 record, in WALK order
//                (its position clamped to the segment); ceres_sort_lists64_k orders it afterwards.
// No store leaves [offsets[r], min(offsets[r + 1], capacity)).  A lane that finds another number of
// hits than n_k raises counters[7].
// counters: {rays, rays with a non-empty segment, rays, records written, node_pairs, tri_tests,
// stack overflow, segment mismatch}.
struct ListParams64 {
    const double2* rays;                         // n_rays x ray64
    const unsigned long long* offsets;           // n_rays + 1
    ulonglong2* hits;                            // `capacity` hit32 records (NULL only with capacity 0)
    unsigned long long capacity;
    unsigned long long* counters;                // 8 x u64 (zeroed before the launch) or NULL
    const SiblingPair64* pairs;
    const Tri96* tris;
    const uint32_t* orig;
    uint32_t n_rays, list_entries;               // list_entries = L
    uint32_t stack_entries, lds_entries;         // as AllParams64
    uint32_t root_leaf_count, root_leaf_first;
};

// trace_all's sink for one lane: the LDS list, or (seg != NULL) the lane's own segment.
struct SegList64 {
    static constexpr bool kSegments = true;
    HitList64 lds;
    ulonglong2* seg;
    uint32_t room, written;                      // records of the segment below `capacity`; stores done
    __device__ __forceinline__ void accept(uint32_t pos, double t, double u, double v, uint32_t slot, const uint32_t* orig) {
        if (seg) {
            if (pos < room) {
                seg[2 * size_t(pos)] = hit32_lo(orig[slot], (unsigned long long)__double_as_longlong(t));
                seg[2 * size_t(pos) + 1] = hit32_hi(u, v);
                ++written;
            }
        } else {
            lds.insert(t, slot, orig);
        }
    }
    __device__ __forceinline__ void insert(double, uint32_t, const uint32_t*) {}
};

template <bool kStats, bool kG, class PT>
__device__ __forceinline__ void trace_lists64_body(const PT& P) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const uint32_t lane = threadIdx.x;
    uint32_t* stk = lds + lane;
    const uint32_t r = lane_ray(P, blockIdx.x * uint32_t(kRayB) + lane);   // n_rays < 2^31 (host-checked)
    unsigned long long b = 0, e = 0;
    if (r < P.n_rays) { b = P.offsets[r]; e = P.offsets[size_t(r) + 1]; }
    const uint32_t n_k = e > b ? uint32_t(e - b < 0xffffffffull ? e - b : 0xffffffffull) : 0u;
    bool overflow = false, mismatch = false;
    uint32_t n_pairs = 0, n_tests = 0, written = 0;
    if (n_k) {
        const unsigned long long lo = b < P.capacity ? b : P.capacity, hi = e < P.capacity ? e : P.capacity;
        uint8_t* base = reinterpret_cast<uint8_t*>(lds) + size_t(P.lds_entries) * kRayB * 4;
        SegList64 list;
        list.lds = HitList64{reinterpret_cast<unsigned long long*>(base) + lane,
                             reinterpret_cast<uint32_t*>(base + size_t(P.list_entries) * kRayB * 8) + lane,
                             n_k < P.list_entries ? n_k : P.list_entries, 0u};
        list.room = uint32_t(hi - lo < 0xffffffffull ? hi - lo : 0xffffffffull);
        list.written = 0;
        ulonglong2* seg = P.hits + 2 * lo;                            // never dereferenced when room = 0
        list.seg = n_k > P.list_entries ? seg : nullptr;
        const double2* q = P.rays + 4 * size_t(r);
        const double2 a = q[0], bb = q[1], c = q[2], w = q[3];
        const D3 o{a.x, a.y, bb.x}, d{bb.y, c.x, c.y};
        const CallerRay64 rk{w.x, w.y};
        const uint32_t count = trace_all<kStats, kG, false>(P, o, d, stk, list, n_pairs, n_tests, overflow, rk);
        mismatch = count != n_k;
        written = list.written;
        if (!list.seg) {
            const uint32_t m = list.lds.n < list.room ? list.lds.n : list.room;
            for (uint32_t i = 0; i < m; ++i) {
                const unsigned long long tb = list.lds.t[i * kRayB];
                const uint32_t slot = list.lds.slot[i * kRayB];
                double t, u, v;
                (void)tri_test<kG>(load_tri(P.tris + slot), o, d, rk.tmin(), rk.tmax(), t, u, v);
                seg[2 * i] = hit32_lo(P.orig[slot], tb);
                seg[2 * i + 1] = hit32_hi(u, v);
            }
            written = m;
        }
    }
    if (P.counters) {                                                 // wave-uniform
        const uint32_t nh = __popcll(__ballot(n_k != 0));
        if (nh) {
            const uint32_t ww = wave_sum(written);
            if (lane == 0) {
                atomicAdd(&P.counters[1], (unsigned long long)nh);
                if (ww) atomicAdd(&P.counters[3], (unsigned long long)ww);
            }
            if (kStats) {
                const uint32_t wp = wave_sum(n_pairs), wt = wave_sum(n_tests);
                if (lane == 0) {
                    atomicAdd(&P.counters[4], (unsigned long long)wp);
                    atomicAdd(&P.counters[5], (unsigned long long)wt);
                }
            }
        }
        if (blockIdx.x == 0 && lane == 0) {
            atomicAdd(&P.counters[0], (unsigned long long)launch_rays(P));
            atomicAdd(&P.counters[2], (unsigned long long)launch_rays(P));
        }
        if (overflow) atomicOr(&P.counters[6], 1ull);
        if (mismatch) atomicOr(&P.counters[7], 1ull);
    }
}

template <bool kStats, bool kG>
__global__ __launch_bounds__(kRayB) void ceres_trace_lists64_k(const ListParams64 P) { trace_lists64_body<kStats, kG>(P); }
template <bool kG>
__global__ __launch_bounds__(kRayB) void ceres_trace_lists64_idx_k(const Indexed<ListParams64> P) { trace_lists64_body<false, kG>(P); }

// The segments longer than L, put into key order -- ceres_sort_lists_k's ascending-only bitonic network
// (render_hip.hip: records at and past n stand for +inf, so any n works in place) over 32-byte records.
// The key is t's 64 bits mapped so that unsigned < is double < (-0 first made +0), then the original
// triangle index; keys are unique.  A record moves as its two 16-byte halves, both by the lane that
// compared it and between the same two barriers, so no other lane sees half a swap.  A segment of at
// most sort_cap records is sorted in LDS (32 B per record) and written back; a longer one in place in
// global memory, where the workgroup-scope fence of each round's barrier orders the wavefront's own
// stores and loads.  Segments not wholly below `capacity` are left alone.
struct SortParams64 {
    const unsigned long long* offsets;
    ulonglong2* hits;
    unsigned long long capacity;
    uint32_t n_rays, list_entries, sort_cap;
};

__device__ __forceinline__ bool hit32_before(ulonglong2 a, ulonglong2 b) {   // the first halves of two records
    auto key = [](unsigned long long tb) {
        if (tb == 0x8000000000000000ull) tb = 0ull;
        return (tb >> 63) ? ~tb : (tb | 0x8000000000000000ull);
    };
    const unsigned long long ka = key(a.y), kb = key(b.y);
    return ka < kb || (ka == kb && uint32_t(a.x) < uint32_t(b.x));
}

__device__ __forceinline__ void sort_records64(ulonglong2* a, uint32_t n, uint32_t lane) {   // 2 <= n <= 2^31, wave-uniform
    unsigned long long N = 2;
    while (N < n) N <<= 1;
    const uint32_t half = uint32_t(N >> 1);
    for (unsigned long long k = 2; k <= N; k <<= 1) {
        for (uint32_t j = uint32_t(k >> 1); j > 0; j >>= 1) {
            for (uint32_t c = lane; c < half; c += 64) {
                const uint32_t i = ((c & ~(j - 1)) << 1) | (c & (j - 1));
                if (i >= n) break;                                    // i grows with c, and its partner lies above it
                const uint32_t h = j == uint32_t(k >> 1) ? i ^ uint32_t(k - 1) : i | j;
                if (h < n) {
                    const ulonglong2 x0 = a[2 * size_t(i)], y0 = a[2 * size_t(h)];
                    if (hit32_before(y0, x0)) {
                        const ulonglong2 x1 = a[2 * size_t(i) + 1], y1 = a[2 * size_t(h) + 1];
                        a[2 * size_t(i)] = y0; a[2 * size_t(i) + 1] = y1;
                        a[2 * size_t(h)] = x0; a[2 * size_t(h) + 1] = x1;
                    }
                }
            }
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(64) void ceres_sort_lists64_k(const SortParams64 P) {
    extern __shared__ __attribute__((aligned(16))) ulonglong2 sort_buf64[];
    const uint32_t lane = threadIdx.x, first = blockIdx.x * 64u;
    const uint32_t r = first + lane;
    unsigned long long b = 0, e = 0;
    if (r < P.n_rays) { b = P.offsets[r]; e = P.offsets[size_t(r) + 1]; }
    unsigned long long todo = __ballot(e > b && e - b > P.list_entries && e - b <= (1ull << 31) && e <= P.capacity);
    while (todo) {                                                    // wave-uniform
        const uint32_t i = uint32_t(__ffsll(todo)) - 1u;
        todo &= todo - 1;
        const unsigned long long sb = P.offsets[first + i], se = P.offsets[size_t(first + i) + 1];
        const uint32_t n = uint32_t(se - sb);
        ulonglong2* seg = P.hits + 2 * sb;
        if (n < 2) continue;
        if (n <= P.sort_cap) {
            for (uint32_t k = lane; k < 2 * n; k += 64) sort_buf64[k] = seg[k];
            __syncthreads();
            sort_records64(sort_buf64, n, lane);
            for (uint32_t k = lane; k < 2 * n; k += 64) seg[k] = sort_buf64[k];
            __syncthreads();
        } else {
            sort_records64(seg, n, lane);
        }
    }
}

}  // namespace dev64
}  // namespace ceres

using namespace ceres;
using namespace ceres::dev64;

namespace {

// one render into device buffers; counters summed from the shards on the host
int render64(ceres_scene* s, const double basis12[12], const double sun[3], int mode, size_t W, size_t H, double* d_px,
             uint8_t* d_rgb, int32_t* d_prim, double* d_tuv, int8_t* d_sh, ceres_stats* st) {
    if (!s || !basis12 || !sun) return set_error(CERES_EINVAL, "ceres_render_f64: null argument");
    if (!s->f64) return set_error(CERES_EINVAL, "scene is single precision: use ceres_render_f32");
    const bool gfma = (mode & CERES_MODE_FMA) != 0;                 // the reference CMake build's FMA contraction
    mode &= ~CERES_MODE_FMA;
    if (mode != CERES_MODE_FULL && mode != CERES_MODE_PRIMARY) return set_error(CERES_EINVAL, "bad mode %d", mode);
    if (W == 0 || H == 0 || W > 65535u * kTile || H > 65535u * kTile) return set_error(CERES_EINVAL, "bad frame size %zux%zu", W, H);
    HIP_TRY(hipSetDevice(s->device));
    KParams64 P{};
    std::memcpy(P.cam.eye, basis12, 3 * sizeof(double));
    std::memcpy(P.cam.dir, basis12 + 3, 3 * sizeof(double));
    std::memcpy(P.cam.iu, basis12 + 6, 3 * sizeof(double));
    std::memcpy(P.cam.iv, basis12 + 9, 3 * sizeof(double));
    std::memcpy(P.cam.sun, sun, 3 * sizeof(double));
    P.W = uint32_t(W); P.H = uint32_t(H);
    scene_params(P, s);
    P.norms = s->d_norms64;
    P.pixels = d_px; P.rgb8 = d_rgb; P.shards = s->d_shards;
    P.rec_prim = d_prim; P.rec_tuv = d_tuv; P.rec_shadow = d_sh;
    EventPair ev;                                                   // destroyed on every return
    hipEvent_t &e0 = ev.e0, &e1 = ev.e1;
    HIP_TRY(hipEventCreate(&e0));
    HIP_TRY(hipEventCreate(&e1));
    HIP_TRY(hipMemsetAsync(s->d_shards, 0, sizeof(Shard) * kShards, s->stream));
    s->shards_dirty = true;
    const uint32_t tx = (uint32_t(W) + kTile - 1) / kTile, ty = (uint32_t(H) + kTile - 1) / kTile;
    if (int rc = frame_tile_order(s, W, H, kTile, s->stream, &P.tile_order)) return rc;
    P.tiles_x = tx;
    const dim3 grid(tx * ty), block(kBlock);
    const size_t lds = size_t(s->stack_entries) * kBlock * 4;
    HIP_TRY(hipEventRecord(e0, s->stream));
    if (mode == CERES_MODE_PRIMARY && gfma) hipLaunchKernelGGL((ceres_render64<CERES_MODE_PRIMARY, true>), grid, block, lds, s->stream, P);
    else if (mode == CERES_MODE_PRIMARY) hipLaunchKernelGGL((ceres_render64<CERES_MODE_PRIMARY, false>), grid, block, lds, s->stream, P);
    else if (gfma) hipLaunchKernelGGL((ceres_render64<CERES_MODE_FULL, true>), grid, block, lds, s->stream, P);
    else hipLaunchKernelGGL((ceres_render64<CERES_MODE_FULL, false>), grid, block, lds, s->stream, P);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(e1, s->stream));
    std::vector<Shard> sh(kShards);
    HIP_TRY(hipMemcpyAsync(sh.data(), s->d_shards, sizeof(Shard) * kShards, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e0, e1);
    uint64_t shadow = 0, hits = 0;
    uint32_t err = 0;
    for (const Shard& x : sh) { shadow += x.queued; hits += x.hits; err |= x.error; }
    if (st) {
        st->primary_rays = uint64_t(W) * H; st->shadow_rays = shadow;
        st->rays = st->primary_rays + shadow; st->hits = hits;
        st->node_pairs = st->tri_tests = 0; st->ms = ms;
    }
    if (err) return set_error(CERES_ESTACK, "traversal stack overflow");
    return CERES_OK;
}

}  // namespace

extern "C" {

// Scene for render<double>: the reference's own double arrays (Triangle<double>[], tri_norms,
// Bvh<double> nodes + primitive_indices), re-laid as double sibling pairs in depth-first order.
ceres_scene* ceres_scene_create_f64(const double* tri96, size_t n_tri, const double* norm72, const void* nodes64,
                                    size_t n_nodes, const uint64_t* prim64, int device, uint32_t flags) {
    if (!tri96 || !norm72 || !nodes64 || !prim64 || n_tri == 0 || n_nodes == 0) {
        set_error(CERES_EINVAL, "ceres_scene_create_f64: empty scene or null argument");
        return nullptr;
    }
    if (n_tri > 0xffffffffull || n_nodes > 0xffffffffull) { set_error(CERES_EUNSUPPORTED, "scene too large"); return nullptr; }
    std::vector<SiblingPair64> pairs;
    std::vector<Tri96> leaf;
    std::vector<uint32_t> orig;
    uint32_t depth = 0, rlc = 0, rlf = 0;
    if (relayout_bvh64(static_cast<const RefNode64*>(nodes64), n_nodes, prim64, n_tri, reinterpret_cast<const Tri96*>(tri96),
                       pairs, leaf, orig, depth, rlc, rlf))
        return nullptr;
    auto* s = new (std::nothrow) ceres_scene;
    if (!s) { set_error(CERES_ENOMEM, "out of host memory"); return nullptr; }
    s->f64 = true;
    s->device = device; s->flags = flags; s->n_tri = n_tri; s->n_pairs = pairs.size();
    s->depth = depth; s->root_leaf_count = rlc; s->root_leaf_first = rlf;
    s->stack_entries = std::max<uint32_t>(1, depth);
    scene_set_list_constants(s);
    auto fail = [&]() -> ceres_scene* { scene_release(s); delete s; return nullptr; };
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { set_error(CERES_EHIP, "no HIP device available"); return fail(); }
    if (device < 0 || device >= ndev) { set_error(CERES_EINVAL, "device %d out of range (%d devices)", device, ndev); return fail(); }
    auto body = [&]() -> int {
        HIP_TRY(hipSetDevice(device));
        hipDeviceProp_t prop;
        HIP_TRY(hipGetDeviceProperties(&prop, device));
        if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
            return set_error(CERES_EHIP, "device %d is %s, this build targets gfx950 only", device, prop.gcnArchName);
        s->num_cus = prop.multiProcessorCount;
        s->max_lds_per_block = prop.sharedMemPerBlock;
        HIP_TRY(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
        HIP_TRY(hipMalloc(&s->d_counters, 8 * sizeof(uint64_t)));   // ceres_trace_rays_f64
        HIP_TRY(hipMalloc(&s->d_pairs64, pairs.size() * sizeof(SiblingPair64)));
        HIP_TRY(hipMalloc(&s->d_tris64, n_tri * sizeof(Tri96)));
        HIP_TRY(hipMalloc(&s->d_orig, n_tri * sizeof(uint32_t)));
        HIP_TRY(hipMalloc(&s->d_norms64, n_tri * 72));
        HIP_TRY(hipMalloc(&s->d_shards, sizeof(Shard) * kShards));
        HIP_TRY(hipMemcpy(s->d_pairs64, pairs.data(), pairs.size() * sizeof(SiblingPair64), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(s->d_tris64, leaf.data(), n_tri * sizeof(Tri96), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(s->d_orig, orig.data(), n_tri * sizeof(uint32_t), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(s->d_norms64, norm72, n_tri * 72, hipMemcpyHostToDevice));
        return CERES_OK;
    };
    if (body()) return fail();
    return s;
}

// render<double>() with host buffers (render.hpp:86-156, Scalar = double): pixels (3*W*H
// doubles, bottom row first) and/or the RGB8 PPM body; rays/hits in stats.
int ceres_render_f64(ceres_scene* s, const double basis12[12], const double sun[3], int mode, double* pixels,
                     uint8_t* rgb8, size_t W, size_t H, ceres_stats* stats) {
    if (!s) return set_error(CERES_EINVAL, "null scene");
    HIP_TRY(hipSetDevice(s->device));
    const size_t n = W * H;
    double* dp = nullptr;
    uint8_t* dr = nullptr;
    auto cleanup = [&] { dfree(dp); dfree(dr); };
    if ((pixels && hipMalloc(&dp, n * 24) != hipSuccess) || (rgb8 && hipMalloc(&dr, n * 3) != hipSuccess)) {
        cleanup();
        return set_error(CERES_ENOMEM, "ceres_render_f64: device allocation failed");
    }
    int rc = render64(s, basis12, sun, mode, W, H, dp, dr, nullptr, nullptr, nullptr, stats);
    if (!rc && ((pixels && hipMemcpy(pixels, dp, n * 24, hipMemcpyDeviceToHost) != hipSuccess) ||
                (rgb8 && hipMemcpy(rgb8, dr, n * 3, hipMemcpyDeviceToHost) != hipSuccess)))
        rc = set_error(CERES_EHIP, "ceres_render_f64: copy back failed");
    cleanup();
    return rc;
}

// Per-pixel hit records of render<double> (pixel = j*W + i): original triangle (-1 on a miss),
// t / u / v (double), shadow (-1 none, 0 lit, 1 occluded).
int ceres_render_records_f64(ceres_scene* s, const double basis12[12], const double sun[3], int mode, size_t W, size_t H,
                             int32_t* prim, double* tuv, int8_t* shadow, ceres_stats* stats) {
    if (!s || !prim || !tuv || !shadow) return set_error(CERES_EINVAL, "ceres_render_records_f64: null argument");
    HIP_TRY(hipSetDevice(s->device));
    const size_t n = W * H;
    int32_t* dp = nullptr;
    double* dt = nullptr;
    int8_t* ds = nullptr;
    auto cleanup = [&] { dfree(dp); dfree(dt); dfree(ds); };
    if (hipMalloc(&dp, n * 4) != hipSuccess || hipMalloc(&dt, n * 24) != hipSuccess || hipMalloc(&ds, n) != hipSuccess) {
        cleanup();
        return set_error(CERES_ENOMEM, "ceres_render_records_f64: device allocation failed");
    }
    int rc = render64(s, basis12, sun, mode, W, H, nullptr, nullptr, dp, dt, ds, stats);
    if (!rc && (hipMemcpy(prim, dp, n * 4, hipMemcpyDeviceToHost) != hipSuccess ||
                hipMemcpy(tuv, dt, n * 24, hipMemcpyDeviceToHost) != hipSuccess ||
                hipMemcpy(shadow, ds, n, hipMemcpyDeviceToHost) != hipSuccess))
        rc = set_error(CERES_EHIP, "ceres_render_records_f64: copy back failed");
    cleanup();
    return rc;
}

}  // extern "C"

// Ray queries on a double scene (dev64::ceres_trace_rays64_k).  The argument rules the two GPU calls
// share (ceres_render.h): a negative ceres_status when the call is refused, 1 when there is nothing
// to trace (n_rays = 0), 0 when there is.
static int check_trace64_args(const ceres_scene* s, const void* rays, size_t n_rays, int mode, const void* hits,
                              const void* occluded) {
    if (!s) return set_error(CERES_EINVAL, "ceres_trace_rays_f64: null scene");
    if (!s->f64) return set_error(CERES_EUNSUPPORTED, "ceres_trace_rays_f64: the scene is single precision (use ceres_trace_rays)");
    if (mode & ~(CERES_MODE_FMA | CERES_MODE_ROBUST))
        return set_error(CERES_EINVAL, "ceres_trace_rays_f64: bad mode %d (0 or CERES_MODE_FMA)", mode);
    if (mode & CERES_MODE_ROBUST) return set_error(CERES_EUNSUPPORTED, "ceres_trace_rays_f64: CERES_MODE_ROBUST takes float scenes");
    if (!hits && !occluded) return set_error(CERES_EINVAL, "ceres_trace_rays_f64: neither hits nor occluded asked for");
    if (n_rays >= (size_t(1) << 31)) return set_error(CERES_EUNSUPPORTED, "ceres_trace_rays_f64: %zu rays (below 2^31 per call)", n_rays);
    if (n_rays == 0) return 1;
    if (!rays) return set_error(CERES_EINVAL, "ceres_trace_rays_f64: null rays");
    return 0;
}

extern "C" {

// The plain call and the indexed one (indexed: lane i takes ray d_index[i], indexed_params.hpp): the
// same refusals and parameter block; the list's own refusals come last, before any launch.
static int trace_rays64_launch(ceres_scene* s, const void* d_rays64, size_t n_rays, const uint32_t* d_index, size_t n_index,
                               bool indexed, int mode, void* d_hits32, uint8_t* d_occluded, uint64_t* d_counters, void* stream_) {
    if (const int chk = check_trace64_args(s, d_rays64, n_rays, mode, d_hits32, d_occluded)) return chk < 0 ? chk : CERES_OK;
    if ((reinterpret_cast<uintptr_t>(d_rays64) | reinterpret_cast<uintptr_t>(d_hits32)) & 15u)
        return set_error(CERES_EINVAL, "ceres_trace_rays_f64: rays and hits must be 16-byte aligned");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    HIP_TRY(hipSetDevice(s->device));
    Indexed<RayParams64> P{};
    P.index = d_index; P.n_index = uint32_t(n_index);
    P.rays = static_cast<const double2*>(d_rays64);
    P.hits = static_cast<ulonglong2*>(d_hits32);
    P.occluded = d_occluded;
    P.counters = reinterpret_cast<unsigned long long*>(d_counters);
    scene_params(P, s);
    P.n_rays = uint32_t(n_rays);
    const size_t lds = size_t(s->stack_entries) * kRayB * 4;          // u32 [entry][lane]
    if (lds > s->max_lds_per_block)
        return set_error(CERES_EINVAL, "ceres_trace_rays_f64: a traversal stack of %u entries needs %zu B of LDS per workgroup "
                         "(%zu available)", s->stack_entries, lds, s->max_lds_per_block);
    if (indexed)
        if (const int chk = check_index_list("ceres_trace_rays_f64_indexed", s, d_index, n_index)) return chk < 0 ? chk : CERES_OK;
    if (d_counters) HIP_TRY(hipMemsetAsync(d_counters, 0, 8 * sizeof(uint64_t), stream));
    const dim3 grid(uint32_t(((indexed ? n_index : n_rays) + kRayB - 1) / kRayB)), block(kRayB);
    const bool stats = (s->flags & CERES_SCENE_STATS) != 0, gfma = (mode & CERES_MODE_FMA) != 0;
    const RayParams64& P0 = P;                                        // the plain kernels' block
    dispatch_bools([&](auto st, auto gt) {
        constexpr bool S = decltype(st)::value, G = decltype(gt)::value;
        if constexpr (!S) {                                           // a stats scene has no indexed kernel
            if (indexed) { hipLaunchKernelGGL((ceres_trace_rays64_idx_k<G>), grid, block, lds, stream, P); return; }
        }
        hipLaunchKernelGGL((ceres_trace_rays64_k<S, G>), grid, block, lds, stream, P0);
    }, stats, gfma);
    HIP_TRY(hipGetLastError());
    return CERES_OK;
}

int ceres_trace_rays_f64_device(ceres_scene* s, const void* d_rays64, size_t n_rays, int mode, void* d_hits32,
                                uint8_t* d_occluded, uint64_t* d_counters, void* stream) {
    return trace_rays64_launch(s, d_rays64, n_rays, nullptr, 0, false, mode, d_hits32, d_occluded, d_counters, stream);
}

int ceres_trace_rays_f64_indexed_device(ceres_scene* s, const void* d_rays64, size_t n_rays, const uint32_t* d_index, size_t n_index,
                                        int mode, void* d_hits32, uint8_t* d_occluded, uint64_t* d_counters, void* stream) {
    return trace_rays64_launch(s, d_rays64, n_rays, d_index, n_index, true, mode, d_hits32, d_occluded, d_counters, stream);
}

int ceres_trace_rays_f64(ceres_scene* s, const void* rays64, size_t n_rays, int mode, void* hits32, uint8_t* occluded,
                         ceres_stats* stats) {
    uint64_t c[8] = {0};
    if (const int chk = check_trace64_args(s, rays64, n_rays, mode, hits32, occluded)) {
        if (chk < 0) return chk;
        fill_stats(stats, c, 0.0);                            // n_rays = 0: a successful no-op
        return CERES_OK;
    }
    HIP_TRY(hipSetDevice(s->device));
    RoundTrip t("ceres_trace_rays_f64", s);
    void* dr = t.alloc(true, n_rays * 64);
    void* dh = t.alloc(hits32, n_rays * 32);
    uint8_t* dc = static_cast<uint8_t*>(t.alloc(occluded, n_rays));
    t.upload(dr, rays64, n_rays * 64);
    if (!t.rc) t.rc = ceres_trace_rays_f64_device(s, dr, n_rays, mode, dh, dc, s->d_counters, s->stream);
    t.stop();
    t.download(c, s->d_counters, sizeof c);
    t.download(hits32, dh, n_rays * 32);
    t.download(occluded, dc, n_rays);
    return t.finish(stats, c);
}

}  // extern "C"

// Shaded ray queries on a double scene (dev64::ceres_shade_rays64_k): render<double>()'s pixel for
// caller-supplied rays.  Like the ray queries they share the scene's buffers and nothing else.  The
// argument rules are the ray queries': a negative ceres_status when the call is refused, 1 when there
// is nothing to shade, 0 when there is.
static int check_shade64_args(const ceres_scene* s, const void* rays, size_t n_rays, const double* sun, int mode, bool any_output) {
    if (!s) return set_error(CERES_EINVAL, "ceres_shade_rays_f64: null scene");
    if (!s->f64) return set_error(CERES_EUNSUPPORTED, "ceres_shade_rays_f64: the scene is single precision (use ceres_shade_rays)");
    if (mode & ~(CERES_MODE_FMA | CERES_MODE_ROBUST))
        return set_error(CERES_EINVAL, "ceres_shade_rays_f64: bad mode %d (0 or CERES_MODE_FMA)", mode);
    if (mode & CERES_MODE_ROBUST) return set_error(CERES_EUNSUPPORTED, "ceres_shade_rays_f64: CERES_MODE_ROBUST takes float scenes");
    if (!any_output) return set_error(CERES_EINVAL, "ceres_shade_rays_f64: none of pixels, rgb8, hits and status asked for");
    if (n_rays >= (size_t(1) << 31)) return set_error(CERES_EUNSUPPORTED, "ceres_shade_rays_f64: %zu rays (below 2^31 per call)", n_rays);
    if (n_rays == 0) return 1;
    if (!rays || !sun) return set_error(CERES_EINVAL, "ceres_shade_rays_f64: null rays or sun");
    return 0;
}

extern "C" {

static int shade_rays64_launch(ceres_scene* s, const void* d_rays64, size_t n_rays, const uint32_t* d_index, size_t n_index,
                               bool indexed, const double sun[3], int mode, double* d_pixels, uint8_t* d_rgb8, void* d_hits32,
                               uint8_t* d_status, uint64_t* d_counters, void* stream_) {
    if (const int chk = check_shade64_args(s, d_rays64, n_rays, sun, mode, d_pixels || d_rgb8 || d_hits32 || d_status))
        return chk < 0 ? chk : CERES_OK;
    if ((reinterpret_cast<uintptr_t>(d_rays64) | reinterpret_cast<uintptr_t>(d_hits32)) & 15u)
        return set_error(CERES_EINVAL, "ceres_shade_rays_f64: rays and hits must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_pixels) & 7u) return set_error(CERES_EINVAL, "ceres_shade_rays_f64: pixels must be 8-byte aligned");
    const size_t lds = size_t(s->stack_entries) * kRayB * 4;          // u32 [entry][lane], the two walks one after the other
    if (lds > s->max_lds_per_block)
        return set_error(CERES_EINVAL, "ceres_shade_rays_f64: a traversal stack of %u entries needs %zu B of LDS per workgroup "
                         "(%zu available)", s->stack_entries, lds, s->max_lds_per_block);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    HIP_TRY(hipSetDevice(s->device));
    if (indexed)
        if (const int chk = check_index_list("ceres_shade_rays_f64_indexed", s, d_index, n_index)) return chk < 0 ? chk : CERES_OK;
    Indexed<ShadeParams64> P{};
    P.index = d_index; P.n_index = uint32_t(n_index);
    P.rays = static_cast<const double2*>(d_rays64);
    P.pixels = d_pixels; P.rgb8 = d_rgb8;
    P.hits = static_cast<ulonglong2*>(d_hits32);
    P.status = d_status;
    P.counters = reinterpret_cast<unsigned long long*>(d_counters);
    scene_params(P, s);
    P.norms = s->d_norms64;
    P.n_rays = uint32_t(n_rays);
    for (int k = 0; k < 3; ++k) P.sun[k] = sun[k];
    if (d_counters) HIP_TRY(hipMemsetAsync(d_counters, 0, 8 * sizeof(uint64_t), stream));
    const dim3 grid(uint32_t(((indexed ? n_index : n_rays) + kRayB - 1) / kRayB)), block(kRayB);
    const ShadeParams64& P0 = P;                                      // the plain kernels' block
    const bool gfma = (mode & CERES_MODE_FMA) != 0;
    dispatch_bools([&](auto gt) {
        constexpr bool G = decltype(gt)::value;
        if (indexed) hipLaunchKernelGGL((ceres_shade_rays64_idx_k<G>), grid, block, lds, stream, P);
        else hipLaunchKernelGGL((ceres_shade_rays64_k<G>), grid, block, lds, stream, P0);
    }, gfma);
    HIP_TRY(hipGetLastError());
    return CERES_OK;
}

int ceres_shade_rays_f64_device(ceres_scene* s, const void* d_rays64, size_t n_rays, const double sun[3], int mode,
                                double* d_pixels, uint8_t* d_rgb8, void* d_hits32, uint8_t* d_status, uint64_t* d_counters,
                                void* stream) {
    return shade_rays64_launch(s, d_rays64, n_rays, nullptr, 0, false, sun, mode, d_pixels, d_rgb8, d_hits32, d_status, d_counters,
                               stream);
}

int ceres_shade_rays_f64_indexed_device(ceres_scene* s, const void* d_rays64, size_t n_rays, const uint32_t* d_index, size_t n_index,
                                        const double sun[3], int mode, double* d_pixels, uint8_t* d_rgb8, void* d_hits32,
                                        uint8_t* d_status, uint64_t* d_counters, void* stream) {
    return shade_rays64_launch(s, d_rays64, n_rays, d_index, n_index, true, sun, mode, d_pixels, d_rgb8, d_hits32, d_status,
                               d_counters, stream);
}

int ceres_shade_rays_f64(ceres_scene* s, const void* rays64, size_t n_rays, const double sun[3], int mode, double* pixels,
                         uint8_t* rgb8, void* hits32, uint8_t* status, ceres_stats* stats) {
    uint64_t c[8] = {0};
    if (const int chk = check_shade64_args(s, rays64, n_rays, sun, mode, pixels || rgb8 || hits32 || status)) {
        if (chk < 0) return chk;
        fill_stats(stats, c, 0.0);                            // n_rays = 0: a successful no-op
        return CERES_OK;
    }
    HIP_TRY(hipSetDevice(s->device));
    RoundTrip t("ceres_shade_rays_f64", s);
    void* dr = t.alloc(true, n_rays * 64);
    void* dh = t.alloc(hits32, n_rays * 32);
    double* dp = static_cast<double*>(t.alloc(pixels, n_rays * 24));
    uint8_t* dq = static_cast<uint8_t*>(t.alloc(rgb8, n_rays * 3));
    uint8_t* ds = static_cast<uint8_t*>(t.alloc(status, n_rays));
    t.upload(dr, rays64, n_rays * 64);
    if (!t.rc) t.rc = ceres_shade_rays_f64_device(s, dr, n_rays, sun, mode, dp, dq, dh, ds, s->d_counters, s->stream);
    t.stop();
    t.download(c, s->d_counters, sizeof c);
    t.download(pixels, dp, n_rays * 24);
    t.download(rgb8, dq, n_rays * 3);
    t.download(hits32, dh, n_rays * 32);
    t.download(status, ds, n_rays);
    return t.finish(stats, c);
}

}  // extern "C"

// All-hits ray queries and complete hit lists on a double scene (dev64::ceres_trace_all64_k,
// ceres_trace_lists64_k, ceres_sort_lists64_k).  The argument rules are the float calls' in the float
// calls' order, with ceres_trace_rays_f64's for the scene and the mode: a negative ceres_status when the
// call is refused, 1 when there is nothing to trace.
static int check_all64_scene_mode(const char* name, const ceres_scene* s, int mode) {
    if (!s) return set_error(CERES_EINVAL, "%s: null scene", name);
    if (!s->f64) return set_error(CERES_EUNSUPPORTED, "%s: the scene is single precision (use the call without _f64)", name);
    if (mode & ~(CERES_MODE_FMA | CERES_MODE_ROBUST)) return set_error(CERES_EINVAL, "%s: bad mode %d (0 or CERES_MODE_FMA)", name, mode);
    if (mode & CERES_MODE_ROBUST) return set_error(CERES_EUNSUPPORTED, "%s: CERES_MODE_ROBUST takes float scenes", name);
    return 0;
}

static int check_trace_all64_args(const ceres_scene* s, const void* rays, size_t n_rays, int mode, uint32_t max_hits,
                                  const void* counts, const void* hits) {
    const char* name = "ceres_trace_rays_all_f64";
    if (const int rc = check_all64_scene_mode(name, s, mode)) return rc;
    if (!counts && !hits) return set_error(CERES_EINVAL, "%s: neither counts nor hits asked for", name);
    if (hits && (max_hits == 0 || max_hits > CERES_MAX_HITS))
        return set_error(CERES_EINVAL, "%s: max_hits %u (1 .. %d with a hit buffer)", name, max_hits, CERES_MAX_HITS);
    if (n_rays >= (size_t(1) << 31)) return set_error(CERES_EUNSUPPORTED, "%s: %zu rays (below 2^31 per call)", name, n_rays);
    if (n_rays == 0) return 1;
    if (!rays) return set_error(CERES_EINVAL, "%s: null rays", name);
    return 0;
}

static int check_trace_lists64_args(const ceres_scene* s, const void* rays, size_t n_rays, int mode, const void* hits,
                                    uint64_t capacity) {
    const char* name = "ceres_trace_rays_lists_f64";
    if (const int rc = check_all64_scene_mode(name, s, mode)) return rc;
    if (!hits && capacity) return set_error(CERES_EINVAL, "%s: null hits with capacity %llu", name, (unsigned long long)capacity);
    if (n_rays >= (size_t(1) << 31)) return set_error(CERES_EUNSUPPORTED, "%s: %zu rays (below 2^31 per call)", name, n_rays);
    if (n_rays == 0) return 1;
    if (!rays) return set_error(CERES_EINVAL, "%s: null rays", name);
    return 0;
}

// The LDS of one 64-ray workgroup: stack slots 0 .. stack_entries (u32 [entry][lane]), then per list
// entry an 8-byte and a 4-byte column per lane.
constexpr size_t kListEntryBytes64 = size_t(kRayB) * 12;
static size_t stack_bytes64(const ceres_scene* s) { return (size_t(s->stack_entries) + 1) * kRayB * 4; }

// The flag-to-status rule of the fill call's counters (ceres_trace_rays_lists_f64 applies it to its own).
static int lists64_status(const uint64_t c[8]) {
    if (c[6]) return set_error(CERES_ESTACK, "traversal stack overflow");
    if (c[7]) return set_error(CERES_EHIP, "ceres_trace_rays_lists_f64: a ray's hits do not match its segment (offsets of another "
                               "query, or a scene changed between the count and the fill)");
    return CERES_OK;
}

extern "C" {

static int trace_all64_launch(ceres_scene* s, const void* d_rays64, size_t n_rays, const uint32_t* d_index, size_t n_index,
                              bool indexed, int mode, uint32_t max_hits, uint32_t* d_counts, void* d_hits32, uint64_t* d_counters,
                              void* stream_) {
    if (const int chk = check_trace_all64_args(s, d_rays64, n_rays, mode, max_hits, d_counts, d_hits32)) return chk < 0 ? chk : CERES_OK;
    if ((reinterpret_cast<uintptr_t>(d_rays64) | reinterpret_cast<uintptr_t>(d_hits32)) & 15u)
        return set_error(CERES_EINVAL, "ceres_trace_rays_all_f64: rays and hits must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_counts) & 3u) return set_error(CERES_EINVAL, "ceres_trace_rays_all_f64: counts must be 4-byte aligned");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    HIP_TRY(hipSetDevice(s->device));
    const bool keep = d_hits32 != nullptr;
    Indexed<AllParams64> P{};
    P.index = d_index; P.n_index = uint32_t(n_index);
    P.rays = static_cast<const double2*>(d_rays64);
    P.hits = static_cast<ulonglong2*>(d_hits32);
    P.counts = d_counts;
    P.counters = reinterpret_cast<unsigned long long*>(d_counters);
    scene_params(P, s);
    P.n_rays = uint32_t(n_rays);
    P.max_hits = keep ? max_hits : 0u;
    P.lds_entries = s->stack_entries + 1;
    const size_t stack_bytes = stack_bytes64(s), list_bytes = size_t(P.max_hits) * kListEntryBytes64;
    const size_t lds = stack_bytes + list_bytes;
    if (lds > s->max_lds_per_block)
        return set_error(CERES_EINVAL, "ceres_trace_rays_all_f64: the traversal stack (%zu B) and the hit list (%zu B) exceed the LDS "
                         "of a workgroup (%zu B available)", stack_bytes, list_bytes, s->max_lds_per_block);
    if (indexed)
        if (const int chk = check_index_list("ceres_trace_rays_all_f64_indexed", s, d_index, n_index)) return chk < 0 ? chk : CERES_OK;
    if (d_counters) HIP_TRY(hipMemsetAsync(d_counters, 0, 8 * sizeof(uint64_t), stream));
    const dim3 grid(uint32_t(((indexed ? n_index : n_rays) + kRayB - 1) / kRayB)), block(kRayB);
    const bool stats = (s->flags & CERES_SCENE_STATS) != 0, gfma = (mode & CERES_MODE_FMA) != 0;
    const AllParams64& P0 = P;                                        // the plain kernels' block
    dispatch_bools([&](auto st, auto gt, auto kt) {
        constexpr bool S = decltype(st)::value, G = decltype(gt)::value, K = decltype(kt)::value;
        if constexpr (!S) {                                           // a stats scene has no indexed kernel
            if (indexed) { hipLaunchKernelGGL((ceres_trace_all64_idx_k<G, K>), grid, block, lds, stream, P); return; }
        }
        hipLaunchKernelGGL((ceres_trace_all64_k<S, G, K>), grid, block, lds, stream, P0);
    }, stats, gfma, keep);
    HIP_TRY(hipGetLastError());
    return CERES_OK;
}

int ceres_trace_rays_all_f64_device(ceres_scene* s, const void* d_rays64, size_t n_rays, int mode, uint32_t max_hits,
                                    uint32_t* d_counts, void* d_hits32, uint64_t* d_counters, void* stream) {
    return trace_all64_launch(s, d_rays64, n_rays, nullptr, 0, false, mode, max_hits, d_counts, d_hits32, d_counters, stream);
}

int ceres_trace_rays_all_f64_indexed_device(ceres_scene* s, const void* d_rays64, size_t n_rays, const uint32_t* d_index,
                                            size_t n_index, int mode, uint32_t max_hits, uint32_t* d_counts, void* d_hits32,
                                            uint64_t* d_counters, void* stream) {
    return trace_all64_launch(s, d_rays64, n_rays, d_index, n_index, true, mode, max_hits, d_counts, d_hits32, d_counters, stream);
}

int ceres_trace_rays_all_f64(ceres_scene* s, const void* rays64, size_t n_rays, int mode, uint32_t max_hits, uint32_t* counts,
                             void* hits32, ceres_stats* stats) {
    uint64_t c[8] = {0};
    if (const int chk = check_trace_all64_args(s, rays64, n_rays, mode, max_hits, counts, hits32)) {
        if (chk < 0) return chk;
        fill_stats(stats, c, 0.0);                            // n_rays = 0: a successful no-op
        return CERES_OK;
    }
    HIP_TRY(hipSetDevice(s->device));
    const size_t hit_bytes = hits32 ? n_rays * size_t(max_hits) * 32 : 0;
    RoundTrip t("ceres_trace_rays_all_f64", s);
    void* dr = t.alloc(true, n_rays * 64);
    void* dh = t.alloc(hits32, hit_bytes);
    uint32_t* dn = static_cast<uint32_t*>(t.alloc(counts, n_rays * 4));
    t.upload(dr, rays64, n_rays * 64);
    if (!t.rc) t.rc = ceres_trace_rays_all_f64_device(s, dr, n_rays, mode, max_hits, dn, dh, s->d_counters, s->stream);
    t.stop();
    t.download(c, s->d_counters, sizeof c);
    t.download(hits32, dh, hit_bytes);
    t.download(counts, dn, n_rays * 4);
    return t.finish(stats, c);
}

static int trace_lists64_launch(ceres_scene* s, const void* d_rays64, size_t n_rays, const uint32_t* d_index, size_t n_index,
                                bool indexed, int mode, const uint64_t* d_offsets, void* d_hits32, uint64_t capacity,
                                uint64_t* d_counters, void* stream_) {
    if (const int chk = check_trace_lists64_args(s, d_rays64, n_rays, mode, d_hits32, capacity)) return chk < 0 ? chk : CERES_OK;
    if (!d_offsets) return set_error(CERES_EINVAL, "ceres_trace_rays_lists_f64: null offsets");
    if ((reinterpret_cast<uintptr_t>(d_rays64) | reinterpret_cast<uintptr_t>(d_hits32)) & 15u)
        return set_error(CERES_EINVAL, "ceres_trace_rays_lists_f64: rays and hits must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_offsets) & 7u) return set_error(CERES_EINVAL, "ceres_trace_rays_lists_f64: offsets must be 8-byte aligned");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    Indexed<ListParams64> P{};
    P.index = d_index; P.n_index = uint32_t(n_index);
    P.rays = static_cast<const double2*>(d_rays64);
    P.offsets = reinterpret_cast<const unsigned long long*>(d_offsets);
    P.hits = static_cast<ulonglong2*>(d_hits32);
    P.capacity = capacity;
    P.counters = reinterpret_cast<unsigned long long*>(d_counters);
    scene_params(P, s);
    P.n_rays = uint32_t(n_rays);
    P.lds_entries = s->stack_entries + 1;
    // the LDS carve-up of ceres_trace_rays_all_f64 with L list entries; a deep scene keeps as many as fit
    const size_t stack_bytes = stack_bytes64(s);
    if (stack_bytes + kListEntryBytes64 > s->max_lds_per_block)
        return set_error(CERES_EINVAL, "ceres_trace_rays_lists_f64: the traversal stack (%zu B) and one list entry (%zu B) exceed the "
                         "LDS of a workgroup (%zu B available)", stack_bytes, kListEntryBytes64, s->max_lds_per_block);
    P.list_entries = uint32_t(std::min<size_t>(s->list_entries, (s->max_lds_per_block - stack_bytes) / kListEntryBytes64));
    const size_t lds = stack_bytes + P.list_entries * kListEntryBytes64;
    SortParams64 Q{};
    Q.offsets = P.offsets; Q.hits = P.hits; Q.capacity = capacity;
    Q.n_rays = P.n_rays; Q.list_entries = P.list_entries;
    Q.sort_cap = uint32_t(std::min<size_t>(s->list_sort_cap, s->max_lds_per_block / 32));
    if (indexed)
        if (const int chk = check_index_list("ceres_trace_rays_lists_f64_indexed", s, d_index, n_index)) return chk < 0 ? chk : CERES_OK;
    HIP_TRY(hipSetDevice(s->device));
    if (d_counters) HIP_TRY(hipMemsetAsync(d_counters, 0, 8 * sizeof(uint64_t), stream));
    const dim3 grid(uint32_t(((indexed ? n_index : n_rays) + kRayB - 1) / kRayB)), block(kRayB);
    const dim3 sort_grid(uint32_t((n_rays + kRayB - 1) / kRayB));     // the sort pass: every ray's segment
    const bool stats = (s->flags & CERES_SCENE_STATS) != 0, gfma = (mode & CERES_MODE_FMA) != 0;
    const ListParams64& P0 = P;                                       // the plain kernels' block
    dispatch_bools([&](auto st, auto gt) {
        constexpr bool S = decltype(st)::value, G = decltype(gt)::value;
        if constexpr (!S) {                                           // a stats scene has no indexed kernel
            if (indexed) { hipLaunchKernelGGL((ceres_trace_lists64_idx_k<G>), grid, block, lds, stream, P); return; }
        }
        hipLaunchKernelGGL((ceres_trace_lists64_k<S, G>), grid, block, lds, stream, P0);
    }, stats, gfma);
    HIP_TRY(hipGetLastError());
    if (capacity) {                                                   // nothing was written otherwise
        hipLaunchKernelGGL(ceres_sort_lists64_k, sort_grid, dim3(64), size_t(Q.sort_cap) * 32, stream, Q);
        HIP_TRY(hipGetLastError());
    }
    return CERES_OK;
}

int ceres_trace_rays_lists_f64_device(ceres_scene* s, const void* d_rays64, size_t n_rays, int mode, const uint64_t* d_offsets,
                                      void* d_hits32, uint64_t capacity, uint64_t* d_counters, void* stream) {
    return trace_lists64_launch(s, d_rays64, n_rays, nullptr, 0, false, mode, d_offsets, d_hits32, capacity, d_counters, stream);
}

int ceres_trace_rays_lists_f64_indexed_device(ceres_scene* s, const void* d_rays64, size_t n_rays, const uint32_t* d_index,
                                              size_t n_index, int mode, const uint64_t* d_offsets, void* d_hits32, uint64_t capacity,
                                              uint64_t* d_counters, void* stream) {
    return trace_lists64_launch(s, d_rays64, n_rays, d_index, n_index, true, mode, d_offsets, d_hits32, capacity, d_counters, stream);
}

int ceres_trace_rays_lists_f64(ceres_scene* s, const void* rays64, size_t n_rays, int mode, uint64_t* offsets, void* hits32,
                               uint64_t capacity, uint64_t* total, ceres_stats* stats) {
    uint64_t c[8] = {0}, cf[8] = {0};
    if (const int chk = check_trace_lists64_args(s, rays64, n_rays, mode, hits32, capacity)) {
        if (chk < 0) return chk;
        fill_stats(stats, c, 0.0);                            // n_rays = 0: a successful no-op
        if (offsets) offsets[0] = 0;
        if (total) *total = 0;
        return CERES_OK;
    }
    HIP_TRY(hipSetDevice(s->device));
    // the count phase: the all-hits count, then the offsets
    const size_t scratch = ceres_hit_offsets_scratch_bytes(n_rays);
    uint64_t tot = 0;
    RoundTrip t("ceres_trace_rays_lists_f64", s);
    void* dr = t.alloc(true, n_rays * 64);
    uint32_t* dn = static_cast<uint32_t*>(t.alloc(true, n_rays * 4));
    uint64_t* dof = static_cast<uint64_t*>(t.alloc(true, (n_rays + 1) * 8));
    void* dsc = t.alloc(true, scratch);
    t.upload(dr, rays64, n_rays * 64);
    if (!t.rc) t.rc = ceres_trace_rays_all_f64_device(s, dr, n_rays, mode, 0, dn, nullptr, s->d_counters, s->stream);
    t.download(c, s->d_counters, sizeof c);
    if (!t.rc) t.rc = ceres_hit_offsets_device(s, dn, n_rays, dof, dsc, scratch, s->stream);
    t.stop();
    t.download(&tot, dof + n_rays, 8);
    t.download(offsets, dof, (n_rays + 1) * 8);
    const double ms = t.finish();
    if (t.rc) return t.rc;
    if (total) *total = tot;
    fill_stats(stats, c, ms);
    if (c[6]) return set_error(CERES_ESTACK, "traversal stack overflow");
    if (capacity < tot)
        return set_error(CERES_ENOMEM, "ceres_trace_rays_lists_f64: capacity %llu, the rays have %llu hits", (unsigned long long)capacity,
                         (unsigned long long)tot);
    if (tot == 0) return CERES_OK;
    // the fill phase, timed on its own
    void* dh = t.alloc(true, tot * 32);
    if (!dh) return set_error(CERES_ENOMEM, "ceres_trace_rays_lists_f64: device allocation failed (%llu hits)", (unsigned long long)tot);
    t.restart();
    if (!t.rc) t.rc = ceres_trace_rays_lists_f64_device(s, dr, n_rays, mode, dof, dh, tot, s->d_counters, s->stream);
    t.stop();
    t.download(cf, s->d_counters, sizeof cf);
    t.download(hits32, dh, tot * 32);
    const double ms2 = t.finish();
    if (t.rc) return t.rc;
    if (stats) stats->ms = ms + ms2;
    return lists64_status(cf);
}

}  // extern "C"
