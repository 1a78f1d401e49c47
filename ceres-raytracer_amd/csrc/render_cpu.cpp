// render_cpu.cpp -- the product's CPU render path: render<float>() (render.hpp:86-156) on host
// cores, behind `./render --cpu` ("the CLI can run the CPU path, so
// config 1 works with no GPU").  It is chosen explicitly (ceres_render_cpu_f32 / --cpu); nothing
// falls back to it -- without a GPU the device calls still fail loudly.
//
// It walks the product's own scene layout (ceres_types.hpp: 64-B sibling-pair records, leaf-ordered
// triangles, orig[] slot -> original index) in the reference's order, with the same per-ray
// arithmetic the gfx950 kernels compute (render_hip.hip: trace, tri_test, hit_point, shade), so its
// images are the reference's bit for bit in both arithmetics:
//   * CERES_MODE_FMA: GCC's contraction sites of the reference CMake build (CMakeLists.txt:11-13;
//     oracle/contraction_sites.txt) as explicit std::fma; without it every expression is plain (this
//     file is compiled with -ffp-contract=off, so the compiler adds none);
//   * FastNodeIntersector (node_intersectors.hpp:83-103) or, with CERES_MODE_ROBUST, the
//     RobustNodeIntersector (:54-79);
//   * the shadow ray is traced like the reference traces it: the closest-hit traversal
//     (render.hpp:135-136; only whether it hits is used), so the traversal statistics are the
//     reference's Statistics (single_ray_traverser.hpp:83,53) for primary and shadow rays alike.
// Rows are spread over OpenMP threads (render.hpp:103, `omp parallel for`).
#include <algorithm>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <new>
#include <type_traits>
#include <vector>

#include <omp.h>

#include "ceres_render.h"
#include "ceres_types.hpp"
#include "closest_point.hpp"
#include "closest_point64.hpp"
#include "host_common.hpp"
#include "pow24.hpp"
#include "ray_key.hpp"

using namespace ceres;

struct ceres_cpu_scene {
    bool f64 = false;                 // render<double> (anim.cpp -d): the *64 arrays
    std::vector<SiblingPair> pairs;   // pair k: the two children of an inner node (pairs[0]: the root's)
    std::vector<Tri48> tris;          // leaf order
    std::vector<SiblingPair64> pairs64;
    std::vector<Tri96> tris64;
    std::vector<uint32_t> orig;       // leaf slot -> original triangle index (tri_norms order)
    std::vector<float> norms;         // 9 scalars per original triangle (obj_norms.hpp:113-115)
    std::vector<double> norms64;
    uint32_t depth = 0, root_leaf_count = 0, root_leaf_first = 0;
    double built_cost = 0.0;          // the baseline of ceres_cpu_scene_update*: unknown until the first
    bool built_cost_known = false;    // update or rebuild measures it
};

namespace {

// The scene's arrays for one Scalar.
template <class S> struct Arr;
template <> struct Arr<float> {
    static const std::vector<SiblingPair>& pairs(const ceres_cpu_scene& s) { return s.pairs; }
    static const std::vector<Tri48>& tris(const ceres_cpu_scene& s) { return s.tris; }
    static const float* norms(const ceres_cpu_scene& s) { return s.norms.data(); }
    static constexpr float eps = FLT_EPSILON, big = FLT_MAX;
};
template <> struct Arr<double> {
    static const std::vector<SiblingPair64>& pairs(const ceres_cpu_scene& s) { return s.pairs64; }
    static const std::vector<Tri96>& tris(const ceres_cpu_scene& s) { return s.tris64; }
    static const double* norms(const ceres_cpu_scene& s) { return s.norms64.data(); }
    static constexpr double eps = DBL_EPSILON, big = DBL_MAX;
};

template <class S> struct V3 { S x, y, z; };
template <class S> inline V3<S> operator+(V3<S> a, V3<S> b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
template <class S> inline V3<S> operator-(V3<S> a, V3<S> b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
template <class S> inline V3<S> operator*(V3<S> a, S s) { return {a.x * s, a.y * s, a.z * s}; }
template <class S> inline V3<S> v3(const S* p) { return {p[0], p[1], p[2]}; }

// vector.hpp:134-167 as each build computes it (see render_hip.hip dotA / dotB / crossG, render64.hip
// for double: GCC fuses the double path at the same sites): dot "A" fma(a2, b2, fma(a0, b0, a1 b1)),
// Triangle::intersect's v = dot(r, e1) as "B" fma(a2, b2, fma(a1, b1, a0 b0)), cross a_j b_k - a_k b_j
// as fma(a_j, b_k, -(a_k b_j)).
template <bool G, class S> inline S dot_a(V3<S> a, V3<S> b) {
    if constexpr (G) return std::fma(a.z, b.z, std::fma(a.x, b.x, a.y * b.y));
    S s = a.x * b.x; s += a.y * b.y; s += a.z * b.z;
    return s;
}
template <bool G, class S> inline S dot_b(V3<S> a, V3<S> b) {
    if constexpr (G) return std::fma(a.z, b.z, std::fma(a.y, b.y, a.x * b.x));
    return dot_a<false>(a, b);
}
template <bool G, class S> inline V3<S> cross_g(V3<S> a, V3<S> b) {
    if constexpr (G) return {std::fma(a.y, b.z, -(a.z * b.y)), std::fma(a.z, b.x, -(a.x * b.z)), std::fma(a.x, b.y, -(a.y * b.x))};
    return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
template <bool G, class S> inline V3<S> normalize_g(V3<S> v) { const S inv = S(1) / std::sqrt(dot_a<G>(v, v)); return v * inv; }

// fminf / fmaxf (the non-NaN operand when one is NaN; the sign of a zero result is never observed:
// only comparisons read these values), written out so they inline instead of calling libm
template <class S> inline S min_nn(S x, S y) { return (x < y || std::isnan(y)) ? x : y; }
template <class S> inline S max_nn(S x, S y) { return (x > y || std::isnan(y)) ? x : y; }

// The slab constants of a ray and the test of one box (entry e, exit x; hit iff e <= x).
//   fast: inv = safe_inverse(d) (vector.hpp:69-74), s = -o inv, each slab fma(bound, inv, s); the
//         octant's near / far bound is min / max of the two fmas (fma is monotone in the bound);
//   robust (float scenes): inv = 1 / d, the exit slabs scaled by inv padded by 2 ulps
//         (utilities.hpp:102-106).
template <bool R, class S> struct SlabC { S ix, iy, iz, sx, sy, sz; V3<S> o; };
inline float pad2(float x) { uint32_t b; std::memcpy(&b, &x, 4); b += 2; float y; std::memcpy(&y, &b, 4); return std::isfinite(x) ? y : x; }
template <bool R, class S> inline SlabC<R, S> slab_of(V3<S> o, V3<S> d) {
    SlabC<R, S> s;
    if constexpr (R) {
        static_assert(std::is_same<S, float>::value, "robust slabs: float scenes");
        s.ix = 1.0f / d.x; s.iy = 1.0f / d.y; s.iz = 1.0f / d.z;
        s.sx = pad2(s.ix); s.sy = pad2(s.iy); s.sz = pad2(s.iz);
    } else {
        auto safe_inv = [](S x) { return S(1) / (std::fabs(x) < Arr<S>::eps ? std::copysign(Arr<S>::eps, x) : x); };
        s.ix = safe_inv(d.x); s.iy = safe_inv(d.y); s.iz = safe_inv(d.z);
        s.sx = (-o.x) * s.ix; s.sy = (-o.y) * s.iy; s.sz = (-o.z) * s.iz;
    }
    s.o = o;
    return s;
}
// Sel (fast test): each axis's entry / exit bound is picked by the ray's octant as NodeIntersector::intersect
// does (node_intersectors.hpp:35-47) instead of by min / max of the two fmas.  The two agree on every box with
// lo <= hi; an INVERTED box (a leaf whose triangles are all NaN on an axis keeps the empty +-FLT_MAX there)
// is a miss to the reference and a hit to the min / max form.
template <bool R, class S, bool Sel = false> inline bool box_hit(const SlabC<R, S>& s, const S* b, S tmin, S tmax, S& entry) {
    S e, x;                                       // b: xmin, xmax, ymin, ymax, zmin, zmax
    if constexpr (!R && Sel) {
        const bool nx = std::signbit(s.ix), ny = std::signbit(s.iy), nz = std::signbit(s.iz);
        const S ex = std::fma(nx ? b[1] : b[0], s.ix, s.sx), xx = std::fma(nx ? b[0] : b[1], s.ix, s.sx);
        const S ey = std::fma(ny ? b[3] : b[2], s.iy, s.sy), xy = std::fma(ny ? b[2] : b[3], s.iy, s.sy);
        const S ez = std::fma(nz ? b[5] : b[4], s.iz, s.sz), xz = std::fma(nz ? b[4] : b[5], s.iz, s.sz);
        e = max_nn(ex, max_nn(ey, max_nn(ez, tmin)));
        x = min_nn(xx, min_nn(xy, min_nn(xz, tmax)));
    } else if constexpr (R) {
        const bool nx = std::signbit(s.ix), ny = std::signbit(s.iy), nz = std::signbit(s.iz);
        const S ex = ((nx ? b[1] : b[0]) - s.o.x) * s.ix, xx = ((nx ? b[0] : b[1]) - s.o.x) * s.sx;
        const S ey = ((ny ? b[3] : b[2]) - s.o.y) * s.iy, xy = ((ny ? b[2] : b[3]) - s.o.y) * s.sy;
        const S ez = ((nz ? b[5] : b[4]) - s.o.z) * s.iz, xz = ((nz ? b[4] : b[5]) - s.o.z) * s.sz;
        e = max_nn(ex, max_nn(ey, max_nn(ez, tmin)));
        x = min_nn(xx, min_nn(xy, min_nn(xz, tmax)));
    } else {
        const S a0 = std::fma(b[0], s.ix, s.sx), a1 = std::fma(b[1], s.ix, s.sx);
        const S b0 = std::fma(b[2], s.iy, s.sy), b1 = std::fma(b[3], s.iy, s.sy);
        const S c0 = std::fma(b[4], s.iz, s.sz), c1 = std::fma(b[5], s.iz, s.sz);
        e = max_nn(min_nn(a0, a1), max_nn(min_nn(b0, b1), max_nn(min_nn(c0, c1), tmin)));
        x = min_nn(max_nn(a0, a1), min_nn(max_nn(b0, b1), min_nn(max_nn(c0, c1), tmax)));
    }
    entry = e;
    return e <= x;
}

// Triangle::intersect (triangle.hpp:95-115): Moller-Trumbore, left-handed normal, IEEE 1 / det.
template <bool G, class S, class Tri> inline bool tri_hit(const Tri& tr, V3<S> o, V3<S> d, S tmin, S tmax, S& t_out, S& u_out,
                                                         S& v_out) {
    const V3<S> c = v3(tr.p0) - o;
    const V3<S> r = cross_g<G>(d, c);
    const S inv_det = S(1) / dot_a<G>(v3(tr.n), d);
    const S u = dot_a<G>(r, v3(tr.e2)) * inv_det;
    const S v = dot_b<G>(r, v3(tr.e1)) * inv_det;
    const S w = S(1) - u - v;
    if (u >= 0 && v >= 0 && w >= 0) {
        const S t = dot_a<G>(v3(tr.n), c) * inv_det;
        if (t >= tmin && t <= tmax) { t_out = t; u_out = u; v_out = v; return true; }
    }
    return false;
}

template <class S> struct HitRec { uint32_t slot; S t, u, v; };

// SingleRayTraverser::intersect (single_ray_traverser.hpp:68-126) with a closest-primitive
// intersector over the sibling-pair records: both children's boxes against the step's tmax, left
// leaf then right leaf in leaf order (each accepted hit lowers tmax, the last accepted one wins),
// the far child pushed, ties left.  steps / tests: the reference's Statistics.  [tmin, tmax] is the
// ray's window (ray.hpp:10-22; render()'s rays: [0, max]); tmax shrinks from it.
template <bool G, bool R, class S>
bool trace_closest(const ceres_cpu_scene& s, V3<S> o, V3<S> d, S tmin, S tmax, uint32_t* stack, uint32_t cap, HitRec<S>& best,
                   uint64_t& steps, uint64_t& tests, bool& overflow) {
    const auto& pairs = Arr<S>::pairs(s);
    const auto& tris = Arr<S>::tris(s);
    bool have = false;
    auto leaf = [&](uint32_t first, uint32_t count) {                      // intersect_leaf, :43-63
        tests += count;
        for (uint32_t k = first; k < first + count; ++k) {
            S t, u, v;
            if (tri_hit<G>(tris[k], o, d, tmin, tmax, t, u, v)) { best = {k, t, u, v}; have = true; tmax = t; }
        }
    };
    if (s.root_leaf_count) {                                                // :72-73
        leaf(s.root_leaf_first, s.root_leaf_count);
        return have;
    }
    const SlabC<R, S> sl = slab_of<R>(o, d);
    uint32_t sp = 0, cur = 0;
    while (true) {
        ++steps;                                                            // :83
        const auto& p = pairs[cur];
        S el, er;
        const bool hl = box_hit<R>(sl, p.lb, tmin, tmax, el), hr = box_hit<R>(sl, p.rb, tmin, tmax, er);
        if (hl && p.lcount) leaf(p.lfirst, p.lcount);                       // :89-97
        if (hr && p.rcount) leaf(p.rfirst, p.rcount);                       // :99-107
        const bool go_l = hl && !p.lcount, go_r = hr && !p.rcount;
        if (go_l && go_r) {                                                 // :109-115
            const bool swap = el > er;
            if (sp >= cap) { overflow = true; return have; }
            stack[sp++] = swap ? p.lfirst : p.rfirst;
            cur = swap ? p.rfirst : p.lfirst;
        } else if (go_l || go_r) {                                          // :115-117
            cur = go_l ? p.lfirst : p.rfirst;
        } else {                                                            // :118-121
            if (sp == 0) break;
            cur = stack[--sp];
        }
    }
    return have;
}

// The same walk with an any-hit intersector (ClosestPrimitiveIntersector<..., true>,
// primitive_intersectors.hpp): the window never shrinks and the first accepted hit ends it.  Every
// leaf the closest query reaches is reached here too (its window is never the wider one), and a leaf
// reached only here holds no hit the closest query's narrowed window could still accept without
// already holding one: the answer is "trace_closest finds a hit".
template <bool G, bool R, class S>
bool trace_any(const ceres_cpu_scene& s, V3<S> o, V3<S> d, S tmin, S tmax, uint32_t* stack, uint32_t cap, bool& overflow) {
    const auto& pairs = Arr<S>::pairs(s);
    const auto& tris = Arr<S>::tris(s);
    auto leaf = [&](uint32_t first, uint32_t count) {
        for (uint32_t k = first; k < first + count; ++k) {
            S t, u, v;
            if (tri_hit<G>(tris[k], o, d, tmin, tmax, t, u, v)) return true;
        }
        return false;
    };
    if (s.root_leaf_count) return leaf(s.root_leaf_first, s.root_leaf_count);
    const SlabC<R, S> sl = slab_of<R>(o, d);
    uint32_t sp = 0, cur = 0;
    while (true) {
        const auto& p = pairs[cur];
        S el, er;
        const bool hl = box_hit<R>(sl, p.lb, tmin, tmax, el), hr = box_hit<R>(sl, p.rb, tmin, tmax, er);
        if (hl && p.lcount && leaf(p.lfirst, p.lcount)) return true;
        if (hr && p.rcount && leaf(p.rfirst, p.rcount)) return true;
        const bool go_l = hl && !p.lcount, go_r = hr && !p.rcount;
        if (go_l && go_r) {
            const bool swap = el > er;
            if (sp >= cap) { overflow = true; return false; }
            stack[sp++] = swap ? p.lfirst : p.rfirst;
            cur = swap ? p.rfirst : p.lfirst;
        } else if (go_l || go_r) {
            cur = go_l ? p.lfirst : p.rfirst;
        } else {
            if (sp == 0) break;
            cur = stack[--sp];
        }
    }
    return false;
}

// The same walk with an intersector that never lowers tmax (its distance() is the ray's own tmax,
// single_ray_traverser.hpp:43-63): every box test and every triangle test against the original window,
// every accepted triangle a hit.  The hit set is this walk's, not a brute force's (the fast slab test
// is not conservative); with a fixed window neither the set nor steps / tests depend on the visiting
// order, so the walk goes left and pushes right.  The fast box test picks its bounds by the octant
// (box_hit's Sel), so that the leaves reached -- tri_tests -- are the reference's on inverted boxes too.  Returns the size of the set; `best` (cap entries, may
// be NULL for a count-only query) keeps the smallest hits sorted by t (float <), equal t by original
// triangle index; *kept their number.
template <bool G, bool R, class S>
uint32_t trace_all(const ceres_cpu_scene& s, V3<S> o, V3<S> d, S tmin, S tmax, uint32_t* stack, uint32_t cap, HitRec<S>* best,
                   uint32_t max_hits, uint32_t* kept, uint64_t& steps, uint64_t& tests, bool& overflow,
                   std::vector<HitRec<S>>* every = nullptr) {
    const auto& pairs = Arr<S>::pairs(s);
    const auto& tris = Arr<S>::tris(s);
    uint32_t count = 0, n = 0;
    auto before = [&](const HitRec<S>& a, const HitRec<S>& b) {
        return a.t < b.t || (a.t == b.t && s.orig[a.slot] < s.orig[b.slot]);
    };
    auto leaf = [&](uint32_t first, uint32_t cnt) {
        tests += cnt;
        for (uint32_t k = first; k < first + cnt; ++k) {
            S t, u, v;
            if (!tri_hit<G>(tris[k], o, d, tmin, tmax, t, u, v)) continue;
            ++count;
            if (every) every->push_back(HitRec<S>{k, t, u, v});       // the complete list, in walk order (trace_rays_lists)
            if (!best) continue;
            const HitRec<S> h{k, t, u, v};
            uint32_t i = n;
            if (n == max_hits) {
                if (!before(h, best[n - 1])) continue;
                i = n - 1;
            } else {
                ++n;
            }
            for (; i > 0 && before(h, best[i - 1]); --i) best[i] = best[i - 1];
            best[i] = h;
        }
    };
    if (s.root_leaf_count) {
        leaf(s.root_leaf_first, s.root_leaf_count);
    } else {
        const SlabC<R, S> sl = slab_of<R>(o, d);
        uint32_t sp = 0, cur = 0;
        while (true) {
            ++steps;
            const auto& p = pairs[cur];
            S el, er;
            const bool hl = box_hit<R, S, true>(sl, p.lb, tmin, tmax, el), hr = box_hit<R, S, true>(sl, p.rb, tmin, tmax, er);
            if (hl && p.lcount) leaf(p.lfirst, p.lcount);
            if (hr && p.rcount) leaf(p.rfirst, p.rcount);
            const bool go_l = hl && !p.lcount, go_r = hr && !p.rcount;
            if (go_l && go_r) {
                if (sp >= cap) { overflow = true; break; }
                stack[sp++] = p.rfirst;
                cur = p.lfirst;
            } else if (go_l || go_r) {
                cur = go_l ? p.lfirst : p.rfirst;
            } else {
                if (sp == 0) break;
                cur = stack[--sp];
            }
        }
    }
    if (kept) *kept = n;
    return count;
}

// Hit point + self-intersection offset (render.hpp:127-133; p1 = p0 - e1, p2 = p0 + e2).
template <bool G, class S, class Tri> inline V3<S> hit_point(const Tri& tr, V3<S> normal, S hu, S hv) {
    const V3<S> p0 = v3(tr.p0), p1 = p0 - v3(tr.e1), p2 = p0 + v3(tr.e2);
    const S scale = -0.00001;
    const S w = 1 - hu - hv;
    if constexpr (G) {
        auto c = [&](S a, S q1, S q2, S n) { return std::fma(n, scale, std::fma(w, q2, std::fma(hv, q1, hu * a))); };
        return {c(p0.x, p1.x, p2.x, normal.x), c(p0.y, p1.y, p2.y, normal.y), c(p0.z, p1.z, p2.z, normal.z)};
    }
    const V3<S> p = p0 * hu + p1 * hv + p2 * w;
    return p + normal * scale;
}

// smooth_shading (render.hpp:46-84).  lambertian and blinn_phong_spec return float and
// std::pow(Scalar, 24) is the double pow narrowed to float (render.hpp:46-54): float scenes use
// pow24f (pinned against glibc for every float by tests/test_pow24.py), double scenes call the pow
// itself; the colour accumulates in float, `c[k] += w * clamp(...)` (double weights for double
// scenes: float(double + double), render64.hip).
template <bool G, class S> inline void shade(V3<S> sun_line, const S* nrm, V3<S> view, S u, S v, float c[3]) {
    c[0] = c[1] = c[2] = 0.0f;
    const float amb = 0.2;
    const V3<S> vneg = view * S(-1);
    const S w[3] = {u, v, 1 - u - v};
    for (int k = 0; k < 3; ++k) {
        const V3<S> N{nrm[3 * k], nrm[3 * k + 1], nrm[3 * k + 2]};
        const float lam = float(std::fabs(dot_a<G>(sun_line, N)));
        const S x = dot_a<G>(N, normalize_g<G>(sun_line + vneg));
        float p24;
        if constexpr (std::is_same<S, float>::value) p24 = pow24f(x);
        else p24 = float(std::pow(x, 24.0));
        const float spec = 0.8f * p24;
        const float base = G ? std::fma(lam, 0.5f, amb) : amb + 0.5f * lam;
        auto clamp01 = [](float y) { return (y < 0.f) ? 0.f : (1.f < y) ? 1.f : y; };   // std::clamp
        auto ch = [&](float k2) { return G ? std::fma(base, k2, spec) : base * k2 + spec; };
        for (int ch_i = 0; ch_i < 3; ++ch_i) {
            const float kk = ch_i == 0 ? 0.5f : ch_i == 1 ? 0.0f : 0.8f;
            if constexpr (std::is_same<S, float>::value) c[ch_i] += w[k] * clamp01(ch(kk));
            else c[ch_i] = float(double(c[ch_i]) + w[k] * double(clamp01(ch(kk))));
        }
    }
}

template <class S> inline uint8_t quantize(S x) {                          // static.cpp:141-143
    const S a = x * 255;
    const S m = (S(255) < a) ? S(255) : a;
    const S q = (m < S(0)) ? S(0) : m;
    return static_cast<uint8_t>(static_cast<int>(q));
}

struct Counts { uint64_t primary = 0, shadow = 0, hits = 0, steps = 0, tests = 0; bool overflow = false; };

// The primary ray direction of pixel (i, j), render.hpp:105-111 (GCC: dir + fma(iv, v, iu u)).
template <bool G, class S> inline V3<S> primary_view(V3<S> dir, V3<S> iu, V3<S> iv, size_t i, size_t j, size_t W, size_t H) {
    const S u = 2 * (S(i) + S(0.5)) / S(W) - S(1);
    const S v = 2 * (S(j) + S(0.5)) / S(H) - S(1);
    const V3<S> a = G ? V3<S>{dir.x + std::fma(iv.x, v, iu.x * u), dir.y + std::fma(iv.y, v, iu.y * u),
                              dir.z + std::fma(iv.z, v, iu.z * u)}
                      : iu * u + iv * v + dir;
    return normalize_g<G>(a);
}

template <bool G, bool R, class S>
void render_rows(const ceres_cpu_scene& s, const S* b12, const S* sun, bool full, S* pixels, uint8_t* rgb8,
                 size_t W, size_t H, int threads, Counts& tot) {
    const V3<S> eye = v3(b12), dir = v3(b12 + 3), iu = v3(b12 + 6), iv = v3(b12 + 9), sunp = v3(sun);
    const auto& tris = Arr<S>::tris(s);
    const S* norms = Arr<S>::norms(s);
    const uint32_t cap = std::max<uint32_t>(1, s.depth);                    // a push per level: <= depth - 1 entries
    uint64_t primary = 0, shadow = 0, hits = 0, steps = 0, tests = 0;
    int overflow = 0;
#pragma omp parallel num_threads(threads > 0 ? threads : omp_get_max_threads()) reduction(+ : primary, shadow, hits, steps, tests) reduction(| : overflow)
    {
        std::vector<uint32_t> stack(cap);
#pragma omp for schedule(dynamic, 1)
        for (long long jj = 0; jj < (long long)H; ++jj) {
            const size_t j = size_t(jj);
            bool ov = false;
            for (size_t i = 0; i < W; ++i) {
                const V3<S> view = primary_view<G>(dir, iu, iv, i, j, W, H);
                HitRec<S> h{0, 0, 0, 0};
                ++primary;
                S c[3] = {0, 0, 0};                                          // a miss: render.hpp:116-117
                if (trace_closest<G, R>(s, eye, view, S(0), Arr<S>::big, stack.data(), cap, h, steps, tests, ov)) {
                    ++hits;
                    const auto& tr = tris[h.slot];
                    const V3<S> normal = normalize_g<G>(v3(tr.n));
                    if (!full) {                                             // render.hpp:123-125 (primary only)
                        c[0] = std::fabs(normal.x); c[1] = std::fabs(normal.y); c[2] = std::fabs(normal.z);
                    } else {
                        const V3<S> p = hit_point<G>(tr, normal, h.u, h.v);
                        const V3<S> sun_line = normalize_g<G>(sunp - p);     // render.hpp:135
                        HitRec<S> hs{0, 0, 0, 0};
                        ++shadow;
                        if (trace_closest<G, R>(s, p, sun_line, S(0), Arr<S>::big, stack.data(), cap, hs, steps, tests, ov)) {
                            ++hits;                                          // render.hpp:146-149: occluded, RGB 0
                        } else {
                            float col[3];
                            shade<G>(sun_line, norms + 9 * size_t(s.orig[h.slot]), view, h.u, h.v, col);
                            c[0] = col[0]; c[1] = col[1]; c[2] = col[2];
                        }
                    }
                }
                const size_t px = W * j + i;                                 // render.hpp:107
                if (pixels) { pixels[3 * px] = c[0]; pixels[3 * px + 1] = c[1]; pixels[3 * px + 2] = c[2]; }
                if (rgb8) {                                                  // static.cpp:135-147: top row first
                    uint8_t* q = rgb8 + 3 * (W * (H - 1 - j) + i);
                    q[0] = quantize(c[0]); q[1] = quantize(c[1]); q[2] = quantize(c[2]);
                }
            }
            overflow |= ov ? 1 : 0;
        }
    }
    tot.primary = primary; tot.shadow = shadow; tot.hits = hits; tot.steps = steps; tot.tests = tests;
    tot.overflow = overflow != 0;
}

template <class S>
int render_cpu(const ceres_cpu_scene* scene, const S* basis12, const S* sun, int mode, S* pixels, uint8_t* rgb8, size_t width,
               size_t height, ceres_stats* stats, int threads) {
    if (!scene || !basis12 || !sun || width == 0 || height == 0) return set_error(CERES_EINVAL, "render (cpu): bad argument");
    if (scene->f64 != std::is_same<S, double>::value)
        return set_error(CERES_EINVAL, "render (cpu): the scene is %s precision", scene->f64 ? "double" : "single");
    if (width > 0xffffffu || height > 0xffffffu) return set_error(CERES_EINVAL, "render (cpu): image too large");
    if (mode & CERES_MODE_QBVH4) return set_error(CERES_EUNSUPPORTED, "render (cpu): CERES_MODE_QBVH4 is a GPU mode");
    if (scene->f64 && (mode & CERES_MODE_ROBUST))
        return set_error(CERES_EUNSUPPORTED, "render (cpu): CERES_MODE_ROBUST takes float scenes");
    const int base = mode & ~(CERES_MODE_ROBUST | CERES_MODE_FMA);
    if (base != CERES_MODE_FULL && base != CERES_MODE_PRIMARY) return set_error(CERES_EINVAL, "render (cpu): bad mode %d", mode);
    const bool full = base == CERES_MODE_FULL, g = (mode & CERES_MODE_FMA) != 0, r = (mode & CERES_MODE_ROBUST) != 0;
    const auto t0 = std::chrono::steady_clock::now();
    Counts c;
    if constexpr (std::is_same<S, float>::value) {
        if (g && r) render_rows<true, true, S>(*scene, basis12, sun, full, pixels, rgb8, width, height, threads, c);
        else if (r) render_rows<false, true, S>(*scene, basis12, sun, full, pixels, rgb8, width, height, threads, c);
    }
    if (!r) {
        if (g) render_rows<true, false, S>(*scene, basis12, sun, full, pixels, rgb8, width, height, threads, c);
        else render_rows<false, false, S>(*scene, basis12, sun, full, pixels, rgb8, width, height, threads, c);
    }
    if (c.overflow) return set_error(CERES_ESTACK, "render (cpu): traversal stack overflow");
    if (stats) {
        stats->rays = c.primary + c.shadow;
        stats->hits = c.hits;
        stats->primary_rays = c.primary;
        stats->shadow_rays = c.shadow;
        stats->node_pairs = c.steps;
        stats->tri_tests = c.tests;
        stats->ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    return CERES_OK;
}

// ceres_trace_rays_cpu / ceres_trace_rays_cpu_f64: closest hit and / or occlusion of caller-supplied
// ray32 / ray64 records, rays spread over OpenMP threads (each ray's result depends on that ray alone).
struct Ray32 { float o[3], d[3], tmin, tmax; };
struct Hit16 { int32_t prim; float t, u, v; };
struct Ray64 { double o[3], d[3], tmin, tmax; };
struct Hit32 { int32_t prim; uint32_t reserved; double t, u, v; };
static_assert(sizeof(Ray32) == 32 && sizeof(Hit16) == 16, "ray32 / hit16");
static_assert(sizeof(Ray64) == 64 && sizeof(Hit32) == 32, "ray64 / hit32");
template <class S> struct Rec;
template <> struct Rec<float> {
    using Ray = Ray32; using Hit = Hit16;
    static Hit16 hit(int32_t prim, float t, float u, float v) { return Hit16{prim, t, u, v}; }
};
template <> struct Rec<double> {
    using Ray = Ray64; using Hit = Hit32;
    static Hit32 hit(int32_t prim, double t, double u, double v) { return Hit32{prim, 0u, t, u, v}; }
};

template <bool G, bool R, class S>
void trace_rays(const ceres_cpu_scene& s, const typename Rec<S>::Ray* rays, size_t n, typename Rec<S>::Hit* hits, uint8_t* occluded,
                int threads, Counts& tot) {
    const uint32_t cap = std::max<uint32_t>(1, s.depth);
    uint64_t nhit = 0, steps = 0, tests = 0;
    int overflow = 0;
#pragma omp parallel num_threads(threads > 0 ? threads : omp_get_max_threads()) reduction(+ : nhit, steps, tests) reduction(| : overflow)
    {
        std::vector<uint32_t> stack(cap);
#pragma omp for schedule(dynamic, 256)
        for (long long kk = 0; kk < (long long)n; ++kk) {
            const auto& r = rays[kk];
            const V3<S> o = v3(r.o), d = v3(r.d);
            bool ov = false, hit = false, occ = false;
            // a NaN bound fails every box and triangle test of the reference (robust_max(x, NaN) is NaN,
            // utilities.hpp:58-70; max_nn would drop it): the empty window [+inf, -inf] fails the same tests
            const bool nan = std::isnan(r.tmin) || std::isnan(r.tmax);
            const S tmin = nan ? S(INFINITY) : r.tmin, tmax = nan ? S(-INFINITY) : r.tmax;
            if (hits) {
                HitRec<S> h{0, 0, 0, 0};
                hit = trace_closest<G, R>(s, o, d, tmin, tmax, stack.data(), cap, h, steps, tests, ov);
                hits[kk] = hit ? Rec<S>::hit(int32_t(s.orig[h.slot]), h.t, h.u, h.v) : Rec<S>::hit(-1, S(0), S(0), S(0));
            }
            if (occluded) {
                occ = trace_any<G, R>(s, o, d, tmin, tmax, stack.data(), cap, ov);
                occluded[kk] = occ ? 1 : 0;
            }
            nhit += (hits ? hit : occ) ? 1 : 0;
            overflow |= ov ? 1 : 0;
        }
    }
    tot.primary = n; tot.hits = nhit; tot.steps = steps; tot.tests = tests; tot.overflow = overflow != 0;
}

// The argument rules and the dispatch of both precisions (`name`: the entry point, for messages).
template <class S>
int trace_rays_cpu(const char* name, const ceres_cpu_scene* scene, const void* rays_, size_t n_rays, int mode, void* hits_,
                   uint8_t* occluded, ceres_stats* stats, int threads) {
    constexpr bool f64 = std::is_same<S, double>::value;
    if (!scene) return set_error(CERES_EINVAL, "%s: null scene", name);
    if (scene->f64 != f64)
        return set_error(CERES_EUNSUPPORTED, "%s: the scene is %s precision", name, scene->f64 ? "double" : "single");
    if (mode & ~(CERES_MODE_FMA | CERES_MODE_ROBUST))
        return set_error(CERES_EINVAL, "%s: bad mode %d (%s)", name, mode,
                         f64 ? "0 or CERES_MODE_FMA" : "0, CERES_MODE_FMA, CERES_MODE_ROBUST or both");
    if (f64 && (mode & CERES_MODE_ROBUST)) return set_error(CERES_EUNSUPPORTED, "%s: CERES_MODE_ROBUST takes float scenes", name);
    if (!hits_ && !occluded) return set_error(CERES_EINVAL, "%s: neither hits nor occluded asked for", name);
    if (n_rays >= (size_t(1) << 31)) return set_error(CERES_EUNSUPPORTED, "%s: %zu rays (below 2^31 per call)", name, n_rays);
    Counts c;
    const auto t0 = std::chrono::steady_clock::now();
    if (n_rays) {
        if (!rays_) return set_error(CERES_EINVAL, "%s: null rays", name);
        const auto* rays = static_cast<const typename Rec<S>::Ray*>(rays_);
        auto* hits = static_cast<typename Rec<S>::Hit*>(hits_);
        const bool g = (mode & CERES_MODE_FMA) != 0, r = (mode & CERES_MODE_ROBUST) != 0;
        if constexpr (!f64) {
            if (g && r) trace_rays<true, true, S>(*scene, rays, n_rays, hits, occluded, threads, c);
            else if (r) trace_rays<false, true, S>(*scene, rays, n_rays, hits, occluded, threads, c);
        }
        if (!r) {
            if (g) trace_rays<true, false, S>(*scene, rays, n_rays, hits, occluded, threads, c);
            else trace_rays<false, false, S>(*scene, rays, n_rays, hits, occluded, threads, c);
        }
    }
    if (c.overflow) return set_error(CERES_ESTACK, "%s: traversal stack overflow", name);
    if (stats) {
        stats->rays = c.primary; stats->hits = c.hits; stats->primary_rays = c.primary; stats->shadow_rays = 0;
        stats->node_pairs = c.steps; stats->tri_tests = c.tests;
        stats->ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    return CERES_OK;
}

// ceres_trace_rays_all_cpu / ceres_trace_rays_all_cpu_f64: the all-hits query of caller-supplied ray32 /
// ray64 records, rays spread over OpenMP threads; each ray's row is its sorted buffer, then misses.
template <bool G, bool R, class S>
void trace_rays_all(const ceres_cpu_scene& s, const typename Rec<S>::Ray* rays, size_t n, uint32_t max_hits, uint32_t* counts,
                    typename Rec<S>::Hit* hits, int threads, Counts& tot) {
    const uint32_t cap = std::max<uint32_t>(1, s.depth);
    uint64_t nhit = 0, steps = 0, tests = 0;
    int overflow = 0;
#pragma omp parallel num_threads(threads > 0 ? threads : omp_get_max_threads()) reduction(+ : nhit, steps, tests) reduction(| : overflow)
    {
        std::vector<uint32_t> stack(cap);
        std::vector<HitRec<S>> best(hits ? max_hits : 0);
#pragma omp for schedule(dynamic, 256)
        for (long long kk = 0; kk < (long long)n; ++kk) {
            const auto& r = rays[kk];
            const V3<S> o = v3(r.o), d = v3(r.d);
            bool ov = false;
            const bool nan = std::isnan(r.tmin) || std::isnan(r.tmax);   // the empty window, as trace_rays
            const S tmin = nan ? S(INFINITY) : r.tmin, tmax = nan ? S(-INFINITY) : r.tmax;
            uint32_t kept = 0;
            const uint32_t count = trace_all<G, R>(s, o, d, tmin, tmax, stack.data(), cap, hits ? best.data() : nullptr, max_hits,
                                                   &kept, steps, tests, ov);
            if (counts) counts[kk] = count;
            if (hits) {
                auto* row = hits + size_t(kk) * max_hits;
                for (uint32_t i = 0; i < max_hits; ++i)
                    row[i] = i < kept ? Rec<S>::hit(int32_t(s.orig[best[i].slot]), best[i].t, best[i].u, best[i].v)
                                      : Rec<S>::hit(-1, S(0), S(0), S(0));
            }
            nhit += count ? 1 : 0;
            overflow |= ov ? 1 : 0;
        }
    }
    tot.primary = n; tot.hits = nhit; tot.steps = steps; tot.tests = tests; tot.overflow = overflow != 0;
}

// The argument rules the all-hits and the complete-list calls of both precisions share, up to the ray
// count (`name`: the entry point, for messages).  The float-named calls refuse a double scene in their
// own words; the _f64 calls have no robust intersector, as ceres_trace_rays_cpu_f64.
template <class S>
int check_all_scene_mode(const char* name, const ceres_cpu_scene* scene, int mode) {
    constexpr bool f64 = std::is_same<S, double>::value;
    if (!scene) return set_error(CERES_EINVAL, "%s: null scene", name);
    if (!f64 && scene->f64) return set_error(CERES_EUNSUPPORTED, "%s: all-hits queries take float scenes", name);
    if (f64 && !scene->f64) return set_error(CERES_EUNSUPPORTED, "%s: the scene is single precision", name);
    if (mode & ~(CERES_MODE_FMA | CERES_MODE_ROBUST))
        return set_error(CERES_EINVAL, "%s: bad mode %d (%s)", name, mode,
                         f64 ? "0 or CERES_MODE_FMA" : "0, CERES_MODE_FMA, CERES_MODE_ROBUST or both");
    if (f64 && (mode & CERES_MODE_ROBUST)) return set_error(CERES_EUNSUPPORTED, "%s: CERES_MODE_ROBUST takes float scenes", name);
    return CERES_OK;
}

template <class S>
int trace_rays_all_cpu(const char* name, const ceres_cpu_scene* scene, const void* rays_, size_t n_rays, int mode, uint32_t max_hits,
                       uint32_t* counts, void* hits_, ceres_stats* stats, int threads) {
    constexpr bool f64 = std::is_same<S, double>::value;
    if (const int rc = check_all_scene_mode<S>(name, scene, mode)) return rc;
    if (!counts && !hits_) return set_error(CERES_EINVAL, "%s: neither counts nor hits asked for", name);
    if (hits_ && (max_hits == 0 || max_hits > CERES_MAX_HITS))
        return set_error(CERES_EINVAL, "%s: max_hits %u (1 .. %d with a hit buffer)", name, max_hits, CERES_MAX_HITS);
    if (n_rays >= (size_t(1) << 31)) return set_error(CERES_EUNSUPPORTED, "%s: %zu rays (below 2^31 per call)", name, n_rays);
    Counts c;
    const auto t0 = std::chrono::steady_clock::now();
    if (n_rays) {
        if (!rays_) return set_error(CERES_EINVAL, "%s: null rays", name);
        const auto* rays = static_cast<const typename Rec<S>::Ray*>(rays_);
        auto* hits = static_cast<typename Rec<S>::Hit*>(hits_);
        const bool g = (mode & CERES_MODE_FMA) != 0, r = (mode & CERES_MODE_ROBUST) != 0;
        if constexpr (!f64) {
            if (g && r) trace_rays_all<true, true, S>(*scene, rays, n_rays, max_hits, counts, hits, threads, c);
            else if (r) trace_rays_all<false, true, S>(*scene, rays, n_rays, max_hits, counts, hits, threads, c);
        }
        if (!r) {
            if (g) trace_rays_all<true, false, S>(*scene, rays, n_rays, max_hits, counts, hits, threads, c);
            else trace_rays_all<false, false, S>(*scene, rays, n_rays, max_hits, counts, hits, threads, c);
        }
    }
    if (c.overflow) return set_error(CERES_ESTACK, "%s: traversal stack overflow", name);
    if (stats) {
        stats->rays = c.primary; stats->hits = c.hits; stats->primary_rays = c.primary; stats->shadow_rays = 0;
        stats->node_pairs = c.steps; stats->tri_tests = c.tests;
        stats->ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    return CERES_OK;
}

// ceres_trace_rays_lists_cpu / ceres_trace_rays_lists_cpu_f64: the complete hit lists as a CSR pair.  Each
// ray's walk fills a vector, std::sort puts it into key order (t by <, which takes -0 and +0 as equal;
// then the original triangle index -- unique, a triangle sits in one leaf), a prefix sum over the rays
// gives the offsets, and the lists are copied into the caller's buffer if it holds them all.
template <bool G, bool R, class S>
void trace_rays_lists(const ceres_cpu_scene& s, const typename Rec<S>::Ray* rays, size_t n,
                      std::vector<std::vector<typename Rec<S>::Hit>>& lists, int threads, Counts& tot) {
    const uint32_t cap = std::max<uint32_t>(1, s.depth);
    uint64_t nhit = 0, steps = 0, tests = 0;
    int overflow = 0;
#pragma omp parallel num_threads(threads > 0 ? threads : omp_get_max_threads()) reduction(+ : nhit, steps, tests) reduction(| : overflow)
    {
        std::vector<uint32_t> stack(cap);
        std::vector<HitRec<S>> every;
#pragma omp for schedule(dynamic, 256)
        for (long long kk = 0; kk < (long long)n; ++kk) {
            const auto& r = rays[kk];
            const V3<S> o = v3(r.o), d = v3(r.d);
            bool ov = false;
            const bool nan = std::isnan(r.tmin) || std::isnan(r.tmax);   // the empty window, as trace_rays
            const S tmin = nan ? S(INFINITY) : r.tmin, tmax = nan ? S(-INFINITY) : r.tmax;
            every.clear();
            const uint32_t count = trace_all<G, R>(s, o, d, tmin, tmax, stack.data(), cap, static_cast<HitRec<S>*>(nullptr), 0u,
                                                   nullptr, steps, tests, ov, &every);
            std::sort(every.begin(), every.end(), [&](const HitRec<S>& a, const HitRec<S>& b) {
                return a.t < b.t || (a.t == b.t && s.orig[a.slot] < s.orig[b.slot]);
            });
            auto& out = lists[size_t(kk)];
            out.reserve(every.size());
            for (const auto& h : every) out.push_back(Rec<S>::hit(int32_t(s.orig[h.slot]), h.t, h.u, h.v));
            nhit += count ? 1 : 0;
            overflow |= ov ? 1 : 0;
        }
    }
    tot.primary = n; tot.hits = nhit; tot.steps = steps; tot.tests = tests; tot.overflow = overflow != 0;
}

template <class S>
int trace_rays_lists_cpu(const char* name, const ceres_cpu_scene* scene, const void* rays_, size_t n_rays, int mode, uint64_t* offsets,
                         void* hits_, uint64_t capacity, uint64_t* total, ceres_stats* stats, int threads) {
    constexpr bool f64 = std::is_same<S, double>::value;
    using Hit = typename Rec<S>::Hit;
    if (const int rc = check_all_scene_mode<S>(name, scene, mode)) return rc;
    if (!hits_ && capacity) return set_error(CERES_EINVAL, "%s: null hits with capacity %llu", name, (unsigned long long)capacity);
    if (n_rays >= (size_t(1) << 31)) return set_error(CERES_EUNSUPPORTED, "%s: %zu rays (below 2^31 per call)", name, n_rays);
    if (n_rays && !rays_) return set_error(CERES_EINVAL, "%s: null rays", name);
    Counts c;
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<std::vector<Hit>> lists(n_rays);
    if (n_rays) {
        const auto* rays = static_cast<const typename Rec<S>::Ray*>(rays_);
        const bool g = (mode & CERES_MODE_FMA) != 0, r = (mode & CERES_MODE_ROBUST) != 0;
        if constexpr (!f64) {
            if (g && r) trace_rays_lists<true, true, S>(*scene, rays, n_rays, lists, threads, c);
            else if (r) trace_rays_lists<false, true, S>(*scene, rays, n_rays, lists, threads, c);
        }
        if (!r) {
            if (g) trace_rays_lists<true, false, S>(*scene, rays, n_rays, lists, threads, c);
            else trace_rays_lists<false, false, S>(*scene, rays, n_rays, lists, threads, c);
        }
    }
    if (c.overflow) return set_error(CERES_ESTACK, "%s: traversal stack overflow", name);
    std::vector<uint64_t> own;
    if (!offsets) { own.resize(n_rays + 1); offsets = own.data(); }
    uint64_t tot = 0;
    for (size_t k = 0; k < n_rays; ++k) { offsets[k] = tot; tot += lists[k].size(); }
    offsets[n_rays] = tot;
    if (total) *total = tot;
    if (stats) {
        stats->rays = c.primary; stats->hits = c.hits; stats->primary_rays = c.primary; stats->shadow_rays = 0;
        stats->node_pairs = c.steps; stats->tri_tests = c.tests;
    }
    if (capacity < tot)
        return set_error(CERES_ENOMEM, "%s: capacity %llu, the rays have %llu hits", name, (unsigned long long)capacity,
                         (unsigned long long)tot);
    auto* hits = static_cast<Hit*>(hits_);
#pragma omp parallel for schedule(static) num_threads(threads > 0 ? threads : omp_get_max_threads())
    for (long long k = 0; k < (long long)n_rays; ++k)
        if (!lists[size_t(k)].empty()) std::memcpy(hits + offsets[k], lists[size_t(k)].data(), lists[size_t(k)].size() * sizeof(Hit));
    if (stats) stats->ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return CERES_OK;
}

// ceres_shade_rays_cpu / ceres_shade_rays_cpu_f64: render_rows' pixel body (render.hpp:114-150) for
// caller-supplied ray32 / ray64 records -- the closest query of trace_rays (the ray's own window), then
// render_rows' own shadow query and shading with the ray's direction as `view`.  status: 0 miss, 1 lit,
// 2 in shadow.  Pixels are the float colour, widened for double scenes as render_rows stores it.
template <bool G, bool R, class S>
void shade_rays(const ceres_cpu_scene& s, const typename Rec<S>::Ray* rays, size_t n, const S* sun, S* pixels, uint8_t* rgb8,
                typename Rec<S>::Hit* hits, uint8_t* status, int threads, Counts& tot) {
    const V3<S> sunp = v3(sun);
    const auto& tris = Arr<S>::tris(s);
    const S* norms = Arr<S>::norms(s);
    const uint32_t cap = std::max<uint32_t>(1, s.depth);
    uint64_t nhit = 0, nblocked = 0, steps = 0, tests = 0;
    int overflow = 0;
#pragma omp parallel num_threads(threads > 0 ? threads : omp_get_max_threads()) reduction(+ : nhit, nblocked, steps, tests) reduction(| : overflow)
    {
        std::vector<uint32_t> stack(cap);
#pragma omp for schedule(dynamic, 256)
        for (long long kk = 0; kk < (long long)n; ++kk) {
            const auto& r = rays[kk];
            const V3<S> o = v3(r.o), d = v3(r.d);
            bool ov = false;
            const bool nan = std::isnan(r.tmin) || std::isnan(r.tmax);          // the empty window, as trace_rays
            const S tmin = nan ? S(INFINITY) : r.tmin, tmax = nan ? S(-INFINITY) : r.tmax;
            HitRec<S> h{0, 0, 0, 0};
            const bool hit = trace_closest<G, R>(s, o, d, tmin, tmax, stack.data(), cap, h, steps, tests, ov);
            if (hits) hits[kk] = hit ? Rec<S>::hit(int32_t(s.orig[h.slot]), h.t, h.u, h.v) : Rec<S>::hit(-1, S(0), S(0), S(0));
            float c[3] = {0, 0, 0};                                              // a miss: render.hpp:116-117
            bool blocked = false;
            if (hit) {
                ++nhit;
                const auto& tr = tris[h.slot];
                const V3<S> normal = normalize_g<G>(v3(tr.n));
                const V3<S> p = hit_point<G>(tr, normal, h.u, h.v);
                const V3<S> sun_line = normalize_g<G>(sunp - p);                // render.hpp:135
                HitRec<S> hs{0, 0, 0, 0};
                blocked = trace_closest<G, R>(s, p, sun_line, S(0), Arr<S>::big, stack.data(), cap, hs, steps, tests, ov);
                if (blocked) ++nblocked;                                         // render.hpp:146-149: occluded, RGB 0
                else shade<G>(sun_line, norms + 9 * size_t(s.orig[h.slot]), d, h.u, h.v, c);
            }
            if (pixels) { pixels[3 * kk] = c[0]; pixels[3 * kk + 1] = c[1]; pixels[3 * kk + 2] = c[2]; }
            if (rgb8) {
                rgb8[3 * kk] = quantize(S(c[0])); rgb8[3 * kk + 1] = quantize(S(c[1])); rgb8[3 * kk + 2] = quantize(S(c[2]));
            }
            if (status) status[kk] = hit ? (blocked ? 2 : 1) : 0;
            overflow |= ov ? 1 : 0;
        }
    }
    tot.primary = n; tot.shadow = nhit; tot.hits = nhit + nblocked; tot.steps = steps; tot.tests = tests;
    tot.overflow = overflow != 0;
}

// The argument rules and the dispatch of both precisions (`name`: the entry point, for messages).
template <class S>
int shade_rays_cpu(const char* name, const ceres_cpu_scene* scene, const void* rays_, size_t n_rays, const S* sun, int mode,
                   S* pixels, uint8_t* rgb8, void* hits_, uint8_t* status, ceres_stats* stats, int threads) {
    constexpr bool f64 = std::is_same<S, double>::value;
    if (!scene) return set_error(CERES_EINVAL, "%s: null scene", name);
    if (scene->f64 != f64)
        return set_error(CERES_EUNSUPPORTED, "%s: the scene is %s precision (use %s)", name, scene->f64 ? "double" : "single",
                         scene->f64 ? "ceres_shade_rays_cpu_f64" : "ceres_shade_rays_cpu");
    if (mode & ~(CERES_MODE_FMA | CERES_MODE_ROBUST))
        return set_error(CERES_EINVAL, "%s: bad mode %d (%s)", name, mode,
                         f64 ? "0 or CERES_MODE_FMA" : "0, CERES_MODE_FMA, CERES_MODE_ROBUST or both");
    if (f64 && (mode & CERES_MODE_ROBUST)) return set_error(CERES_EUNSUPPORTED, "%s: CERES_MODE_ROBUST takes float scenes", name);
    if (!pixels && !rgb8 && !hits_ && !status)
        return set_error(CERES_EINVAL, "%s: none of pixels, rgb8, hits and status asked for", name);
    if (n_rays >= (size_t(1) << 31)) return set_error(CERES_EUNSUPPORTED, "%s: %zu rays (below 2^31 per call)", name, n_rays);
    Counts c;
    const auto t0 = std::chrono::steady_clock::now();
    if (n_rays) {
        if (!rays_ || !sun) return set_error(CERES_EINVAL, "%s: null rays or sun", name);
        const auto* rays = static_cast<const typename Rec<S>::Ray*>(rays_);
        auto* hits = static_cast<typename Rec<S>::Hit*>(hits_);
        const bool g = (mode & CERES_MODE_FMA) != 0, r = (mode & CERES_MODE_ROBUST) != 0;
        if constexpr (!f64) {
            if (g && r) shade_rays<true, true, S>(*scene, rays, n_rays, sun, pixels, rgb8, hits, status, threads, c);
            else if (r) shade_rays<false, true, S>(*scene, rays, n_rays, sun, pixels, rgb8, hits, status, threads, c);
        }
        if (!r) {
            if (g) shade_rays<true, false, S>(*scene, rays, n_rays, sun, pixels, rgb8, hits, status, threads, c);
            else shade_rays<false, false, S>(*scene, rays, n_rays, sun, pixels, rgb8, hits, status, threads, c);
        }
    }
    if (c.overflow) return set_error(CERES_ESTACK, "%s: traversal stack overflow", name);
    if (stats) {
        stats->rays = c.primary + c.shadow; stats->hits = c.hits; stats->primary_rays = c.primary; stats->shadow_rays = c.shadow;
        stats->node_pairs = c.steps; stats->tri_tests = c.tests;
        stats->ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    return CERES_OK;
}

// The W x H ray records of a view's primary rays (ray j*W + i, origin = eye, window [0, max]).
template <class S>
int camera_rays(const char* name, const S* basis12, size_t width, size_t height, int arith, void* rays_) {
    if (!basis12 || !rays_ || width == 0 || height == 0) return set_error(CERES_EINVAL, "%s: bad argument", name);
    if (arith != CERES_ARITH_EXACT && arith != CERES_ARITH_FMA) return set_error(CERES_EINVAL, "%s: bad arith %d", name, arith);
    if (width > 0xffffffu || height > 0xffffffu) return set_error(CERES_EINVAL, "%s: image too large", name);
    const V3<S> eye = v3(basis12), dir = v3(basis12 + 3), iu = v3(basis12 + 6), iv = v3(basis12 + 9);
    auto* rays = static_cast<typename Rec<S>::Ray*>(rays_);
    for (size_t j = 0; j < height; ++j)
        for (size_t i = 0; i < width; ++i) {
            const V3<S> d = arith == CERES_ARITH_FMA ? primary_view<true>(dir, iu, iv, i, j, width, height)
                                                     : primary_view<false>(dir, iu, iv, i, j, width, height);
            rays[width * j + i] = typename Rec<S>::Ray{{eye.x, eye.y, eye.z}, {d.x, d.y, d.z}, S(0), Arr<S>::big};
        }
    return CERES_OK;
}

// Refit (hierarchy_refitter.hpp:17-32 with the leaf update): the moved triangles regathered into
// leaf order, then every box recomputed.  relayout_bvh numbers a child pair after its parent (it
// is appended while the parent is visited), so ONE REVERSE PASS over the pairs meets both
// children of every inner node before the node itself; the pass checks that.  min / max only:
// exact, order-independent.
template <class S, class Pair, class Tri>
int refit_cpu(std::vector<Pair>& pairs, std::vector<Tri>& tris, const std::vector<uint32_t>& orig, const Tri* moved, bool root_leaf) {
    const size_t n_tri = tris.size();
    for (size_t k = 0; k < n_tri; ++k)
        if (orig[k] >= n_tri) return set_error(CERES_EINVAL, "refit: original index out of range");
    if (!root_leaf)
        for (size_t k = 0; k < pairs.size(); ++k) {
            const Pair& P = pairs[k];
            const uint32_t cnt[2] = {P.lcount, P.rcount}, first[2] = {P.lfirst, P.rfirst};
            for (int side = 0; side < 2; ++side)
                if (cnt[side] ? uint64_t(first[side]) + cnt[side] > n_tri : (first[side] <= k || first[side] >= pairs.size()))
                    return set_error(CERES_EINVAL, "refit: sibling pairs are not numbered parents first");
        }
    for (size_t k = 0; k < n_tri; ++k) tris[k] = moved[orig[k]];
    if (root_leaf) return CERES_OK;
    auto lesser = [](S a, S b) { return b < a ? b : a; };
    auto greater = [](S a, S b) { return a < b ? b : a; };
    for (size_t k = pairs.size(); k-- > 0;) {
        Pair& P = pairs[k];
        const uint32_t cnt[2] = {P.lcount, P.rcount}, first[2] = {P.lfirst, P.rfirst};
        S* box[2] = {P.lb, P.rb};
        for (int side = 0; side < 2; ++side) {
            S* b = box[side];
            if (!cnt[side]) {
                const Pair& C = pairs[first[side]];
                for (int a = 0; a < 6; a += 2) { b[a] = lesser(C.lb[a], C.rb[a]); b[a + 1] = greater(C.lb[a + 1], C.rb[a + 1]); }
                continue;
            }
            b[0] = b[2] = b[4] = std::numeric_limits<S>::infinity();
            b[1] = b[3] = b[5] = -std::numeric_limits<S>::infinity();
            for (uint32_t t = first[side]; t < first[side] + cnt[side]; ++t) {
                const Tri& T = tris[t];
                for (int a = 0; a < 3; ++a) {                        // Triangle::bounding_box(), triangle.hpp:36-44
                    const S p[3] = {T.p0[a], T.p0[a] - T.e1[a], T.p0[a] + T.e2[a]};
                    for (S v : p) { b[2 * a] = lesser(b[2 * a], v); b[2 * a + 1] = greater(b[2 * a + 1], v); }
                }
            }
        }
    }
    return CERES_OK;
}

// Scene upkeep (ceres_render.h "scene upkeep").  The SAH cost, SahBasedAlgorithm::compute_cost
// (sah_based_algorithm.hpp:21-32, traversal_cost = 1) over the sibling pairs: half areas in double on
// the stored bounds, one serial sum in record order (the CPU path is not hot), ROOT = the union of pair
// 0's boxes, the division as written.
template <class S> inline double half_area(const S* b) {
    const double d0 = double(b[1]) - double(b[0]), d1 = double(b[3]) - double(b[2]), d2 = double(b[5]) - double(b[4]);
    return (d0 + d1) * d2 + d0 * d1;
}
template <class Pair>
double sah_cost_cpu(const std::vector<Pair>& pairs, uint32_t root_leaf_count) {
    if (root_leaf_count || pairs.empty()) return double(root_leaf_count);
    double sum = 0.0;
    for (const Pair& P : pairs) {
        sum += half_area(P.lb) * double(P.lcount ? P.lcount : 1u);
        sum += half_area(P.rb) * double(P.rcount ? P.rcount : 1u);
    }
    const Pair& P = pairs[0];
    decltype(P.lb[0] + P.lb[0]) root[6];
    for (int k = 0; k < 6; k += 2) {
        root[k] = P.rb[k] < P.lb[k] ? P.rb[k] : P.lb[k];
        root[k + 1] = P.lb[k + 1] < P.rb[k + 1] ? P.rb[k + 1] : P.lb[k + 1];
    }
    const double ha = half_area(root);
    return (ha + sum) / ha;
}
double scene_cost(const ceres_cpu_scene& s) {
    return s.f64 ? sah_cost_cpu(s.pairs64, s.root_leaf_count) : sah_cost_cpu(s.pairs, s.root_leaf_count);
}

// The host builder and relayout of each scalar type, and the scene's arrays they fill.
template <class S> struct Up;
template <> struct Up<float> {
    using Node = uint32_t; using Tri = Tri48;
    static int build(const float* t, size_t n, Node** nodes, size_t* m, uint64_t** prim, int arith) {
        return ceres_bvh_build_arith(t, n, nodes, m, prim, arith);
    }
    static int relayout(const Node* nodes, size_t m, const uint64_t* prim, size_t n, const float* t, ceres_cpu_scene& s) {
        return relayout_bvh(reinterpret_cast<const RefNode*>(nodes), m, prim, n, reinterpret_cast<const Tri48*>(t), s.pairs, s.tris,
                            s.orig, s.depth, s.root_leaf_count, s.root_leaf_first);
    }
    static void adopt(ceres_cpu_scene& s, ceres_cpu_scene& from) { s.pairs.swap(from.pairs); s.tris.swap(from.tris); }
    static std::vector<float>& norms(ceres_cpu_scene& s) { return s.norms; }
    static size_t n_tri(const ceres_cpu_scene& s) { return s.tris.size(); }
    static int refit(ceres_cpu_scene* s, const float* t, size_t n, const float* nn) { return ceres_cpu_scene_refit(s, t, n, nn); }
};
template <> struct Up<double> {
    using Node = uint64_t; using Tri = Tri96;
    static int build(const double* t, size_t n, Node** nodes, size_t* m, uint64_t** prim, int arith) {
        return ceres_bvh_build_f64_arith(t, n, nodes, m, prim, arith);
    }
    static int relayout(const Node* nodes, size_t m, const uint64_t* prim, size_t n, const double* t, ceres_cpu_scene& s) {
        return relayout_bvh64(reinterpret_cast<const RefNode64*>(nodes), m, prim, n, reinterpret_cast<const Tri96*>(t), s.pairs64,
                              s.tris64, s.orig, s.depth, s.root_leaf_count, s.root_leaf_first);
    }
    static void adopt(ceres_cpu_scene& s, ceres_cpu_scene& from) { s.pairs64.swap(from.pairs64); s.tris64.swap(from.tris64); }
    static std::vector<double>& norms(ceres_cpu_scene& s) { return s.norms64; }
    static size_t n_tri(const ceres_cpu_scene& s) { return s.tris64.size(); }
    static int refit(ceres_cpu_scene* s, const double* t, size_t n, const double* nn) { return ceres_cpu_scene_refit_f64(s, t, n, nn); }
};

// every refusal of a rebuild or an update, before anything is written
template <class S>
int check_moved(const char* who, const ceres_cpu_scene* s, const S* tri, size_t n_tri, int arith) {
    constexpr bool f64 = std::is_same<S, double>::value;
    if (!s || !tri) return set_error(CERES_EINVAL, "%s: null argument", who);
    if (s->f64 != f64) return set_error(CERES_EINVAL, "%s: the scene is a %s scene", who, s->f64 ? "double" : "float");
    if (n_tri != Up<S>::n_tri(*s)) return set_error(CERES_EINVAL, "%s: %zu triangles, the scene has %zu", who, n_tri, Up<S>::n_tri(*s));
    if (arith != CERES_ARITH_EXACT && arith != CERES_ARITH_FMA) return set_error(CERES_EINVAL, "%s: unknown arithmetic %d", who, arith);
    return CERES_OK;
}

// arguments already checked: the host build and relayout into a scratch scene, adopted only when complete
template <class S>
int rebuild_cpu(ceres_cpu_scene* s, const S* tri, size_t n_tri, const S* norm, int arith) {
    typename Up<S>::Node* nodes = nullptr;
    uint64_t* prim = nullptr;
    size_t n_nodes = 0;
    if (int rc = Up<S>::build(tri, n_tri, &nodes, &n_nodes, &prim, arith)) return rc;
    int rc = CERES_OK;
    try {
        ceres_cpu_scene fresh;
        rc = Up<S>::relayout(nodes, n_nodes, prim, n_tri, tri, fresh);
        if (rc == CERES_OK) {
            if (norm) Up<S>::norms(*s).assign(norm, norm + 9 * n_tri);
            Up<S>::adopt(*s, fresh);
            s->orig.swap(fresh.orig);
            s->depth = fresh.depth; s->root_leaf_count = fresh.root_leaf_count; s->root_leaf_first = fresh.root_leaf_first;
            s->built_cost = scene_cost(*s);                          // the new tree is the baseline
            s->built_cost_known = true;
        }
    } catch (const std::bad_alloc&) {
        rc = set_error(CERES_ENOMEM, "out of host memory");
    }
    ceres_free(nodes); ceres_free(prim);
    return rc;
}

template <class S>
int update_cpu(const char* who, ceres_cpu_scene* s, const S* tri, size_t n_tri, const S* norm, int arith, double max_ratio,
               ceres_update_info* info) {
    if (int rc = check_moved<S>(who, s, tri, n_tri, arith)) return rc;
    if (!(max_ratio > 0.0)) return set_error(CERES_EINVAL, "%s: max_ratio must be positive (+inf: never rebuild)", who);
    if (!s->built_cost_known) {                                      // the tree as first seen is the baseline
        s->built_cost = scene_cost(*s);
        s->built_cost_known = true;
    }
    if (int rc = Up<S>::refit(s, tri, n_tri, norm)) return rc;
    ceres_update_info u{};
    u.cost = u.new_cost = scene_cost(*s);
    u.built_cost = s->built_cost;
    if (u.cost > max_ratio * u.built_cost) {                         // false for a NaN on either side
        if (int rc = rebuild_cpu<S>(s, tri, n_tri, norm, arith)) return rc;
        u.rebuilt = 1;
        u.new_cost = s->built_cost;
    }
    if (info) *info = u;
    return CERES_OK;
}

// The coherent ray order on the host: ray_key.hpp's key per ray, then a stable sort of the indices --
// the array ceres_ray_order_device writes, entry for entry.
template <class S>
int ray_order_cpu(const char* name, const ceres_cpu_scene* scene, const void* rays_, size_t n_rays, uint32_t* order) {
    constexpr bool f64 = std::is_same<S, double>::value;
    if (!scene) return set_error(CERES_EINVAL, "%s: null scene", name);
    if (scene->f64 != f64)
        return set_error(CERES_EUNSUPPORTED, "%s: the scene is %s precision", name, scene->f64 ? "double" : "single");
    if (n_rays >= (size_t(1) << 31)) return set_error(CERES_EUNSUPPORTED, "%s: %zu rays (below 2^31 per call)", name, n_rays);
    if (n_rays == 0) return CERES_OK;
    if (!rays_ || !order) return set_error(CERES_EINVAL, "%s: null rays or order", name);
    const auto& pairs = Arr<S>::pairs(*scene);
    const S zero[6] = {0, 0, 0, 0, 0, 0};
    const bool leaf = scene->root_leaf_count != 0 || pairs.empty();
    const OrderBox<S> box = order_box<S>(leaf ? zero : pairs[0].lb, leaf ? zero : pairs[0].rb, leaf ? 1u : 0u);
    const S* rays = static_cast<const S*>(rays_);
    std::vector<uint32_t> keys;
    try {
        keys.resize(n_rays);
    } catch (const std::bad_alloc&) {
        return set_error(CERES_ENOMEM, "%s: out of host memory", name);
    }
    for (size_t r = 0; r < n_rays; ++r) {
        const S* q = rays + 8 * r;
        const uint32_t sign = (std::signbit(q[3]) ? 1u : 0u) | (std::signbit(q[4]) ? 2u : 0u) | (std::signbit(q[5]) ? 4u : 0u);
        keys[r] = ray_key<S>(q, q + 3, q[6], q[7], sign, box);
        order[r] = uint32_t(r);
    }
    std::stable_sort(order, order + n_rays, [&](uint32_t a, uint32_t b) { return keys[a] < keys[b]; });
    return CERES_OK;
}

// ceres_closest_points_cpu: closest_point.hpp's formula, selection and pruning rule over the scene's pairs
// -- the walk of closest_point.hip (nearer leaf first, the child with the smaller bound next and the other
// pushed with its bound, a stale entry dropped at pop), though the answer does not depend on it.
struct Point16 { float x, y, z, r2max; };
struct Near16 { int32_t prim; float d2, u, v; };
static_assert(sizeof(Point16) == 16 && sizeof(Near16) == 16, "point16 / near16");
struct NearEntry { uint32_t pair; float bound; };

void closest_point(const ceres_cpu_scene& s, const Point16& pt, NearEntry* stack, uint32_t cap, NearBest& best, uint64_t& steps,
                   uint64_t& tests, bool& overflow) {
    const uint32_t n_tri = uint32_t(s.tris.size()), n_pairs = uint32_t(s.pairs.size());
    auto leaf = [&](uint32_t first, uint32_t count) {
        if (first >= n_tri) return;
        const uint32_t end = count < n_tri - first ? first + count : n_tri;
        for (uint32_t k = first; k < end; ++k) {
            float v, w;
            const float d2 = near_tri(pt.x, pt.y, pt.z, s.tris[k].p0, s.tris[k].e1, s.tris[k].e2, v, w);
            const uint32_t o = s.orig[k];
            if (o < n_tri && near_better(d2, o, best)) best = NearBest{d2, int32_t(o), v, w};
        }
        tests += end - first;
    };
    if (s.root_leaf_count) { leaf(s.root_leaf_first, s.root_leaf_count); return; }
    uint32_t sp = 0, cur = 0;
    while (cur < n_pairs) {
        ++steps;
        const SiblingPair& p = s.pairs[cur];
        const float ll = near_box(pt.x, pt.y, pt.z, p.lb[0], p.lb[1], p.lb[2], p.lb[3], p.lb[4], p.lb[5]);
        const float lr = near_box(pt.x, pt.y, pt.z, p.rb[0], p.rb[1], p.rb[2], p.rb[3], p.rb[4], p.rb[5]);
        const bool right_first = lr < ll;
        if (right_first) {
            if (p.rcount && !(lr > best.d2)) leaf(p.rfirst, p.rcount);
            if (p.lcount && !(ll > best.d2)) leaf(p.lfirst, p.lcount);
        } else {
            if (p.lcount && !(ll > best.d2)) leaf(p.lfirst, p.lcount);
            if (p.rcount && !(lr > best.d2)) leaf(p.rfirst, p.rcount);
        }
        const bool go_l = !p.lcount && !(ll > best.d2), go_r = !p.rcount && !(lr > best.d2);
        if (go_l && go_r) {
            if (sp >= cap) { overflow = true; return; }
            stack[sp++] = right_first ? NearEntry{p.lfirst, ll} : NearEntry{p.rfirst, lr};
            cur = right_first ? p.rfirst : p.lfirst;
        } else if (go_l || go_r) {
            cur = go_l ? p.lfirst : p.rfirst;
        } else {
            cur = 0xffffffffu;
            while (sp) {
                --sp;
                if (stack[sp].bound > best.d2) continue;
                cur = stack[sp].pair;
                break;
            }
        }
    }
}

int closest_points_cpu(const ceres_cpu_scene* scene, const void* points_, size_t n_points, void* near_, ceres_stats* stats, int threads) {
    const char* name = "ceres_closest_points_cpu";
    if (!scene) return set_error(CERES_EINVAL, "%s: null scene", name);
    if (scene->f64) return set_error(CERES_EUNSUPPORTED, "%s: closest-point queries take float scenes", name);
    if (!near_) return set_error(CERES_EINVAL, "%s: null output", name);
    if (n_points >= (size_t(1) << 31)) return set_error(CERES_EUNSUPPORTED, "%s: %zu points (below 2^31 per call)", name, n_points);
    if (n_points && !points_) return set_error(CERES_EINVAL, "%s: null points", name);
    const auto t0 = std::chrono::steady_clock::now();
    const auto* points = static_cast<const Point16*>(points_);
    auto* near = static_cast<Near16*>(near_);
    const uint32_t cap = std::max<uint32_t>(1, scene->depth);
    uint64_t found = 0, steps = 0, tests = 0;
    int overflow = 0;
    if (n_points) {
#pragma omp parallel num_threads(threads > 0 ? threads : omp_get_max_threads()) reduction(+ : found, steps, tests) reduction(| : overflow)
        {
            std::vector<NearEntry> stack(cap);
#pragma omp for schedule(dynamic, 256)
            for (long long kk = 0; kk < (long long)n_points; ++kk) {
                NearBest best{points[kk].r2max, -1, 0.f, 0.f};
                bool ov = false;
                closest_point(*scene, points[kk], stack.data(), cap, best, steps, tests, ov);
                near[kk] = best.prim >= 0 ? Near16{best.prim, best.d2, best.u, best.v} : Near16{-1, 0.f, 0.f, 0.f};
                found += best.prim >= 0 ? 1 : 0;
                overflow |= ov ? 1 : 0;
            }
        }
    }
    if (overflow) return set_error(CERES_ESTACK, "%s: traversal stack overflow", name);
    if (stats) {
        stats->rays = n_points; stats->hits = found; stats->primary_rays = n_points; stats->shadow_rays = 0;
        stats->node_pairs = steps; stats->tri_tests = tests;
        stats->ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    return CERES_OK;
}

// ceres_closest_points_cpu_f64: the same walk over pairs64 and tris64 with closest_point64.hpp's arithmetic.
struct Point32 { double x, y, z, r2max; };
struct Near32 { int32_t prim, pad; double d2, u, v; };
static_assert(sizeof(Point32) == 32 && sizeof(Near32) == 32, "point32 / near32");
struct NearEntry64 { uint32_t pair; double bound; };

void closest_point64(const ceres_cpu_scene& s, const Point32& pt, NearEntry64* stack, uint32_t cap, NearBest64& best, uint64_t& steps,
                     uint64_t& tests, bool& overflow) {
    const uint32_t n_tri = uint32_t(s.tris64.size()), n_pairs = uint32_t(s.pairs64.size());
    auto leaf = [&](uint32_t first, uint32_t count) {
        if (first >= n_tri) return;
        const uint32_t end = count < n_tri - first ? first + count : n_tri;
        for (uint32_t k = first; k < end; ++k) {
            double v, w;
            const double d2 = near64_tri(pt.x, pt.y, pt.z, s.tris64[k].p0, s.tris64[k].e1, s.tris64[k].e2, v, w);
            const uint32_t o = s.orig[k];
            if (o < n_tri && near64_better(d2, o, best)) best = NearBest64{d2, int32_t(o), v, w};
        }
        tests += end - first;
    };
    if (s.root_leaf_count) { leaf(s.root_leaf_first, s.root_leaf_count); return; }
    uint32_t sp = 0, cur = 0;
    while (cur < n_pairs) {
        ++steps;
        const SiblingPair64& p = s.pairs64[cur];
        const double ll = near64_box(pt.x, pt.y, pt.z, p.lb[0], p.lb[1], p.lb[2], p.lb[3], p.lb[4], p.lb[5]);
        const double lr = near64_box(pt.x, pt.y, pt.z, p.rb[0], p.rb[1], p.rb[2], p.rb[3], p.rb[4], p.rb[5]);
        const bool right_first = lr < ll;
        if (right_first) {
            if (p.rcount && !(lr > best.d2)) leaf(p.rfirst, p.rcount);
            if (p.lcount && !(ll > best.d2)) leaf(p.lfirst, p.lcount);
        } else {
            if (p.lcount && !(ll > best.d2)) leaf(p.lfirst, p.lcount);
            if (p.rcount && !(lr > best.d2)) leaf(p.rfirst, p.rcount);
        }
        const bool go_l = !p.lcount && !(ll > best.d2), go_r = !p.rcount && !(lr > best.d2);
        if (go_l && go_r) {
            if (sp >= cap) { overflow = true; return; }
            stack[sp++] = right_first ? NearEntry64{p.lfirst, ll} : NearEntry64{p.rfirst, lr};
            cur = right_first ? p.rfirst : p.lfirst;
        } else if (go_l || go_r) {
            cur = go_l ? p.lfirst : p.rfirst;
        } else {
            cur = 0xffffffffu;
            while (sp) {
                --sp;
                if (stack[sp].bound > best.d2) continue;
                cur = stack[sp].pair;
                break;
            }
        }
    }
}

int closest_points_cpu64(const ceres_cpu_scene* scene, const void* points_, size_t n_points, void* near_, ceres_stats* stats, int threads) {
    const char* name = "ceres_closest_points_cpu_f64";
    if (!scene) return set_error(CERES_EINVAL, "%s: null scene", name);
    if (!scene->f64) return set_error(CERES_EUNSUPPORTED, "%s: the _f64 closest-point calls take double scenes", name);
    if (!near_) return set_error(CERES_EINVAL, "%s: null output", name);
    if (n_points >= (size_t(1) << 31)) return set_error(CERES_EUNSUPPORTED, "%s: %zu points (below 2^31 per call)", name, n_points);
    if (n_points && !points_) return set_error(CERES_EINVAL, "%s: null points", name);
    const auto t0 = std::chrono::steady_clock::now();
    const auto* points = static_cast<const Point32*>(points_);
    auto* near = static_cast<Near32*>(near_);
    const uint32_t cap = std::max<uint32_t>(1, scene->depth);
    uint64_t found = 0, steps = 0, tests = 0;
    int overflow = 0;
    if (n_points) {
#pragma omp parallel num_threads(threads > 0 ? threads : omp_get_max_threads()) reduction(+ : found, steps, tests) reduction(| : overflow)
        {
            std::vector<NearEntry64> stack(cap);
#pragma omp for schedule(dynamic, 256)
            for (long long kk = 0; kk < (long long)n_points; ++kk) {
                NearBest64 best{points[kk].r2max, -1, 0.0, 0.0};
                bool ov = false;
                closest_point64(*scene, points[kk], stack.data(), cap, best, steps, tests, ov);
                near[kk] = best.prim >= 0 ? Near32{best.prim, 0, best.d2, best.u, best.v} : Near32{-1, 0, 0.0, 0.0, 0.0};
                found += best.prim >= 0 ? 1 : 0;
                overflow |= ov ? 1 : 0;
            }
        }
    }
    if (overflow) return set_error(CERES_ESTACK, "%s: traversal stack overflow", name);
    if (stats) {
        stats->rays = n_points; stats->hits = found; stats->primary_rays = n_points; stats->shadow_rays = 0;
        stats->node_pairs = steps; stats->tri_tests = tests;
        stats->ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    return CERES_OK;
}

}  // namespace

extern "C" {

int ceres_closest_points_cpu(const ceres_cpu_scene* scene, const void* points16, size_t n_points, void* near16, ceres_stats* stats,
                             int threads) {
    return closest_points_cpu(scene, points16, n_points, near16, stats, threads);
}

int ceres_closest_points_cpu_f64(const ceres_cpu_scene* scene, const void* points32, size_t n_points, void* near32, ceres_stats* stats,
                                 int threads) {
    return closest_points_cpu64(scene, points32, n_points, near32, stats, threads);
}

int ceres_cpu_scene_sah_cost(const ceres_cpu_scene* scene, double* cost) {
    if (!scene || !cost) return set_error(CERES_EINVAL, "ceres_cpu_scene_sah_cost: null argument");
    *cost = scene_cost(*scene);
    return CERES_OK;
}

int ceres_cpu_scene_rebuild(ceres_cpu_scene* scene, const float* tri48, size_t n_tri, const float* norm36, int arith) {
    if (int rc = check_moved<float>("ceres_cpu_scene_rebuild", scene, tri48, n_tri, arith)) return rc;
    return rebuild_cpu<float>(scene, tri48, n_tri, norm36, arith);
}

int ceres_cpu_scene_rebuild_f64(ceres_cpu_scene* scene, const double* tri96, size_t n_tri, const double* norm72, int arith) {
    if (int rc = check_moved<double>("ceres_cpu_scene_rebuild_f64", scene, tri96, n_tri, arith)) return rc;
    return rebuild_cpu<double>(scene, tri96, n_tri, norm72, arith);
}

int ceres_cpu_scene_update(ceres_cpu_scene* scene, const float* tri48, size_t n_tri, const float* norm36, int arith,
                           double max_ratio, ceres_update_info* info) {
    return update_cpu<float>("ceres_cpu_scene_update", scene, tri48, n_tri, norm36, arith, max_ratio, info);
}

int ceres_cpu_scene_update_f64(ceres_cpu_scene* scene, const double* tri96, size_t n_tri, const double* norm72, int arith,
                               double max_ratio, ceres_update_info* info) {
    return update_cpu<double>("ceres_cpu_scene_update_f64", scene, tri96, n_tri, norm72, arith, max_ratio, info);
}

int ceres_shade_rays_cpu(const ceres_cpu_scene* scene, const void* rays32, size_t n_rays, const float sun[3], int mode,
                         float* pixels, uint8_t* rgb8, void* hits16, uint8_t* status, ceres_stats* stats, int threads) {
    return shade_rays_cpu<float>("ceres_shade_rays_cpu", scene, rays32, n_rays, sun, mode, pixels, rgb8, hits16, status, stats,
                                 threads);
}

int ceres_shade_rays_cpu_f64(const ceres_cpu_scene* scene, const void* rays64, size_t n_rays, const double sun[3], int mode,
                             double* pixels, uint8_t* rgb8, void* hits32, uint8_t* status, ceres_stats* stats, int threads) {
    return shade_rays_cpu<double>("ceres_shade_rays_cpu_f64", scene, rays64, n_rays, sun, mode, pixels, rgb8, hits32, status,
                                  stats, threads);
}

int ceres_camera_rays(const float basis12[12], size_t width, size_t height, int arith, void* rays32) {
    return camera_rays<float>("ceres_camera_rays", basis12, width, height, arith, rays32);
}

int ceres_camera_rays_f64(const double basis12[12], size_t width, size_t height, int arith, void* rays64) {
    return camera_rays<double>("ceres_camera_rays_f64", basis12, width, height, arith, rays64);
}

int ceres_trace_rays_cpu(const ceres_cpu_scene* scene, const void* rays32, size_t n_rays, int mode, void* hits16,
                         uint8_t* occluded, ceres_stats* stats, int threads) {
    return trace_rays_cpu<float>("ceres_trace_rays_cpu", scene, rays32, n_rays, mode, hits16, occluded, stats, threads);
}

int ceres_trace_rays_cpu_f64(const ceres_cpu_scene* scene, const void* rays64, size_t n_rays, int mode, void* hits32,
                             uint8_t* occluded, ceres_stats* stats, int threads) {
    return trace_rays_cpu<double>("ceres_trace_rays_cpu_f64", scene, rays64, n_rays, mode, hits32, occluded, stats, threads);
}

int ceres_ray_order_cpu(const ceres_cpu_scene* scene, const void* rays32, size_t n_rays, uint32_t* order) {
    return ray_order_cpu<float>("ceres_ray_order_cpu", scene, rays32, n_rays, order);
}
int ceres_ray_order_cpu_f64(const ceres_cpu_scene* scene, const void* rays64, size_t n_rays, uint32_t* order) {
    return ray_order_cpu<double>("ceres_ray_order_cpu_f64", scene, rays64, n_rays, order);
}

// The order box (ray_key.hpp) as doubles {lo xyz, hi xyz}, and whether the key uses it.
int ceres_cpu_scene_order_box(const ceres_cpu_scene* scene, double box6[6], int* usable) {
    if (!scene || !box6 || !usable) return set_error(CERES_EINVAL, "ceres_cpu_scene_order_box: null argument");
    for (int k = 0; k < 6; ++k) box6[k] = 0.0;
    *usable = 0;
    if (scene->root_leaf_count) return CERES_OK;
    if (scene->f64 && !scene->pairs64.empty()) {
        const OrderBox<double> b = order_box<double>(scene->pairs64[0].lb, scene->pairs64[0].rb, 0u);
        for (int a = 0; a < 3; ++a) { box6[a] = b.lo[a]; box6[3 + a] = b.hi[a]; }
        *usable = b.ok ? 1 : 0;
    } else if (!scene->f64 && !scene->pairs.empty()) {
        const OrderBox<float> b = order_box<float>(scene->pairs[0].lb, scene->pairs[0].rb, 0u);
        for (int a = 0; a < 3; ++a) { box6[a] = double(b.lo[a]); box6[3 + a] = double(b.hi[a]); }
        *usable = b.ok ? 1 : 0;
    }
    return CERES_OK;
}

int ceres_trace_rays_lists_cpu(const ceres_cpu_scene* scene, const void* rays32, size_t n_rays, int mode, uint64_t* offsets,
                               void* hits16, uint64_t capacity, uint64_t* total, ceres_stats* stats, int threads) {
    return trace_rays_lists_cpu<float>("ceres_trace_rays_lists_cpu", scene, rays32, n_rays, mode, offsets, hits16, capacity, total, stats,
                                       threads);
}
int ceres_trace_rays_all_cpu(const ceres_cpu_scene* scene, const void* rays32, size_t n_rays, int mode, uint32_t max_hits,
                             uint32_t* counts, void* hits16, ceres_stats* stats, int threads) {
    return trace_rays_all_cpu<float>("ceres_trace_rays_all_cpu", scene, rays32, n_rays, mode, max_hits, counts, hits16, stats, threads);
}
int ceres_trace_rays_lists_cpu_f64(const ceres_cpu_scene* scene, const void* rays64, size_t n_rays, int mode, uint64_t* offsets,
                                   void* hits32, uint64_t capacity, uint64_t* total, ceres_stats* stats, int threads) {
    return trace_rays_lists_cpu<double>("ceres_trace_rays_lists_cpu_f64", scene, rays64, n_rays, mode, offsets, hits32, capacity, total,
                                        stats, threads);
}
int ceres_trace_rays_all_cpu_f64(const ceres_cpu_scene* scene, const void* rays64, size_t n_rays, int mode, uint32_t max_hits,
                                 uint32_t* counts, void* hits32, ceres_stats* stats, int threads) {
    return trace_rays_all_cpu<double>("ceres_trace_rays_all_cpu_f64", scene, rays64, n_rays, mode, max_hits, counts, hits32, stats,
                                      threads);
}

ceres_cpu_scene* ceres_cpu_scene_create(const float* tri48, size_t n_tri, const float* norm36, const void* nodes32,
                                        size_t n_nodes, const uint64_t* prim64) {
    if (!tri48 || !norm36 || !nodes32 || !prim64 || n_tri == 0 || n_nodes == 0) {
        set_error(CERES_EINVAL, "ceres_cpu_scene_create: empty scene or null argument");
        return nullptr;
    }
    if (n_tri > 0xffffffffull || n_nodes > 0xffffffffull) { set_error(CERES_EUNSUPPORTED, "scene too large"); return nullptr; }
    auto* s = new (std::nothrow) ceres_cpu_scene;
    if (!s) { set_error(CERES_ENOMEM, "out of host memory"); return nullptr; }
    try {
        if (relayout_bvh(static_cast<const RefNode*>(nodes32), n_nodes, prim64, n_tri, reinterpret_cast<const Tri48*>(tri48),
                         s->pairs, s->tris, s->orig, s->depth, s->root_leaf_count, s->root_leaf_first)) {
            delete s;
            return nullptr;
        }
        s->norms.assign(norm36, norm36 + 9 * n_tri);
    } catch (const std::bad_alloc&) {
        delete s;
        set_error(CERES_ENOMEM, "out of host memory");
        return nullptr;
    }
    return s;
}

ceres_cpu_scene* ceres_cpu_scene_create_f64(const double* tri96, size_t n_tri, const double* norm72, const void* nodes64,
                                            size_t n_nodes, const uint64_t* prim64) {
    if (!tri96 || !norm72 || !nodes64 || !prim64 || n_tri == 0 || n_nodes == 0) {
        set_error(CERES_EINVAL, "ceres_cpu_scene_create_f64: empty scene or null argument");
        return nullptr;
    }
    if (n_tri > 0xffffffffull || n_nodes > 0xffffffffull) { set_error(CERES_EUNSUPPORTED, "scene too large"); return nullptr; }
    auto* s = new (std::nothrow) ceres_cpu_scene;
    if (!s) { set_error(CERES_ENOMEM, "out of host memory"); return nullptr; }
    s->f64 = true;
    try {
        if (relayout_bvh64(static_cast<const RefNode64*>(nodes64), n_nodes, prim64, n_tri, reinterpret_cast<const Tri96*>(tri96),
                           s->pairs64, s->tris64, s->orig, s->depth, s->root_leaf_count, s->root_leaf_first)) {
            delete s;
            return nullptr;
        }
        s->norms64.assign(norm72, norm72 + 9 * n_tri);
    } catch (const std::bad_alloc&) {
        delete s;
        set_error(CERES_ENOMEM, "out of host memory");
        return nullptr;
    }
    return s;
}

void ceres_cpu_scene_destroy(ceres_cpu_scene* scene) { delete scene; }

int ceres_cpu_scene_refit(ceres_cpu_scene* scene, const float* tri48, size_t n_tri, const float* norm36) {
    if (!scene || !tri48) return set_error(CERES_EINVAL, "ceres_cpu_scene_refit: null argument");
    if (scene->f64) return set_error(CERES_EINVAL, "ceres_cpu_scene_refit: the scene is a double scene");
    if (n_tri != scene->tris.size()) return set_error(CERES_EINVAL, "ceres_cpu_scene_refit: %zu triangles, the scene has %zu", n_tri, scene->tris.size());
    if (int rc = refit_cpu<float>(scene->pairs, scene->tris, scene->orig, reinterpret_cast<const Tri48*>(tri48), scene->root_leaf_count != 0))
        return rc;
    if (norm36) scene->norms.assign(norm36, norm36 + 9 * n_tri);
    return CERES_OK;
}

int ceres_cpu_scene_refit_f64(ceres_cpu_scene* scene, const double* tri96, size_t n_tri, const double* norm72) {
    if (!scene || !tri96) return set_error(CERES_EINVAL, "ceres_cpu_scene_refit_f64: null argument");
    if (!scene->f64) return set_error(CERES_EINVAL, "ceres_cpu_scene_refit_f64: the scene is a float scene");
    if (n_tri != scene->tris64.size()) return set_error(CERES_EINVAL, "ceres_cpu_scene_refit_f64: %zu triangles, the scene has %zu", n_tri, scene->tris64.size());
    if (int rc = refit_cpu<double>(scene->pairs64, scene->tris64, scene->orig, reinterpret_cast<const Tri96*>(tri96), scene->root_leaf_count != 0))
        return rc;
    if (norm72) scene->norms64.assign(norm72, norm72 + 9 * n_tri);
    return CERES_OK;
}

int ceres_render_cpu_f32(const ceres_cpu_scene* scene, const float basis12[12], const float sun[3], int mode, float* pixels,
                         uint8_t* rgb8, size_t width, size_t height, ceres_stats* stats, int threads) {
    return render_cpu<float>(scene, basis12, sun, mode, pixels, rgb8, width, height, stats, threads);
}

int ceres_render_cpu_f64(const ceres_cpu_scene* scene, const double basis12[12], const double sun[3], int mode,
                         double* pixels, uint8_t* rgb8, size_t width, size_t height, ceres_stats* stats, int threads) {
    return render_cpu<double>(scene, basis12, sun, mode, pixels, rgb8, width, height, stats, threads);
}

}  // extern "C"
