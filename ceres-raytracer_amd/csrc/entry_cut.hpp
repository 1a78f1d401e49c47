// entry_cut.hpp -- per-tile entry nodes of the primary walk: the scene's cut table and the pixel
// rectangle of a box, stated once for host and device (render_hip.hip).
//
// A CUT is a set of up to 64 nodes of the reference BVH such that every root-to-leaf path holds
// exactly one of them: the root's two children, then the open inner node of largest surface area
// split again and again (leaves stay).  Cut nodes are numbered in depth-first order, so the lowest
// common ancestor of a set of them is the LCA of its lowest and highest members.  A batch launch
// projects every cut box to a pixel rectangle (box_rect, the background cull's construction); a
// tile's 64 lanes test one rectangle each, and the walk of the tile's primary rays starts at the
// record of the LCA of the cut nodes whose rectangle reaches the tile -- see "Entry nodes" in
// render_hip.hip for why that changes no pixel.
#pragma once
#include <cmath>
#include <cstdint>

#include "ceres_types.hpp"

#if defined(__HIPCC__)
#define CERES_CUT_HD __host__ __device__
#else
#define CERES_CUT_HD
#endif

namespace ceres {

// The cut table, in 32-bit words (one device buffer per scene; ceres_entry_cut_build fills a host copy).
constexpr uint32_t kCutMax = 64;
constexpr uint32_t kCutN = 0;            // cut nodes (0: the root is a leaf; otherwise >= 2)
constexpr uint32_t kCutOk = 1;           // entry_ok: every box from the root's children down to the cut nodes' children
                                         // lies inside its parent's box (exact float compare); 0: enter at the root
constexpr uint32_t kCutChecks = 2;       // entries of the two check lists below
constexpr uint32_t kCutBroken = 3;       // a link outside the pair array was met: entry_ok stays 0
constexpr uint32_t kCutSrc = 4;          // [64] where the node's box lives: pair << 1 | side (0: lb, 1: rb)
constexpr uint32_t kCutChild = 68;       // [64] the pair record of the node's two children (kCutLeaf: a leaf)
constexpr uint32_t kCutBox = 132;        // [64][6] floats, the boxes (bvh.hpp:25-30 order)
constexpr uint32_t kCutLca = 516;        // [64][64] the pair record that holds the LCA's two children (0: the root's)
constexpr uint32_t kCutCheckRec = 4612;  // [128] a pair record whose lb and rb must lie inside ...
constexpr uint32_t kCutCheckBox = 4740;  // [128] ... this box: pair << 1 | side, or kCutRoot (the scene's root box)
constexpr uint32_t kCutDepth = 4868;     // [64][64] depth of the LCA (0: the root), for diagnostics
constexpr uint32_t kCutRootBox = 4868 + 4096;   // [6] floats, the scene's root box
constexpr uint32_t kCutWords = kCutRootBox + 6;
constexpr uint32_t kCutLeaf = 0xffffffffu, kCutRoot = 0xffffffffu;

CERES_CUT_HD inline const float* cut_src_box(const SiblingPair* pairs, uint32_t src) {
    return (src & 1u) ? pairs[src >> 1].rb : pairs[src >> 1].lb;
}
CERES_CUT_HD inline bool cut_inside(const float* c, const float* p) {
    return c[0] >= p[0] && c[1] <= p[1] && c[2] >= p[2] && c[3] <= p[3] && c[4] >= p[4] && c[5] <= p[5];
}
// cut node k's box, read again from its pair (after a refit)
CERES_CUT_HD inline void cut_load_box(const SiblingPair* pairs, uint32_t* T, uint32_t k) {
    const float* b = cut_src_box(pairs, T[kCutSrc + k]);
    float* out = reinterpret_cast<float*>(T + kCutBox) + 6 * k;
    for (int a = 0; a < 6; ++a) out[a] = b[a];
}
// check k of the table: both children of a record inside the box of their parent
CERES_CUT_HD inline bool cut_check(const SiblingPair* pairs, const float* root_box, const uint32_t* T, uint32_t k) {
    const SiblingPair& r = pairs[T[kCutCheckRec + k]];
    const uint32_t bs = T[kCutCheckBox + k];
    const float* p = bs == kCutRoot ? root_box : cut_src_box(pairs, bs);
    return cut_inside(r.lb, p) && cut_inside(r.rb, p);
}
// boxes and entry_ok from the pairs as they are now, one thread (the host; device scenes refresh
// with one thread per box and per check, ceres_cut_refresh)
CERES_CUT_HD inline void cut_refresh_serial(const SiblingPair* pairs, const float* root_box, uint32_t* T) {
    for (int a = 0; a < 6; ++a) reinterpret_cast<float*>(T + kCutRootBox)[a] = root_box[a];
    bool ok = !T[kCutBroken] && T[kCutN] >= 2;
    for (uint32_t k = 0; k < T[kCutN]; ++k) cut_load_box(pairs, T, k);
    for (uint32_t k = 0; k < T[kCutChecks]; ++k) ok = cut_check(pairs, root_box, T, k) && ok;
    T[kCutOk] = ok ? 1u : 0u;
}

CERES_CUT_HD inline float cut_area(const float* b) {
    const float dx = b[1] - b[0], dy = b[3] - b[2], dz = b[5] - b[4];
    return dx * dy + dy * dz + dz * dx;
}

// The whole table from a pair array.  Serial: a scene is built once per topology (creation and
// rebuild), and device-built scenes run this in one thread on the stream that made the pairs.
CERES_CUT_HD inline void cut_build(const SiblingPair* pairs, uint32_t n_pairs, uint32_t root_leaf_count, const float* root_box,
                               uint32_t* T) {
    for (uint32_t k = 0; k < kCutWords; ++k) T[k] = 0u;              // every LCA the root, every depth 0
    for (uint32_t k = 0; k < kCutMax; ++k) T[kCutChild + k] = kCutLeaf;
    for (int a = 0; a < 6; ++a) reinterpret_cast<float*>(T + kCutRootBox)[a] = root_box[a];
    if (root_leaf_count || n_pairs == 0) return;
    // the cut in depth-first order: a split puts the two children in their parent's place.  path:
    // the turns from the root (bit d - 1: the turn into depth d, 1 = right); depth <= 63.
    uint64_t path[kCutMax], ipath[kCutMax];
    uint32_t depth[kCutMax], idepth[kCutMax], irec[kCutMax];
    uint32_t n = 0, ni = 0, checks = 0;
    bool broken = false;
    auto child_of = [&](const SiblingPair& r, int side) {
        const uint32_t count = side ? r.rcount : r.lcount, first = side ? r.rfirst : r.lfirst;
        if (count) return kCutLeaf;
        if (first >= n_pairs || first == 0) { broken = true; return kCutLeaf; }
        return first;
    };
    auto add_check = [&](uint32_t rec, uint32_t box) { T[kCutCheckRec + checks] = rec; T[kCutCheckBox + checks] = box; ++checks; };
    for (int side = 0; side < 2; ++side) {
        T[kCutSrc + n] = uint32_t(side); T[kCutChild + n] = child_of(pairs[0], side);
        path[n] = uint64_t(side); depth[n] = 1;
        ++n;
    }
    add_check(0u, kCutRoot);
    ipath[ni] = 0; idepth[ni] = 0; irec[ni] = 0; ++ni;
    while (n < kCutMax) {
        uint32_t best = kCutMax;
        float best_area = -1.f;
        for (uint32_t k = 0; k < n; ++k) {
            if (T[kCutChild + k] == kCutLeaf) continue;
            const float a = cut_area(cut_src_box(pairs, T[kCutSrc + k]));
            if (a > best_area) { best_area = a; best = k; }
        }
        if (best == kCutMax) break;
        const uint32_t rec = T[kCutChild + best], src = T[kCutSrc + best], d = depth[best];
        const uint64_t p = path[best];
        add_check(rec, src);
        ipath[ni] = p; idepth[ni] = d; irec[ni] = rec; ++ni;
        for (uint32_t k = n; k > best + 1; --k) {
            T[kCutSrc + k] = T[kCutSrc + k - 1]; T[kCutChild + k] = T[kCutChild + k - 1];
            path[k] = path[k - 1]; depth[k] = depth[k - 1];
        }
        ++n;
        for (int side = 0; side < 2; ++side) {
            T[kCutSrc + best + side] = rec << 1 | uint32_t(side);
            T[kCutChild + best + side] = child_of(pairs[rec], side);
            path[best + side] = p | uint64_t(side) << d;
            depth[best + side] = d + 1;
        }
    }
    // the LCA of i < j: the inner node above the cut with i below its left child and j below its right
    for (uint32_t t = 0; t < ni; ++t) {
        const uint32_t d = idepth[t];
        const uint64_t mask = (uint64_t(1) << d) - 1u;
        for (uint32_t i = 0; i < n; ++i) {
            if ((path[i] & mask) != ipath[t] || (path[i] >> d & 1u)) continue;
            for (uint32_t j = i + 1; j < n; ++j) {
                if ((path[j] & mask) != ipath[t] || !(path[j] >> d & 1u)) continue;
                T[kCutLca + i * kCutMax + j] = T[kCutLca + j * kCutMax + i] = irec[t];
                T[kCutDepth + i * kCutMax + j] = T[kCutDepth + j * kCutMax + i] = d;
            }
        }
    }
    // one cut node alone: its own children's record; a leaf has none and enters at its parent's
    for (uint32_t k = 0; k < n; ++k) {
        const bool inner = T[kCutChild + k] != kCutLeaf;
        T[kCutLca + k * kCutMax + k] = inner ? T[kCutChild + k] : T[kCutSrc + k] >> 1;
        T[kCutDepth + k * kCutMax + k] = inner ? depth[k] : depth[k] - 1u;
        if (inner) add_check(T[kCutChild + k], T[kCutSrc + k]);
    }
    T[kCutN] = n; T[kCutChecks] = checks; T[kCutBroken] = broken ? 1u : 0u;
    cut_refresh_serial(pairs, root_box, T);
}

// std::max / std::min (their answer when an operand is NaN included), callable on the device
template <class V> CERES_CUT_HD inline V cut_max(V a, V b) { return a < b ? b : a; }
template <class V> CERES_CUT_HD inline V cut_min(V a, V b) { return b < a ? b : a; }
CERES_CUT_HD inline void cut_cross(const double* a, const double* b, double* o) {
    o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
}
CERES_CUT_HD inline uint32_t cut_clamp_floor(double x, uint32_t n) { return x <= 0 ? 0u : x >= n ? n : uint32_t(floor(x)); }

// The pixels whose primary rays may reach a box, as a rectangle of columns and global rows.  The
// primary ray of image coordinates (u, v) is eye + s (iu u + iv v + dir) (render.hpp:109-111), so a
// point X projects to (p / w, q / w) with (p, q, w) = [iu iv dir]^-1 (X - eye).  Every corner of the
// box, EXPANDED by 1e-4 of the scene / eye coordinate scale, must lie in front of the eye (w > 0.01
// |X - eye|); then the expanded box's image lies inside the bounding rectangle of the corner images
// (a convex set in front of the eye projects into the hull of its corners' images), and a pixel
// whose (u, v) = (2 (i + 0.5) / W - 1, 2 (j + 0.5) / H - 1) lies outside that rectangle widened by
// m = 2e-3 (1 + max |corner coordinate|) -- two pixels at 1080p -- has a ray that misses the
// expanded box.  The kernel's float ray (render.hpp:109-113: rounding of ~1e-6 in (u, v) and in the
// unit direction) and float slab test (~1e-6 relative in the slab distances,
// node_intersectors.hpp:83-103) stay far inside those margins, so its test of the box fails too.
// Computed in double; anything degenerate (a corner behind the eye, NaN, a frame wider than 65,535
// pixels) keeps every pixel.
CERES_CUT_HD inline CullRect box_rect(const FrameCam& c, const float box[6], uint32_t W, uint32_t H) {
    const CullRect keep{0u, 0xffffu, 0u, 0xffffu};
    if (W > 0xffffu || H > 0xffffu) return keep;
    double e[3], iu[3], iv[3], d[3];
    for (int k = 0; k < 3; ++k) { e[k] = c.eye[k]; iu[k] = c.iu[k]; iv[k] = c.iv[k]; d[k] = c.dir[k]; }
    double sc = 0;
    for (int k = 0; k < 3; ++k) sc = cut_max(sc, fabs(e[k]));
    for (int k = 0; k < 6; ++k) sc = cut_max(sc, fabs(double(box[k])));
    const double pad = 1e-4 * sc;
    double c0[3], c1[3], c2[3];
    cut_cross(iv, d, c0); cut_cross(d, iu, c1); cut_cross(iu, iv, c2);
    const double det = iu[0] * c0[0] + iu[1] * c0[1] + iu[2] * c0[2];
    double u0 = HUGE_VAL, u1 = -HUGE_VAL, v0 = HUGE_VAL, v1 = -HUGE_VAL;
    for (int k = 0; k < 8; ++k) {
        const double X[3] = {(k & 1) ? box[1] + pad : box[0] - pad, (k & 2) ? box[3] + pad : box[2] - pad,
                             (k & 4) ? box[5] + pad : box[4] - pad};
        const double r[3] = {X[0] - e[0], X[1] - e[1], X[2] - e[2]};
        const double pw = r[0] * c0[0] + r[1] * c0[1] + r[2] * c0[2], qw = r[0] * c1[0] + r[1] * c1[1] + r[2] * c1[2];
        const double ww = r[0] * c2[0] + r[1] * c2[1] + r[2] * c2[2];
        if (!(ww / det > 0.01 * sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]))) return keep;
        u0 = cut_min(u0, pw / ww); u1 = cut_max(u1, pw / ww); v0 = cut_min(v0, qw / ww); v1 = cut_max(v1, qw / ww);
    }
    const double m = 2e-3 * (1 + cut_max(cut_max(fabs(u0), fabs(u1)), cut_max(fabs(v0), fabs(v1))));
    // pixels whose u lies in [u0 - m, u1 + m]: i in [(u0 - m + 1) W / 2 - 0.5, (u1 + m + 1) W / 2 - 0.5], one more each side
    const double a0 = (u0 - m + 1) * W / 2 - 0.5 - 1, a1 = (u1 + m + 1) * W / 2 - 0.5 + 1;
    const double b0 = (v0 - m + 1) * H / 2 - 0.5 - 1, b1 = (v1 + m + 1) * H / 2 - 0.5 + 1;
    if (!(a0 == a0 && a1 == a1 && b0 == b0 && b1 == b1)) return keep;
    if (a1 < 0 || b1 < 0) return CullRect{1u, 0u, 1u, 0u};            // empty: the whole frame misses
    return CullRect{uint16_t(cut_clamp_floor(a0, W)), uint16_t(cut_min<double>(ceil(a1), 0xffff)),
                    uint16_t(cut_clamp_floor(b0, H)), uint16_t(cut_min<double>(ceil(b1), 0xffff))};
}

// One frame's rectangles of a cut table, lane by lane as the launch writes them: rectangle k for
// cut node k, empty for the lanes past the cut; every lane "keep" (so every tile enters at the
// root, lca[0][63]) when the table has no usable cut or the root box's own rectangle is "keep" --
// the eye inside the box, a corner behind it, a camera that is not finite: frames the cull leaves
// alone enter at the root as well.
CERES_CUT_HD inline bool cut_is_keep(const CullRect& r) { return r.i0 == 0u && r.i1 == 0xffffu && r.j0 == 0u && r.j1 == 0xffffu; }
CERES_CUT_HD inline CullRect cut_lane_rect(const uint32_t* T, const FrameCam& c, uint32_t W, uint32_t H, uint32_t lane) {
    const uint32_t n = T[kCutN];
    if (n < 2u || !T[kCutOk]) return CullRect{0u, 0xffffu, 0u, 0xffffu};
    if (cut_is_keep(box_rect(c, reinterpret_cast<const float*>(T + kCutRootBox), W, H))) return CullRect{0u, 0xffffu, 0u, 0xffffu};
    if (lane >= n) return CullRect{1u, 0u, 1u, 0u};
    return box_rect(c, reinterpret_cast<const float*>(T + kCutBox) + 6 * lane, W, H);
}
// Whether cut rectangle r reaches tile (bx, by) of a W x rows frame (whole frames: local row = global row)
CERES_CUT_HD inline bool cut_rect_hits_tile(const CullRect& r, uint32_t W, uint32_t rows, uint32_t bx, uint32_t by) {
    const uint32_t a = 8u * bx, b = a + 7u < W - 1u ? a + 7u : W - 1u;
    const uint32_t p = 8u * by, q = p + 7u < rows - 1u ? p + 7u : rows - 1u;
    return cut_max<uint32_t>(a, r.i0) <= cut_min<uint32_t>(b, r.i1) && cut_max<uint32_t>(p, r.j0) <= cut_min<uint32_t>(q, r.j1);
}

// The same for a rectangle as a launch packs it: x = i0 | i1 << 16, y = j0 | j1 << 16
// (its row part alone: the launch's live mask asks it once per tile-row before it tests the columns)
CERES_CUT_HD inline bool cut_words_hit_rows(uint32_t y, uint32_t rows, uint32_t by) {
    const uint32_t p = 8u * by, q = p + 7u < rows - 1u ? p + 7u : rows - 1u;
    return cut_max(p, y & 0xffffu) <= cut_min(q, y >> 16);
}
CERES_CUT_HD inline bool cut_words_hit_tile(uint32_t x, uint32_t y, uint32_t W, uint32_t rows, uint32_t bx, uint32_t by) {
    const uint32_t a = 8u * bx, b = a + 7u < W - 1u ? a + 7u : W - 1u;
    return cut_max(a, x & 0xffffu) <= cut_min(b, x >> 16) && cut_words_hit_rows(y, rows, by);
}

}  // namespace ceres
