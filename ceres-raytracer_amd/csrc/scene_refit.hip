// scene_refit.hip -- refit a device scene in place when its triangles move (ceres_scene_refit*):
// the reference's HierarchyRefitter (hierarchy_refitter.hpp:17-32 with the usual leaf update) on the
// GPU layout.  Topology, leaf assignment and record numbering stay; every box is recomputed:
//
//   regather   leaf_tris[k] = tris[orig[k]]                      one thread per leaf slot, 16-B accesses
//   leaves     a leaf child's box = the union over its run of leaf-order triangles of
//              Triangle::bounding_box() (triangle.hpp:36-44: p0, p0 - e1, p0 + e2), one thread per
//              (pair, side), in the scene's scalar type
//   inner      an inner child's box = the union of its own pair's two boxes (bounding_box.hpp:23-26),
//              ONE LAUNCH PER TREE LEVEL, deepest first, over a level-sorted list of pair indices made
//              at the first refit (a breadth-first walk on the device) and kept in the scene.  The kernel boundary is the only
//              synchronisation: a child pair's boxes are written by an earlier launch than the one
//              that reads them, so no arrival counter, fence or cross-workgroup hand-off exists (the
//              per-XCD L2s are not coherent inside a launch; a single-launch bottom-up walk would need
//              an agent-scope release / acquire per node)
//   BVH4       child box = the sibling-pair side it stands for, gathered through the per-child source
//              words kept from creation (ceres_scene::d_src4); empty slots keep the inverted infinite box
//   root       the union of pair 0's two boxes (a root leaf: of its triangles), read back once (72 B)
//              because later launches receive the root box by value (KParams)
//
// Only min / max of the inputs is involved, so the boxes are exact and do not depend on the order of
// evaluation (but for the sign of a zero, which no comparison downstream distinguishes).  No index
// depends on a coordinate: every index comes from the topology validated at creation and is checked
// against its array again here, so non-finite input cannot cause an out-of-range access.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <vector>

#include "ceres_render.h"
#include "ceres_types.hpp"
#include "hip_try.hpp"
#include "host_common.hpp"
#include "scene_internal.hpp"

namespace ceres {
namespace refit {

template <class S> __device__ __forceinline__ S lesser(S a, S b) { return b < a ? b : a; }
template <class S> __device__ __forceinline__ S greater(S a, S b) { return a < b ? b : a; }

template <class S> __device__ __forceinline__ void box_empty(S* b) {
    b[0] = b[2] = b[4] = S(INFINITY);
    b[1] = b[3] = b[5] = -S(INFINITY);
}
template <class S> __device__ __forceinline__ void box_point(S* b, S x, S y, S z) {
    b[0] = lesser(b[0], x); b[1] = greater(b[1], x);
    b[2] = lesser(b[2], y); b[3] = greater(b[3], y);
    b[4] = lesser(b[4], z); b[5] = greater(b[5], z);
}
// Triangle::bounding_box() (triangle.hpp:36-44): the points p0, p1 = p0 - e1, p2 = p0 + e2
template <class S, class Tri> __device__ __forceinline__ void box_triangle(S* b, const Tri& t) {
    box_point(b, t.p0[0], t.p0[1], t.p0[2]);
    box_point(b, t.p0[0] - t.e1[0], t.p0[1] - t.e1[1], t.p0[2] - t.e1[2]);
    box_point(b, t.p0[0] + t.e2[0], t.p0[1] + t.e2[1], t.p0[2] + t.e2[2]);
}

// leaf_tris[k] = tris[orig[k]]; V 16-byte words per triangle (3: Tri48, 6: Tri96)
template <int V>
__global__ void __launch_bounds__(256) k_regather(const uint4* __restrict__ tris, const uint32_t* __restrict__ orig, uint32_t n_tri,
                                                  uint4* __restrict__ leaf_tris) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= n_tri) return;
    const uint32_t o = orig[k];
    if (o >= n_tri) return;
    uint4 w[V];
    for (int v = 0; v < V; ++v) w[v] = tris[size_t(o) * V + v];
    for (int v = 0; v < V; ++v) leaf_tris[size_t(k) * V + v] = w[v];
}

// one thread per (pair, side): a leaf child's box from its run of leaf-order triangles
template <class Pair, class Tri, class S>
__global__ void __launch_bounds__(256) k_leaf_boxes(Pair* __restrict__ pairs, uint32_t n_pairs, const Tri* __restrict__ tris,
                                                    uint32_t n_tri) {
    const uint64_t i = uint64_t(blockIdx.x) * 256u + threadIdx.x;
    const uint64_t pair = i >> 1;
    if (pair >= n_pairs) return;
    Pair& P = pairs[pair];
    const bool right = i & 1u;
    const uint32_t count = right ? P.rcount : P.lcount, first = right ? P.rfirst : P.lfirst;
    if (!count || uint64_t(first) + count > n_tri) return;
    S b[6];
    box_empty(b);
    for (uint32_t t = first; t < first + count; ++t) box_triangle(b, tris[t]);
    S* out = right ? P.rb : P.lb;
    for (int k = 0; k < 6; ++k) out[k] = b[k];
}

// one thread per (listed pair, side): an inner child's box = the union of its own pair's two boxes,
// which an EARLIER launch (a deeper level, or k_leaf_boxes) has written
template <class Pair, class S>
__global__ void __launch_bounds__(256) k_inner_boxes(Pair* pairs, uint32_t n_pairs, const uint32_t* __restrict__ list, uint32_t n) {
    const uint64_t i = uint64_t(blockIdx.x) * 256u + threadIdx.x;
    if ((i >> 1) >= n) return;
    const uint32_t pair = list[i >> 1];
    if (pair >= n_pairs) return;
    Pair& P = pairs[pair];
    const bool right = i & 1u;
    const uint32_t count = right ? P.rcount : P.lcount, child = right ? P.rfirst : P.lfirst;
    if (count || child >= n_pairs) return;
    const Pair& C = pairs[child];
    S* out = right ? P.rb : P.lb;
    for (int k = 0; k < 6; k += 2) {
        out[k] = lesser<S>(C.lb[k], C.rb[k]);
        out[k + 1] = greater<S>(C.lb[k + 1], C.rb[k + 1]);
    }
}

// one thread per (BVH4 record, child slot): the box of the sibling-pair side the child stands for
__global__ void __launch_bounds__(256) k_nodes4_boxes(Node4* __restrict__ nodes4, uint32_t n_nodes4, const uint32_t* __restrict__ src4,
                                                      const SiblingPair* __restrict__ pairs, uint32_t n_pairs) {
    const uint64_t i = uint64_t(blockIdx.x) * 256u + threadIdx.x;
    if ((i >> 2) >= n_nodes4) return;
    const uint32_t src = src4[i];
    if (src == kNode4NoSource || (src >> 1) >= n_pairs) return;
    const SiblingPair& P = pairs[src >> 1];
    const float* b = (src & 1u) ? P.rb : P.lb;
    Node4& N = nodes4[i >> 2];
    const uint32_t c = uint32_t(i) & 3u;
    N.lo_x[c] = b[0]; N.hi_x[c] = b[1];
    N.lo_y[c] = b[2]; N.hi_y[c] = b[3];
    N.lo_z[c] = b[4]; N.hi_z[c] = b[5];
}

// out[0..6): the root box; out[6..18): pair 0's lb and rb (what set_root_box compares it with)
__global__ void k_root_box(const SiblingPair* __restrict__ pairs, const Tri48* __restrict__ tris, uint32_t n_tri,
                           uint32_t root_leaf_count, uint32_t root_leaf_first, float* __restrict__ out) {
    if (blockIdx.x || threadIdx.x) return;
    float b[6];
    box_empty(b);
    if (root_leaf_count) {
        if (uint64_t(root_leaf_first) + root_leaf_count <= n_tri)
            for (uint32_t t = root_leaf_first; t < root_leaf_first + root_leaf_count; ++t) box_triangle(b, tris[t]);
        for (int k = 0; k < 12; ++k) out[6 + k] = 0.f;
    } else {
        const SiblingPair& P = pairs[0];
        for (int k = 0; k < 6; k += 2) {
            b[k] = lesser(P.lb[k], P.rb[k]);
            b[k + 1] = greater(P.lb[k + 1], P.rb[k + 1]);
        }
        for (int k = 0; k < 6; ++k) { out[6 + k] = P.lb[k]; out[12 + k] = P.rb[k]; }
    }
    for (int k = 0; k < 6; ++k) out[k] = b[k];
}

inline dim3 grid_for(uint64_t threads) { return dim3(uint32_t((threads + 255) / 256)); }

// Scalar-specific layout of a scene
template <bool F64> struct Lay;
template <> struct Lay<false> {
    using Pair = SiblingPair; using Tri = Tri48; using S = float;
    static constexpr int kTriVec = 3;
    static constexpr size_t kNormBytes = 36;
    static Pair* pairs(ceres_scene* s) { return s->d_pairs; }
    static Tri* tris(ceres_scene* s) { return s->d_tris; }
    static void* norms(ceres_scene* s) { return s->d_norms; }
};
template <> struct Lay<true> {
    using Pair = SiblingPair64; using Tri = Tri96; using S = double;
    static constexpr int kTriVec = 6;
    static constexpr size_t kNormBytes = 72;
    static Pair* pairs(ceres_scene* s) { return s->d_pairs64; }
    static Tri* tris(ceres_scene* s) { return s->d_tris64; }
    static void* norms(ceres_scene* s) { return s->d_norms64; }
};

// First refit: the pair indices sorted by tree level, by a breadth-first walk on the device that
// writes straight into the list -- level l is list[off[l] .. off[l + 1]); the kernel reads that
// segment and appends the inner children's pairs behind the tail (list[n_pairs] is the tail counter).
// One launch and one 4-byte readback per level, once per scene; the order inside a level does not matter.
template <class Pair>
__global__ void __launch_bounds__(256) k_next_level(const Pair* __restrict__ pairs, uint32_t n_pairs, uint32_t* list, uint32_t begin,
                                                    uint32_t end) {
    const uint64_t i = uint64_t(begin) + uint64_t(blockIdx.x) * 256u + threadIdx.x;
    if (i >= end) return;
    const uint32_t pair = list[i];
    if (pair >= n_pairs) return;
    const Pair& P = pairs[pair];
    const uint32_t count[2] = {P.lcount, P.rcount}, first[2] = {P.lfirst, P.rfirst};
    for (int side = 0; side < 2; ++side) {
        if (count[side] || first[side] >= n_pairs) continue;
        const uint32_t pos = atomicAdd(&list[n_pairs], 1u);
        if (pos < n_pairs) list[pos] = first[side];              // a tree never gets here with pos >= n_pairs (checked on the host)
    }
}

template <bool F64>
int ensure_levels(ceres_scene* s, hipStream_t st) {
    using L = Lay<F64>;
    if (!F64 && !s->d_refit_root) HIP_TRY(hipMalloc(&s->d_refit_root, 18 * sizeof(float)));
    if (s->root_leaf_count || !s->refit_level_off.empty()) return CERES_OK;
    const uint32_t np = uint32_t(s->n_pairs);
    uint32_t* list = nullptr;
    HIP_TRY(hipMalloc(&list, (size_t(np) + 1) * sizeof(uint32_t)));
    auto body = [&](std::vector<uint32_t>& off) -> int {
        const uint32_t zero = 0, one = 1;
        HIP_TRY(hipMemcpyAsync(list, &zero, 4, hipMemcpyHostToDevice, st));          // level 0: pair 0
        HIP_TRY(hipMemcpyAsync(list + np, &one, 4, hipMemcpyHostToDevice, st));      // the tail
        for (uint32_t begin = 0, end = 1; begin < end;) {
            if (off.size() > 65) return set_error(CERES_EINVAL, "refit: sibling pairs deeper than 64 levels");
            hipLaunchKernelGGL((k_next_level<typename L::Pair>), grid_for(end - begin), dim3(256), 0, st, L::pairs(s), np, list, begin, end);
            HIP_TRY(hipGetLastError());
            uint32_t tail = 0;
            HIP_TRY(hipMemcpyAsync(&tail, list + np, 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            if (tail > np) return set_error(CERES_EINVAL, "refit: sibling pairs do not form a tree");
            off.push_back(end);
            begin = end;
            end = tail;
        }
        return CERES_OK;
    };
    std::vector<uint32_t> off{0};
    if (int rc = body(off)) { (void)hipFree(list); return rc; }
    s->d_refit_levels = list;
    s->refit_level_off = std::move(off);
    return CERES_OK;
}

template <bool F64>
int refit_device(ceres_scene* s, const void* d_tri, size_t n_tri, const void* d_norm, hipStream_t stream, const char* who) {
    using L = Lay<F64>;
    using Pair = typename L::Pair; using Tri = typename L::Tri; using S = typename L::S;
    if (!s || !d_tri) return set_error(CERES_EINVAL, "%s: null argument", who);
    if (s->f64 != F64) return set_error(CERES_EINVAL, "%s: the scene is a %s scene", who, s->f64 ? "double" : "float");
    if (n_tri != s->n_tri) return set_error(CERES_EINVAL, "%s: %zu triangles, the scene has %zu", who, n_tri, s->n_tri);
    if (reinterpret_cast<uintptr_t>(d_tri) & 15u) return set_error(CERES_EINVAL, "%s: triangles not 16-byte aligned", who);
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t st = stream;                                     // NULL: the default stream, as ceres_render_device
    if (int rc = ensure_levels<F64>(s, st)) return rc;
    const uint32_t nt = uint32_t(n_tri), np = uint32_t(s->n_pairs);
    hipLaunchKernelGGL((k_regather<L::kTriVec>), grid_for(nt), dim3(256), 0, st, static_cast<const uint4*>(d_tri), s->d_orig, nt,
                       reinterpret_cast<uint4*>(L::tris(s)));
    HIP_TRY(hipGetLastError());
    if (d_norm) HIP_TRY(hipMemcpyAsync(L::norms(s), d_norm, n_tri * L::kNormBytes, hipMemcpyDeviceToDevice, st));
    if (!s->root_leaf_count) {
        hipLaunchKernelGGL((k_leaf_boxes<Pair, Tri, S>), grid_for(2ull * np), dim3(256), 0, st, L::pairs(s), np, L::tris(s), nt);
        HIP_TRY(hipGetLastError());
        // the deepest level has no inner child; every other level reads the one below it
        const std::vector<uint32_t>& off = s->refit_level_off;
        const int levels = int(off.size()) - 1;                  // level l = list[off[l] .. off[l + 1])
        for (int l = levels - 2; l >= 0; --l) {
            const uint32_t n = off[l + 1] - off[l];
            hipLaunchKernelGGL((k_inner_boxes<Pair, S>), grid_for(2ull * n), dim3(256), 0, st, L::pairs(s), np,
                               s->d_refit_levels + off[l], n);
            HIP_TRY(hipGetLastError());
        }
    }
    if constexpr (!F64) {
        if (!s->root_leaf_count && s->d_src4 && s->d_nodes4) {
            hipLaunchKernelGGL(k_nodes4_boxes, grid_for(4ull * s->n_nodes4), dim3(256), 0, st, s->d_nodes4, uint32_t(s->n_nodes4),
                               s->d_src4, s->d_pairs, np);
            HIP_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL(k_root_box, dim3(1), dim3(64), 0, st, s->d_pairs, s->d_tris, nt, s->root_leaf_count, s->root_leaf_first,
                           s->d_refit_root);
        HIP_TRY(hipGetLastError());
        if (int rc = scene_refresh_cut(s, s->d_refit_root, st)) return rc;   // entry nodes: the cut's boxes moved too
        float h[18];
        HIP_TRY(hipMemcpyAsync(h, s->d_refit_root, sizeof h, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        SiblingPair p0{};
        std::memcpy(p0.lb, h + 6, sizeof p0.lb);
        std::memcpy(p0.rb, h + 12, sizeof p0.rb);
        return scene_after_refit(s, h, p0);
    } else {
        HIP_TRY(hipStreamSynchronize(st));      // double scenes keep no root box; later launches on any stream follow
        return CERES_OK;
    }
}

// host arrays: staged through a device buffer the scene keeps (triangles, then normals)
template <bool F64>
int refit_host(ceres_scene* s, const void* tri, size_t n_tri, const void* norm, const char* who) {
    using L = Lay<F64>;
    if (!s || !tri) return set_error(CERES_EINVAL, "%s: null argument", who);
    if (s->f64 != F64) return set_error(CERES_EINVAL, "%s: the scene is a %s scene", who, s->f64 ? "double" : "float");
    if (n_tri != s->n_tri) return set_error(CERES_EINVAL, "%s: %zu triangles, the scene has %zu", who, n_tri, s->n_tri);
    HIP_TRY(hipSetDevice(s->device));
    const size_t tri_bytes = n_tri * sizeof(typename L::Tri), norm_bytes = n_tri * L::kNormBytes;
    if (!s->d_refit_stage) HIP_TRY(hipMalloc(&s->d_refit_stage, tri_bytes + norm_bytes));
    char* stage = static_cast<char*>(s->d_refit_stage);
    HIP_TRY(hipMemcpyAsync(stage, tri, tri_bytes, hipMemcpyHostToDevice, s->stream));
    if (norm) HIP_TRY(hipMemcpyAsync(stage + tri_bytes, norm, norm_bytes, hipMemcpyHostToDevice, s->stream));
    return refit_device<F64>(s, stage, n_tri, norm ? stage + tri_bytes : nullptr, s->stream, who);
}

}  // namespace refit
}  // namespace ceres

using namespace ceres;

extern "C" {

int ceres_scene_refit(ceres_scene* s, const float* tri48, size_t n_tri, const float* norm36) {
    return refit::refit_host<false>(s, tri48, n_tri, norm36, "ceres_scene_refit");
}
int ceres_scene_refit_device(ceres_scene* s, const float* d_tri48, size_t n_tri, const float* d_norm36, void* stream) {
    return refit::refit_device<false>(s, d_tri48, n_tri, d_norm36, static_cast<hipStream_t>(stream), "ceres_scene_refit_device");
}
int ceres_scene_refit_f64(ceres_scene* s, const double* tri96, size_t n_tri, const double* norm72) {
    return refit::refit_host<true>(s, tri96, n_tri, norm72, "ceres_scene_refit_f64");
}
int ceres_scene_refit_f64_device(ceres_scene* s, const double* d_tri96, size_t n_tri, const double* d_norm72, void* stream) {
    return refit::refit_device<true>(s, d_tri96, n_tri, d_norm72, static_cast<hipStream_t>(stream), "ceres_scene_refit_f64_device");
}

int ceres_scene_read_boxes(ceres_scene* s, void* pair_boxes, size_t* n_pairs, float* node4_boxes, size_t* n_nodes4) {
    if (!s) return set_error(CERES_EINVAL, "ceres_scene_read_boxes: null scene");
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipDeviceSynchronize());
    const bool tree = !s->root_leaf_count;                      // a root leaf has no pair and no BVH4 record
    const size_t np = tree ? s->n_pairs : 0, n4 = tree && !s->f64 ? s->n_nodes4 : 0;
    if (n_pairs) *n_pairs = np;
    if (n_nodes4) *n_nodes4 = n4;
    if (pair_boxes && np) {
        if (s->f64) HIP_TRY(hipMemcpy2D(pair_boxes, 96, s->d_pairs64, sizeof(SiblingPair64), 96, np, hipMemcpyDeviceToHost));
        else HIP_TRY(hipMemcpy2D(pair_boxes, 48, s->d_pairs, sizeof(SiblingPair), 48, np, hipMemcpyDeviceToHost));
    }
    if (node4_boxes && n4) HIP_TRY(hipMemcpy2D(node4_boxes, 96, s->d_nodes4, sizeof(Node4), 96, n4, hipMemcpyDeviceToHost));
    return CERES_OK;
}

}  // extern "C"
