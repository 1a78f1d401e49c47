// scene_device64.hip -- device-resident preparation of a double scene: relayout_bvh64
// (scene_host.cpp) rebuilt as gfx950 kernels over device arrays, and ceres_scene_create_f64_device
// on top of it, so a double scene goes from triangles in HBM (ceres_bvh_build_f64_device) to its
// GPU layout without a host copy.  The double sibling of scene_device.hip, without its BVH4 and
// cut-table parts: double scenes have neither.
//
// Same records as the host relayout, numbered differently: the host numbers sibling pairs in a
// depth-first walk; here pair(X) = rank of inner node X among the reachable inner nodes in node
// order.  Traversal order and results depend only on the topology, never on record numbers, so
// every image, hit record and query answer is identical (tests/test_gpu_scene_f64_device.py).
//
// One breadth-first pass over the BVH2 (one launch per level, <= 64 levels) validates the tree --
// child indices in range, leaf ranges inside primitive_indices, no node reached twice -- before
// any record is written from it, and gives the depth (the traversal stack needs depth - 1 entries).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <new>

#include "ceres_render.h"
#include "ceres_types.hpp"
#include "dev_scan.hpp"
#include "hip_try.hpp"
#include "host_common.hpp"
#include "scene_internal.hpp"

namespace ceres {
namespace scenedev64 {

using namespace devscan;

enum : uint32_t { kErrRange = 1, kErrLeaf = 2, kErrShared = 4, kErrPrim = 8 };

struct LevelCtx {
    const RefNode64* nodes;
    uint32_t n_nodes, n_tri;
    uint32_t* visited;      // per node: reached
    uint32_t* inner;        // per node: reachable inner node
    uint32_t* err;
};

__device__ bool check_child(const LevelCtx& C, uint64_t ch) {
    if (atomicExch(&C.visited[ch], 1u) != 0u) { atomicOr(C.err, uint32_t(kErrShared)); return false; }
    const RefNode64& n = C.nodes[ch];
    if (n.primitive_count) {
        if (n.primitive_count > C.n_tri || n.first_child_or_primitive > C.n_tri - n.primitive_count) { atomicOr(C.err, uint32_t(kErrLeaf)); return false; }
        return true;
    }
    if (n.first_child_or_primitive >= C.n_nodes || n.first_child_or_primitive + 1 >= C.n_nodes) { atomicOr(C.err, uint32_t(kErrRange)); return false; }
    return true;
}

// one frontier of inner nodes whose own child index is already known to be in range
__global__ void __launch_bounds__(256) k_level(LevelCtx C, const uint32_t* __restrict__ frontier, uint32_t nf,
                                               uint32_t* __restrict__ next, uint32_t* __restrict__ n_next) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= nf) return;
    const uint32_t x = frontier[i];
    const uint64_t c = C.nodes[x].first_child_or_primitive;
    bool ok[2];
    for (int k = 0; k < 2; ++k) ok[k] = check_child(C, c + k);
    if (!ok[0] || !ok[1]) return;
    for (int k = 0; k < 2; ++k) {
        if (C.nodes[c + k].primitive_count) continue;
        C.inner[c + k] = 1;
        const uint32_t slot = atomicAdd(n_next, 1u);
        if (slot < C.n_nodes) next[slot] = uint32_t(c + k);     // (a node is reached once, so slot < n_nodes)
    }
}

// one SiblingPair64 per reachable inner node (relayout_bvh64's record, scene_host.cpp)
__global__ void __launch_bounds__(256) k_pairs(const RefNode64* __restrict__ nodes, uint32_t n_nodes, const uint32_t* __restrict__ inner,
                                               const uint32_t* __restrict__ pair_of, SiblingPair64* __restrict__ pairs) {
    const uint32_t x = blockIdx.x * 256u + threadIdx.x;
    if (x >= n_nodes || !inner[x]) return;
    const uint64_t c = nodes[x].first_child_or_primitive;
    const RefNode64& L = nodes[c];
    const RefNode64& R = nodes[c + 1];
    SiblingPair64 r;
    for (int k = 0; k < 6; ++k) { r.lb[k] = L.bounds[k]; r.rb[k] = R.bounds[k]; }
    r.lcount = uint32_t(L.primitive_count); r.lfirst = L.primitive_count ? uint32_t(L.first_child_or_primitive) : pair_of[c];
    r.rcount = uint32_t(R.primitive_count); r.rfirst = R.primitive_count ? uint32_t(R.first_child_or_primitive) : pair_of[c + 1];
    pairs[pair_of[x]] = r;
}

// triangles in leaf order + original indices (relayout_bvh64)
__global__ void __launch_bounds__(256) k_leaf_tris(const Tri96* __restrict__ tris, const uint32_t* __restrict__ prim, uint32_t n_tri,
                                                   Tri96* __restrict__ leaf_tris, uint32_t* __restrict__ orig, uint32_t* __restrict__ err) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= n_tri) return;
    const uint32_t p = prim[k];
    if (p >= n_tri) { atomicOr(err, uint32_t(kErrPrim)); return; }
    leaf_tris[k] = tris[p];
    orig[k] = p;
}

struct Layout64 {
    SiblingPair64* pairs = nullptr;
    Tri96* tris = nullptr;
    uint32_t* orig = nullptr;
    size_t n_pairs = 0;
    uint32_t depth = 0, root_leaf_count = 0, root_leaf_first = 0;
};

// Device relayout; outputs are hipMalloc'd (the caller owns them, on failure too).
int relayout_device64(const Tri96* d_tris, uint32_t n_tri, const RefNode64* d_nodes, uint32_t n_nodes, const uint32_t* d_prim,
                      hipStream_t stream, Layout64& out) {
    int rc = CERES_OK;
    uint32_t* ws = nullptr;
    auto fail_hip = [&](hipError_t e, const char* what) { return set_error(CERES_EHIP, "%s: %s", what, hipGetErrorString(e)); };
#define SD64_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { rc = fail_hip(e_, #expr); goto done; } } while (0)
    {
        // workspace: visited, inner, pair_of(+1), 2 frontiers, counters, partials
        const size_t N = n_nodes;
        const size_t parts = scan_blocks(n_nodes) + 2;
        const size_t words = 3 * (N + 1) + 2 * N + 8 + parts;
        uint32_t *visited, *inner, *pair_of, *fr[2], *ctr, *part;
        uint32_t h_ctr[4] = {0, 0, 0, 0};
        uint32_t nf = 1, level = 0, cur = 0;
        SD64_TRY(hipMallocAsync(reinterpret_cast<void**>(&ws), words * 4, stream));
        SD64_TRY(hipMemsetAsync(ws, 0, words * 4, stream));
        visited = ws; inner = visited + N + 1; pair_of = inner + N + 1; fr[0] = pair_of + N + 1; fr[1] = fr[0] + N;
        ctr = fr[1] + N; part = ctr + 8;          // ctr: [0] next count, [2] err
        RefNode64 root;
        SD64_TRY(hipMemcpyAsync(&root, d_nodes, sizeof root, hipMemcpyDeviceToHost, stream));
        SD64_TRY(hipStreamSynchronize(stream));
        out.root_leaf_count = out.root_leaf_first = 0;
        if (root.primitive_count) {                                  // the root is a leaf (single_ray_traverser.hpp:72-73)
            if (root.primitive_count > n_tri || root.first_child_or_primitive > n_tri - root.primitive_count) {
                rc = set_error(CERES_EINVAL, "root leaf range out of bounds");
                goto done;
            }
            out.root_leaf_count = uint32_t(root.primitive_count);
            out.root_leaf_first = uint32_t(root.first_child_or_primitive);
            out.depth = 0;
            out.n_pairs = 1;
            SD64_TRY(hipMalloc(&out.pairs, sizeof(SiblingPair64)));
            SD64_TRY(hipMemsetAsync(out.pairs, 0, sizeof(SiblingPair64), stream));
        } else {
            if (root.first_child_or_primitive >= n_nodes || root.first_child_or_primitive + 1 >= n_nodes) {
                rc = set_error(CERES_EINVAL, "root child index out of range");
                goto done;
            }
            const uint32_t one = 1, zero = 0;
            SD64_TRY(hipMemcpyAsync(fr[0], &zero, 4, hipMemcpyHostToDevice, stream));
            SD64_TRY(hipMemcpyAsync(visited, &one, 4, hipMemcpyHostToDevice, stream));
            SD64_TRY(hipMemcpyAsync(inner, &one, 4, hipMemcpyHostToDevice, stream));
            LevelCtx C{d_nodes, n_nodes, n_tri, visited, inner, ctr + 2};
            while (nf) {
                if (++level > 65) { rc = set_error(CERES_EINVAL, "BVH deeper than 64 levels or cyclic"); goto done; }
                SD64_TRY(hipMemsetAsync(ctr, 0, 4, stream));
                hipLaunchKernelGGL(k_level, dim3((nf + 255) / 256), dim3(256), 0, stream, C, fr[cur], nf, fr[cur ^ 1], ctr);
                SD64_TRY(hipGetLastError());
                SD64_TRY(hipMemcpyAsync(h_ctr, ctr, 12, hipMemcpyDeviceToHost, stream));
                SD64_TRY(hipStreamSynchronize(stream));
                if (h_ctr[2]) break;
                nf = std::min(h_ctr[0], n_nodes);
                cur ^= 1;
            }
            if (h_ctr[2]) {
                rc = set_error(CERES_EINVAL, "invalid BVH (%s%s%s)", h_ctr[2] & kErrRange ? "child index out of range " : "",
                               h_ctr[2] & kErrLeaf ? "leaf range out of bounds " : "", h_ctr[2] & kErrShared ? "node reached twice " : "");
                goto done;
            }
            out.depth = level;                                       // levels of inner nodes (root = 1)
            SD64_TRY(exclusive_scan(inner, n_nodes, pair_of, part, stream));
            uint32_t np = 0;
            SD64_TRY(hipMemcpyAsync(&np, pair_of + n_nodes, 4, hipMemcpyDeviceToHost, stream));
            SD64_TRY(hipStreamSynchronize(stream));
            out.n_pairs = np;
            SD64_TRY(hipMalloc(&out.pairs, size_t(np) * sizeof(SiblingPair64)));
            hipLaunchKernelGGL(k_pairs, dim3((n_nodes + 255) / 256), dim3(256), 0, stream, d_nodes, n_nodes, inner, pair_of, out.pairs);
            SD64_TRY(hipGetLastError());
        }
        // leaf-order triangles (every index is checked against n_tri before it is used)
        SD64_TRY(hipMalloc(&out.tris, size_t(n_tri) * sizeof(Tri96)));
        SD64_TRY(hipMalloc(&out.orig, size_t(n_tri) * 4));
        hipLaunchKernelGGL(k_leaf_tris, dim3((n_tri + 255) / 256), dim3(256), 0, stream, d_tris, d_prim, n_tri, out.tris, out.orig,
                           ctr + 2);
        SD64_TRY(hipGetLastError());
        uint32_t perr = 0;
        SD64_TRY(hipMemcpyAsync(&perr, ctr + 2, 4, hipMemcpyDeviceToHost, stream));
        SD64_TRY(hipStreamSynchronize(stream));
        if (perr & kErrPrim) { rc = set_error(CERES_EINVAL, "invalid BVH (primitive index out of range)"); goto done; }
    }
#undef SD64_TRY
done:
    if (ws) { (void)hipFreeAsync(ws, stream); (void)hipStreamSynchronize(stream); }
    return rc;
}

}  // namespace scenedev64
}  // namespace ceres

using namespace ceres;

extern "C" {

// A double scene from arrays already in HBM (device `device`): Triangle<double>[] / tri_norms and a
// Bvh<double> with u32 primitive_indices (ceres_bvh_build_f64_device's outputs); relayout on the
// GPU.  The caller keeps its buffers.  Work is ordered on `stream` (NULL: the scene's own stream).
// To every double call the scene is the one ceres_scene_create_f64 makes from the same arrays.
ceres_scene* ceres_scene_create_f64_device(const double* d_tri96, size_t n_tri, const double* d_norm72, const uint64_t* d_nodes64,
                                           size_t n_nodes, const uint32_t* d_prim32, int device, uint32_t flags, void* stream) {
    if (!d_tri96 || !d_norm72 || !d_nodes64 || !d_prim32 || n_tri == 0 || n_nodes == 0) {
        set_error(CERES_EINVAL, "ceres_scene_create_f64_device: empty scene or null argument");
        return nullptr;
    }
    if (n_tri > 0xffffffffull || n_nodes > 0xffffffffull) { set_error(CERES_EUNSUPPORTED, "scene too large"); return nullptr; }
    if ((reinterpret_cast<uintptr_t>(d_tri96) | reinterpret_cast<uintptr_t>(d_nodes64)) & 15u) {
        set_error(CERES_EINVAL, "ceres_scene_create_f64_device: device triangles and nodes must be 16-byte aligned");
        return nullptr;
    }
    auto* s = new (std::nothrow) ceres_scene;
    if (!s) { set_error(CERES_ENOMEM, "out of host memory"); return nullptr; }
    scenedev64::Layout64 L;
    auto fail = [&]() -> ceres_scene* {
        if (L.pairs) (void)hipFree(L.pairs);
        if (L.tris) (void)hipFree(L.tris);
        if (L.orig) (void)hipFree(L.orig);
        scene_release(s); delete s; return nullptr;
    };
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { set_error(CERES_EHIP, "no HIP device available"); return fail(); }
    if (device < 0 || device >= ndev) { set_error(CERES_EINVAL, "device %d out of range (%d devices)", device, ndev); return fail(); }
    s->f64 = true;
    s->device = device; s->flags = flags; s->n_tri = n_tri;
    ceres::scene_set_list_constants(s);
    auto body = [&]() -> int {
        HIP_TRY(hipSetDevice(device));
        hipDeviceProp_t prop;
        HIP_TRY(hipGetDeviceProperties(&prop, device));
        if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
            return set_error(CERES_EHIP, "device %d is %s, this build targets gfx950 only", device, prop.gcnArchName);
        s->num_cus = prop.multiProcessorCount;
        s->max_lds_per_block = prop.sharedMemPerBlock;
        HIP_TRY(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
        hipStream_t st = stream ? static_cast<hipStream_t>(stream) : s->stream;
        if (int rc = scenedev64::relayout_device64(reinterpret_cast<const Tri96*>(d_tri96), uint32_t(n_tri),
                                                   reinterpret_cast<const RefNode64*>(d_nodes64), uint32_t(n_nodes), d_prim32, st, L))
            return rc;
        s->d_pairs64 = L.pairs; s->d_tris64 = L.tris; s->d_orig = L.orig;     // owned by the scene now
        L.pairs = nullptr; L.tris = nullptr; L.orig = nullptr;
        s->n_pairs = L.n_pairs;
        s->depth = L.depth; s->root_leaf_count = L.root_leaf_count; s->root_leaf_first = L.root_leaf_first;
        s->stack_entries = std::max<uint32_t>(1, L.depth);
        HIP_TRY(hipMalloc(&s->d_norms64, n_tri * 72));
        HIP_TRY(hipMemcpyAsync(s->d_norms64, d_norm72, n_tri * 72, hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipMalloc(&s->d_shards, sizeof(Shard) * kShards));
        HIP_TRY(hipMalloc(&s->d_counters, 8 * sizeof(uint64_t)));            // ceres_trace_rays_f64
        HIP_TRY(hipStreamSynchronize(st));
        return CERES_OK;
    };
#undef HIP_TRY
    if (body()) return fail();
    return s;
}

}  // extern "C"
