// scene_quality.hip -- upkeep of a device scene whose triangles move: the SAH cost of its tree
// (ceres_scene_sah_cost), an in-place rebuild (ceres_scene_rebuild*) and the call that refits and
// rebuilds only when the cost has grown (ceres_scene_update*).
//
// Cost: SahBasedAlgorithm::compute_cost (sah_based_algorithm.hpp:21-32, traversal_cost = 1) over the
// scene's own sibling-pair records, evaluated in double on the stored bounds:
//
//   HA(box) = (d0 + d1) * d2 + d0 * d1, d = hi - lo                      (bounding_box.hpp:43-46)
//   ROOT    = the union of pair 0's lb and rb (what a refit makes the root box; root_box is not read)
//   cost    = (HA(ROOT) + sum over both children of every pair of HA(child) * w) / HA(ROOT),
//             w = count for a leaf child, 1 for an inner child
//
//   k_cost_partial  one pass over the 64-B (double scenes: 112-B) records, 16-B loads, a grid-stride
//                   loop; the sum inside the wave by cross-lane shuffles, then through LDS per
//                   workgroup; workgroup b writes partial[b]
//   k_cost_final    one workgroup: the partials through LDS, added IN INDEX ORDER, then pair 0's union
//                   and the division; the result lands behind the partials
//
// The kernel boundary is the only synchronisation (no floating-point atomics, no arrival counter: the
// per-XCD L2s are not coherent inside a launch -- scene_refit.hip's idiom).  The grid depends on n_pairs
// only and every order of addition is fixed, so two calls on an unchanged scene return the same bits.
//
// Rebuild: ceres_bvh_build_device_arith on the moved triangles into temporary node / primitive
// buffers, relayout_device, then the scene adopts the new layout exactly as ceres_scene_create_device
// does (scene_adopt_layout).  What was derived from the old topology goes (the quantised BVH4 copy, the
// refit's level list); what depends on the frame shape or the device only stays.  The old arrays are
// released after one device synchronise, never under a launch.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "ceres_render.h"
#include "ceres_types.hpp"
#include "hip_try.hpp"
#include "host_common.hpp"
#include "scene_internal.hpp"

namespace ceres {
namespace quality {

template <class S> __device__ __forceinline__ double half_area(const S* b) {
    const double d0 = double(b[1]) - double(b[0]), d1 = double(b[3]) - double(b[2]), d2 = double(b[5]) - double(b[4]);
    return (d0 + d1) * d2 + d0 * d1;
}

// the workgroup's sum of v in thread 0 (256 threads = 4 waves of 64), in a fixed order
__device__ __forceinline__ double block_sum(double v, double* lds4) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0) lds4[wave] = v;
    __syncthreads();
    return threadIdx.x == 0 ? ((lds4[0] + lds4[1]) + lds4[2]) + lds4[3] : 0.0;
}

template <class Pair>
__global__ void __launch_bounds__(256) k_cost_partial(const Pair* __restrict__ pairs, uint32_t n_pairs, double* __restrict__ partial) {
    __shared__ double lds4[4];
    double acc = 0.0;
    for (uint64_t i = uint64_t(blockIdx.x) * 256u + threadIdx.x; i < n_pairs; i += uint64_t(gridDim.x) * 256u) {
        const Pair P = pairs[i];                                     // 4 (7) x 16-B loads
        acc += half_area(P.lb) * double(P.lcount ? P.lcount : 1u);
        acc += half_area(P.rb) * double(P.rcount ? P.rcount : 1u);
    }
    const double sum = block_sum(acc, lds4);
    if (threadIdx.x == 0) partial[blockIdx.x] = sum;
}

// partial[0 .. n_partial) -> partial[kCostBlocks] = the cost
template <class Pair>
__global__ void __launch_bounds__(256) k_cost_final(const Pair* __restrict__ pairs, double* partial, uint32_t n_partial) {
    __shared__ double lds[kCostBlocks];
    for (uint32_t i = threadIdx.x; i < n_partial && i < kCostBlocks; i += 256u) lds[i] = partial[i];
    __syncthreads();
    if (threadIdx.x) return;
    double sum = 0.0;
    for (uint32_t i = 0; i < n_partial && i < kCostBlocks; ++i) sum += lds[i];
    const Pair& P = pairs[0];
    using S = decltype(P.lb[0] + P.lb[0]);
    S root[6];
    for (int k = 0; k < 6; k += 2) {
        root[k] = P.rb[k] < P.lb[k] ? P.rb[k] : P.lb[k];
        root[k + 1] = P.lb[k + 1] < P.rb[k + 1] ? P.rb[k + 1] : P.lb[k + 1];
    }
    const double ha = half_area(root);
    partial[kCostBlocks] = (ha + sum) / ha;                          // as written: a degenerate root gives inf or NaN
}

// the grid of the partial pass: a function of n_pairs alone (four records per thread, at most
// kCostBlocks workgroups)
inline uint32_t cost_blocks(size_t n_pairs) {
    const size_t b = (n_pairs + 1023) / 1024;
    return uint32_t(b < 1 ? 1 : b > kCostBlocks ? kCostBlocks : b);
}

template <class Pair>
int launch_cost(const Pair* pairs, uint32_t n_pairs, double* d_cost, hipStream_t st) {
    const uint32_t blocks = cost_blocks(n_pairs);
    hipLaunchKernelGGL((k_cost_partial<Pair>), dim3(blocks), dim3(256), 0, st, pairs, n_pairs, d_cost);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL((k_cost_final<Pair>), dim3(1), dim3(256), 0, st, pairs, d_cost, blocks);
    HIP_TRY(hipGetLastError());
    return CERES_OK;
}

// the cost of the scene as it stands, enqueued on `st`, which is synchronised once
int sah_cost(ceres_scene* s, double* cost, hipStream_t st) {
    if (s->root_leaf_count) { *cost = double(s->root_leaf_count); return CERES_OK; }   // no box is read
    if (!s->n_pairs || !(s->f64 ? static_cast<const void*>(s->d_pairs64) : static_cast<const void*>(s->d_pairs)))
        return set_error(CERES_EINVAL, "ceres_scene_sah_cost: the scene has no sibling pairs");
    HIP_TRY(hipSetDevice(s->device));
    if (!s->d_cost) HIP_TRY(hipMalloc(&s->d_cost, (size_t(kCostBlocks) + 1) * sizeof(double)));
    if (int rc = s->f64 ? launch_cost(s->d_pairs64, uint32_t(s->n_pairs), s->d_cost, st)
                        : launch_cost(s->d_pairs, uint32_t(s->n_pairs), s->d_cost, st))
        return rc;
    double h = 0.0;
    HIP_TRY(hipMemcpyAsync(&h, s->d_cost + kCostBlocks, sizeof h, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *cost = h;
    return CERES_OK;
}

// every refusal of a rebuild or an update, before anything is launched, freed or written
int check_moved(const ceres_scene* s, const void* tri, size_t n_tri, int arith, bool device_ptr, const char* who) {
    if (!s || !tri) return set_error(CERES_EINVAL, "%s: null argument", who);
    if (s->f64) return set_error(CERES_EUNSUPPORTED, "%s: in-place rebuild of a double scene is not implemented; recreate it with ceres_scene_create_f64_device", who);
    if (n_tri != s->n_tri) return set_error(CERES_EINVAL, "%s: %zu triangles, the scene has %zu", who, n_tri, s->n_tri);
    if (device_ptr && (reinterpret_cast<uintptr_t>(tri) & 15u)) return set_error(CERES_EINVAL, "%s: triangles not 16-byte aligned", who);
    if (arith != CERES_ARITH_EXACT && arith != CERES_ARITH_FMA) return set_error(CERES_EINVAL, "%s: unknown arithmetic %d", who, arith);
    return CERES_OK;
}
int check_ratio(double max_ratio, const char* who) {
    if (!(max_ratio > 0.0)) return set_error(CERES_EINVAL, "%s: max_ratio must be positive (+inf: never rebuild)", who);
    return CERES_OK;
}

void free_layout(DeviceLayout& L) {
    if (L.pairs) (void)hipFree(L.pairs);
    if (L.nodes4) (void)hipFree(L.nodes4);
    if (L.tris) (void)hipFree(L.tris);
    if (L.orig) (void)hipFree(L.orig);
    if (L.src4) (void)hipFree(L.src4);
    L = DeviceLayout{};
}

// arguments already checked (check_moved)
int rebuild_device(ceres_scene* s, const float* d_tri, size_t n_tri, const float* d_norm, int arith, hipStream_t st) {
    HIP_TRY(hipSetDevice(s->device));
    uint32_t* d_nodes = nullptr;
    uint32_t* d_prim = nullptr;
    DeviceLayout L;
    auto build = [&]() -> int {
        HIP_TRY(hipMalloc(&d_nodes, (2 * n_tri - 1) * sizeof(RefNode)));
        HIP_TRY(hipMalloc(&d_prim, n_tri * sizeof(uint32_t)));
        size_t n_nodes = 0;
        if (int rc = ceres_bvh_build_device_arith(d_tri, n_tri, d_nodes, d_prim, &n_nodes, st, arith)) return rc;
        if (int rc = relayout_device(reinterpret_cast<const Tri48*>(d_tri), uint32_t(n_tri), reinterpret_cast<const RefNode*>(d_nodes),
                                     uint32_t(n_nodes), d_prim, st, L))
            return rc;
        // the scene's old arrays: kernels may still read them, so they outlive the device synchronise below
        void* old[] = {s->d_pairs, s->d_nodes4, s->d_tris, s->d_orig, s->d_src4, s->d_qnodes4, s->d_refit_levels};
        if (int rc = scene_adopt_layout(s, L, st)) return rc;        // only a complete layout is adopted
        s->d_qnodes4 = nullptr;                                      // requantised by the next CERES_MODE_QBVH4 render
        s->d_refit_levels = nullptr;                                 // sorted again by the next refit
        s->refit_level_off.clear();
        hipError_t e = d_norm ? hipMemcpyAsync(s->d_norms, d_norm, n_tri * 36, hipMemcpyDeviceToDevice, st) : hipSuccess;
        const hipError_t e2 = hipDeviceSynchronize();
        for (void* p : old) if (p) (void)hipFree(p);
        if (e == hipSuccess) e = e2;
        if (e != hipSuccess) return set_error(CERES_EHIP, "ceres_scene_rebuild: %s", hipGetErrorString(e));
        return CERES_OK;
    };
    int rc = build();
    if (rc) { (void)hipDeviceSynchronize(); free_layout(L); }
    if (d_nodes) (void)hipFree(d_nodes);
    if (d_prim) (void)hipFree(d_prim);
    if (rc) return rc;
    s->built_cost_known = false;
    if ((rc = sah_cost(s, &s->built_cost, st))) return rc;           // the new tree is the baseline
    s->built_cost_known = true;
    return CERES_OK;
}

// host arrays -> the staging buffer the scene keeps for host-array refits (triangles, then normals)
int stage_host(ceres_scene* s, const float* tri, size_t n_tri, const float* norm, const float** d_tri, const float** d_norm) {
    HIP_TRY(hipSetDevice(s->device));
    const size_t tri_bytes = n_tri * sizeof(Tri48), norm_bytes = n_tri * 36;
    if (!s->d_refit_stage) HIP_TRY(hipMalloc(&s->d_refit_stage, tri_bytes + norm_bytes));
    char* stage = static_cast<char*>(s->d_refit_stage);
    HIP_TRY(hipMemcpyAsync(stage, tri, tri_bytes, hipMemcpyHostToDevice, s->stream));
    if (norm) HIP_TRY(hipMemcpyAsync(stage + tri_bytes, norm, norm_bytes, hipMemcpyHostToDevice, s->stream));
    *d_tri = reinterpret_cast<const float*>(stage);
    *d_norm = norm ? reinterpret_cast<const float*>(stage + tri_bytes) : nullptr;
    return CERES_OK;
}

// arguments already checked (check_moved, check_ratio)
int update_device(ceres_scene* s, const float* d_tri, size_t n_tri, const float* d_norm, int arith, double max_ratio,
                  ceres_update_info* info, hipStream_t st) {
    if (!s->built_cost_known) {                                      // the tree as first seen is the baseline
        if (int rc = sah_cost(s, &s->built_cost, st)) return rc;
        s->built_cost_known = true;
    }
    if (int rc = ceres_scene_refit_device(s, d_tri, n_tri, d_norm, st)) return rc;
    ceres_update_info u{};
    if (int rc = sah_cost(s, &u.cost, st)) return rc;
    u.built_cost = s->built_cost;
    u.new_cost = u.cost;
    if (u.cost > max_ratio * u.built_cost) {                         // false for a NaN on either side
        if (int rc = rebuild_device(s, d_tri, n_tri, d_norm, arith, st)) return rc;
        u.rebuilt = 1;
        u.new_cost = s->built_cost;
    }
    if (info) *info = u;
    return CERES_OK;
}

}  // namespace quality
}  // namespace ceres

using namespace ceres;

extern "C" {

int ceres_scene_sah_cost(ceres_scene* s, double* cost, void* stream) {
    if (!s || !cost) return set_error(CERES_EINVAL, "ceres_scene_sah_cost: null argument");
    return quality::sah_cost(s, cost, static_cast<hipStream_t>(stream));
}

int ceres_scene_rebuild_device(ceres_scene* s, const float* d_tri48, size_t n_tri, const float* d_norm36, int arith, void* stream) {
    if (int rc = quality::check_moved(s, d_tri48, n_tri, arith, true, "ceres_scene_rebuild_device")) return rc;
    return quality::rebuild_device(s, d_tri48, n_tri, d_norm36, arith, static_cast<hipStream_t>(stream));
}

int ceres_scene_rebuild(ceres_scene* s, const float* tri48, size_t n_tri, const float* norm36, int arith) {
    if (int rc = quality::check_moved(s, tri48, n_tri, arith, false, "ceres_scene_rebuild")) return rc;
    const float* d_tri = nullptr;
    const float* d_norm = nullptr;
    if (int rc = quality::stage_host(s, tri48, n_tri, norm36, &d_tri, &d_norm)) return rc;
    return quality::rebuild_device(s, d_tri, n_tri, d_norm, arith, s->stream);
}

int ceres_scene_update_device(ceres_scene* s, const float* d_tri48, size_t n_tri, const float* d_norm36, int arith,
                              double max_ratio, ceres_update_info* info, void* stream) {
    if (int rc = quality::check_moved(s, d_tri48, n_tri, arith, true, "ceres_scene_update_device")) return rc;
    if (int rc = quality::check_ratio(max_ratio, "ceres_scene_update_device")) return rc;
    return quality::update_device(s, d_tri48, n_tri, d_norm36, arith, max_ratio, info, static_cast<hipStream_t>(stream));
}

int ceres_scene_update(ceres_scene* s, const float* tri48, size_t n_tri, const float* norm36, int arith, double max_ratio,
                       ceres_update_info* info) {
    if (int rc = quality::check_moved(s, tri48, n_tri, arith, false, "ceres_scene_update")) return rc;
    if (int rc = quality::check_ratio(max_ratio, "ceres_scene_update")) return rc;
    const float* d_tri = nullptr;
    const float* d_norm = nullptr;
    if (int rc = quality::stage_host(s, tri48, n_tri, norm36, &d_tri, &d_norm)) return rc;
    return quality::update_device(s, d_tri, n_tri, d_norm, arith, max_ratio, info, s->stream);
}

}  // extern "C"
