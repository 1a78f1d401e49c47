// closest_point.hip -- closest-point queries on the GPU (ceres_closest_points_device, _indexed_device)
// and the host-array call over them (ceres_closest_points): for each of the caller's points the nearest
// point of the scene's surface, as {original triangle, squared distance, u, v}.
//
// The answer is the minimum over all triangles of closest_point.hpp's formula, whatever the tree and
// whatever the visiting order (the argument is stated there and in DESIGN.md "Closest-point queries");
// the walk below only decides how few records and triangles it takes to get there:
//   pop      a sibling pair: the 64-B record as four 16-B loads, the bound of both children's boxes.
//   leaves   a passing leaf child has its triangles tested at once, the nearer leaf first (the other is
//            tested against the best the first one left).
//   descent  of two passing inner children the one with the smaller bound (left on a tie) is next and
//            the other is pushed: at most one push per level, so the scene's stack_entries bound holds as
//            it does for the ray walks.  The index is clamped anyway and an overrun reported (counters[6]).
//   stack    in LDS, [entry][lane]: a plane of pair indices and beside it a plane of the pushed children's
//            bounds, so an entry gone stale because the best shrank is dropped at pop without fetching
//            its record -- after the first leaf most of a nearest-neighbour walk's stack is stale.
// One point per lane, 64 points of consecutive index (or of consecutive index-list entries,
// indexed_params.hpp) per single-wavefront workgroup; a point is one dwordx4 load, an answer one dwordx4
// store; tail lanes and skipped index entries run nothing.  Every index read from a record is checked
// against the scene's counts, so non-finite or caller-made scenes give meaningless answers, not faults.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "ceres_render.h"
#include "ceres_types.hpp"
#include "closest_point.hpp"
#include "indexed_params.hpp"
#include "query_host.hpp"

#pragma clang fp contract(off)

using namespace ceres;

namespace {

constexpr int kNearB = 64;                       // one wavefront per workgroup

// A/B switch (DESIGN.md "Closest-point queries" has both figures): 0 keeps a bare index stack -- every
// popped record is fetched and its children pruned by the box tests -- instead of the bound plane.
#ifndef CERES_NEAR_BOUND_PLANE
#define CERES_NEAR_BOUND_PLANE 1
#endif

struct NearParams {
    const float4* points;                        // n_rays x point16 {x, y, z, r2max}
    uint4* near;                                 // n_rays x near16 {prim, d2, u, v}
    unsigned long long* counters;                // 8 x u64 (zeroed before the launch) or NULL
    const SiblingPair* pairs;
    const Tri48* tris;
    const uint32_t* orig;
    uint32_t n_rays;                             // the points of the call (the name indexed_params.hpp reads)
    uint32_t n_pairs, n_tri;                     // the range checks
    uint32_t stack_entries, lds_entries;         // the walk's bound; entries per LDS plane (>= stack_entries)
    uint32_t root_leaf_count, root_leaf_first;
    uint32_t root_box_ok;                        // (unused: scene_params fills the float layout)
    float root_box[6];
};

__device__ __forceinline__ uint32_t wave_sum(uint32_t x) {
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

// the triangles of leaf slots [first, first + count) against the lane's point
template <class PT>
__device__ __forceinline__ void near_leaf(const PT& P, float px, float py, float pz, uint32_t first, uint32_t count, NearBest& best,
                                          uint32_t& n_tests) {
    if (first >= P.n_tri) return;
    const uint32_t end = count < P.n_tri - first ? first + count : P.n_tri;
    for (uint32_t k = first; k < end; ++k) {
        const float4* t = reinterpret_cast<const float4*>(P.tris + k);
        const float4 t0 = t[0], t1 = t[1], t2 = t[2];               // {p0, e1.x}, {e1.yz, e2.xy}, {e2.z, n}
        const float p0[3] = {t0.x, t0.y, t0.z}, e1[3] = {t0.w, t1.x, t1.y}, e2[3] = {t1.z, t1.w, t2.x};
        float v, w;
        const float d2 = near_tri(px, py, pz, p0, e1, e2, v, w);
        const uint32_t o = P.orig[k];
        if (o < P.n_tri && near_better(d2, o, best)) best = NearBest{d2, int32_t(o), v, w};
    }
    n_tests += end - first;
}

template <bool kStats, class PT>
__device__ __forceinline__ void closest_points_body(const PT& P) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const uint32_t lane = threadIdx.x;
    uint32_t* sidx = lds + lane;                                                   // [entry][lane] pair indices
    float* slb = reinterpret_cast<float*>(lds + size_t(P.lds_entries) * kNearB) + lane;   // ... and their bounds
    const uint32_t r = lane_ray(P, blockIdx.x * uint32_t(kNearB) + lane);          // n_rays < 2^31 (host-checked)
    bool found = false, overflow = false;
    uint32_t n_pairs = 0, n_tests = 0;
    if (r < P.n_rays) {
        const float4 pt = P.points[r];
        const float px = pt.x, py = pt.y, pz = pt.z;
        NearBest best{pt.w, -1, 0.f, 0.f};
        if (P.root_leaf_count) {
            near_leaf(P, px, py, pz, P.root_leaf_first, P.root_leaf_count, best, n_tests);
        } else {
            uint32_t sp = 0, cur = 0;
            while (cur < P.n_pairs) {
                ++n_pairs;
                const float4* q = reinterpret_cast<const float4*>(P.pairs + cur);
                const float4 q0 = q[0], q1 = q[1], q2 = q[2];
                const uint4 link = reinterpret_cast<const uint4*>(q)[3];           // lcount, lfirst, rcount, rfirst
                const float ll = near_box(px, py, pz, q0.x, q0.y, q0.z, q0.w, q1.x, q1.y);
                const float lr = near_box(px, py, pz, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w);
                const bool right_first = lr < ll;
                // leaves: the nearer first, the other against what it left
                if (right_first) {
                    if (link.z && !(lr > best.d2)) near_leaf(P, px, py, pz, link.w, link.z, best, n_tests);
                    if (link.x && !(ll > best.d2)) near_leaf(P, px, py, pz, link.y, link.x, best, n_tests);
                } else {
                    if (link.x && !(ll > best.d2)) near_leaf(P, px, py, pz, link.y, link.x, best, n_tests);
                    if (link.z && !(lr > best.d2)) near_leaf(P, px, py, pz, link.w, link.z, best, n_tests);
                }
                const bool go_l = !link.x && !(ll > best.d2), go_r = !link.z && !(lr > best.d2);
                if (go_l && go_r) {
                    if (sp >= P.stack_entries) { overflow = true; break; }
                    sidx[size_t(sp) * kNearB] = right_first ? link.y : link.w;
                    if (CERES_NEAR_BOUND_PLANE) slb[size_t(sp) * kNearB] = right_first ? ll : lr;
                    ++sp;
                    cur = right_first ? link.w : link.y;
                } else if (go_l || go_r) {
                    cur = go_l ? link.y : link.w;
                } else {
                    cur = 0xffffffffu;                                             // nothing left: ends the walk
                    while (sp) {
                        --sp;
                        if (CERES_NEAR_BOUND_PLANE && slb[size_t(sp) * kNearB] > best.d2) continue;   // stale: dropped without its record
                        cur = sidx[size_t(sp) * kNearB];
                        break;
                    }
                }
            }
        }
        found = best.prim >= 0;
        P.near[r] = found ? make_uint4(uint32_t(best.prim), __float_as_uint(best.d2), __float_as_uint(best.u), __float_as_uint(best.v))
                          : make_uint4(0xffffffffu, 0u, 0u, 0u);                   // nothing found: {-1, 0, 0, 0}
    }
    if (P.counters) {                                                              // wave-uniform
        const uint32_t nf = __popcll(__ballot(found));
        if (lane == 0 && nf) atomicAdd(&P.counters[1], (unsigned long long)nf);
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

// The plain launch (lane i takes point i) and the indexed one (lane i takes point index[i]): one body,
// chosen by the parameter block.  Indexed launches have no stats instantiation.
template <bool kStats>
__global__ __launch_bounds__(kNearB) void ceres_closest_points_k(const NearParams P) {
    closest_points_body<kStats>(P);
}
__global__ __launch_bounds__(kNearB) void ceres_closest_points_idx_k(const Indexed<NearParams> P) {
    closest_points_body<false>(P);
}

// The argument rules all calls share: a negative ceres_status when the call is refused, 1 when there is
// nothing to do (n_points = 0), 0 when there is.
int check_near_args(const ceres_scene* s, const void* points, size_t n_points, const void* near) {
    if (!s) return set_error(CERES_EINVAL, "ceres_closest_points: null scene");
    if (s->f64) return set_error(CERES_EUNSUPPORTED, "ceres_closest_points: closest-point queries take float scenes");
    if (!near) return set_error(CERES_EINVAL, "ceres_closest_points: null output");
    if (n_points >= (size_t(1) << 31))
        return set_error(CERES_EUNSUPPORTED, "ceres_closest_points: %zu points (below 2^31 per call)", n_points);
    if (n_points == 0) return 1;
    if (!points) return set_error(CERES_EINVAL, "ceres_closest_points: null points");
    return 0;
}

int closest_points_launch(ceres_scene* s, const void* d_points16, size_t n_points, const uint32_t* d_index, size_t n_index, bool indexed,
                          void* d_near16, uint64_t* d_counters, void* stream_) {
    if (const int chk = check_near_args(s, d_points16, n_points, d_near16)) return chk < 0 ? chk : CERES_OK;
    if ((reinterpret_cast<uintptr_t>(d_points16) | reinterpret_cast<uintptr_t>(d_near16)) & 15u)
        return set_error(CERES_EINVAL, "ceres_closest_points: points and answers must be 16-byte aligned");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    HIP_TRY(hipSetDevice(s->device));
    Indexed<NearParams> P{};
    P.index = d_index; P.n_index = uint32_t(n_index);
    P.points = static_cast<const float4*>(d_points16);
    P.near = static_cast<uint4*>(d_near16);
    P.counters = reinterpret_cast<unsigned long long*>(d_counters);
    scene_params(P, s);
    P.n_rays = uint32_t(n_points);
    P.n_pairs = uint32_t(s->n_pairs); P.n_tri = uint32_t(s->n_tri);
    P.lds_entries = std::max<uint32_t>(1, P.stack_entries);
    // two [entry][lane] planes of 4-byte words: the pair indices, then the bounds
    const size_t lds = size_t(P.lds_entries) * kNearB * 8;
    if (lds > s->max_lds_per_block)
        return set_error(CERES_EINVAL, "ceres_closest_points: the traversal stack needs %zu B of LDS per workgroup (%zu available)", lds,
                         s->max_lds_per_block);
    if (indexed)
        if (const int chk = check_index_list("ceres_closest_points_indexed", s, d_index, n_index)) return chk < 0 ? chk : CERES_OK;
    if (d_counters) HIP_TRY(hipMemsetAsync(d_counters, 0, 8 * sizeof(uint64_t), stream));
    const dim3 grid(uint32_t(((indexed ? n_index : n_points) + kNearB - 1) / kNearB)), block(kNearB);
    const NearParams& P0 = P;                                         // the plain kernels' block
    if (indexed) {                                                    // (a stats scene was refused above)
        hipLaunchKernelGGL(ceres_closest_points_idx_k, grid, block, lds, stream, P);
    } else {
        dispatch_bools([&](auto st) {
            hipLaunchKernelGGL(ceres_closest_points_k<decltype(st)::value>, grid, block, lds, stream, P0);
        }, (s->flags & CERES_SCENE_STATS) != 0);
    }
    HIP_TRY(hipGetLastError());
    return CERES_OK;
}

}  // namespace

extern "C" {

int ceres_closest_points_device(ceres_scene* s, const void* d_points16, size_t n_points, void* d_near16, uint64_t* d_counters,
                                void* stream) {
    return closest_points_launch(s, d_points16, n_points, nullptr, 0, false, d_near16, d_counters, stream);
}

int ceres_closest_points_indexed_device(ceres_scene* s, const void* d_points16, size_t n_points, const uint32_t* d_index,
                                        size_t n_index, void* d_near16, uint64_t* d_counters, void* stream) {
    return closest_points_launch(s, d_points16, n_points, d_index, n_index, true, d_near16, d_counters, stream);
}

int ceres_closest_points(ceres_scene* s, const void* points16, size_t n_points, void* near16, ceres_stats* stats) {
    uint64_t c[8] = {0};
    if (const int chk = check_near_args(s, points16, n_points, near16)) {
        if (chk < 0) return chk;
        fill_stats(stats, c, 0.0);                                    // n_points = 0: a successful no-op
        return CERES_OK;
    }
    HIP_TRY(hipSetDevice(s->device));
    RoundTrip t("ceres_closest_points", s);
    void* dp = t.alloc(true, n_points * 16);
    void* dn = t.alloc(true, n_points * 16);
    t.upload(dp, points16, n_points * 16);
    if (!t.rc) t.rc = ceres_closest_points_device(s, dp, n_points, dn, s->d_counters, s->stream);
    t.stop();
    t.download(c, s->d_counters, sizeof c);
    t.download(near16, dn, n_points * 16);
    return t.finish(stats, c);
}

}  // extern "C"
