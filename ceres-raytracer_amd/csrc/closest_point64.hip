// closest_point64.hip -- closest-point queries on double scenes on the GPU (ceres_closest_points_f64_device,
// _f64_indexed_device) and the host-array call over them (ceres_closest_points_f64): closest_point.hip's
// query over the scene's Tri96 triangles and SiblingPair64 boxes, in double.
//
// The answer is the minimum over all triangles of closest_point64.hpp's formula, whatever the tree and
// whatever the visiting order (DESIGN.md "Closest-point queries on double scenes"); the walk is the float
// kernel's:
//   pop      a sibling pair: the 112-B record as seven 16-B loads, the bound of both children's boxes.
//   leaves   a passing leaf child has its triangles tested at once, the nearer leaf first.
//   descent  of two passing inner children the one with the smaller bound (left on a tie) is next and
//            the other is pushed: at most one push per level, so the scene's stack_entries bound holds.
//            The index is clamped anyway and an overrun reported (counters[6]).
//   stack    in LDS, [entry][lane]: a plane of 4-byte pair indices, 256 B per tree level.  The float
//            kernel's second plane -- the pushed children's bounds, so that an entry gone stale is dropped
//            at pop without fetching its record -- is compiled out here: measured, it saves 6-11 % of the
//            record fetches and still costs 1-3 % of the time (DESIGN.md has the figures).
//            -DCERES_NEAR_BOUND_PLANE=1 builds it: 8-byte bounds behind the indices, 12 B per entry per
//            lane; lane l's bound lies on banks 2l, 2l + 1 (mod 64), so a ds_read_b64 / ds_write_b64 of
//            32 lanes is conflict-free.
// One point per lane, 64 points per single-wavefront workgroup; a point is two 16-B loads, an answer two
// 16-B stores; tail lanes and skipped index entries run nothing.  Every index read from a record is
// checked against the scene's counts, so non-finite or caller-made scenes give meaningless answers, not
// faults.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "ceres_render.h"
#include "ceres_types.hpp"
#include "closest_point64.hpp"
#include "indexed_params.hpp"
#include "query_host.hpp"

#pragma clang fp contract(off)

using namespace ceres;

namespace {

constexpr int kNearB = 64;                       // one wavefront per workgroup

// A/B switch (DESIGN.md "Closest-point queries on double scenes" has both figures): 0, the default here,
// keeps a bare index stack -- every popped record is fetched and its children pruned by the box tests
// -- 1 adds the bound plane.
#ifndef CERES_NEAR_BOUND_PLANE
#define CERES_NEAR_BOUND_PLANE 0
#endif
constexpr size_t kNearEntryBytes = CERES_NEAR_BOUND_PLANE ? 12 : 4;   // LDS per stack entry per lane

struct Near64Params {
    const double2* points;                       // n_rays x point32 {x, y, z, r2max}: 2 x 16 B
    uint4* near;                                 // n_rays x near32 {prim, 0, d2, u, v}: 2 x 16 B
    unsigned long long* counters;                // 8 x u64 (zeroed before the launch) or NULL
    const SiblingPair64* pairs;
    const Tri96* tris;
    const uint32_t* orig;
    uint32_t n_rays;                             // the points of the call (the name indexed_params.hpp reads)
    uint32_t n_pairs, n_tri;                     // the range checks
    uint32_t stack_entries, lds_entries;         // the walk's bound; entries per LDS plane (>= stack_entries)
    uint32_t root_leaf_count, root_leaf_first;
};

__device__ __forceinline__ uint32_t wave_sum(uint32_t x) {
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

// the triangles of leaf slots [first, first + count) against the lane's point
template <class PT>
__device__ __forceinline__ void near_leaf(const PT& P, double px, double py, double pz, uint32_t first, uint32_t count, NearBest64& best,
                                          uint32_t& n_tests) {
    if (first >= P.n_tri) return;
    const uint32_t end = count < P.n_tri - first ? first + count : P.n_tri;
    for (uint32_t k = first; k < end; ++k) {
        const double2* t = reinterpret_cast<const double2*>(P.tris + k);
        const double2 t0 = t[0], t1 = t[1], t2 = t[2], t3 = t[3], t4 = t[4];   // {p0.xy}, {p0.z, e1.x}, {e1.yz}, {e2.xy}, {e2.z, n.x}
        const double p0[3] = {t0.x, t0.y, t1.x}, e1[3] = {t1.y, t2.x, t2.y}, e2[3] = {t3.x, t3.y, t4.x};
        double v, w;
        const double d2 = near64_tri(px, py, pz, p0, e1, e2, v, w);
        const uint32_t o = P.orig[k];
        if (o < P.n_tri && near64_better(d2, o, best)) best = NearBest64{d2, int32_t(o), v, w};
    }
    n_tests += end - first;
}

template <bool kStats, class PT>
__device__ __forceinline__ void closest_points64_body(const PT& P) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const uint32_t lane = threadIdx.x;
    uint32_t* sidx = lds + lane;                                                   // [entry][lane] pair indices
    // ... and, with the bound plane, their bounds: the index plane is lds_entries x 256 B long, so the
    // 8-byte plane is aligned
    [[maybe_unused]] double* slb = reinterpret_cast<double*>(lds + size_t(P.lds_entries) * kNearB) + lane;
    const uint32_t r = lane_ray(P, blockIdx.x * uint32_t(kNearB) + lane);          // n_rays < 2^31 (host-checked)
    bool found = false, overflow = false;
    uint32_t n_pairs = 0, n_tests = 0;
    if (r < P.n_rays) {
        const double2 pa = P.points[2 * size_t(r)], pb = P.points[2 * size_t(r) + 1];
        const double px = pa.x, py = pa.y, pz = pb.x;
        NearBest64 best{pb.y, -1, 0.0, 0.0};
        if (P.root_leaf_count) {
            near_leaf(P, px, py, pz, P.root_leaf_first, P.root_leaf_count, best, n_tests);
        } else {
            uint32_t sp = 0, cur = 0;
            while (cur < P.n_pairs) {
                ++n_pairs;
                const double2* q = reinterpret_cast<const double2*>(P.pairs + cur);
                const double2 A = q[0], B = q[1], C = q[2], D = q[3], E = q[4], F = q[5];
                const uint4 link = reinterpret_cast<const uint4*>(q)[6];           // lcount, lfirst, rcount, rfirst
                const double ll = near64_box(px, py, pz, A.x, A.y, B.x, B.y, C.x, C.y);
                const double lr = near64_box(px, py, pz, D.x, D.y, E.x, E.y, F.x, F.y);
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
        uint4* out = P.near + 2 * size_t(r);
        if (found) {
            out[0] = make_uint4(uint32_t(best.prim), 0u, uint32_t(__double2loint(best.d2)), uint32_t(__double2hiint(best.d2)));
            out[1] = make_uint4(uint32_t(__double2loint(best.u)), uint32_t(__double2hiint(best.u)), uint32_t(__double2loint(best.v)),
                                uint32_t(__double2hiint(best.v)));
        } else {                                                                   // nothing found: {-1, 0, 0.0, 0.0, 0.0}
            out[0] = make_uint4(0xffffffffu, 0u, 0u, 0u);
            out[1] = make_uint4(0u, 0u, 0u, 0u);
        }
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
__global__ __launch_bounds__(kNearB) void ceres_closest_points64_k(const Near64Params P) {
    closest_points64_body<kStats>(P);
}
__global__ __launch_bounds__(kNearB) void ceres_closest_points64_idx_k(const Indexed<Near64Params> P) {
    closest_points64_body<false>(P);
}

// The argument rules all calls share, in the float calls' order: a negative ceres_status when the call is
// refused, 1 when there is nothing to do (n_points = 0), 0 when there is.
int check_near64_args(const ceres_scene* s, const void* points, size_t n_points, const void* near) {
    if (!s) return set_error(CERES_EINVAL, "ceres_closest_points_f64: null scene");
    if (!s->f64) return set_error(CERES_EUNSUPPORTED, "ceres_closest_points_f64: the _f64 closest-point calls take double scenes");
    if (!near) return set_error(CERES_EINVAL, "ceres_closest_points_f64: null output");
    if (n_points >= (size_t(1) << 31))
        return set_error(CERES_EUNSUPPORTED, "ceres_closest_points_f64: %zu points (below 2^31 per call)", n_points);
    if (n_points == 0) return 1;
    if (!points) return set_error(CERES_EINVAL, "ceres_closest_points_f64: null points");
    return 0;
}

int closest_points64_launch(ceres_scene* s, const void* d_points32, size_t n_points, const uint32_t* d_index, size_t n_index, bool indexed,
                            void* d_near32, uint64_t* d_counters, void* stream_) {
    if (const int chk = check_near64_args(s, d_points32, n_points, d_near32)) return chk < 0 ? chk : CERES_OK;
    if ((reinterpret_cast<uintptr_t>(d_points32) | reinterpret_cast<uintptr_t>(d_near32)) & 15u)
        return set_error(CERES_EINVAL, "ceres_closest_points_f64: points and answers must be 16-byte aligned");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    HIP_TRY(hipSetDevice(s->device));
    Indexed<Near64Params> P{};
    P.index = d_index; P.n_index = uint32_t(n_index);
    P.points = static_cast<const double2*>(d_points32);
    P.near = static_cast<uint4*>(d_near32);
    P.counters = reinterpret_cast<unsigned long long*>(d_counters);
    scene_params(P, s);
    P.n_rays = uint32_t(n_points);
    P.n_pairs = uint32_t(s->n_pairs); P.n_tri = uint32_t(s->n_tri);
    P.lds_entries = std::max<uint32_t>(1, P.stack_entries);
    // the [entry][lane] plane of 4-byte pair indices (and, with the bound plane, of 8-byte bounds)
    const size_t lds = size_t(P.lds_entries) * kNearB * kNearEntryBytes;
    if (lds > s->max_lds_per_block)
        return set_error(CERES_EINVAL, "ceres_closest_points_f64: the traversal stack needs %zu B of LDS per workgroup (%zu available)", lds,
                         s->max_lds_per_block);
    if (indexed)
        if (const int chk = check_index_list("ceres_closest_points_f64_indexed", s, d_index, n_index)) return chk < 0 ? chk : CERES_OK;
    if (d_counters) HIP_TRY(hipMemsetAsync(d_counters, 0, 8 * sizeof(uint64_t), stream));
    const dim3 grid(uint32_t(((indexed ? n_index : n_points) + kNearB - 1) / kNearB)), block(kNearB);
    const Near64Params& P0 = P;                                       // the plain kernels' block
    if (indexed) {                                                    // (a stats scene was refused above)
        hipLaunchKernelGGL(ceres_closest_points64_idx_k, grid, block, lds, stream, P);
    } else {
        dispatch_bools([&](auto st) {
            hipLaunchKernelGGL(ceres_closest_points64_k<decltype(st)::value>, grid, block, lds, stream, P0);
        }, (s->flags & CERES_SCENE_STATS) != 0);
    }
    HIP_TRY(hipGetLastError());
    return CERES_OK;
}

}  // namespace

extern "C" {

int ceres_closest_points_f64_device(ceres_scene* s, const void* d_points32, size_t n_points, void* d_near32, uint64_t* d_counters,
                                    void* stream) {
    return closest_points64_launch(s, d_points32, n_points, nullptr, 0, false, d_near32, d_counters, stream);
}

int ceres_closest_points_f64_indexed_device(ceres_scene* s, const void* d_points32, size_t n_points, const uint32_t* d_index,
                                            size_t n_index, void* d_near32, uint64_t* d_counters, void* stream) {
    return closest_points64_launch(s, d_points32, n_points, d_index, n_index, true, d_near32, d_counters, stream);
}

int ceres_closest_points_f64(ceres_scene* s, const void* points32, size_t n_points, void* near32, ceres_stats* stats) {
    uint64_t c[8] = {0};
    if (const int chk = check_near64_args(s, points32, n_points, near32)) {
        if (chk < 0) return chk;
        fill_stats(stats, c, 0.0);                                    // n_points = 0: a successful no-op
        return CERES_OK;
    }
    HIP_TRY(hipSetDevice(s->device));
    RoundTrip t("ceres_closest_points_f64", s);
    void* dp = t.alloc(true, n_points * 32);
    void* dn = t.alloc(true, n_points * 32);
    t.upload(dp, points32, n_points * 32);
    if (!t.rc) t.rc = ceres_closest_points_f64_device(s, dp, n_points, dn, s->d_counters, s->stream);
    t.stop();
    t.download(c, s->d_counters, sizeof c);
    t.download(near32, dn, n_points * 32);
    return t.finish(stats, c);
}

}  // extern "C"
