// ray_order.hip -- the coherent ray order on the GPU (ceres_ray_order_device, _f64_device) and the
// host-array calls that use it (ceres_trace_rays_coherent, _f64).
//
// A caller's rays have no screen order, and a wavefront of the query kernels takes 64 consecutive
// entries: it runs as long as its longest ray, and a wavefront of mixed octants loses the
// octant-specialised box loop.  The order is a permutation of the ray indices that puts rays alike in
// octant and entry cell next to each other and gathers the rays that cannot reach the scene at the
// end; the indexed queries (indexed_params.hpp) take it as their index list and write every answer to
// its own ray's slot, so nothing is moved and nothing is scattered back.
//
//   key kernel   one ray per lane: the record (two dwordx4 loads, four for a double ray), ray_key.hpp's
//                key, stores of the key and of the lane's own index.  The order box comes from pair 0
//                of the scene's sibling pairs: wave-uniform loads of one cached record, so a refitted
//                or rebuilt scene needs no state of the order's own.
//   sort         rocprim's stable radix sort of the (key >> kRayKeyBeginBit, index) pairs over the 25 used
//                bits: equal keys stay in index order, so the result is one
//                fixed array for given inputs -- ceres_ray_order_cpu's.
// Everything is enqueued on the caller's stream and nothing is synchronised or allocated: the scratch
// is the caller's, [keys | sorted keys | indices | rocprim's temporary storage].
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>
#include <cstdint>
#include <type_traits>

#include "ceres_render.h"
#include "ceres_types.hpp"
#include "query_host.hpp"
#include "ray_key.hpp"

#pragma clang fp contract(off)

using namespace ceres;

namespace {

constexpr int kKeyBlock = 256;
constexpr size_t kAlign = 256;
constexpr size_t align_up(size_t x) { return (x + kAlign - 1) / kAlign * kAlign; }

// An upper bound of rocprim::radix_sort_pairs's temporary storage for n (u32, u32) pairs, from n alone
// (the size query itself needs a device): its double buffers (8 n), one look-back state per digit and
// block of at least 256 items (256 x 4 B x n / 256 = 4 n, counted thrice for the batch tail and the
// alignment of each part), histograms and block ids.  ray_order_launch checks it against rocprim's
// own figure and refuses to run when it falls short.
constexpr size_t sort_temp_bound(size_t n) { return 24 * n + (size_t(256) << 10); }

template <class S> struct Pairs;
template <> struct Pairs<float> {
    using type = SiblingPair;
    static const type* of(const ceres_scene* s) { return s->d_pairs; }
};
template <> struct Pairs<double> {
    using type = SiblingPair64;
    static const type* of(const ceres_scene* s) { return s->d_pairs64; }
};

template <class S>
__global__ __launch_bounds__(kKeyBlock) void ceres_ray_key_k(const void* __restrict__ rays_, uint32_t n_rays,
                                                            const typename Pairs<S>::type* __restrict__ pairs,
                                                            uint32_t root_leaf_count, uint32_t* __restrict__ keys,
                                                            uint32_t* __restrict__ index) {
    const uint32_t r = blockIdx.x * uint32_t(kKeyBlock) + threadIdx.x;   // n_rays < 2^31 (host-checked)
    if (r >= n_rays) return;
    const S zero[6] = {0, 0, 0, 0, 0, 0};
    const OrderBox<S> box = root_leaf_count ? order_box<S>(zero, zero, 1u) : order_box<S>(pairs[0].lb, pairs[0].rb, 0u);
    S o[3], d[3], tmin, tmax;
    uint32_t sign;
    if constexpr (std::is_same<S, float>::value) {
        const float4* q = static_cast<const float4*>(rays_) + 2 * size_t(r);
        const float4 a = q[0], b = q[1];
        o[0] = a.x; o[1] = a.y; o[2] = a.z; d[0] = a.w; d[1] = b.x; d[2] = b.y; tmin = b.z; tmax = b.w;
        sign = (__float_as_uint(d[0]) >> 31) | ((__float_as_uint(d[1]) >> 31) << 1) | ((__float_as_uint(d[2]) >> 31) << 2);
    } else {
        const double2* q = static_cast<const double2*>(rays_) + 4 * size_t(r);
        const double2 a = q[0], b = q[1], c = q[2], w = q[3];
        o[0] = a.x; o[1] = a.y; o[2] = b.x; d[0] = b.y; d[1] = c.x; d[2] = c.y; tmin = w.x; tmax = w.y;
        auto sb = [](double x) { return uint32_t((unsigned long long)__double_as_longlong(x) >> 63); };
        sign = sb(d[0]) | (sb(d[1]) << 1) | (sb(d[2]) << 2);
    }
    keys[r] = ray_key<S>(o, d, tmin, tmax, sign, box) >> kRayKeyBeginBit;   // the sorted bits, from bit 0 (ray_order_launch)
    index[r] = r;
}

template <class S>
int ray_order_launch(const char* name, ceres_scene* s, const void* d_rays, size_t n_rays, uint32_t* d_order, void* d_scratch,
                     size_t scratch_bytes, void* stream_) {
    constexpr bool f64 = std::is_same<S, double>::value;
    if (!s) return set_error(CERES_EINVAL, "%s: null scene", name);
    if (s->f64 != f64) return set_error(CERES_EUNSUPPORTED, "%s: the scene is %s precision", name, s->f64 ? "double" : "single");
    if (n_rays >= (size_t(1) << 31)) return set_error(CERES_EUNSUPPORTED, "%s: %zu rays (below 2^31 per call)", name, n_rays);
    if (n_rays == 0) return CERES_OK;
    if (!d_rays || !d_order || !d_scratch) return set_error(CERES_EINVAL, "%s: null rays, order or scratch", name);
    if (reinterpret_cast<uintptr_t>(d_rays) & 15u) return set_error(CERES_EINVAL, "%s: rays must be 16-byte aligned", name);
    if (reinterpret_cast<uintptr_t>(d_order) & 3u) return set_error(CERES_EINVAL, "%s: order must be 4-byte aligned", name);
    if (reinterpret_cast<uintptr_t>(d_scratch) & 15u) return set_error(CERES_EINVAL, "%s: scratch must be 16-byte aligned", name);
    if (scratch_bytes < ceres_ray_order_scratch_bytes(n_rays))
        return set_error(CERES_EINVAL, "%s: %zu B of scratch, %zu rays need %zu (ceres_ray_order_scratch_bytes)", name, scratch_bytes,
                         n_rays, ceres_ray_order_scratch_bytes(n_rays));
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    HIP_TRY(hipSetDevice(s->device));
    // the carve-up: every part starts at a multiple of kAlign (the size includes the slack for the first)
    const uintptr_t base = reinterpret_cast<uintptr_t>(d_scratch), first = align_up(base);
    const size_t part = align_up(4 * n_rays);
    uint32_t* keys = reinterpret_cast<uint32_t*>(first);
    uint32_t* keys_sorted = reinterpret_cast<uint32_t*>(first + part);
    uint32_t* index = reinterpret_cast<uint32_t*>(first + 2 * part);
    void* temp = reinterpret_cast<void*>(first + 3 * part);
    const size_t temp_have = scratch_bytes - (first - base) - 3 * part;
    size_t temp_need = 0;
    // The array holds key >> kRayKeyBeginBit and the sort reads its bits from 0: rocprim's merge-sort path
    // (mid-sized inputs) builds its mask with 1 << (begin_bit + bits), which is 1 << 32 for a range that
    // starts above bit 0 and ends at bit 32.
    constexpr unsigned kSortBits = kRayKeyEndBit - kRayKeyBeginBit;
    HIP_TRY(rocprim::radix_sort_pairs(nullptr, temp_need, keys, keys_sorted, index, d_order, n_rays, 0u, kSortBits, stream));
    if (temp_need > temp_have)
        return set_error(CERES_EUNSUPPORTED, "%s: the sort of %zu rays needs %zu B of temporary storage, the scratch bound leaves %zu",
                         name, n_rays, temp_need, temp_have);
    const dim3 grid(uint32_t((n_rays + kKeyBlock - 1) / kKeyBlock)), block(kKeyBlock);
    hipLaunchKernelGGL(ceres_ray_key_k<S>, grid, block, 0, stream, d_rays, uint32_t(n_rays), Pairs<S>::of(s), s->root_leaf_count, keys,
                       index);
    HIP_TRY(hipGetLastError());
    size_t temp_bytes = temp_have;
    HIP_TRY(rocprim::radix_sort_pairs(temp, temp_bytes, keys, keys_sorted, index, d_order, n_rays, 0u, kSortBits, stream));
    return CERES_OK;
}

// ceres_trace_rays's host-array flow with the order computed and the indexed kernel launched.  The
// plain call's refusals come from the indexed device call (nothing has been launched before it).
template <class S>
int trace_rays_coherent(const char* name, ceres_scene* s, const void* rays, size_t n_rays, int mode, void* hits, uint8_t* occluded,
                        ceres_stats* stats) {
    constexpr bool f64 = std::is_same<S, double>::value;
    constexpr size_t kRay = f64 ? 64 : 32, kHit = f64 ? 32 : 16;
    uint64_t c[8] = {0};
    if (!s) return set_error(CERES_EINVAL, "%s: null scene", name);
    if (s->f64 != f64) return set_error(CERES_EUNSUPPORTED, "%s: the scene is %s precision", name, s->f64 ? "double" : "single");
    if (s->flags & CERES_SCENE_STATS)
        return set_error(CERES_EUNSUPPORTED, "%s: CERES_SCENE_STATS scenes take the plain calls (statistics are theirs)", name);
    if (mode & ~(CERES_MODE_FMA | CERES_MODE_ROBUST)) return set_error(CERES_EINVAL, "%s: bad mode %d", name, mode);
    if (f64 && (mode & CERES_MODE_ROBUST)) return set_error(CERES_EUNSUPPORTED, "%s: CERES_MODE_ROBUST takes float scenes", name);
    if (!hits && !occluded) return set_error(CERES_EINVAL, "%s: neither hits nor occluded asked for", name);
    if (n_rays >= (size_t(1) << 31)) return set_error(CERES_EUNSUPPORTED, "%s: %zu rays (below 2^31 per call)", name, n_rays);
    if (n_rays == 0) { fill_stats(stats, c, 0.0); return CERES_OK; }
    if (!rays) return set_error(CERES_EINVAL, "%s: null rays", name);
    HIP_TRY(hipSetDevice(s->device));
    const size_t scratch = ceres_ray_order_scratch_bytes(n_rays);
    RoundTrip t(name, s);
    void* dr = t.alloc(true, n_rays * kRay);
    void* dh = t.alloc(hits, n_rays * kHit);
    uint8_t* dc = static_cast<uint8_t*>(t.alloc(occluded, n_rays));
    uint32_t* dord = static_cast<uint32_t*>(t.alloc(true, n_rays * 4));
    void* dsc = t.alloc(true, scratch);
    t.upload(dr, rays, n_rays * kRay);
    if (!t.rc) t.rc = ray_order_launch<S>(name, s, dr, n_rays, dord, dsc, scratch, s->stream);
    if (!t.rc) {
        if constexpr (f64) t.rc = ceres_trace_rays_f64_indexed_device(s, dr, n_rays, dord, n_rays, mode, dh, dc, s->d_counters, s->stream);
        else t.rc = ceres_trace_rays_indexed_device(s, dr, n_rays, dord, n_rays, mode, dh, dc, s->d_counters, s->stream);
    }
    t.stop();
    t.download(c, s->d_counters, sizeof c);
    t.download(hits, dh, n_rays * kHit);
    t.download(occluded, dc, n_rays);
    return t.finish(stats, c);
}

}  // namespace

extern "C" {

size_t ceres_ray_order_scratch_bytes(size_t n_rays) { return kAlign + 3 * align_up(4 * n_rays) + sort_temp_bound(n_rays); }

int ceres_ray_order_device(ceres_scene* s, const void* d_rays32, size_t n_rays, uint32_t* d_order, void* d_scratch,
                           size_t scratch_bytes, void* stream) {
    return ray_order_launch<float>("ceres_ray_order", s, d_rays32, n_rays, d_order, d_scratch, scratch_bytes, stream);
}

int ceres_ray_order_f64_device(ceres_scene* s, const void* d_rays64, size_t n_rays, uint32_t* d_order, void* d_scratch,
                               size_t scratch_bytes, void* stream) {
    return ray_order_launch<double>("ceres_ray_order_f64", s, d_rays64, n_rays, d_order, d_scratch, scratch_bytes, stream);
}

int ceres_trace_rays_coherent(ceres_scene* s, const void* rays32, size_t n_rays, int mode, void* hits16, uint8_t* occluded,
                              ceres_stats* stats) {
    return trace_rays_coherent<float>("ceres_trace_rays_coherent", s, rays32, n_rays, mode, hits16, occluded, stats);
}

int ceres_trace_rays_coherent_f64(ceres_scene* s, const void* rays64, size_t n_rays, int mode, void* hits32, uint8_t* occluded,
                                  ceres_stats* stats) {
    return trace_rays_coherent<double>("ceres_trace_rays_coherent_f64", s, rays64, n_rays, mode, hits32, occluded, stats);
}

}  // extern "C"
