// query_host.hpp -- the host layer the ray-query entry points share (render_hip.hip: float scenes,
// render64.hip: double scenes, ray_order.hip: the coherent calls).  Host code only; no kernel is here.
//
// A query family writes its own argument checks, fills its parameter block (scene_params for the
// scene's part), picks its kernel with one dispatch_bools call, and -- for its host-array call --
// wraps the device call in one RoundTrip.
#pragma once
#include <type_traits>
#include <utility>
#include <vector>

#include "hip_try.hpp"
#include "scene_internal.hpp"

namespace ceres {
namespace {   // nothing of this layer is a symbol of the library

template <typename T>
void dfree(T*& p) { if (p) { (void)hipFree(p); p = nullptr; } }

// the query kernels' eight counters and the call's device time as the caller sees them
inline void fill_stats(ceres_stats* st, const uint64_t c[8], double ms) {
    if (!st) return;
    st->rays = c[0]; st->hits = c[1]; st->primary_rays = c[2]; st->shadow_rays = c[3];
    st->node_pairs = c[4]; st->tri_tests = c[5]; st->ms = ms;
}

template <class P, class = void> struct has_root_box : std::false_type {};
template <class P> struct has_root_box<P, std::void_t<decltype(std::declval<P&>().root_box_ok)>> : std::true_type {};

// The scene's part of a parameter block: the float blocks (those with a root box) take the float
// layout, the double blocks the double one.
template <class P>
void scene_params(P& p, const ceres_scene* s) {
    if constexpr (has_root_box<P>::value) {
        p.pairs = s->d_pairs; p.tris = s->d_tris;
        for (int k = 0; k < 6; ++k) p.root_box[k] = s->root_box[k];
        p.root_box_ok = s->root_box_ok;
    } else {
        p.pairs = s->d_pairs64; p.tris = s->d_tris64;
    }
    p.orig = s->d_orig;
    p.stack_entries = s->stack_entries;
    p.root_leaf_count = s->root_leaf_count; p.root_leaf_first = s->root_leaf_first;
}

// Runtime booleans as template arguments: dispatch_bools(f, a, b) calls f(std::bool_constant<a>{},
// std::bool_constant<b>{}), one instantiation of f per combination.
template <class F>
void dispatch_bools(F&& f) { f(); }
template <class F, class... Bs>
void dispatch_bools(F&& f, bool b, Bs... rest) {
    if (b) dispatch_bools([&](auto... t) { f(std::true_type{}, t...); }, rest...);
    else dispatch_bools([&](auto... t) { f(std::false_type{}, t...); }, rest...);
}

// a start and an end event, destroyed with their owner
struct EventPair {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    EventPair() = default;
    EventPair(const EventPair&) = delete;
    EventPair& operator=(const EventPair&) = delete;
    ~EventPair() {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
};

// A host-array call's trip over the scene's stream: the device temporaries and the event pair, owned
// until the call returns.  The stream operations come in the order the caller writes them --
//   alloc ..., upload (+ start event), the device call(s), stop (end event), download ..., finish
// (synchronise, elapsed time) -- and each is skipped once `rc` is set, so the caller tests `rc` once
// at the end.  A second timed phase starts with restart().  After a CERES_EHIP work may still be in
// flight: the destructor synchronises the stream before it frees what that work reads.
class RoundTrip {
public:
    int rc = CERES_OK;

    RoundTrip(const char* name, ceres_scene* s) : name_(name), s_(s) {}
    ~RoundTrip() {
        if (rc == CERES_EHIP) (void)hipStreamSynchronize(s_->stream);
        for (void* p : bufs_) (void)hipFree(p);
    }

    // `bytes` of device memory when this buffer was asked for (null otherwise, and after a failure)
    void* alloc(bool wanted, size_t bytes) {
        void* p = nullptr;
        if (rc || !wanted) return nullptr;
        if (hipMalloc(&p, bytes) != hipSuccess) { rc = set_error(CERES_ENOMEM, "%s: device allocation failed", name_); return nullptr; }
        bufs_.push_back(p);
        return p;
    }
    void upload(void* d_rays, const void* rays, size_t bytes) {
        if (rc) return;
        if (hipEventCreate(&ev_.e0) != hipSuccess || hipEventCreate(&ev_.e1) != hipSuccess ||
            hipMemcpyAsync(d_rays, rays, bytes, hipMemcpyHostToDevice, s_->stream) != hipSuccess ||
            hipEventRecord(ev_.e0, s_->stream) != hipSuccess)
            rc = set_error(CERES_EHIP, "%s: upload failed", name_);
    }
    void restart() {
        if (!rc && hipEventRecord(ev_.e0, s_->stream) != hipSuccess) rc = set_error(CERES_EHIP, "%s: event failed", name_);
    }
    void stop() {
        if (!rc) copy_back(hipEventRecord(ev_.e1, s_->stream));
    }
    // a null `dst` is an output that was not asked for
    void download(void* dst, const void* d_src, size_t bytes) {
        if (!rc && dst) copy_back(hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, s_->stream));
    }
    // the milliseconds between the start and the end event
    double finish() {
        float ms = 0.f;
        if (!rc) copy_back(hipStreamSynchronize(s_->stream));
        if (!rc) copy_back(hipEventElapsedTime(&ms, ev_.e0, ev_.e1));
        return double(ms);
    }
    // finish(), then what a one-phase call returns: the statistics from its counters `c`, whose flag
    // of a traversal-stack overflow becomes the status
    int finish(ceres_stats* stats, const uint64_t c[8]) {
        const double ms = finish();
        if (rc) return rc;
        fill_stats(stats, c, ms);
        if (c[6]) return set_error(CERES_ESTACK, "traversal stack overflow");
        return CERES_OK;
    }

private:
    void copy_back(hipError_t e) {
        if (e != hipSuccess) rc = set_error(CERES_EHIP, "%s: copy back failed", name_);
    }
    const char* name_;
    ceres_scene* s_;
    std::vector<void*> bufs_;
    EventPair ev_;                      // which also makes a RoundTrip non-copyable
};

}  // namespace
}  // namespace ceres
