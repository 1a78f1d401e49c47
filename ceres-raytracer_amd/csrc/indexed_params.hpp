// indexed_params.hpp -- the index list of the indexed ray queries (ceres_*_indexed_device), shared by
// render_hip.hip and render64.hip.
//
// A query kernel's body is a template over its parameter block.  With the plain block, lane i of the
// launch takes ray i; with Indexed<block> it takes ray index[i] and writes that ray's own output
// slots, so a list may be a subset (trace only the survivors) or a permutation (a coherent order,
// ray_order.hip).  An entry at or past n_rays makes its lane idle -- no load, no store, no count --
// exactly as a tail lane of the plain launch is, so no list can address outside the caller's arrays.
// The choice is made at compile time: the plain instantiations contain no trace of the list.
#pragma once

#include <cstdint>
#include <type_traits>

namespace ceres {

template <class Base>
struct Indexed : Base {
    const uint32_t* index;                       // n_index entries; an entry >= n_rays is skipped
    uint32_t n_index;                            // below 2^31 (host-checked)
};

template <class PT> struct is_indexed : std::false_type {};
template <class Base> struct is_indexed<Indexed<Base>> : std::true_type {};

// The ray of launch position i (block * 64 + lane); 0xffffffff (>= any n_rays) where there is none.
template <class PT>
__device__ __forceinline__ uint32_t lane_ray(const PT& P, uint32_t i) {
    if constexpr (is_indexed<PT>::value) return i < P.n_index ? P.index[i] : 0xffffffffu;
    else return i;
}

// What counters[0] and [2] report: the rays of the launch.
template <class PT>
__device__ __forceinline__ uint32_t launch_rays(const PT& P) {
    if constexpr (is_indexed<PT>::value) return P.n_index;
    else return P.n_rays;
}

}  // namespace ceres
