// bvh_build64.hip -- the reference's binned-SAH build of a Bvh<double> on gfx950: bvh_build.hip
// with every value a double (BinnedSahBuilder<Bvh<double>,16>, binned_sah_builder.hpp:39-234).
//
// Same topology, primitive_indices order and node boxes as the host model bvh_build<double, G>
// (scene_host.cpp), down to the sign of a zero, in both arithmetics; only node NUMBERING differs,
// and it is deterministic: breadth-first for the large nodes, then every small subtree
// contiguously.  A file of its own, so the float builder's generated code does not change.
//
// Two regimes, as in the float builder:
//   * large items (> kSmall primitives; > kSmallFew in a mesh below kFewPrims): level-synchronous, one thread per primitive position;
//     std::partition reproduced with a prefix sum (bvh_build.hip).
//   * small items (<= kSmall): one wavefront builds the whole subtree in LDS; its bins are the same
//     value and tie words as the large items', in LDS, one lane per primitive (position = the
//     primitive's place in the reference's sequential loop).
//
// The order-independent reduction of the large items' bins and of the root box.  The fold to
// reproduce starts from the empty box and takes std::min / std::max over the bounds in position
// order: among equal values the first wins, -0.0 == +0.0, and a NaN (which never arrives first:
// the fold starts from +-DBL_MAX) never wins.  A double and a position do not fit one 64-bit
// atomic, so a bound is two words reduced INDEPENDENTLY:
//   * value: a 64-bit atomicMin / atomicMax of the order-preserving image of the double's bits,
//     with -0 mapped to +0 and a NaN mapped to the empty key.  This alone gives the fold's VALUE
//     for every order of arrival.
//   * tie:   a 32-bit atomicMin of (position << 1 | sign bit) that only contributors whose bound
//     is +-0 touch (for a maximum too: the first of equal values wins in both folds).
// Two doubles that compare equal differ in bits only when both are zeros, so the fold's result
// is decided by the value word unless that value is zero; then -- and only then -- the tie word
// is read, and it names the first zero in position order, whose sign the sequential fold keeps
// (every later zero compares equal and is dropped).  A partial reduction (a lane's run, a
// workgroup's LDS bin) forwards a tie only when ITS value is zero, with the position of its first
// zero; if the final value is zero every partial that held a zero has forwarded one, so the
// minimum over them is the first zero overall.  If the final value is not zero the tie word is
// never read.
//
// No value passes through a float.  Compiled with -ffp-contract=off; the only fma in the exact
// flavour is the bin index's fast_multiply_add (binned_sah_builder.hpp:144-147); CERES_ARITH_FMA
// adds the three SAH-cost contractions of the reference's CMake build (oracle/contraction_sites.txt).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cstdint>
#include <cstdlib>
#include <cstring>

#include "ceres_render.h"
#include "ceres_types.hpp"
#include "hip_try.hpp"
#include "host_common.hpp"
#include "dev_scan.hpp"

#pragma clang fp contract(off)

namespace ceres {
namespace bvhdev64 {

using namespace devscan;

constexpr int kBins = 16;
constexpr uint32_t kMaxDepth = 64;       // top_down_builder.hpp:36
constexpr uint32_t kMaxLeaf = 16;        // top_down_builder.hpp:41
constexpr uint32_t kSmall = 256;         // subtree-per-wavefront threshold (primitives): 20 KB of staged records
// ... and the threshold of a mesh below kFewPrims primitives.  A wavefront builds its subtree node by node
// (about 60 nodes for 256 primitives: 1.0 ms, whatever the mesh), and a small mesh has too few subtrees to
// hide that behind other wavefronts; two more cheap large levels and four times as many, shorter subtrees
// are faster there.  Scheduling only: the tree does not depend on the threshold.
constexpr uint32_t kSmallFew = 64;
constexpr uint32_t kFewPrims = 65536;
inline uint32_t small_for(uint32_t n) { return n < kFewPrims ? kSmallFew : kSmall; }
constexpr int kChunk = 4096;             // most positions per binning workgroup (256 threads x 16)
constexpr int kChunkMin = 256;           // ... and fewest: one 64-record run per wavefront
// Positions per binning workgroup for n primitives: a multiple of 256, about n / 128, so that a small mesh
// still spreads over a hundred workgroups (a wavefront's runs are sequential: 16 runs of one wavefront
// cost 16 times one run, and 23 k positions in chunks of 4096 keep 6 of 256 CUs busy).  The bins do not
// depend on it: every order and grouping of the partial results gives the same words.
inline uint32_t chunk_for(uint32_t n) {
    const uint32_t c = ((n / 128u + 255u) / 256u) * 256u;
    return c < uint32_t(kChunkMin) ? uint32_t(kChunkMin) : (c > uint32_t(kChunk) ? uint32_t(kChunk) : c);
}
constexpr int kStack = 72;               // small-subtree work stack (depth <= 64 -> <= 66 entries)

// One primitive in position order: centre (the bin key), box, original index.  80 B, moved
// together with the index by the partition.
struct alignas(16) PrimRec {
    double cx, cy, cz;
    double lx, ly, lz;
    double hx, hy, hz;
    uint32_t idx, pad;
};
static_assert(sizeof(PrimRec) == 80, "PrimRec");

struct BinKeys {                         // reduced bin (large items), 80 B
    unsigned long long lo[3], hi[3];     // value words
    uint32_t tlo[3], thi[3];             // tie words (read only where the value is zero)
    uint32_t count, pad;
};

struct Item {                            // one large work item (top_down_builder.hpp:13-24)
    uint32_t node, begin, end, depth;
    double c2b[3], off[3];               // center_to_bin, bin_offset (binned_sah_builder.hpp:144-145)
    uint32_t state;                      // 0 leaf, 1 split candidate, 2 split
    uint32_t axis, split, sah_split;     // final axis, split index, best_splits[axis].second
    uint32_t T, M;                       // #true (left size), #misplaced pairs
    uint32_t next_left, next_right;      // next-level item index of each child, or ~0u (small/leaf)
    uint32_t child;                      // first child node index
    uint32_t pad;
};

struct SmallItem { uint32_t node, begin, end, depth; };

struct Counters {                        // host-visible per-level totals
    uint32_t n_items;                    // large items of the next level
    uint32_t n_small;                    // small items so far
    uint32_t n_nodes;                    // top-level nodes so far
    uint32_t pad;
};

// ---- value and tie words (see the header comment) ------------------------------------------
constexpr unsigned long long kSign = 0x8000000000000000ull;
__device__ __forceinline__ unsigned long long ord_bits(double d) {
    unsigned long long u = static_cast<unsigned long long>(__double_as_longlong(d));
    if (u == kSign) u = 0ull;
    return (u & kSign) ? ~u : (u | kSign);
}
constexpr unsigned long long kKeyMinEmpty = 0x7fefffffffffffffull | kSign;     // ord_bits(DBL_MAX)
constexpr unsigned long long kKeyMaxEmpty = ~0xffefffffffffffffull;            // ord_bits(-DBL_MAX)
constexpr uint32_t kTieEmpty = 0xffffffffu;
// a bound that may be a NaN contributes the empty key (it never wins the sequential fold)
__device__ __forceinline__ unsigned long long key_min_bound(double d) { return d == d ? ord_bits(d) : kKeyMinEmpty; }
__device__ __forceinline__ unsigned long long key_max_bound(double d) { return d == d ? ord_bits(d) : kKeyMaxEmpty; }
__device__ __forceinline__ uint32_t tie_word(double d, uint32_t pos) {            // d == 0.0
    return (pos << 1) | uint32_t(static_cast<unsigned long long>(__double_as_longlong(d)) >> 63);
}
__device__ __forceinline__ double key_value(unsigned long long k, uint32_t tie) {
    unsigned long long u = (k & kSign) ? (k & ~kSign) : ~k;
    if (u == 0ull && (tie & 1u)) u = kSign;                        // a -0 that was the first zero
    return __longlong_as_double(static_cast<long long>(u));
}

// std::min(a, b) / std::max(a, b) exactly (keep the current value on ties)
__device__ __forceinline__ double lesser(double a, double b) { return (b < a) ? b : a; }
__device__ __forceinline__ double greater(double a, double b) { return (a < b) ? b : a; }

// compute_bin_index, binned_sah_builder.hpp:146-149: min(15, size_t(max(0, fma(c, c2b, off)))),
// with x86-64's double -> size_t conversion (no AVX-512: values >= 2^64, infinity included,
// convert to 0); a NaN fails `0 < f` and gives 0.
__device__ __forceinline__ uint32_t bin_of(double c, double c2b, double off) {
    double f = fma(c, c2b, off);
    f = (0.0 < f) ? f : 0.0;
    if (f >= 18446744073709551616.0) return 0u;
    if (f >= 15.0) return kBins - 1;
    return uint32_t(f);
}

// half_area (bounding_box.hpp:43-46) and its contractions in the reference CMake build (G = true):
// the FIRST product in find_split's sweeps, the SECOND in the node's max_split_cost, and the sweep
// cost as fma(count, half_area, right_cost) (oracle/contraction_sites.txt)
template <bool G> __device__ __forceinline__ double half_area_sweep(const double lo[3], const double hi[3]) {
    const double d0 = hi[0] - lo[0], d1 = hi[1] - lo[1], d2 = hi[2] - lo[2];
    return G ? fma(d0 + d1, d2, d0 * d1) : (d0 + d1) * d2 + d0 * d1;
}
template <bool G> __device__ __forceinline__ double half_area_node(const double lo[3], const double hi[3]) {
    const double d0 = hi[0] - lo[0], d1 = hi[1] - lo[1], d2 = hi[2] - lo[2];
    return G ? fma(d0, d1, (d0 + d1) * d2) : (d0 + d1) * d2 + d0 * d1;
}
template <bool G> __device__ __forceinline__ double sweep_cost(double ha, uint32_t cnt, double right) {
    return G ? fma(double(cnt), ha, right) : ha * double(cnt) + right;
}

struct BinD { double lo[3], hi[3]; uint32_t count; uint32_t pad; };

// The split decision of BinnedSahBuildTask::build for one node (binned_sah_builder.hpp:86-114,
// 166-196): SAH sweeps per axis, axis choice, leaf test, 0.4-quantile fallback.  `nb` is the
// node box in RefNode order.  Returns false for "make a leaf now".
template <bool G>
__device__ bool sah_decide(const BinD* bins, uint32_t m, const double nb[6], uint32_t& axis_out,
                           uint32_t& split_out, uint32_t& sah_split_out) {
    double best_cost[3];
    uint32_t best_split[3];
    for (int a = 0; a < 3; ++a) {
        const BinD* row = bins + a * kBins;
        double right[kBins];
        double lo[3] = {DBL_MAX, DBL_MAX, DBL_MAX}, hi[3] = {-DBL_MAX, -DBL_MAX, -DBL_MAX};
        uint32_t cnt = 0;
        for (int i = kBins - 1; i > 0; --i) {
            for (int k = 0; k < 3; ++k) { lo[k] = lesser(lo[k], row[i].lo[k]); hi[k] = greater(hi[k], row[i].hi[k]); }
            cnt += row[i].count;
            right[i] = half_area_sweep<G>(lo, hi) * double(cnt);
        }
        for (int k = 0; k < 3; ++k) { lo[k] = DBL_MAX; hi[k] = -DBL_MAX; }
        cnt = 0;
        best_cost[a] = DBL_MAX;
        best_split[a] = kBins;
        for (int i = 0; i < kBins - 1; ++i) {
            for (int k = 0; k < 3; ++k) { lo[k] = lesser(lo[k], row[i].lo[k]); hi[k] = greater(hi[k], row[i].hi[k]); }
            cnt += row[i].count;
            const double cost = sweep_cost<G>(half_area_sweep<G>(lo, hi), cnt, right[i + 1]);
            if (cost < best_cost[a]) { best_cost[a] = cost; best_split[a] = uint32_t(i + 1); }
        }
    }
    uint32_t axis = 0;
    if (best_cost[0] > best_cost[1]) axis = 1;
    if (best_cost[axis] > best_cost[2]) axis = 2;
    uint32_t split = best_split[axis];
    const double nlo[3] = {nb[0], nb[2], nb[4]}, nhi[3] = {nb[1], nb[3], nb[5]};
    const double leaf_cost = half_area_node<G>(nlo, nhi) * (double(m) - 1.0);     // traversal_cost = 1
    if (best_split[axis] == kBins || best_cost[axis] >= leaf_cost) {
        if (m <= kMaxLeaf) return false;
        const double d[3] = {nhi[0] - nlo[0], nhi[1] - nlo[1], nhi[2] - nlo[2]};  // largest_axis
        axis = 0;
        if (d[0] < d[1]) axis = 1;
        if (d[axis] < d[2]) axis = 2;
        uint32_t cnt = 0;
        for (int i = 0; i < kBins - 1; ++i) {
            cnt += bins[axis * kBins + i].count;
            if (cnt >= (m * 2u / 5u + 1u)) { split = uint32_t(i + 1); break; }
        }
    }
    axis_out = axis;
    split_out = split;
    sah_split_out = best_split[axis];
    return true;
}

// Child boxes (binned_sah_builder.hpp:216-224), including the reference's use of
// best_splits[axis].second (not the fallback split) as the end of the LEFT range.
__device__ void child_boxes(const BinD* bins, uint32_t axis, uint32_t split, uint32_t sah_split, double lb[6], double rb[6]) {
    double llo[3] = {DBL_MAX, DBL_MAX, DBL_MAX}, lhi[3] = {-DBL_MAX, -DBL_MAX, -DBL_MAX};
    double rlo[3] = {DBL_MAX, DBL_MAX, DBL_MAX}, rhi[3] = {-DBL_MAX, -DBL_MAX, -DBL_MAX};
    const BinD* row = bins + axis * kBins;
    for (uint32_t i = 0; i < sah_split && i < uint32_t(kBins); ++i)
        for (int k = 0; k < 3; ++k) { llo[k] = lesser(llo[k], row[i].lo[k]); lhi[k] = greater(lhi[k], row[i].hi[k]); }
    for (uint32_t i = split; i < uint32_t(kBins); ++i)
        for (int k = 0; k < 3; ++k) { rlo[k] = lesser(rlo[k], row[i].lo[k]); rhi[k] = greater(rhi[k], row[i].hi[k]); }
    for (int k = 0; k < 3; ++k) { lb[2 * k] = llo[k]; lb[2 * k + 1] = lhi[k]; rb[2 * k] = rlo[k]; rb[2 * k + 1] = rhi[k]; }
}

__device__ __forceinline__ double comp3(double x, double y, double z, uint32_t a) { return a == 0 ? x : (a == 1 ? y : z); }
__device__ __forceinline__ uint32_t sel3(uint32_t x, uint32_t y, uint32_t z, uint32_t a) { return a == 0 ? x : (a == 1 ? y : z); }

// ---- init: per-primitive box + centre (triangle.hpp:39-48), root box ---------------------
// Box: p0 extended by p1() = p0 - e1 then p2() = p0 + e2; centre (p0 + p1 + p2) * (1/3).
constexpr int kInitPer = 8;              // primitives per thread in k_init
__global__ void __launch_bounds__(256) k_init(const Tri96* __restrict__ tris, uint32_t n, PrimRec* __restrict__ rec,
                                              int32_t* __restrict__ seg, int32_t seg0,
                                              unsigned long long* __restrict__ root_keys, uint32_t* __restrict__ root_ties) {
    __shared__ unsigned long long red[6][256];
    __shared__ uint32_t tred[6][256];
    unsigned long long k[6] = {kKeyMinEmpty, kKeyMinEmpty, kKeyMinEmpty, kKeyMaxEmpty, kKeyMaxEmpty, kKeyMaxEmpty};
    uint32_t t[6] = {kTieEmpty, kTieEmpty, kTieEmpty, kTieEmpty, kTieEmpty, kTieEmpty};
    for (int r = 0; r < kInitPer; ++r) {
        const uint32_t i = (blockIdx.x * kInitPer + uint32_t(r)) * 256u + threadIdx.x;
        if (i >= n) break;
        const Tri96 tr = tris[i];
        double lo[3], hi[3], c[3];
        for (int a = 0; a < 3; ++a) {
            const double p0 = tr.p0[a];
            const double p1 = p0 - tr.e1[a];
            const double p2 = p0 + tr.e2[a];
            lo[a] = lesser(lesser(p0, p1), p2);
            hi[a] = greater(greater(p0, p1), p2);
            c[a] = (p0 + p1 + p2) * (1.0 / 3.0);
        }
        PrimRec pr;
        pr.cx = c[0]; pr.cy = c[1]; pr.cz = c[2];
        pr.lx = lo[0]; pr.ly = lo[1]; pr.lz = lo[2];
        pr.hx = hi[0]; pr.hy = hi[1]; pr.hz = hi[2];
        pr.idx = i; pr.pad = 0;
        rec[i] = pr;
        seg[i] = seg0;
        for (int a = 0; a < 3; ++a) {
            k[a] = min(k[a], key_min_bound(lo[a]));
            k[3 + a] = max(k[3 + a], key_max_bound(hi[a]));
            if (lo[a] == 0.0) t[a] = min(t[a], tie_word(lo[a], i));
            if (hi[a] == 0.0) t[3 + a] = min(t[3 + a], tie_word(hi[a], i));
        }
    }
    for (int v = 0; v < 6; ++v) { red[v][threadIdx.x] = k[v]; tred[v][threadIdx.x] = t[v]; }
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < unsigned(s))
            for (int v = 0; v < 6; ++v) {
                const unsigned long long o = red[v][threadIdx.x + s];
                red[v][threadIdx.x] = v < 3 ? min(red[v][threadIdx.x], o) : max(red[v][threadIdx.x], o);
                tred[v][threadIdx.x] = min(tred[v][threadIdx.x], tred[v][threadIdx.x + s]);
            }
        __syncthreads();
    }
    if (threadIdx.x < 3) atomicMin(&root_keys[threadIdx.x], red[threadIdx.x][0]);
    else if (threadIdx.x < 6) atomicMax(&root_keys[threadIdx.x], red[threadIdx.x][0]);
    if (threadIdx.x < 6 && tred[threadIdx.x][0] != kTieEmpty) atomicMin(&root_ties[threadIdx.x], tred[threadIdx.x][0]);
}

__global__ void k_root(RefNode64* nodes, const unsigned long long* root_keys, const uint32_t* root_ties, uint32_t n, Item* items,
                       SmallItem* small, Counters* ctr, uint32_t thr) {
    if (threadIdx.x != 0) return;
    RefNode64 r;
    for (int a = 0; a < 3; ++a) {
        r.bounds[2 * a] = key_value(root_keys[a], root_ties[a]);
        r.bounds[2 * a + 1] = key_value(root_keys[3 + a], root_ties[3 + a]);
    }
    r.primitive_count = 0; r.first_child_or_primitive = 0;
    nodes[0] = r;
    if (n > thr) {
        Item it{};
        it.node = 0; it.begin = 0; it.end = n; it.depth = 0;
        items[0] = it;
        ctr->n_items = 1; ctr->n_small = 0;
    } else {
        small[0] = SmallItem{0, 0, n, 0};
        ctr->n_items = 0; ctr->n_small = 1;
    }
    ctr->n_nodes = 1;
}

// ---- large items: one level ------------------------------------------------------------
// per item: bin parameters from the node box, bins cleared
__global__ void k_item_prep(Item* items, uint32_t n_items, const RefNode64* nodes, BinKeys* bins) {
    const uint32_t s = blockIdx.x;
    if (s >= n_items) return;
    if (threadIdx.x < 3u * kBins) {
        BinKeys& b = bins[size_t(s) * 3 * kBins + threadIdx.x];
        for (int k = 0; k < 3; ++k) { b.lo[k] = kKeyMinEmpty; b.hi[k] = kKeyMaxEmpty; b.tlo[k] = kTieEmpty; b.thi[k] = kTieEmpty; }
        b.count = 0; b.pad = 0;
    }
    if (threadIdx.x == 0) {
        Item& it = items[s];
        const RefNode64& nd = nodes[it.node];
        for (int a = 0; a < 3; ++a) {
            const double lo = nd.bounds[2 * a], hi = nd.bounds[2 * a + 1];
            const double c2b = (1.0 / (hi - lo)) * double(kBins);          // diagonal().inverse() * bin_count
            it.c2b[a] = c2b;
            it.off[a] = (-lo) * c2b;                                       // -bbox.min * center_to_bin
        }
        it.state = 0;
    }
}

// Fill the bins of every large item (binned_sah_builder.hpp:157-164).  Lane (axis, bin) of each
// wavefront walks the wavefront's positions in order and keeps its bin's running box exactly like
// the reference's sequential loop (ties keep the earlier value; a NaN bound fails `<` and is
// dropped), remembering which position supplied each bound; the partial bin is flushed as value
// and tie words when the item changes (LDS for the workgroup's first item, else L2).  Reads are
// LDS broadcasts of staged 64-record runs.
__global__ void __launch_bounds__(256) k_bin(const PrimRec* __restrict__ rec, const int32_t* __restrict__ seg, uint32_t n,
                                             const Item* __restrict__ items, BinKeys* __restrict__ bins, uint32_t chunk) {
    __shared__ unsigned long long slo[3 * kBins][3], shi[3 * kBins][3];
    __shared__ uint32_t stlo[3 * kBins][3], sthi[3 * kBins][3];
    __shared__ uint32_t scount[3 * kBins];
    __shared__ PrimRec stage[4][64];
    __shared__ int32_t sseg[4][64];
    __shared__ int32_t s0_sh;
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t blk = blockIdx.x * chunk;
    const uint32_t base = blk + wave * (chunk / 4u);
    const uint32_t my_axis = lane >> 4, my_bin = lane & 15u;
    const bool binlane = lane < 3u * kBins;
    if (threadIdx.x < 3u * kBins) {
        for (int k = 0; k < 3; ++k) {
            slo[threadIdx.x][k] = kKeyMinEmpty; shi[threadIdx.x][k] = kKeyMaxEmpty;
            stlo[threadIdx.x][k] = kTieEmpty; sthi[threadIdx.x][k] = kTieEmpty;
        }
        scount[threadIdx.x] = 0;
    }
    if (threadIdx.x == 0) s0_sh = blk < n ? seg[blk] : -1;
    __syncthreads();
    const int32_t s0 = s0_sh;
    int32_t cur = -1;
    double mc2b = 0.0, moff = 0.0;
    double lo[3], hi[3];
    uint32_t plo[3], phi[3], cnt = 0;
    auto reset = [&]() {
        for (int k = 0; k < 3; ++k) { lo[k] = DBL_MAX; hi[k] = -DBL_MAX; plo[k] = 0x7fffffffu; phi[k] = 0x7fffffffu; }
        cnt = 0;
    };
    auto flush = [&]() {
        if (cur < 0 || !binlane || cnt == 0) return;
        const uint32_t idx = lane;
        if (cur == s0) {
            atomicAdd(&scount[idx], cnt);
            for (int k = 0; k < 3; ++k) {
                atomicMin(&slo[idx][k], ord_bits(lo[k]));
                atomicMax(&shi[idx][k], ord_bits(hi[k]));
                if (lo[k] == 0.0) atomicMin(&stlo[idx][k], tie_word(lo[k], plo[k]));
                if (hi[k] == 0.0) atomicMin(&sthi[idx][k], tie_word(hi[k], phi[k]));
            }
        } else {
            BinKeys& g = bins[size_t(cur) * 3 * kBins + idx];
            atomicAdd(&g.count, cnt);
            for (int k = 0; k < 3; ++k) {
                atomicMin(&g.lo[k], ord_bits(lo[k]));
                atomicMax(&g.hi[k], ord_bits(hi[k]));
                if (lo[k] == 0.0) atomicMin(&g.tlo[k], tie_word(lo[k], plo[k]));
                if (hi[k] == 0.0) atomicMin(&g.thi[k], tie_word(hi[k], phi[k]));
            }
        }
    };
    auto take = [&](const PrimRec& pr, uint32_t p) {
        ++cnt;
        const double vl[3] = {pr.lx, pr.ly, pr.lz}, vh[3] = {pr.hx, pr.hy, pr.hz};
        for (int k = 0; k < 3; ++k) {
            if (vl[k] < lo[k]) { lo[k] = vl[k]; plo[k] = p; }
            if (hi[k] < vh[k]) { hi[k] = vh[k]; phi[k] = p; }
        }
    };
    auto enter = [&](int32_t s) {
        flush();
        reset();
        cur = s;
        if (s >= 0) {
            const Item& it = items[s];
            mc2b = comp3(it.c2b[0], it.c2b[1], it.c2b[2], my_axis);
            moff = comp3(it.off[0], it.off[1], it.off[2], my_axis);
        }
    };
    reset();
    for (uint32_t r = 0; r < chunk / 4u / 64u; ++r) {
        const uint32_t p0 = base + r * 64u;
        if (p0 + lane < n) { stage[wave][lane] = rec[p0 + lane]; sseg[wave][lane] = seg[p0 + lane]; }
        else sseg[wave][lane] = -1;
        __syncthreads();
        const int32_t s_run = sseg[wave][0];
        if (__ballot(sseg[wave][lane] == s_run) == ~0ull) {            // one item (or none) in this run
            if (s_run != cur) enter(s_run);
            if (s_run >= 0 && binlane) {
#pragma unroll 4
                for (uint32_t j = 0; j < 64; ++j) {
                    const PrimRec& pr = stage[wave][j];
                    if (bin_of(comp3(pr.cx, pr.cy, pr.cz, my_axis), mc2b, moff) == my_bin) take(pr, p0 + j);
                }
            }
            __syncthreads();
            continue;
        }
        for (uint32_t j = 0; j < 64; ++j) {
            const int32_t sj = sseg[wave][j];
            if (sj != cur) enter(sj);
            if (sj < 0) continue;
            const PrimRec& pr = stage[wave][j];
            if (binlane && bin_of(comp3(pr.cx, pr.cy, pr.cz, my_axis), mc2b, moff) == my_bin) take(pr, p0 + j);
        }
        __syncthreads();
    }
    flush();
    __syncthreads();
    if (s0 >= 0 && threadIdx.x < 3u * kBins && scount[threadIdx.x]) {
        BinKeys& g = bins[size_t(s0) * 3 * kBins + threadIdx.x];
        atomicAdd(&g.count, scount[threadIdx.x]);
        for (int k = 0; k < 3; ++k) {
            atomicMin(&g.lo[k], slo[threadIdx.x][k]);
            atomicMax(&g.hi[k], shi[threadIdx.x][k]);
            if (stlo[threadIdx.x][k] != kTieEmpty) atomicMin(&g.tlo[k], stlo[threadIdx.x][k]);
            if (sthi[threadIdx.x][k] != kTieEmpty) atomicMin(&g.thi[k], sthi[threadIdx.x][k]);
        }
    }
}

// One wavefront per item: lane (axis, bin) decodes its bin into LDS (48 independent loads instead of one
// thread's chain of them); the decision itself stays the sequential code, on lane 0.
__device__ __forceinline__ void decode_bins(const BinKeys* g, BinD* out) {
    const uint32_t b = threadIdx.x;
    if (b < 3u * kBins) {
        for (int k = 0; k < 3; ++k) { out[b].lo[k] = key_value(g[b].lo[k], g[b].tlo[k]); out[b].hi[k] = key_value(g[b].hi[k], g[b].thi[k]); }
        out[b].count = g[b].count;
        out[b].pad = 0;
    }
    __syncthreads();
}

// Split decision per large item (one wavefront each, see decode_bins); leaves are final here.
template <bool G>
__global__ void __launch_bounds__(64) k_split(Item* items, uint32_t n_items, RefNode64* nodes, const BinKeys* bins) {
    __shared__ BinD b[3 * kBins];
    const uint32_t s = blockIdx.x;
    if (s >= n_items) return;
    Item& it = items[s];
    const uint32_t m = it.end - it.begin;
    RefNode64& nd = nodes[it.node];
    if (m <= 1 || it.depth >= kMaxDepth) {                  // (uniform over the wavefront)
        if (threadIdx.x == 0) {
            nd.primitive_count = m; nd.first_child_or_primitive = it.begin;
            it.state = 0;
        }
        return;
    }
    decode_bins(bins + size_t(s) * 3 * kBins, b);
    if (threadIdx.x != 0) return;
    double nb[6];
    for (int k = 0; k < 6; ++k) nb[k] = nd.bounds[k];
    uint32_t axis, split, sah;
    if (!sah_decide<G>(b, m, nb, axis, split, sah)) {
        nd.primitive_count = m; nd.first_child_or_primitive = it.begin;
        it.state = 0;
        return;
    }
    it.axis = axis; it.split = split; it.sah_split = sah;
    it.state = 1;
}

// partition predicate per position of split candidates (binned_sah_builder.hpp:199-201)
__global__ void __launch_bounds__(256) k_flags(const PrimRec* __restrict__ rec, const int32_t* __restrict__ seg, uint32_t n,
                                               const Item* __restrict__ items, uint32_t* __restrict__ flag) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= n) return;
    uint32_t f = 0;
    const int32_t s = seg[p];
    if (s >= 0) {
        const Item& it = items[s];
        if (it.state == 1) {
            const PrimRec& pr = rec[p];
            const double c = comp3(pr.cx, pr.cy, pr.cz, it.axis);
            f = bin_of(c, comp3(it.c2b[0], it.c2b[1], it.c2b[2], it.axis), comp3(it.off[0], it.off[1], it.off[2], it.axis)) < it.split ? 1u : 0u;
        }
    }
    flag[p] = f;
}

// ---- per-level plan (one workgroup): finalize splits, allocate child nodes and items ------
__global__ void __launch_bounds__(256) k_plan(Item* items, uint32_t n_items, const uint32_t* __restrict__ X, RefNode64* nodes,
                                              Counters* ctr, SmallItem* small, uint32_t thr) {
    __shared__ uint32_t sh[264];
    __shared__ uint32_t carry_nodes, carry_large, carry_small;
    if (threadIdx.x == 0) { carry_nodes = ctr->n_nodes; carry_large = 0; carry_small = ctr->n_small; }
    __syncthreads();
    for (uint32_t base = 0; base < n_items; base += 256) {
        const uint32_t s = base + threadIdx.x;
        uint32_t split = 0, nlarge = 0, nsmall = 0;
        Item it{};
        if (s < n_items) {
            it = items[s];
            if (it.state == 1) {
                const uint32_t m = it.end - it.begin;
                const uint32_t T = X[it.end] - X[it.begin];
                if (T == 0 || T == m) {                             // one side empty: leaf (:204, :230)
                    nodes[it.node].primitive_count = m;
                    nodes[it.node].first_child_or_primitive = it.begin;
                    it.state = 0;
                } else {
                    it.state = 2;
                    it.T = T;
                    it.M = T - (X[it.begin + T] - X[it.begin]);         // falses left of the split point
                    split = 1;
                    nlarge = (T > thr) + (m - T > thr);
                    nsmall = 2 - nlarge;
                }
            }
        }
        uint32_t tot;
        const uint32_t ex_split = block_exclusive_scan_256(split, sh, tot);
        const uint32_t tot_split = tot;
        const uint32_t ex_large = block_exclusive_scan_256(nlarge, sh, tot);
        const uint32_t tot_large = tot;
        const uint32_t ex_small = block_exclusive_scan_256(nsmall, sh, tot);
        const uint32_t tot_small = tot;
        if (s < n_items) {
            if (it.state == 2) {
                it.child = carry_nodes + 2 * ex_split;
                const uint32_t m = it.end - it.begin;
                uint32_t lb = carry_large + ex_large, sb = carry_small + ex_small;
                const bool left_large = it.T > thr, right_large = m - it.T > thr;
                it.next_left = left_large ? lb++ : ~0u;
                it.next_right = right_large ? lb++ : ~0u;
                if (!left_large) small[sb++] = SmallItem{it.child, it.begin, it.begin + it.T, it.depth + 1};
                if (!right_large) small[sb++] = SmallItem{it.child + 1, it.begin + it.T, it.end, it.depth + 1};
            } else {
                it.next_left = it.next_right = ~0u;
            }
            items[s] = it;
        }
        __syncthreads();
        if (threadIdx.x == 0) { carry_nodes += 2 * tot_split; carry_large += tot_large; carry_small += tot_small; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { ctr->n_nodes = carry_nodes; ctr->n_items = carry_large; ctr->n_small = carry_small; }
}

// parent link, child boxes, next-level items (one wavefront per split item, see decode_bins)
__global__ void __launch_bounds__(64) k_emit(const Item* items, uint32_t n_items, RefNode64* nodes, const BinKeys* bins,
                                             Item* next) {
    __shared__ BinD b[3 * kBins];
    const uint32_t s = blockIdx.x;
    if (s >= n_items) return;
    const Item it = items[s];
    if (it.state != 2) return;                              // (uniform over the wavefront)
    decode_bins(bins + size_t(s) * 3 * kBins, b);
    if (threadIdx.x != 0) return;
    double lb[6], rb[6];
    child_boxes(b, it.axis, it.split, it.sah_split, lb, rb);
    RefNode64& nd = nodes[it.node];
    nd.primitive_count = 0;
    nd.first_child_or_primitive = it.child;
    RefNode64 l, r;
    for (int k = 0; k < 6; ++k) { l.bounds[k] = lb[k]; r.bounds[k] = rb[k]; }
    l.primitive_count = r.primitive_count = 0;
    l.first_child_or_primitive = r.first_child_or_primitive = 0;
    nodes[it.child] = l;
    nodes[it.child + 1] = r;
    if (it.next_left != ~0u) { Item c{}; c.node = it.child; c.begin = it.begin; c.end = it.begin + it.T; c.depth = it.depth + 1; next[it.next_left] = c; }
    if (it.next_right != ~0u) { Item c{}; c.node = it.child + 1; c.begin = it.begin + it.T; c.end = it.end; c.depth = it.depth + 1; next[it.next_right] = c; }
}

// misplaced elements of each split item: the k-th "false" left of the split point and the
// k-th "true" right of it (counted from the end) are swapped by std::partition.
__global__ void __launch_bounds__(256) k_pos(const int32_t* __restrict__ seg, uint32_t n, const Item* __restrict__ items,
                                             const uint32_t* __restrict__ flag, const uint32_t* __restrict__ X,
                                             uint32_t* __restrict__ posF, uint32_t* __restrict__ posT) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= n) return;
    const int32_t s = seg[p];
    if (s < 0) return;
    const Item& it = items[s];
    if (it.state != 2) return;
    const uint32_t mid = it.begin + it.T;
    const uint32_t tr = X[p] - X[it.begin];                 // trues in [begin, p)
    if (p < mid) {
        if (!flag[p]) posF[it.begin + (p - it.begin - tr)] = p;
    } else {
        if (flag[p]) posT[it.begin + (it.T - 1 - tr)] = p;
    }
}

__global__ void __launch_bounds__(256) k_swap_seg(PrimRec* __restrict__ rec, int32_t* __restrict__ seg, uint32_t n,
                                                  const Item* __restrict__ items, const uint32_t* __restrict__ posF,
                                                  const uint32_t* __restrict__ posT) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= n) return;
    const int32_t s = seg[p];
    if (s < 0) return;
    const Item& it = items[s];
    if (it.state != 2) { seg[p] = -1; return; }
    const uint32_t k = p - it.begin;
    if (k < it.M) {
        const uint32_t a = posF[it.begin + k], b = posT[it.begin + k];
        const PrimRec ra = rec[a], rb = rec[b];
        rec[a] = rb;
        rec[b] = ra;
    }
    const uint32_t nx = p < it.begin + it.T ? it.next_left : it.next_right;
    seg[p] = nx == ~0u ? -1 : int32_t(nx);
}

// ---- small items: one wavefront builds a whole subtree ----------------------------------
// Nodes of the subtree (except its root, a top-level node) go to tnodes[2 * begin + local];
// inner nodes' first_child is local until k_place rebases them.
struct StackEntry { uint32_t begin, end, depth; int32_t local; double box[6]; };

// 16-lane segmented scans over the bins of one axis (lane = axis * 16 + bin).  The combine keeps
// the EARLIER bin on ties, as the reference's ascending extend loops do (sign of zero exact).
struct LaneBox { double lo[3], hi[3]; uint32_t cnt; };

__device__ __forceinline__ LaneBox prefix16(LaneBox v, uint32_t i) {           // bins 0..i
    for (int d = 1; d < 16; d <<= 1) {
        LaneBox u;
        for (int k = 0; k < 3; ++k) { u.lo[k] = __shfl_up(v.lo[k], d, 16); u.hi[k] = __shfl_up(v.hi[k], d, 16); }
        u.cnt = __shfl_up(v.cnt, d, 16);
        if (i >= uint32_t(d)) {
            for (int k = 0; k < 3; ++k) { v.lo[k] = lesser(u.lo[k], v.lo[k]); v.hi[k] = greater(u.hi[k], v.hi[k]); }
            v.cnt += u.cnt;
        }
    }
    return v;
}
__device__ __forceinline__ LaneBox suffix16(LaneBox v, uint32_t i) {           // bins i..15
    for (int d = 1; d < 16; d <<= 1) {
        LaneBox u;
        for (int k = 0; k < 3; ++k) { u.lo[k] = __shfl_down(v.lo[k], d, 16); u.hi[k] = __shfl_down(v.hi[k], d, 16); }
        u.cnt = __shfl_down(v.cnt, d, 16);
        if (i + uint32_t(d) < 16u) {
            for (int k = 0; k < 3; ++k) { v.lo[k] = lesser(v.lo[k], u.lo[k]); v.hi[k] = greater(v.hi[k], u.hi[k]); }
            v.cnt += u.cnt;
        }
    }
    return v;
}

// One wavefront builds the whole subtree of a small item.  Bins: value and tie words in LDS, one lane
// per primitive (a lane per (axis, bin) walking the primitives in order costs a full-wavefront step per
// primitive: 1.0 ms for a 23 k-triangle mesh's subtrees); SAH sweeps: segmented scans, 16 lanes per
// axis (the costs depend only on box values and counts, so they are bit-identical to the
// sequential sweeps of binned_sah_builder.hpp:89-114); the first minimal cost wins (strict <).
// The work stack cannot overrun: an entry whose children would not fit becomes a leaf (never
// reached: depth <= 64 keeps the stack below 66 entries).
template <bool G>
__global__ void __launch_bounds__(64) k_small(PrimRec* __restrict__ rec, const SmallItem* __restrict__ small, uint32_t n_small,
                                              RefNode64* __restrict__ nodes, RefNode64* __restrict__ tnodes,
                                              uint32_t* __restrict__ small_count, uint32_t* __restrict__ prim_out) {
    __shared__ PrimRec R[kSmall];
    __shared__ StackEntry st[kStack];
    __shared__ uint16_t posF[kSmall / 2], posT[kSmall / 2];
    __shared__ unsigned long long klo[3 * kBins][3], khi[3 * kBins][3];
    __shared__ uint32_t ktlo[3 * kBins][3], kthi[3 * kBins][3], kcnt[3 * kBins];
    const uint32_t s = blockIdx.x;
    if (s >= n_small) return;
    const uint32_t lane = threadIdx.x;
    const SmallItem si = small[s];
    const uint32_t b0 = si.begin, m0 = min(si.end - si.begin, kSmall);
    for (uint32_t k = lane; k < m0; k += 64) R[k] = rec[b0 + k];
    if (lane == 0) {
        StackEntry e;
        e.begin = 0; e.end = m0; e.depth = si.depth; e.local = -1;
        for (int k = 0; k < 6; ++k) e.box[k] = nodes[si.node].bounds[k];
        st[0] = e;
    }
    __syncthreads();
    int sp = 1;
    uint32_t nc = 0;                                         // local nodes allocated
    RefNode64* const tbase = tnodes + 2 * size_t(b0);
    const uint32_t my_axis = lane >> 4, bi = lane & 15u;     // lanes 48..63: padding group
    while (sp > 0) {
        const StackEntry e = st[--sp];
        __syncthreads();
        RefNode64* const nd = e.local < 0 ? nodes + si.node : tbase + e.local;
        const uint32_t m = e.end - e.begin;
        if (m <= 1 || e.depth >= kMaxDepth || sp + 2 > kStack) {
            if (lane == 0) { nd->primitive_count = m; nd->first_child_or_primitive = b0 + e.begin; }
            continue;
        }
        double c2b[3], off[3];
        for (int a = 0; a < 3; ++a) {
            const double lo = e.box[2 * a], hi = e.box[2 * a + 1];
            c2b[a] = (1.0 / (hi - lo)) * double(kBins);
            off[a] = (-lo) * c2b[a];
        }
        LaneBox v;
        for (int k = 0; k < 3; ++k) { v.lo[k] = DBL_MAX; v.hi[k] = -DBL_MAX; }
        v.cnt = 0;
        if (lane < 3u * kBins) {
            for (int k = 0; k < 3; ++k) { klo[lane][k] = kKeyMinEmpty; khi[lane][k] = kKeyMaxEmpty; ktlo[lane][k] = kTieEmpty; kthi[lane][k] = kTieEmpty; }
            kcnt[lane] = 0;
        }
        __syncthreads();
        for (uint32_t p = e.begin + lane; p < e.end; p += 64) {
            const PrimRec& pr = R[p];
            const double c[3] = {pr.cx, pr.cy, pr.cz}, lo[3] = {pr.lx, pr.ly, pr.lz}, hi[3] = {pr.hx, pr.hy, pr.hz};
            for (int a = 0; a < 3; ++a) {
                const uint32_t b = uint32_t(a) * kBins + bin_of(c[a], c2b[a], off[a]);
                atomicAdd(&kcnt[b], 1u);
                for (int k = 0; k < 3; ++k) {
                    atomicMin(&klo[b][k], key_min_bound(lo[k]));
                    atomicMax(&khi[b][k], key_max_bound(hi[k]));
                    if (lo[k] == 0.0) atomicMin(&ktlo[b][k], tie_word(lo[k], p));
                    if (hi[k] == 0.0) atomicMin(&kthi[b][k], tie_word(hi[k], p));
                }
            }
        }
        __syncthreads();
        if (lane < 3u * kBins) {
            for (int k = 0; k < 3; ++k) { v.lo[k] = key_value(klo[lane][k], ktlo[lane][k]); v.hi[k] = key_value(khi[lane][k], kthi[lane][k]); }
            v.cnt = kcnt[lane];
        }
        const LaneBox L = prefix16(v, bi), Rs = suffix16(v, bi);
        const double rcost = half_area_sweep<G>(Rs.lo, Rs.hi) * double(Rs.cnt);
        const double rnext = __shfl_down(rcost, 1, 16);
        const double cost = sweep_cost<G>(half_area_sweep<G>(L.lo, L.hi), L.cnt, rnext);
        // first minimal valid cost of this axis (sequential "if (cost < best)" from DBL_MAX)
        const bool valid = bi < 15u && cost < DBL_MAX;
        double bc = valid ? cost : double(INFINITY);
        uint32_t bs = valid ? bi + 1u : uint32_t(kBins);
        for (int d = 8; d > 0; d >>= 1) {
            const double oc = __shfl_xor(bc, d, 16);
            const uint32_t os = __shfl_xor(bs, d, 16);
            if (oc < bc || (oc == bc && os < bs)) { bc = oc; bs = os; }
        }
        if (bs == uint32_t(kBins)) bc = DBL_MAX;
        const double bcost[3] = {__shfl(bc, 0), __shfl(bc, 16), __shfl(bc, 32)};
        const uint32_t bsplit[3] = {uint32_t(__shfl(int(bs), 0)), uint32_t(__shfl(int(bs), 16)), uint32_t(__shfl(int(bs), 32))};
        uint32_t axis = 0;
        if (bcost[0] > bcost[1]) axis = 1;
        if (comp3(bcost[0], bcost[1], bcost[2], axis) > bcost[2]) axis = 2;
        uint32_t split = sel3(bsplit[0], bsplit[1], bsplit[2], axis);
        const double nlo[3] = {e.box[0], e.box[2], e.box[4]}, nhi[3] = {e.box[1], e.box[3], e.box[5]};
        const double leaf_cost = half_area_node<G>(nlo, nhi) * (double(m) - 1.0);
        bool make_leaf = false;
        if (split == uint32_t(kBins) || comp3(bcost[0], bcost[1], bcost[2], axis) >= leaf_cost) {
            if (m <= kMaxLeaf) {
                make_leaf = true;
            } else {
                const double d0 = nhi[0] - nlo[0], d1 = nhi[1] - nlo[1], d2 = nhi[2] - nlo[2];   // largest_axis
                axis = 0;
                if (d0 < d1) axis = 1;
                if (comp3(d0, d1, d2, axis) < d2) axis = 2;
                const unsigned long long hit = __ballot(my_axis == axis && bi < 15u && L.cnt >= (m * 2u / 5u + 1u));
                if (hit) split = uint32_t(__ffsll(hit) - 1) - axis * kBins + 1u;
            }
        }
        if (make_leaf) {
            if (lane == 0) { nd->primitive_count = m; nd->first_child_or_primitive = b0 + e.begin; }
            continue;
        }
        const uint32_t sah = sel3(bsplit[0], bsplit[1], bsplit[2], axis);
        const double ac2b = comp3(c2b[0], c2b[1], c2b[2], axis), aoff = comp3(off[0], off[1], off[2], axis);
        // partition: count, then misplaced positions, then swaps (libstdc++ std::partition)
        uint32_t T = 0;
        for (uint32_t base = e.begin; base < e.end; base += 64) {
            const uint32_t p = base + lane;
            const bool f = p < e.end && bin_of(comp3(R[p].cx, R[p].cy, R[p].cz, axis), ac2b, aoff) < split;
            T += uint32_t(__popcll(__ballot(f)));
        }
        if (T == 0 || T == m) {
            if (lane == 0) { nd->primitive_count = m; nd->first_child_or_primitive = b0 + e.begin; }
            continue;
        }
        const uint32_t mid = e.begin + T;
        uint32_t tr = 0, M = 0;
        for (uint32_t base = e.begin; base < e.end; base += 64) {
            const uint32_t p = base + lane;
            const bool f = p < e.end && bin_of(comp3(R[p].cx, R[p].cy, R[p].cz, axis), ac2b, aoff) < split;
            const unsigned long long mask = __ballot(f);
            const uint32_t trp = tr + uint32_t(__popcll(mask & ((1ull << lane) - 1ull)));   // trues in [begin, p)
            if (p < e.end) {
                if (p < mid && !f) posF[(p - e.begin) - trp] = uint16_t(p);
                else if (p >= mid && f) posT[T - 1 - trp] = uint16_t(p);
            }
            M += uint32_t(__popcll(__ballot(p < mid && p < e.end && !f)));
            tr += uint32_t(__popcll(mask));
        }
        __syncthreads();
        for (uint32_t k = lane; k < M; k += 64) {
            const uint32_t a = posF[k], b = posT[k];
            const PrimRec ra = R[a], rb = R[b];
            R[a] = rb;
            R[b] = ra;
        }
        // child boxes (binned_sah_builder.hpp:216-224): left = bins [0, sah), right = bins [split, 16)
        double lb[6], rb[6];
        const int lsrc = int(axis * kBins + sah - 1u), rsrc = int(axis * kBins + split);
        for (int k = 0; k < 3; ++k) {
            lb[2 * k] = __shfl(L.lo[k], lsrc); lb[2 * k + 1] = __shfl(L.hi[k], lsrc);
            rb[2 * k] = __shfl(Rs.lo[k], rsrc); rb[2 * k + 1] = __shfl(Rs.hi[k], rsrc);
        }
        const uint32_t child = nc;
        nc += 2;
        __syncthreads();
        if (lane == 0) {
            RefNode64 l, r;
            for (int k = 0; k < 6; ++k) { l.bounds[k] = lb[k]; r.bounds[k] = rb[k]; }
            l.primitive_count = r.primitive_count = 0;
            l.first_child_or_primitive = r.first_child_or_primitive = 0;
            tbase[child] = l;
            tbase[child + 1] = r;
            nd->primitive_count = 0;
            nd->first_child_or_primitive = child;
            StackEntry er, el;
            er.begin = mid; er.end = e.end; er.depth = e.depth + 1; er.local = int32_t(child + 1);
            el.begin = e.begin; el.end = mid; el.depth = e.depth + 1; el.local = int32_t(child);
            for (int k = 0; k < 6; ++k) { er.box[k] = rb[k]; el.box[k] = lb[k]; }
            st[sp] = er;
            st[sp + 1] = el;
        }
        sp += 2;
        __syncthreads();
    }
    for (uint32_t k = lane; k < m0; k += 64) prim_out[b0 + k] = R[k].idx;
    if (lane == 0) small_count[s] = nc;
}

// Final permutation for positions that ended in top-level leaves (k_small overwrites its ranges).
__global__ void __launch_bounds__(256) k_prim_out(const PrimRec* __restrict__ rec, uint32_t n, uint32_t* __restrict__ prim_out) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p < n) prim_out[p] = rec[p].idx;
}

// Move each subtree's nodes after the top-level nodes, rebasing local child links.
__global__ void __launch_bounds__(64) k_place(const SmallItem* __restrict__ small, uint32_t n_small, const uint32_t* __restrict__ base,
                                              const RefNode64* __restrict__ tnodes, RefNode64* __restrict__ nodes, uint32_t top_nodes) {
    const uint32_t s = blockIdx.x;
    if (s >= n_small) return;
    const SmallItem si = small[s];
    const uint32_t cnt = base[s + 1] - base[s];
    const uint32_t dst = top_nodes + base[s];
    const RefNode64* src = tnodes + 2 * size_t(si.begin);
    for (uint32_t k = threadIdx.x; k < cnt; k += 64) {
        RefNode64 r = src[k];
        if (r.primitive_count == 0) r.first_child_or_primitive += dst;
        nodes[dst + k] = r;
    }
    if (threadIdx.x == 0 && cnt) nodes[si.node].first_child_or_primitive = dst;
}

}  // namespace bvhdev64
}  // namespace ceres

// --------------------------------------------------------------------------- host side
using namespace ceres;
using namespace ceres::bvhdev64;

namespace {

size_t align_up64(size_t x) { return (x + 255) & ~size_t(255); }
bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

extern "C" {

// Device build: d_tri96 = n_tri bvh::Triangle<double> in device memory; d_nodes64 must hold
// 2 * n_tri - 1 RefNode64s, d_prim32 n_tri u32.  Stream-ordered; returns after the build
// (the node count is read back).  Workspace comes from hipMallocAsync on `stream`.
int ceres_bvh_build_f64_device_arith(const double* d_tri96, size_t n_tri, uint64_t* d_nodes64, uint32_t* d_prim32,
                                     size_t* n_nodes, void* stream_, int arith) {
    if (!d_tri96 || !d_nodes64 || !d_prim32 || !n_nodes) return set_error(CERES_EINVAL, "ceres_bvh_build_f64_device: null argument");
    if (arith != CERES_ARITH_EXACT && arith != CERES_ARITH_FMA) return set_error(CERES_EINVAL, "unknown arithmetic %d", arith);
    const bool gfma = arith == CERES_ARITH_FMA;
    if (n_tri == 0) return set_error(CERES_EINVAL, "The given scene is empty or cannot be loaded");
    if (n_tri > 0x7fffffffu) return set_error(CERES_EUNSUPPORTED, "more than 2^31 triangles");
    if (!aligned16(d_tri96) || !aligned16(d_nodes64) || !aligned16(d_prim32))
        return set_error(CERES_EINVAL, "ceres_bvh_build_f64_device: device pointers must be 16-byte aligned");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const uint32_t n = uint32_t(n_tri);
    RefNode64* nodes = reinterpret_cast<RefNode64*>(d_nodes64);
    const uint32_t thr = small_for(n);
    const uint32_t cap_items = n / (thr + 1) + 2;
    const uint32_t cap_small = uint32_t(std::min<size_t>(n, size_t(128) * n / thr + 4));
    const uint32_t scan_blocks = (n + kScanBlock - 1) / kScanBlock;
    const uint32_t chunk = chunk_for(n);
    const uint32_t chunks = (n + chunk - 1) / chunk;
    // workspace layout
    size_t off = 0;
    auto carve = [&](size_t bytes) { size_t o = off; off = align_up64(off + bytes); return o; };
    const size_t o_rec = carve(size_t(n) * sizeof(PrimRec));
    const size_t o_seg = carve(size_t(n) * 4);
    const size_t o_flag = carve(size_t(n) * 4);
    const size_t o_X = carve(size_t(n + 1) * 4);
    const size_t o_part = carve(size_t(std::max(scan_blocks, cap_small) + 1) * 4);
    const size_t o_posF = carve(size_t(n) * 4);
    const size_t o_posT = carve(size_t(n) * 4);
    const size_t o_items0 = carve(size_t(cap_items) * sizeof(Item));
    const size_t o_items1 = carve(size_t(cap_items) * sizeof(Item));
    const size_t o_bins = carve(size_t(cap_items) * 3 * kBins * sizeof(BinKeys));
    const size_t o_small = carve(size_t(cap_small) * sizeof(SmallItem));
    const size_t o_scount = carve(size_t(cap_small + 1) * 4);
    const size_t o_tnodes = carve(size_t(2) * n * sizeof(RefNode64));
    const size_t o_keys = carve(6 * 8 + 6 * 4);
    const size_t o_ctr = carve(sizeof(Counters));
    char* ws = nullptr;
    int rc = CERES_OK;
    Counters h{};
    uint32_t n_items = 0, levels = 0;
    int cur = 0;
    HIP_TRY_DONE(hipMallocAsync(reinterpret_cast<void**>(&ws), off, stream));
    {
        PrimRec* rec = reinterpret_cast<PrimRec*>(ws + o_rec);
        int32_t* seg = reinterpret_cast<int32_t*>(ws + o_seg);
        uint32_t* flag = reinterpret_cast<uint32_t*>(ws + o_flag);
        uint32_t* X = reinterpret_cast<uint32_t*>(ws + o_X);
        uint32_t* part = reinterpret_cast<uint32_t*>(ws + o_part);
        uint32_t* posF = reinterpret_cast<uint32_t*>(ws + o_posF);
        uint32_t* posT = reinterpret_cast<uint32_t*>(ws + o_posT);
        Item* items[2] = {reinterpret_cast<Item*>(ws + o_items0), reinterpret_cast<Item*>(ws + o_items1)};
        BinKeys* bins = reinterpret_cast<BinKeys*>(ws + o_bins);
        SmallItem* small = reinterpret_cast<SmallItem*>(ws + o_small);
        uint32_t* scount = reinterpret_cast<uint32_t*>(ws + o_scount);
        RefNode64* tnodes = reinterpret_cast<RefNode64*>(ws + o_tnodes);
        unsigned long long* keys = reinterpret_cast<unsigned long long*>(ws + o_keys);
        uint32_t* ties = reinterpret_cast<uint32_t*>(ws + o_keys + 6 * 8);
        Counters* ctr = reinterpret_cast<Counters*>(ws + o_ctr);
        struct { unsigned long long k[6]; uint32_t t[6]; } key_init = {
            {kKeyMinEmpty, kKeyMinEmpty, kKeyMinEmpty, kKeyMaxEmpty, kKeyMaxEmpty, kKeyMaxEmpty},
            {kTieEmpty, kTieEmpty, kTieEmpty, kTieEmpty, kTieEmpty, kTieEmpty}};
        static_assert(sizeof key_init == 6 * 8 + 6 * 4, "key_init");
        HIP_TRY_DONE(hipMemcpyAsync(keys, &key_init, sizeof key_init, hipMemcpyHostToDevice, stream));
        const uint32_t g256 = (n + 255) / 256;
        hipLaunchKernelGGL(k_init, dim3((n + 256 * kInitPer - 1) / (256 * kInitPer)), dim3(256), 0, stream,
                           reinterpret_cast<const Tri96*>(d_tri96), n, rec, seg, n > thr ? 0 : -1, keys, ties);
        HIP_TRY_DONE(hipGetLastError());
        hipLaunchKernelGGL(k_root, dim3(1), dim3(64), 0, stream, nodes, keys, ties, n, items[0], small, ctr, thr);
        HIP_TRY_DONE(hipGetLastError());
        n_items = n > thr ? 1 : 0;
        h.n_small = n > thr ? 0 : 1;
        h.n_nodes = 1;
        while (n_items) {
            if (n_items > cap_items) { rc = set_error(CERES_EINVAL, "bvh build: item capacity exceeded"); goto done; }
            if (++levels > kMaxDepth + 1) { rc = set_error(CERES_EINVAL, "bvh build: more than 64 levels"); goto done; }
            Item* it = items[cur];
            hipLaunchKernelGGL(k_item_prep, dim3(n_items), dim3(64), 0, stream, it, n_items, nodes, bins);
            hipLaunchKernelGGL(k_bin, dim3(chunks), dim3(256), 0, stream, rec, seg, n, it, bins, chunk);
            if (gfma) hipLaunchKernelGGL(k_split<true>, dim3(n_items), dim3(64), 0, stream, it, n_items, nodes, bins);
            else hipLaunchKernelGGL(k_split<false>, dim3(n_items), dim3(64), 0, stream, it, n_items, nodes, bins);
            hipLaunchKernelGGL(k_flags, dim3(g256), dim3(256), 0, stream, rec, seg, n, it, flag);
            hipLaunchKernelGGL(k_scan_reduce, dim3(scan_blocks), dim3(256), 0, stream, flag, n, part);
            hipLaunchKernelGGL(k_scan_partials, dim3(1), dim3(256), 0, stream, part, scan_blocks);
            hipLaunchKernelGGL(k_scan_down, dim3(scan_blocks), dim3(256), 0, stream, flag, n, part, X);
            hipLaunchKernelGGL(k_plan, dim3(1), dim3(256), 0, stream, it, n_items, X, nodes, ctr, small, thr);
            hipLaunchKernelGGL(k_emit, dim3(n_items), dim3(64), 0, stream, it, n_items, nodes, bins, items[cur ^ 1]);
            hipLaunchKernelGGL(k_pos, dim3(g256), dim3(256), 0, stream, seg, n, it, flag, X, posF, posT);
            hipLaunchKernelGGL(k_swap_seg, dim3(g256), dim3(256), 0, stream, rec, seg, n, it, posF, posT);
            HIP_TRY_DONE(hipGetLastError());
            HIP_TRY_DONE(hipMemcpyAsync(&h, ctr, sizeof h, hipMemcpyDeviceToHost, stream));
            HIP_TRY_DONE(hipStreamSynchronize(stream));
            n_items = h.n_items;
            cur ^= 1;
            if (h.n_small > cap_small) { rc = set_error(CERES_EINVAL, "bvh build: small-item capacity exceeded"); goto done; }
        }
        const uint32_t n_small = h.n_small;
        hipLaunchKernelGGL(k_prim_out, dim3(g256), dim3(256), 0, stream, rec, n, d_prim32);
        uint32_t sub_total = 0;
        if (n_small) {                                   // all-large-leaf builds have no subtrees
            if (gfma) hipLaunchKernelGGL(k_small<true>, dim3(n_small), dim3(64), 0, stream, rec, small, n_small, nodes, tnodes, scount, d_prim32);
            else hipLaunchKernelGGL(k_small<false>, dim3(n_small), dim3(64), 0, stream, rec, small, n_small, nodes, tnodes, scount, d_prim32);
            HIP_TRY_DONE(hipGetLastError());
            // exclusive scan of the subtree node counts (n_small + 1 entries)
            HIP_TRY_DONE(hipMemcpyAsync(part, scount, size_t(n_small) * 4, hipMemcpyDeviceToDevice, stream));
            hipLaunchKernelGGL(k_scan_partials, dim3(1), dim3(256), 0, stream, part, n_small);
            hipLaunchKernelGGL(k_place, dim3(n_small), dim3(64), 0, stream, small, n_small, part, tnodes, nodes, h.n_nodes);
            HIP_TRY_DONE(hipGetLastError());
            HIP_TRY_DONE(hipMemcpyAsync(&sub_total, part + n_small, 4, hipMemcpyDeviceToHost, stream));
        }
        HIP_TRY_DONE(hipStreamSynchronize(stream));
        *n_nodes = size_t(h.n_nodes) + sub_total;
    }
done:
    if (ws) (void)hipFreeAsync(ws, stream);
    return rc;
}

int ceres_bvh_build_f64_device(const double* d_tri96, size_t n_tri, uint64_t* d_nodes64, uint32_t* d_prim32,
                               size_t* n_nodes, void* stream_) {
    return ceres_bvh_build_f64_device_arith(d_tri96, n_tri, d_nodes64, d_prim32, n_nodes, stream_, CERES_ARITH_EXACT);
}

// Host-buffer convenience with ceres_bvh_build_f64's signature and output: the same BVH as the
// host builder (canonical topology + leaf order), built on `device`.
int ceres_bvh_build_f64_gpu_arith(const double* tri96, size_t n_tri, uint64_t** nodes64, size_t* n_nodes, uint64_t** prim64,
                                  int device, int arith) {
    if (!tri96 || !nodes64 || !n_nodes || !prim64) return set_error(CERES_EINVAL, "ceres_bvh_build_f64_gpu: null argument");
    if (arith != CERES_ARITH_EXACT && arith != CERES_ARITH_FMA) return set_error(CERES_EINVAL, "unknown arithmetic %d", arith);
    if (n_tri == 0) return set_error(CERES_EINVAL, "The given scene is empty or cannot be loaded");
    if (n_tri > 0x7fffffffu) return set_error(CERES_EUNSUPPORTED, "more than 2^31 triangles");
    *nodes64 = nullptr; *prim64 = nullptr; *n_nodes = 0;
    int rc = CERES_OK;
    double* d_tri = nullptr;
    uint64_t* d_nodes = nullptr;
    uint32_t* d_prim = nullptr;
    hipStream_t stream = nullptr;
    uint32_t* hp = nullptr;
    size_t m = 0;
    const size_t cap_nodes = 2 * n_tri - 1;
    HIP_TRY_DONE(hipSetDevice(device));
    HIP_TRY_DONE(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    HIP_TRY_DONE(hipMalloc(&d_tri, n_tri * sizeof(Tri96)));
    HIP_TRY_DONE(hipMalloc(&d_nodes, cap_nodes * sizeof(RefNode64)));
    HIP_TRY_DONE(hipMalloc(&d_prim, n_tri * 4));
    HIP_TRY_DONE(hipMemcpyAsync(d_tri, tri96, n_tri * sizeof(Tri96), hipMemcpyHostToDevice, stream));
    if ((rc = ceres_bvh_build_f64_device_arith(d_tri, n_tri, d_nodes, d_prim, &m, stream, arith)) != CERES_OK) goto done;
    *nodes64 = static_cast<uint64_t*>(std::malloc(m * sizeof(RefNode64)));
    *prim64 = static_cast<uint64_t*>(std::malloc(n_tri * 8));
    hp = static_cast<uint32_t*>(std::malloc(n_tri * 4));
    if (!*nodes64 || !*prim64 || !hp) { rc = set_error(CERES_ENOMEM, "out of host memory"); goto done; }
    HIP_TRY_DONE(hipMemcpyAsync(*nodes64, d_nodes, m * sizeof(RefNode64), hipMemcpyDeviceToHost, stream));
    HIP_TRY_DONE(hipMemcpyAsync(hp, d_prim, n_tri * 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY_DONE(hipStreamSynchronize(stream));
    for (size_t i = 0; i < n_tri; ++i) (*prim64)[i] = hp[i];
    *n_nodes = m;
done:
    std::free(hp);
    if (rc != CERES_OK) { std::free(*nodes64); std::free(*prim64); *nodes64 = nullptr; *prim64 = nullptr; }
    if (d_tri) (void)hipFree(d_tri);
    if (d_nodes) (void)hipFree(d_nodes);
    if (d_prim) (void)hipFree(d_prim);
    if (stream) (void)hipStreamDestroy(stream);
    return rc;
}

int ceres_bvh_build_f64_gpu(const double* tri96, size_t n_tri, uint64_t** nodes64, size_t* n_nodes, uint64_t** prim64,
                            int device) {
    return ceres_bvh_build_f64_gpu_arith(tri96, n_tri, nodes64, n_nodes, prim64, device, CERES_ARITH_EXACT);
}

}  // extern "C"
