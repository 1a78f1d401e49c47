// scene_internal.hpp -- the opaque ceres_scene of include/ceres_render.h, shared by the
// translation units that implement the ABI (render_hip.hip: float path, render64.hip: double).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <utility>
#include <vector>

#include "ceres_render.h"
#include "ceres_types.hpp"
#include "host_common.hpp"

using ceres::SiblingPair; using ceres::SiblingPair64; using ceres::Node4; using ceres::Tri48; using ceres::Tri96;
using ceres::Shard;

struct ceres_scene {
    int device = 0;
    uint32_t flags = 0;
    size_t n_tri = 0, n_pairs = 0;
    uint32_t depth = 0, stack_entries = 1, root_leaf_count = 0, root_leaf_first = 0;
    float root_box[6] = {0, 0, 0, 0, 0, 0};   // root node bounds; root_box_ok: both children inside it
    uint32_t root_box_ok = 0;
    uint32_t shadow_stack_entries = 1;     // BVH4 stack bound of the nearest-first walk (any child order)
    uint32_t shadow_stack_first = 1;       // ... of first-passing-child walks (order_shadow_bvh4; <= the above)
    size_t n_nodes4 = 0;
    int debug_stack_width = 0;             // CERES_DEBUG_STACK_WIDTH at creation (3 or 4, else 0): render_hip.hip stack_width
    uint32_t list_entries = ceres::kListEntries;     // complete hit lists: L (CERES_DEBUG_LIST_ENTRIES at creation)
    uint32_t list_sort_cap = ceres::kListSortCap;    // ... the LDS sort's longest segment (CERES_DEBUG_LIST_SORT_CAP)
    SiblingPair* d_pairs = nullptr;
    Node4* d_nodes4 = nullptr;
    ceres::QNode4* d_qnodes4 = nullptr;   // compressed shadow BVH4, built on first CERES_MODE_QBVH4 render
    // fused-kernel tile orders, one per (frame size, tiling, batch, tile), never rewritten or
    // freed while a launch that reads them may be in flight (launches on different streams may
    // read different orders concurrently): an evicted order's buffer goes to `retired` and is
    // freed only once retired buffers exceed kRetiredBytes (counted at the allocation granule) or
    // number kMaxRetired, after one device synchronise -- no
    // per-launch events, and no stall while the working set of shapes fits the cache.
    struct TileOrder {
        size_t W = 0, H = 0;
        uint32_t row_block = 0, rank = 0, world = 0, frames = 0, tile = 0, bands = 0;
        bool packed = false;           // entries (f << 26) | (y << 13) | x (pack_tile) instead of linear ids
        uint32_t* d = nullptr;
        size_t cap = 0;                // entries allocated at d
        uint64_t used = 0;
        // batch orders a launch may compact (more than one frame, the whole frame on this rank):
        // the order before the XCD dealing -- the sorted curve, or the order itself where nothing
        // is dealt -- on the device (inside the allocation at d) and on the host, n entries;
        // deal: wavefront groups of the curve per XCD chunk (0: not dealt)
        const uint32_t* d_curve = nullptr;
        uint32_t n = 0, deal = 0;
        // The host's count of the groups a launch keeps (count_kept_tiles) must cost far less than
        // the launch.  `shapes` (frame-major orders whose frames hold the same whole groups): the
        // groups that reach a rectangle of tiles, by inclusion and exclusion over the groups' tile
        // subsets -- per bounding-box extent (w, h) the signed number of subsets by their box's
        // first tile, as a 2-D prefix sum -- so a frame costs one lookup per extent.  Else h_curve,
        // the order on the host, walked entry by entry: small orders only (kCountWalkTiles).
        // Neither: launches of this order are not compacted.
        struct SubsetBoxes {
            uint32_t w = 0, h = 0;
            std::vector<int32_t> sum;          // (tile rows + 1) x (tile columns + 1)
        };
        std::vector<SubsetBoxes> shapes;
        std::vector<uint32_t> h_curve;
        bool countable = false;
    };
    // Compacted tile orders (launch_chunk): launches on different streams run concurrently with
    // different cameras, so each stream has its own buffer; launches of one stream reuse it in
    // stream order.  A buffer that is outgrown, or evicted (the least recently used of
    // kMaxCompactBufs), goes to `retired` like an evicted order.  The last fields describe the
    // stream's latest compacting launch (ceres_debug_compact_order).
    struct CompactBuf {
        hipStream_t stream = nullptr;
        uint32_t* d = nullptr;
        size_t cap = 0;                // words allocated at d
        uint64_t used = 0;
        const uint32_t* src = nullptr; // the source order
        uint32_t n = 0, host_tiles = 0, tpw = 0, deal = 0, off_result = 0;
        // entry nodes of that launch (ceres_debug_entry_nodes): KParams::entry_off (0: it entered at
        // the root), its frames and frame size
        uint32_t entry_off = 0, frames = 0, W = 0, H = 0;
        // retired tiles of that launch (ceres_debug_retire): KParams::retire_off / flag_off (0: unused)
        uint32_t retire_off = 0, flag_off = 0;
    };
    // entry nodes (entry_cut.hpp): the scene's cut table, kCutWords words, made with the topology
    // (creation, rebuild) and refreshed by every refit; null for double scenes.  entry_debug:
    // launches also record the entry record of every order entry (ceres_debug_entry_record).
    uint32_t* d_cut = nullptr;
    bool entry_debug = false;
    std::vector<CompactBuf> compact;
    hipStream_t last_fused_stream = nullptr;   // the latest batch launch ...
    bool last_fused_compacted = false;         // ... and whether it read a compacted order
    std::vector<TileOrder> orders;
    std::vector<uint32_t*> retired;
    size_t retired_bytes = 0;
    uint64_t order_clock = 0;
    Tri48* d_tris = nullptr;
    uint32_t* d_orig = nullptr;
    float* d_norms = nullptr;
    Shard* d_shards = nullptr;
    bool shards_dirty = true;          // shards not known to be zero (see ceres_render_batch)
    uint64_t* d_counters = nullptr;
    float* d_pixels = nullptr;
    uint8_t* d_rgb8 = nullptr;
    size_t px_cap = 0;
    hipStream_t stream = nullptr;
    // host-buffer renders (ceres_render_f32): row bands rendered one after another on `stream`,
    // each band's D2H copy on `copy_stream` as soon as its kernel ends (the copy over the host
    // link, not the kernel, sets the call's length); counters per band
    hipStream_t copy_stream = nullptr;
    uint64_t* d_band_counters = nullptr;
    std::vector<hipEvent_t> band_events;
    // host float framebuffers (ceres_render_f32): the lit pixels -- those with any non-zero bit --
    // compacted on the device into {index, r, g, b} records, copied, and scattered over a host
    // zero fill that overlaps the kernel (host_fill_zero / host_scatter_lit, scene_host.cpp)
    uint4* d_lit = nullptr;
    uint32_t* d_lit_count = nullptr;
    size_t lit_cap = 0;
    uint32_t* h_small = nullptr;       // pinned: lit count + 8 counters
    std::vector<uint4> h_lit;
    uint4* h_lit_pinned = nullptr;     // zero-copy records (pinned host memory the compaction kernel writes)
    bool lit_zc = false;
    double last_lit_frac = 0.0;        // the previous call's lit fraction (dense frames take the full copy)
    uint32_t dense_calls = 0;
    hipEvent_t ev_count = nullptr;
    int num_cus = 256;
    size_t max_lds_per_block = 64 * 1024;   // hipDeviceProp_t::sharedMemPerBlock (set at scene creation)
    unsigned long long* d_wave_log = nullptr;   // stats scenes: per-wave diagnostic records
    size_t wave_log_waves = 0, last_grid_waves = 0;
    // optional per-launch device timing (ceres_scene_set_timing)
    bool timing = false;
    std::vector<hipEvent_t> ev_pool;
    std::vector<hipEvent_t> ev_used;   // pairs: before and after the render's kernel
    // double-precision scene (render<double>, render64.hip): set instead of the float layout
    bool f64 = false;
    SiblingPair64* d_pairs64 = nullptr;
    Tri96* d_tris64 = nullptr;
    double* d_norms64 = nullptr;
    // refit (scene_refit.hip): the BVH4 children's box sources, kept from creation; the rest is
    // made at the first refit and reused by every later one (no allocation per call)
    uint32_t* d_src4 = nullptr;            // float scenes: 4 words per Node4 record, pair << 1 | side
    uint32_t* d_refit_levels = nullptr;    // pair indices sorted by tree level (root's pair first)
    std::vector<uint32_t> refit_level_off; // level l = d_refit_levels[off[l] .. off[l + 1])
    float* d_refit_root = nullptr;         // 18 floats: the new root box, then pair 0's lb and rb
    void* d_refit_stage = nullptr;         // host-array refits: triangles, then normals
    // upkeep (scene_quality.hip): the SAH-cost partials (kCostBlocks doubles, then the result; a fixed
    // size, so a rebuild keeps it) and the baseline ceres_scene_update* compares with -- unknown until
    // the first update or rebuild measures it
    double* d_cost = nullptr;
    double built_cost = 0.0;
    bool built_cost_known = false;
};

namespace ceres {
// The index list of an indexed ray query (ceres_*_indexed_device), checked after every refusal of the
// plain sibling and before any launch: negative when refused, 1 when the list is empty (a successful
// no-op), 0 when there is something to launch.
inline int check_index_list(const char* name, const ceres_scene* s, const uint32_t* d_index, size_t n_index) {
    if (s->flags & CERES_SCENE_STATS)
        return set_error(CERES_EUNSUPPORTED, "%s: CERES_SCENE_STATS scenes take the plain calls (statistics are theirs)", name);
    if (n_index >= (size_t(1) << 31)) return set_error(CERES_EUNSUPPORTED, "%s: %zu index entries (below 2^31 per call)", name, n_index);
    if (n_index == 0) return 1;
    if (!d_index) return set_error(CERES_EINVAL, "%s: null index", name);
    if (reinterpret_cast<uintptr_t>(d_index) & 3u) return set_error(CERES_EINVAL, "%s: index must be 4-byte aligned", name);
    return 0;
}
// host side of the compacted float readback (scene_host.cpp, OpenMP over the caller's cores)
void host_fill_zero(float* dst, size_t n);
void host_scatter_lit(float* dst, const uint32_t* lit4, size_t n);   // records {pixel, r, g, b}
void scene_release(ceres_scene* s);          // frees every device buffer and the stream (render_hip.hip)
// list_entries / list_sort_cap from CERES_DEBUG_LIST_ENTRIES / CERES_DEBUG_LIST_SORT_CAP: every scene
// creation, float and double, calls it once (render_hip.hip)
void scene_set_list_constants(ceres_scene* s);
// a refitted float scene's root box (set_root_box) and the end of its quantised BVH4 copy (render_hip.hip)
int scene_after_refit(ceres_scene* s, const float root[6], const SiblingPair& p0);
// The scene takes a complete device layout (relayout_device) as its own: arrays, counts, depth, stack
// bounds, root-leaf fields and root box (pair 0 is read back on `stream`, which is synchronised).
// Shared by ceres_scene_create_device and the in-place rebuild; on failure nothing has been adopted
// and L is still the caller's.  The arrays the scene held before are NOT freed (render_hip.hip).
int scene_adopt_layout(ceres_scene* s, ceres::DeviceLayout& L, hipStream_t stream);
// entry nodes: the cut table's boxes and entry_ok from the refitted pairs, on `stream` (no
// synchronisation); d_root_box: the new root box on the device (render_hip.hip)
int scene_refresh_cut(ceres_scene* s, const float* d_root_box, hipStream_t stream);
constexpr uint32_t kCostBlocks = 512;        // most workgroups (= partials) of the SAH-cost pass
// centre-first, XCD-balanced order of one whole frame's tile x tile tiles (render_hip.hip)
int frame_tile_order(ceres_scene* s, size_t W, size_t H, uint32_t tile, hipStream_t stream, const uint32_t** out);
constexpr size_t kMaxTileOrders = 16;         // cached orders per scene before LRU eviction
constexpr size_t kCountWalkTiles = size_t(1) << 16;   // orders up to this long may be counted entry by entry ...
constexpr size_t kCountShapes = 32;                   // ... longer ones need at most this many subset-box extents
constexpr size_t kMaxCompactBufs = 16;       // streams with a compacted-order buffer before LRU eviction
constexpr size_t kDramSceneBytes = size_t(64) << 20;   // a scene this large does not stay in the 8 x 4 MB L2s
#ifndef CERES_RETIRED_BYTES
#define CERES_RETIRED_BYTES (64u << 20)
#endif
constexpr size_t kRetiredBytes = CERES_RETIRED_BYTES;   // evicted orders kept until they exceed this ...
constexpr size_t kMaxRetired = 64;                      // ... or number this many buffers
constexpr size_t kAllocGranule = 4096;                  // bytes of a retired buffer counted per started granule
}
