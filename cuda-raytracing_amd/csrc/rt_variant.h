// rt_variant.h -- which instantiation of render_fast_body<STACK, STATS, MODE> (rt_fast_body.h) a frame runs: the
// names of MODE's bits, of the RT_TUNE bits the host reads to choose, and choose_variant, the one statement of
// that choice (rt_render.hip rt_render, rt_batch_calls.hip query_scene, host_hooks.hip rt_variant_host).  Host-only and free of HIP, so a
// plain C++ compiler can replay it (tests/test_variant_cpu.py pins it to the table of the if-chains it replaced).
#pragma once

#include <cstdint>

namespace rtfast {

// MODE, the third template argument of the render kernels.  Bits 0-1, the big-leaf mode (leaves above BIG
// triangles): BIG_PAIRS pair records in the shared-leaf loop and in cooperative rounds, BIG_MIXED pairs in the
// shared-leaf loop and scalar records in cooperative rounds (measured best), BIG_SCALAR scalar records only.
constexpr int BIG_MASK = 3, BIG_PAIRS = 0, BIG_MIXED = 1, BIG_SCALAR = 2;
constexpr int TREE_BIT = 4;     // leaves with a leaf tree walk it: compiled in only for scenes that have them
constexpr int TIMING_BIT = 8;   // phase clocks, per-pixel work (lane_cost), per-wave clock records; no counts
constexpr int SPLIT_BIT = 16;   // inner-node and small-leaf steps in separate wave iterations (rt_fast.h trace)
constexpr int SCREEN_BIT = 32;  // big-leaf screens (rt_fast.h screen_leaf), for mirrors with screen records
constexpr int REFILL_BIT = 64;  // idle lanes take new pixels from a queue (rt_render_params.refill_lanes)
// The fixed-policy ("lean") production variants: RT_TUNE is the compile-time constant 0 and every mirror array
// the variant uses is present (MODE_PROD: spairs, pairs, quads, units, tris; a leaf-tree mode would add tree,
// ltris, flat, face_leaf -- none is built: rt_fast_lean.hip), so neither the knobs nor the fallbacks for a
// missing array are compiled in.  choose_variant sends a frame here only when both hold.
constexpr int LEAN_BIT = 128;
constexpr int MODE_PROD = SPLIT_BIT | BIG_MIXED;  // 17, the production kernel; | TREE_BIT = 21 with leaf trees
constexpr int MODE_NOSPLIT = BIG_MIXED;           // 1, its form without split steps (A/B; 9 with timing)

}  // namespace rtfast

namespace rtk {

// RT_TUNE bits the host reads to choose a kernel.
constexpr uint32_t TUNE_BIG_SHIFT = 4;      // bits 4-5, big-leaf A/B: 0 / 1 production, 2 scalar only, 3 pairs everywhere
constexpr uint32_t TUNE_STATS_TREES = 128;  // a statistics frame counts through the leaf trees
constexpr uint32_t TUNE_TIMING = 256;       // a statistics frame is a timing frame of the production kernel instead
constexpr uint32_t TUNE_NO_SPLIT = 4096;    // no split steps (A/B)
// RT_TUNE bits a render kernel itself reads (rt_fast.h trace / big_round / coop_tree: bits 0, 13-15, 21-24, 26,
// 30, 31; rt_fast_body.h: the XCD run length 16-19, the per-wave clock records 11).  The others choose a
// kernel or drop a mirror array on the host.
constexpr uint32_t kKernelTuneBits = 1u | (1u << 11) | (7u << 13) | (15u << 16) | (7u << 21) | (1u << 24) | (1u << 26) |
                                     (1u << 30) | (1u << 31);

// One translation unit each (rt_render.h, the family table): four in librt_hip.so, then the plugin librt_hip_exp.so's.
enum Family { FAM_PROD, FAM_LEAN, FAM_TIMING, FAM_STATS, FAM_AB, FAM_AB2, FAM_REFILL, FAM_SCREEN, FAM_COUNT };

struct VariantInput {
    uint32_t tune;         // rt_render_params.tune
    bool stats;            // RT_RENDER_STATS
    bool lane_cost;        // the frame records per-pixel work
    bool refill;           // refill_lanes > 0 (never with lane_cost: rt_render refuses that)
    bool has_tree;         // the launch passes leaf trees
    bool screens;          // the mirror has screen records and the frame may use them
    bool arrays_complete;  // the launch passes nodes, tris, spairs, pairs, quads and units: what a lean kernel assumes
    int depth;             // the BVH's depth, < 0 unknown
    bool want_entry;       // entry records are on and the frame is one that may start from them, kernel choice aside
};

struct Variant {
    Family family;
    int mode;           // MODE
    int stack;          // STACK: 30, 40 or 64 entries
    bool needs_plugin;  // refused unless librt_hip_exp.so is loaded
    bool use_entry;     // camera rays start from the entry table (entry_frontier.h)
};

// Stack entries an entry record adds (EF_K - 1: up to EF_K record nodes, where the root walk holds one sibling per level).
constexpr int kEntryStackExtra = 14;

// The traversal stack for a BVH of `depth`: the DFS holds at most depth + 1 entries (+ extra); 30 entries -- 7.5 KB
// of LDS per wave -- still fit 5 waves per SIMD and cover the 4-bunny scene's depth 28.
// The deepest BVH any traversal kernel is launched on: the largest STACK is 64 entries and the walk needs depth + 2
// (rtfast::Stack::put has no bound of its own -- a deeper tree would write past its arrays).  rt_render, rt_trace_rays,
// rt_occluded and rt_ao refuse a deeper scene (rt_kernel.hip depth_refused, rt_host.h) before anything is launched.
constexpr int kMaxBvhDepth = 62;

inline int variant_stack(int depth, int extra = 0) {
    const int need = depth + 2 + extra;
    return (depth >= 0 && need <= 30) ? 30 : (depth >= 0 && need <= 40) ? 40 : 64;
}

inline Variant choose_variant(const VariantInput& in) {
    using namespace rtfast;
    const bool split = (in.tune & TUNE_NO_SPLIT) == 0;
    const uint32_t big = (in.tune >> TUNE_BIG_SHIFT) & 3u;
    const bool timing = in.stats ? (in.tune & TUNE_TIMING) != 0 : in.lane_cost;
    const bool scr = in.screens && split;  // the screen variants are split-step ones
    const int tree = in.has_tree ? TREE_BIT : 0;
    Variant v{};
    if (timing) {  // a timing frame ignores refill and the big-leaf A/B; only a statistics frame's honours no-split
        if (scr) v.family = FAM_SCREEN, v.mode = MODE_PROD | SCREEN_BIT | TIMING_BIT | tree;
        else if (in.stats && !in.has_tree && !split) v.family = FAM_TIMING, v.mode = MODE_NOSPLIT | TIMING_BIT;
        else v.family = FAM_TIMING, v.mode = MODE_PROD | TIMING_BIT | tree;
    } else if (in.stats) {  // the reference's work on scalar records
        v.family = FAM_STATS, v.mode = BIG_SCALAR | ((in.tune & TUNE_STATS_TREES) ? tree : 0);
    } else if (in.refill) {
        v.family = FAM_REFILL, v.mode = MODE_PROD | REFILL_BIT | tree;
    } else if (scr && (in.has_tree || big < 2)) {
        v.family = FAM_SCREEN, v.mode = MODE_PROD | SCREEN_BIT | tree;
    } else if (in.has_tree) {  // leaf-tree scenes have no big-leaf A/B
        if (split) v.family = FAM_PROD, v.mode = MODE_PROD | TREE_BIT;
        else v.family = FAM_AB, v.mode = MODE_NOSPLIT | TREE_BIT;
    } else if (big >= 2) {
        v.family = FAM_AB2, v.mode = big == 2 ? BIG_SCALAR : BIG_PAIRS;
    } else if (!split) {
        v.family = FAM_AB, v.mode = MODE_NOSPLIT;
    } else {
        v.family = FAM_PROD, v.mode = MODE_PROD;
    }
    // MODE_PROD and its timing form run lean when the frame sets no knob the kernel reads (no leaf-tree mode does)
    if ((v.mode & ~TIMING_BIT) == MODE_PROD && (in.tune & kKernelTuneBits) == 0 && in.arrays_complete) {
        v.mode |= LEAN_BIT;
        if (v.family == FAM_PROD) v.family = FAM_LEAN;
    }
    // refill is refused without the plugin even on the statistics / timing frames that ignore it: kept as found
    v.needs_plugin = in.refill || v.family >= FAM_AB;
    // only the lean kernels read entry records; the deepest stack there is must hold the record too
    v.use_entry = in.want_entry && (v.mode & LEAN_BIT) && !in.refill && !in.screens && split && big < 2 &&
                  in.depth >= 0 && in.depth + 2 + kEntryStackExtra <= 64;
    v.stack = variant_stack(in.depth, v.use_entry ? kEntryStackExtra : 0);
    return v;
}

}  // namespace rtk
