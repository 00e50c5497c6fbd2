// rt_render.h -- launchers of the render kernels, one family per translation unit (rt_render.hip chooses and
// launches through the family table below; the families compile in parallel).  `stack` is the traversal stack
// size of the instantiation (30, 40 or 64 entries), `mode` the MODE bits of render_fast_body (rt_fast_body.h;
// both from rt_variant.h choose_variant).  Each returns hipErrorInvalidValue for a mode it does not hold.
#pragma once

#include <hip/hip_runtime.h>

#include "rt_common.h"
#include "rt_variant.h"

namespace rtk {

// The families of render_fast_body, one row each, in Family's order (rt_variant.h): family, launcher, STATS, the
// MODEs its unit instantiates (the unit defines the launcher from its row: rt_fast_body.h RT_FAST_FAMILY).  The
// first four are in librt_hip.so (the product): the kernels the production path launches.  The others are in
// librt_hip_exp.so (rt_exp.hip): exact alternatives kept for A/B measurement and their parity tests, none of which
// serves the benchmark -- loading the library registers them (rt_render then accepts the flags / knobs that select
// them; without it those requests are refused).
#define RT_FAMILY_PROD FAM_PROD, launch_fast_prod, false, rtfast::MODE_PROD, rtfast::MODE_PROD | rtfast::TREE_BIT  // 17, 21
#define RT_FAMILY_LEAN FAM_LEAN, launch_fast_lean, false, rtfast::MODE_PROD | rtfast::LEAN_BIT                    // 17 | 128
#define RT_FAMILY_TIMING /* 25, 29, 9, 25 | 128 */ \
    FAM_TIMING, launch_fast_timing, false, rtfast::MODE_PROD | rtfast::TIMING_BIT, \
    rtfast::MODE_PROD | rtfast::TIMING_BIT | rtfast::TREE_BIT, rtfast::MODE_NOSPLIT | rtfast::TIMING_BIT, \
    rtfast::MODE_PROD | rtfast::TIMING_BIT | rtfast::LEAN_BIT
#define RT_FAMILY_STATS FAM_STATS, launch_fast_stats, true, rtfast::BIG_SCALAR, rtfast::BIG_SCALAR | rtfast::TREE_BIT  // 2, 6
#define RT_FAMILY_AB FAM_AB, launch_fast_ab, false, rtfast::MODE_NOSPLIT, rtfast::MODE_NOSPLIT | rtfast::TREE_BIT  // 1, 5
#define RT_FAMILY_AB2 FAM_AB2, launch_fast_ab2, false, rtfast::BIG_SCALAR, rtfast::BIG_PAIRS                       // 2, 0
#define RT_FAMILY_REFILL /* 81, 85 */ \
    FAM_REFILL, launch_fast_refill, false, rtfast::MODE_PROD | rtfast::REFILL_BIT, \
    rtfast::MODE_PROD | rtfast::REFILL_BIT | rtfast::TREE_BIT
#define RT_FAMILY_SCREEN /* 49, 53, 57, 61 */ \
    FAM_SCREEN, launch_fast_screen, false, rtfast::MODE_PROD | rtfast::SCREEN_BIT, \
    rtfast::MODE_PROD | rtfast::SCREEN_BIT | rtfast::TREE_BIT, rtfast::MODE_PROD | rtfast::SCREEN_BIT | rtfast::TIMING_BIT, \
    rtfast::MODE_PROD | rtfast::SCREEN_BIT | rtfast::TIMING_BIT | rtfast::TREE_BIT
#define RT_APPLY(X, ...) X(__VA_ARGS__)  // X on a row (expanded first)
#define RT_FAST_FAMILIES(X) \
    RT_APPLY(X, RT_FAMILY_PROD) RT_APPLY(X, RT_FAMILY_LEAN) RT_APPLY(X, RT_FAMILY_TIMING) RT_APPLY(X, RT_FAMILY_STATS) \
    RT_APPLY(X, RT_FAMILY_AB) RT_APPLY(X, RT_FAMILY_AB2) RT_APPLY(X, RT_FAMILY_REFILL) RT_APPLY(X, RT_FAMILY_SCREEN)
typedef hipError_t (*FastLauncher)(int stack, int mode, const RenderArgs& a, int waves, hipStream_t s);
#define RT_DECLARE_FAMILY(FAM, NAME, ...) hipError_t NAME(int stack, int mode, const RenderArgs& a, int waves, hipStream_t s);
RT_FAST_FAMILIES(RT_DECLARE_FAMILY)
#undef RT_DECLARE_FAMILY
// The reference-layout tracer (flat = false) or the exact-division flat tracer (rt_ref.hip).
hipError_t launch_ref_tracer(bool flat, const RenderArgs& a, int waves, int depth, bool stats, hipStream_t s);

// The ray-query kernel (rt_query.hip, rt_trace_rays): one ray per lane through rtfast::trace, no shading.
// `rays` null = camera mode (pixel centres of `cam`, width x height).  The mirror arrays are the ones a
// render launch passes to trace (rt_batch_calls.hip query_scene).
struct QueryArgs {
    const rt_ray* rays;
    rt_hit* hits;
    long long count;
    int width, height;
    GPUCamera cam;
    const GeometrySphere* spheres;
    int sphere_count;
    int scene_fast;
    const GPUFace* faces;
    const GPUVertex* vertices;
    const GPUBVHNode* nodes;  // the mirror's private node array
    const FlatTri* tris;
    const float4 *pairs, *quads, *units, *tree, *ltris, *spairs, *flat;
    const uint32_t* face_leaf;
};
// mode MODE_PROD, MODE_PROD | LEAN_BIT or MODE_PROD | TREE_BIT (17, 145, 21); occupancy 5, 6 or 7 waves per SIMD
hipError_t launch_query(int stack, int mode, int waves_per_simd, const QueryArgs& q, hipStream_t s);

// The any-hit kernels (rt_occlude.hip, rt_occluded / rt_ao): the query kernel's variants through trace<.., ANY>.
// `q` carries the scene and the launch size: for rt_occluded its rays and count (hits, width, height, cam, faces and
// vertices unused); for rt_ao the first-hit records in `hits` (read only) and count = width * height pixels.
struct OcclusionArgs {
    QueryArgs q;
    uint8_t* occluded;  // count bytes
};
struct AoArgs {
    QueryArgs q;
    const float4* directions;
    int direction_count, samples;
    float radius, bias;
    float* ao;  // count floats
};
hipError_t launch_occlusion(int stack, int mode, int waves_per_simd, const OcclusionArgs& a, hipStream_t s);
hipError_t launch_ao(int stack, int mode, int waves_per_simd, const AoArgs& a, hipStream_t s);

// The radiance kernel (rt_radiance.hip, rt_radiance): render_fast_body's per-lane sample state machine over a ray
// list, the query kernel's variants.  The kernel's only parameter begins with a RenderArgs, so shade_segment
// (rt_fast_body.h) runs on it unchanged and its COLD reads from the kernel-argument segment find their fields:
// `r` holds what rt_render fills for a scene of its own -- the shading arrays, the sky, the mirror, bounces -- and
// zero everywhere else (no camera, surface, RNG array, tile list, lane map, gate, statistics; tune 0).
struct RadianceArgs {
    RenderArgs r;
    const rt_ray* rays;
    rt_rng_state* rng;  // state i for ray i
    float4* radiance;
    long long count;
    int samples;
};
static_assert(offsetof(RadianceArgs, r) == 0, "the kernel-argument segment starts with the RenderArgs");
hipError_t launch_radiance(int stack, int mode, int waves_per_simd, const RadianceArgs& a, hipStream_t s);

// The adaptive-sampling kernel (rt_adaptive.hip, rt_sample_pixels): render_fast_body's sample state machine over a
// list of (pixel, samples) entries, the query kernel's variants.  As a RadianceArgs it begins with a RenderArgs: `r`
// holds what the radiance kernel's does, and the camera, width, height, the RNG array (state y * width + x), the
// accumulator as `surface` with its `pitch`, and bounces.
struct SampleArgs {
    RenderArgs r;
    const int32_t* pixels;    // null: entry i is pixel i
    const uint16_t* samples;
    float2* moments;          // null: none kept
    long long count;
};
static_assert(offsetof(SampleArgs, r) == 0, "the kernel-argument segment starts with the RenderArgs");
hipError_t launch_sample_pixels(int stack, int mode, int waves_per_simd, const SampleArgs& a, hipStream_t s);

// The scene as the walk kernels read it (rt_closest.hip, rt_hits.hip: rt_batch.h RT_WALK_KERNELS), each lane walking the
// mirror's private nodes, leaf-ordered records and leaf trees itself: query_scene's result without the arrays only
// rtfast::trace reads (rt_batch_calls.hip walk_scene).
struct WalkScene {
    const GeometrySphere* spheres;
    int sphere_count;
    int scene_fast;  // every node bound inside the mirror's `fast` range: the premise of the culls' bounds on the boxes
    const GPUFace* faces;
    const GPUVertex* vertices;
    const GPUBVHNode* nodes;  // the mirror's private node array
    const FlatTri* tris;
    const float4 *tree, *ltris;  // null: the scene has no leaf tree
};

// The closest-point kernel (rt_closest.hip, rt_closest_point): one point per lane, culling by distance to a box
// (closest.h).  Stack 30 / 40 / 64 and the occupancy choose the build.
struct ClosestArgs {
    const rt_point* points;
    rt_nearest* nearest;
    long long count;
    WalkScene s;  // faces: the winner's material; vertices unused
};
hipError_t launch_closest(int stack, int waves_per_simd, const ClosestArgs& a, hipStream_t s);

// The ordered-hits kernel (rt_hits.hip, rt_trace_hits): one ray per lane through the rt_fast.h pieces (make_ray,
// inner_step, pop), the first max_hits accepted distances kept in a register list (hit_list.h).  rays, width, height
// and cam as QueryArgs (rt_batch.h query_ray).  The list's capacity (4 / 8 / 16 >= max_hits), stack 30 / 40 / 64 and
// the occupancy choose the build.
struct HitsArgs {
    const rt_ray* rays;  // null: camera mode
    rt_hit* hits;        // count * max_hits records
    uint32_t* counts;    // null: none kept
    long long count;
    int width, height;
    GPUCamera cam;
    int max_hits;
    uint32_t flags;  // RT_HITS_*
    WalkScene s;
};
hipError_t launch_hits(int stack, int waves_per_simd, const HitsArgs& a, hipStream_t s);

// In librt_hip_exp.so beside its families:
// The lone-pixel kernel (rt_lone.hip): one wave per slot of `lone_slots`, through the treelets.
hipError_t launch_lone(const RenderArgs& a, const int32_t* lone_slots, int lone_count, const void* treelets, hipStream_t s);
// The wavefront tracer (rt_wavefront.hip): shade / trace launches per segment generation.
hipError_t launch_wavefront(const RenderArgs& a, int depth, hipStream_t s);

struct ExperimentalKernels {
    FastLauncher fast[FAM_COUNT];  // the plugin's families; null at the product's
    decltype(&launch_lone) lone;
    decltype(&launch_wavefront) wavefront;
};
// Layout stamp of what the plugin shares with librt_hip.so (RenderArgs by reference, this table): a
// version bumped by hand when a field changes meaning, and the two sizes.  A plugin built against another
// layout is refused at registration instead of reading a different struct (rt_exp_abi_version).
constexpr uint32_t kExperimentalAbi = (3u << 24) ^ ((uint32_t)sizeof(RenderArgs) << 8) ^ (uint32_t)sizeof(ExperimentalKernels);
// rt_render.hip: the registered table (nullptr until librt_hip_exp.so is loaded); a table whose `abi` is
// not this library's kExperimentalAbi is refused (rt_last_error says so, rt_experimental_loaded stays 0).
void register_experimental_kernels(const ExperimentalKernels* k, uint32_t abi);
const ExperimentalKernels* experimental_kernels();

}  // namespace rtk
