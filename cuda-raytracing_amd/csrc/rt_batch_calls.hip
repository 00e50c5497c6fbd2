// rt_batch_calls.hip -- the entry points of the batch calls (rt_abi.h): rt_trace_rays, rt_occluded, rt_closest_point,
// rt_trace_hits, rt_ao, rt_radiance and rt_sample_pixels.  Each makes the checks that need no device first, then the
// scene's and the buffers', then launches its kernel (rt_query.hip, rt_occlude.hip, rt_closest.hip, rt_hits.hip,
// rt_radiance.hip, rt_adaptive.hip: rt_render.h) in the variant a production frame of the scene runs at RT_TUNE 0.
// Stream-ordered: no synchronisation, no allocation.  No kernel lives here.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstring>
#include <string>
#include <type_traits>

#include "rt_abi.h"
#include "rt_host.h"
#include "rt_render.h"
#include "image_entry.h"

using namespace rt_host;
using namespace rtk;
using rt_entry::misaligned;
using rt_entry::overlap;
using rt_entry::refuse;

// The scene half of a ray-batch launch (`who` names the call in the messages): scenes uploaded by rt_scene_upload
// only; the mirror arrays a render launch passes to trace; the variant a production frame of this scene runs at
// RT_TUNE 0 (choose_variant).  `a` is a QueryArgs, or the RenderArgs a RadianceArgs begins with: zeroed, then the
// traversal and shading fields the two name alike.
template <class Args>
static int query_scene(const char* who, const GPUScene* scene, Args* a, Variant* variant) {
    MirrorDevice mir;
    if (!rt_internal_lookup_mirror(scene, &mir) || !mir.owned)
        return refuse(who, "this GPUScene was not uploaded by rt_scene_upload (a foreign scene has no private "
                           "mirror to query; foreign scenes are not supported here)");
    if (!mir.nodes || !mir.tris) return refuse(who, "the scene's mirror has no triangles to traverse");
    if (depth_refused(who, mir.depth)) return 1;
    if (scene->sphere_count > 0 && !scene->gpu_spheres) return refuse(who, "sphere_count without spheres");
    std::memset(a, 0, sizeof(*a));
    if constexpr (std::is_same_v<Args, QueryArgs>) {  // the radiance kernel's RenderArgs has no camera (rt_render.h)
        a->width = a->height = 1;
        a->cam = scene->camera;
    }
    a->spheres = scene->gpu_spheres;
    a->sphere_count = scene->sphere_count;
    a->scene_fast = mir.fast ? 1 : 0;
    a->faces = scene->gpu_faces;
    a->vertices = scene->gpu_vertices;
    a->nodes = (const GPUBVHNode*)mir.nodes;
    a->tris = (const FlatTri*)mir.tris;
    a->pairs = (const float4*)mir.pairs, a->quads = (const float4*)mir.quads, a->units = (const float4*)mir.units;
    a->tree = (const float4*)mir.tree, a->ltris = (const float4*)mir.ltris, a->spairs = (const float4*)mir.spairs;
    a->flat = (const float4*)mir.flat;
    a->face_leaf = (const uint32_t*)mir.face_leaf;
    VariantInput in{};  // tune 0, no statistics / lane_cost / refill / screens / entry records
    in.has_tree = a->tree != nullptr, in.arrays_complete = a->spairs && a->pairs && a->quads && a->units, in.depth = mir.depth;
    *variant = choose_variant(in);
    return 0;
}

// The checks the ray-batch calls share, in the order each call makes them.  Each returns 1 with rt_last_error set.
static int waves_refused(const char* who, int w) {
    return (w != 0 && (w < 5 || w > 7)) ? refuse(who, "waves_per_simd must be 0 (default), 5, 6 or 7") : 0;
}
static int count_refused(const char* who, int64_t count, const char* items) {
    if (count < 0) return refuse(who, "negative count");
    return count > (int64_t)1 << 31 ? refuse(who, std::string("more than 2^31 ") + items + " in one call") : 0;
}
// a short buffer would fault the GPU
static int too_small(const char* who, const char* name, const void* p, size_t need) {
    return bytes_from(p) < need ? refuse(who, std::string(name) + " too small") : 0;
}

// The occupancy of a call that asks for none (waves_per_simd 0), measured.  MODE 17 and its lean form run 7 waves per
// SIMD in every call; the leaf-tree MODE 21 runs 5, or 6 in the any-hit calls.
//  rt_trace_rays (profiles/query_timing.txt): MODE 17 fits 7 with 2 spilled registers (incoherent rays 1.20 vs 1.35 ms
//   at 5); MODE 21 spills ~100 there (5.0 vs 3.9 ms).
//  rt_occluded, rt_ao (profiles/occlusion_timing.txt): MODE 17 at 7 (incoherent rays 0.867 vs 0.874 / 0.929 ms at 6 / 5;
//   rt_ao 2.92 vs 2.96 / 3.07 ms); MODE 21 at 6, not the query kernel's 5 -- without the deferral it spills 10 registers
//   there, not 89, and is the fastest on every batch (incoherent rays 4.28 vs 4.57 / 4.86 ms at 5 / 7; rt_ao 25.6 vs
//   26.9 / 27.5 ms).
//  rt_radiance (profiles/radiance_timing.txt, 2.07 M six-bounce paths): the lean MODE 17 at 7 (config 2's scene 2.27-2.28
//   vs 2.28-2.31 / 2.32-2.37 ms at 6 / 5; the panorama 2.23 / 2.22 / 2.31); MODE 21 at 5, as the renderer (config 4's
//   scene 12.2-12.3 vs 15.8-16.1 / 17.9-18.3 ms at 6 / 7, whose builds spill).  MODE 17 general has no benchmark scene:
//   it follows the lean form.
//  rt_sample_pixels (profiles/adaptive_timing.txt, 16.6 M six-bounce samples, 8 a pixel): the lean MODE 17 at 7, a tie with 6
//   inside the spread (config 2's scene 16.6 vs 16.7 / 17.3 ms at 6 / 5); MODE 21 at 5 (config 4's scene 92 vs 128 / 139 ms at
//   6 / 7): rt_radiance's choices.
static int batch_waves(int asked, const Variant& v, bool any_hit) {
    if (asked) return asked;
    return !(v.mode & rtfast::TREE_BIT) ? 7 : any_hit ? 6 : 5;
}

// Ray queries: the query kernel (rt_query.hip).
extern "C" int rt_trace_rays(const rt_trace_params* p, const GPUScene* scene, void* stream) {
    const char* const who = "rt_trace_rays";
    if (!p) return refuse(who, "null params");
    if (!scene) return refuse(who, "null scene");
    if (!p->hits) return refuse(who, "null hits");
    if (p->flags != 0) return refuse(who, "flags must be 0");
    if (waves_refused(who, p->waves_per_simd)) return 1;
    const bool camera = p->rays == nullptr;
    if (camera && (p->width <= 0 || p->height <= 0)) return refuse(who, "camera mode needs width, height > 0");
    const int64_t count = camera ? (int64_t)p->width * p->height : p->count;
    if (count_refused(who, count, "rays") || misaligned(who, "rays and hits", 16, {p->rays, p->hits})) return 1;
    if (count == 0) return 0;

    QueryArgs q;
    Variant v;
    if (query_scene(who, scene, &q, &v) != 0) return 1;
    if (!camera && too_small(who, "rays", p->rays, (size_t)count * sizeof(rt_ray))) return 1;
    if (too_small(who, "hits", p->hits, (size_t)count * sizeof(rt_hit))) return 1;
    q.rays = p->rays;
    q.hits = p->hits;
    q.count = count;
    q.width = camera ? p->width : 1, q.height = camera ? p->height : 1;
    const int w = batch_waves(p->waves_per_simd, v, false);
    return check(launch_query(v.stack, v.mode, w, q, (hipStream_t)stream), "query_kernel launch");
}

// Occlusion queries: the any-hit kernel (rt_occlude.hip) in rt_trace_rays' variant.
extern "C" int rt_occluded(const rt_occlusion_params* p, const GPUScene* scene, void* stream) {
    const char* const who = "rt_occluded";
    if (!p) return refuse(who, "null params");
    if (!scene) return refuse(who, "null scene");
    if (!p->occluded) return refuse(who, "null occluded");
    if (!p->rays) return refuse(who, "null rays (there is no camera mode)");
    if (p->flags != 0) return refuse(who, "flags must be 0");
    if (waves_refused(who, p->waves_per_simd) || count_refused(who, p->count, "rays") || misaligned(who, "rays", 16, {p->rays}))
        return 1;
    if (p->count == 0) return 0;

    OcclusionArgs a;
    Variant v;
    if (query_scene(who, scene, &a.q, &v) != 0) return 1;
    if (too_small(who, "rays", p->rays, (size_t)p->count * sizeof(rt_ray))) return 1;
    if (too_small(who, "occluded", p->occluded, (size_t)p->count)) return 1;
    a.q.rays = p->rays;
    a.q.count = p->count;
    a.occluded = p->occluded;
    const int w = batch_waves(p->waves_per_simd, v, true);
    return check(launch_occlusion(v.stack, v.mode, w, a, (hipStream_t)stream), "occlusion_kernel launch");
}

// The scene of a walk launch (rt_closest.hip, rt_hits.hip) from query_scene's result.  The walk needs both halves of a
// leaf tree: without `ltris` there is none.
static WalkScene walk_scene(const QueryArgs& q) {
    return {q.spheres, q.sphere_count, q.scene_fast, q.faces, q.vertices, q.nodes, q.tris, q.ltris ? q.tree : nullptr, q.ltris};
}

// The occupancy of rt_closest_point when the call asks for none, measured (profiles/closest_timing.txt, 2^20 points):
// 7 waves per SIMD, a tie with 6 and 5 inside the spread on every batch -- config 2's scene, points uniform in the box,
// radius inf: 7.23 vs 7.24 / 7.25 ms at 6 / 5; on the surface 5.72 vs 5.71 / 5.69; far outside 2.17 vs 2.23 / 2.25;
// config 4's scene (leaf tree) 35.8 vs 35.6 / 35.9, 75.2 vs 73.9 / 73.7 and 9.44 vs 9.50 / 9.66 ms.  The tie is no
// surprise: the kernel takes 60 registers and spills nothing (profiles/closest_resources.txt), so the three builds are
// one code and each fits 8 waves; 7 stays the default, as for the ray calls on scenes without leaf trees.
static int closest_waves(int asked) { return asked ? asked : 7; }

// Closest-point queries: the closest-point kernel (rt_closest.hip) on the scene half of a ray-batch launch.
extern "C" int rt_closest_point(const rt_closest_params* p, const GPUScene* scene, void* stream) {
    const char* const who = "rt_closest_point";
    if (!p) return refuse(who, "null params");
    if (!scene) return refuse(who, "null scene");
    if (!p->nearest) return refuse(who, "null nearest");
    if (!p->points) return refuse(who, "null points");
    if (p->flags != 0) return refuse(who, "flags must be 0");
    if (waves_refused(who, p->waves_per_simd) || count_refused(who, p->count, "points") ||
        misaligned(who, "points and nearest", 16, {p->points, p->nearest}))
        return 1;
    if (p->count == 0) return 0;

    QueryArgs q;
    Variant v;
    if (query_scene(who, scene, &q, &v) != 0) return 1;
    const size_t n = (size_t)p->count;
    if (too_small(who, "points", p->points, n * sizeof(rt_point)) || too_small(who, "nearest", p->nearest, n * sizeof(rt_nearest)))
        return 1;
    // a lane reads its point when it starts: a record written over a later point would change it
    if (overlap(p->nearest, n * sizeof(rt_nearest), p->points, n * sizeof(rt_point))) return refuse(who, "nearest overlaps points");
    const ClosestArgs a{p->points, p->nearest, p->count, walk_scene(q)};
    return check(launch_closest(v.stack, closest_waves(p->waves_per_simd), a, (hipStream_t)stream), "closest_kernel launch");
}

// The occupancy of rt_trace_hits when the call asks for none, from the compiler's figures (profiles/hits_resources.txt):
// the 4-slot list takes 71 registers and spills nothing, so its three builds are one code and run at 7 like the other
// ray calls; the 8- and 16-slot lists spill least at 5 (0 and 29 vector registers, against 26 and 171 at 7).
// tools/hits_timing.py measures the choice (profiles/hits_timing.txt).
static int hits_waves(int asked, int max_hits) { return asked ? asked : max_hits <= 4 ? 7 : 5; }

// Ordered hits: the hits kernel (rt_hits.hip) on the scene half of a ray-batch launch, the device-free checks in the
// order the header states.
extern "C" int rt_trace_hits(const rt_hits_params* p, const GPUScene* scene, void* stream) {
    const char* const who = "rt_trace_hits";
    if (!p) return refuse(who, "null params");
    if (!scene) return refuse(who, "null scene");
    if (!p->hits) return refuse(who, "null hits");
    const uint32_t known = RT_HITS_CULL_BACK | RT_HITS_CULL_FRONT | RT_HITS_COUNT_ALL, both = RT_HITS_CULL_BACK | RT_HITS_CULL_FRONT;
    if (p->flags & ~known) return refuse(who, "unknown flag bits");
    if ((p->flags & both) == both) return refuse(who, "RT_HITS_CULL_BACK and RT_HITS_CULL_FRONT exclude each other");
    if (p->reserved != 0) return refuse(who, "reserved must be 0");
    if (waves_refused(who, p->waves_per_simd)) return 1;
    if (p->max_hits < 1 || p->max_hits > RT_HITS_MAX) return refuse(who, "max_hits must be 1..16");
    const bool camera = p->rays == nullptr;
    if (camera && (p->width <= 0 || p->height <= 0)) return refuse(who, "camera mode needs width, height > 0");
    const int64_t count = camera ? (int64_t)p->width * p->height : p->count;
    if (count_refused(who, count, "rays") || misaligned(who, "rays and hits", 16, {p->rays, p->hits}) ||
        misaligned(who, "counts", 4, {p->counts}))
        return 1;
    if (count == 0) return 0;

    QueryArgs q;
    Variant v;
    if (query_scene(who, scene, &q, &v) != 0) return 1;
    const size_t n = (size_t)count, hit_bytes = n * (size_t)p->max_hits * sizeof(rt_hit);
    if (!camera && too_small(who, "rays", p->rays, n * sizeof(rt_ray))) return 1;
    if (too_small(who, "hits", p->hits, hit_bytes)) return 1;
    if (p->counts && too_small(who, "counts", p->counts, n * 4)) return 1;
    // a lane reads its ray when it starts: a row or a count written over a later ray would change it
    if (overlap(p->hits, hit_bytes, p->rays, n * sizeof(rt_ray))) return refuse(who, "hits overlaps rays");
    if (overlap(p->counts, n * 4, p->rays, n * sizeof(rt_ray))) return refuse(who, "counts overlaps rays");
    if (overlap(p->counts, n * 4, p->hits, hit_bytes)) return refuse(who, "counts overlaps hits");
    const HitsArgs a{p->rays, p->hits, p->counts, count, camera ? p->width : 1, camera ? p->height : 1, q.cam,
                     p->max_hits, p->flags, walk_scene(q)};
    return check(launch_hits(v.stack, hits_waves(p->waves_per_simd, p->max_hits), a, (hipStream_t)stream), "hits_kernel launch");
}

// The fused AO kernel keeps its samples in registers: no scratch.
extern "C" size_t rt_ao_scratch_bytes(int, int, int) { return 0; }

extern "C" int rt_ao(const rt_ao_params* p, const GPUScene* scene, void* stream) {
    const char* const who = "rt_ao";
    if (!p) return refuse(who, "null params");
    if (!scene) return refuse(who, "null scene");
    if (!p->hits) return refuse(who, "null hits");
    if (!p->directions) return refuse(who, "null directions");
    if (!p->ao) return refuse(who, "null ao");
    if (p->flags != 0) return refuse(who, "flags must be 0");
    if (waves_refused(who, p->waves_per_simd)) return 1;
    if (p->width <= 0 || p->height <= 0) return refuse(who, "width and height must be > 0");
    const int64_t count = (int64_t)p->width * p->height;
    if (count > (int64_t)1 << 30) return refuse(who, "more than 2^30 pixels");
    if (p->direction_count < 1 || p->direction_count > 65536) return refuse(who, "direction_count must be 1..65536");
    if (p->samples < 1 || p->samples > 64) return refuse(who, "samples must be 1..64");
    if (!(p->radius > 0.0f)) return refuse(who, "radius must be > 0 and not NaN");
    if (!(p->bias >= 0.0f) || !(p->bias <= FLT_MAX)) return refuse(who, "bias must be >= 0 and finite");
    if (misaligned(who, "hits and directions", 16, {p->hits, p->directions}) || misaligned(who, "ao", 4, {p->ao})) return 1;
    const size_t need = rt_ao_scratch_bytes(p->width, p->height, p->samples);
    if (need && (!p->scratch || p->scratch_bytes < need)) return refuse(who, "scratch too small (rt_ao_scratch_bytes)");

    AoArgs a;
    Variant v;
    if (query_scene(who, scene, &a.q, &v) != 0) return 1;
    if (too_small(who, "hits", p->hits, (size_t)count * sizeof(rt_hit))) return 1;
    if (too_small(who, "directions", p->directions, (size_t)p->direction_count * 16)) return 1;
    if (too_small(who, "ao", p->ao, (size_t)count * 4)) return 1;
    a.q.hits = const_cast<rt_hit*>(p->hits);  // read only (rt_render.h AoArgs)
    a.q.count = count;
    a.directions = (const float4*)p->directions;
    a.direction_count = p->direction_count, a.samples = p->samples;
    a.radius = p->radius, a.bias = p->bias;
    a.ao = p->ao;
    const int w = batch_waves(p->waves_per_simd, v, true);
    return check(launch_ao(v.stack, v.mode, w, a, (hipStream_t)stream), "ao_kernel launch");
}

// Radiance along the caller's rays: the radiance kernel (rt_radiance.hip) in rt_trace_rays' variant, on a RenderArgs
// filled as rt_render fills it for a scene of its own.
extern "C" int rt_radiance(const rt_radiance_params* p, const GPUScene* scene, void* stream) {
    const char* const who = "rt_radiance";
    if (!p) return refuse(who, "null params");
    if (!scene) return refuse(who, "null scene");
    if (!p->rays) return refuse(who, "null rays (there is no camera mode)");
    if (!p->rng) return refuse(who, "null rng");
    if (!p->radiance) return refuse(who, "null radiance");
    if (p->flags != 0) return refuse(who, "flags must be 0");
    if (waves_refused(who, p->waves_per_simd) || count_refused(who, p->count, "rays")) return 1;
    if (p->bounces < 0) return refuse(who, "bounces must be >= 0");
    if (p->samples < 1 || p->samples > (1 << 24)) return refuse(who, "samples must be 1..2^24");
    if (misaligned(who, "rays and radiance", 16, {p->rays, p->radiance}) || misaligned(who, "rng", 8, {p->rng})) return 1;
    if (p->count == 0) return 0;

    RadianceArgs a;
    std::memset(&a, 0, sizeof(a));
    Variant v;
    if (query_scene(who, scene, &a.r, &v) != 0) return 1;
    if (!scene->gpu_materials) return refuse(who, "the scene has no materials");
    a.r.materials = scene->gpu_materials;
    if (fill_sky(who, scene, &a.r) != 0) return 1;
    a.r.bounces = p->bounces;
    const size_t n = (size_t)p->count;
    if (too_small(who, "rays", p->rays, n * sizeof(rt_ray)) || too_small(who, "rng", p->rng, n * sizeof(rt_rng_state)) ||
        too_small(who, "radiance", p->radiance, n * 16))
        return 1;
    // a lane re-reads its ray per sample and its state at the start: an output row written over either would change them
    if (overlap(p->radiance, n * 16, p->rays, n * sizeof(rt_ray))) return refuse(who, "radiance overlaps rays");
    if (overlap(p->radiance, n * 16, p->rng, n * sizeof(rt_rng_state))) return refuse(who, "radiance overlaps rng");
    a.rays = p->rays;
    a.rng = p->rng;
    a.radiance = (float4*)p->radiance;
    a.count = p->count;
    a.samples = p->samples;
    const int w = batch_waves(p->waves_per_simd, v, false);
    return check(launch_radiance(v.stack, v.mode, w, a, (hipStream_t)stream), "radiance_kernel launch");
}

// More samples for listed pixels, the device-free checks in the order the header states: the adaptive kernel
// (rt_adaptive.hip) in rt_trace_rays' variant, on a RenderArgs filled as rt_radiance's plus the camera, the frame, the
// states and the accumulator.
extern "C" int rt_sample_pixels(const rt_sample_pixels_params* p, const GPUScene* scene, void* stream) {
    const char* const who = "rt_sample_pixels";
    if (!p) return refuse(who, "null params");
    if (!scene) return refuse(who, "null scene");
    if (!p->samples) return refuse(who, "null samples");
    if (!p->rng) return refuse(who, "null rng");
    if (!p->accum) return refuse(who, "null accum");
    if (p->flags != 0) return refuse(who, "flags must be 0");
    if (p->reserved != 0) return refuse(who, "reserved must be 0");
    if (waves_refused(who, p->waves_per_simd) || count_refused(who, p->count, "rays")) return 1;
    if (p->width <= 0 || p->height <= 0) return refuse(who, "width and height must be > 0");
    const int64_t pixel_count = (int64_t)p->width * p->height;
    if (pixel_count > (int64_t)1 << 30) return refuse(who, "more than 2^30 pixels");
    if (!p->pixels && p->count != pixel_count) return refuse(who, "null pixels needs count == width * height");
    if (p->bounces < 0) return refuse(who, "bounces must be >= 0");
    const size_t row = (size_t)p->width * 16;
    if (p->accum_pitch < row) return refuse(who, "accum_pitch smaller than width * 16");
    if (p->accum_pitch & 15u) return refuse(who, "accum_pitch must be a multiple of 16");
    if (misaligned(who, "accum", 16, {p->accum}) || misaligned(who, "rng and moments", 8, {p->rng, p->moments}) ||
        misaligned(who, "pixels", 4, {p->pixels}) || misaligned(who, "samples", 2, {p->samples}))
        return 1;
    if (p->count == 0) return 0;

    SampleArgs a;
    std::memset(&a, 0, sizeof(a));
    Variant v;
    if (query_scene(who, scene, &a.r, &v) != 0) return 1;
    if (!scene->gpu_materials) return refuse(who, "the scene has no materials");
    a.r.materials = scene->gpu_materials;
    if (fill_sky(who, scene, &a.r) != 0) return 1;
    const size_t n = (size_t)p->count, px = (size_t)pixel_count;
    const size_t accum_bytes = (size_t)(p->height - 1) * p->accum_pitch + row;
    if ((p->pixels && too_small(who, "pixels", p->pixels, n * 4)) || too_small(who, "samples", p->samples, n * 2) ||
        too_small(who, "rng", p->rng, px * sizeof(rt_rng_state)) || too_small(who, "accum", p->accum, accum_bytes) ||
        (p->moments && too_small(who, "moments", p->moments, px * 8)))
        return 1;
    // a lane re-reads its accumulator per sample: a row written over its state, its moments or the list would change them
    if (overlap(p->accum, accum_bytes, p->rng, px * sizeof(rt_rng_state))) return refuse(who, "accum overlaps rng");
    if (overlap(p->accum, accum_bytes, p->moments, px * 8)) return refuse(who, "accum overlaps moments");
    if (overlap(p->accum, accum_bytes, p->pixels, n * 4)) return refuse(who, "accum overlaps pixels");
    if (overlap(p->accum, accum_bytes, p->samples, n * 2)) return refuse(who, "accum overlaps samples");
    a.r.cam = scene->camera;
    a.r.width = p->width, a.r.height = p->height;
    a.r.rng = p->rng;
    a.r.surface = (char*)p->accum;
    a.r.pitch = p->accum_pitch;
    a.r.bounces = p->bounces;
    a.pixels = p->pixels;
    a.samples = p->samples;
    a.moments = (float2*)p->moments;
    a.count = p->count;
    const int w = batch_waves(p->waves_per_simd, v, false);
    return check(launch_sample_pixels(v.stack, v.mode, w, a, (hipStream_t)stream), "sample_kernel launch");
}
