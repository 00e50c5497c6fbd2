/*
 * rt_abi.h -- the C-ABI drop-in boundary of the MI355X ray tracer (librt_hip.so).
 *
 * Everything here is plain C: POD structs, raw pointers, sizes, integer status codes.
 * No HIP, torch or C++ types appear in a signature, so the same header serves a C++ host
 * (the reference's Scene.cpp / BVH.cpp / RayTracing.cpp), Python ctypes and any other FFI.
 *
 * Reference interfaces replaced (paths relative to the reference repository root):
 *   raytracing_process ...... RayTracing/main_raytracing.cu:202-220 (declared by the caller
 *                             at RayTracing/RayTracing.cpp:12)
 *   init_rng ................ RayTracing/Random.cu:10-13 (caller RayTracing/RayTracing.cpp:13,220)
 *   rt_malloc / rt_free ..... CUDA::DeviceMemory, utils/CUDAHelper.h:114-156
 *   rt_memcpy_* ............. CUDA_CHECK(cudaMemcpy(...)) at RayTracing/Scene.cpp:195-230 and
 *                             RayTracing/RayTracing.cpp:233
 *   rt_cubemap_* ............ CUDA::Texture + Loader::LoadDDSFromFile,
 *                             utils/CUDATexture.cpp:112-172,187-249
 *   GPU data contract ....... RayTracing/GPUScene.h:11-96, RayTracing/Math.h:25-37
 *
 * Error behaviour: every rt_* function returns 0 on success and a nonzero code on
 * failure, with a message available from rt_last_error().  The two reference entry points
 * keep the reference's void signature; like main_raytracing.cu:215-219 they print a launch
 * failure, and additionally record it for rt_last_error().
 */
#ifndef RT_ABI_H
#define RT_ABI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__cplusplus)
#define RT_ALIGNAS(n) alignas(n)
#else
#define RT_ALIGNAS(n) _Alignas(n)
#endif

/* ---------------------------------------------------------------------------------------
 * Data contract.  Field order, sizes and alignment are those of the reference structs
 * (GPUScene.h), so buffers built by the reference's Scene::Upload are consumed unchanged.
 * ------------------------------------------------------------------------------------- */

/* GPUScene.h:11-23.  60 bytes. */
typedef struct GPUCamera {
    float origin[3];
    float viewport_worldspace_size[2];
    float aspect;
    float horizontal[3];
    float vertical[3];
    float lower_left_corner[3];
} GPUCamera;

/* GPUScene.h:25-30.  32 bytes. */
typedef struct GPUVertex {
    RT_ALIGNAS(16) float position[3];
    float normal[3];
    float uv[2];
} GPUVertex;

/* GPUScene.h:32-38.  16 bytes.  NOTE the reference's field order v0, v2, v1: the aggregate
 * initialiser GPUFace{i0, i0+1, i0+2} in Scene::AddTriangle (Scene.cpp:65) therefore lands
 * as v0=i0, v2=i0+1, v1=i0+2, and the kernel reads v1/v2 by name. */
typedef struct GPUFace {
    RT_ALIGNAS(16) uint32_t v0;
    uint32_t v2;
    uint32_t v1;
    uint32_t material;
} GPUFace;

/* GPUScene.h:40-50 + Math.h:25-37 (AABB).  32 bytes.  Leaf iff prim_count > 0; an inner
 * node's children are at first_index and first_index + 1. */
typedef struct GPUBVHNode {
    RT_ALIGNAS(32) float bmin[3];
    float bmax[3];
    uint32_t first_index;
    uint32_t prim_count;
} GPUBVHNode;

/* GPUScene.h:59-64.  32 bytes. */
typedef struct GeometrySphere {
    RT_ALIGNAS(16) float position[3];
    float radius;
    int32_t material;
} GeometrySphere;

/* GPUScene.h:66-74.  64 bytes. */
typedef struct GPUMaterial {
    RT_ALIGNAS(16) float albedo[4];
    float emissive[4];
    float specular[4];
    float roughness;
    float specular_percent;
    float IOR;
} GPUMaterial;

/* GPUScene.h:76-96.  136 bytes.  All pointers are non-owning device pointers.
 * rng_state points at a caller-owned array of rt_rng_state (48 B each, the size of the
 * reference's curandState), one per pixel, indexed y*width + x (GPUScene.h:95).
 * environment_cubemap_tex is a handle from rt_cubemap_create (0 = black sky). */
typedef struct GPUScene {
    const GeometrySphere* gpu_spheres;
    const GPUMaterial* gpu_materials;
    const GPUBVHNode* gpu_bvh_nodes;
    const uint32_t* gpu_bvh_face_indices;
    const GPUVertex* gpu_vertices;
    const GPUFace* gpu_faces;
    int32_t sphere_count;
    int32_t material_count;
    void* rng_state;
    uint64_t environment_cubemap_tex;
    GPUCamera camera;
} GPUScene;

/* Per-pixel XORWOW state.  Same size and the same first 24 bytes as the reference's
 * curandStateXORWOW (d, v[5]); the Box-Muller fields are never used by this path. */
typedef struct rt_rng_state {
    RT_ALIGNAS(8) uint32_t d;
    uint32_t v[5];
    uint32_t unused[6];
} rt_rng_state;

#if defined(__cplusplus)
static_assert(sizeof(GPUCamera) == 60, "GPUCamera");
static_assert(sizeof(GPUVertex) == 32, "GPUVertex");
static_assert(sizeof(GPUFace) == 16 && offsetof(GPUFace, v2) == 4 && offsetof(GPUFace, v1) == 8, "GPUFace");
static_assert(sizeof(GPUBVHNode) == 32 && offsetof(GPUBVHNode, first_index) == 24, "GPUBVHNode");
static_assert(sizeof(GeometrySphere) == 32, "GeometrySphere");
static_assert(sizeof(GPUMaterial) == 64 && offsetof(GPUMaterial, roughness) == 48, "GPUMaterial");
static_assert(sizeof(GPUScene) == 136 && offsetof(GPUScene, sphere_count) == 48 &&
              offsetof(GPUScene, rng_state) == 56 && offsetof(GPUScene, environment_cubemap_tex) == 64 &&
              offsetof(GPUScene, camera) == 72, "GPUScene");
static_assert(sizeof(rt_rng_state) == 48, "rt_rng_state");
#endif

/* ---------------------------------------------------------------------------------------
 * Reference entry points (exact signatures).
 * ------------------------------------------------------------------------------------- */

/* main_raytracing.cu:202.  Renders one progressive frame into the pitched float4 surface:
 * reference constants sample_count = 5 (main_raytracing.cu:166-170, Release) and
 * num_bounces = 6 (:115), on the null stream, asynchronous. */
void raytracing_process(void* surface, void* surface_last_frame, int width, int height, size_t pitch,
                        int frame_index, GPUScene* scene);

/* Random.cu:10.  curand_init(seed, tid, 0) for tid in [0, count*size): XORWOW seeding
 * plus a skip-ahead of tid * 2^67 draws.  Null stream, asynchronous. */
void init_rng(uint32_t thread_block_count, uint32_t thread_block_size, void* rngStates, unsigned int seed);

/* ---------------------------------------------------------------------------------------
 * Extended entry points (runtime parameters the reference hard-codes, streams, shards).
 * ------------------------------------------------------------------------------------- */

typedef struct rt_render_params {
    void* surface;                 /* pitched float4 output (or NULL when out_shard is set) */
    const void* surface_last_frame;/* pitched float4 history, same pitch */
    int32_t width, height;
    uint64_t pitch;                /* bytes per row of both surfaces */
    int32_t frame_index;
    int32_t spp;                   /* reference: 5 (Release) / 1 (Debug) */
    int32_t bounces;               /* reference: 6 */
    int32_t shard_index;           /* tile sharding: this rank renders 16x16 tiles */
    int32_t shard_count;           /*   t = shard_index + k * shard_count (row-major tiles) */
    int32_t flags;                 /* RT_RENDER_* */
    void* out_shard;               /* if non-NULL: compact [k][16*16] float4 shard output */
    uint64_t* stats;               /* RT_RENDER_STATS: RT_STAT_COUNT uint64 counters (zeroed by caller) */
    uint64_t* segment_counter;     /* optional: += ray segments traced (GetRayHit calls) */
    /* Explicit tile list (cost-aware plans, rt_shard_plan): list entry k renders the row-major
     * 16x16 tile tile_list[k] (DEVICE int32 array, tile_count entries, < 0 = padding) instead of
     * the round-robin tile shard_index + k * shard_count.  NULL = round-robin. */
    const int32_t* tile_list;
    int64_t tile_count;
    /* Optional DEVICE uint64 [entries][4]: elapsed ticks of the device's constant 100 MHz clock
     * (s_memrealtime) of each 8x8 sub-tile wave of the production tracer (the cost input of
     * rt_shard_plan). */
    uint64_t* wave_clock;
    uint32_t tune;                 /* diagnostic A/B knobs (tools/); 0 = the production path */
    /* Optional lane map (production tracer only): wave w, lane l renders slot lane_slots[64w + l]
     * (slot k*256 + t = thread t of list entry k, as in the layout rule below; < 0 = idle lane)
     * instead of slot 64w + l.  lane_slot_count (a multiple of 64) sets the number of waves.  Any
     * permutation renders the same pixels bit for bit; rt_lane_plan builds one that isolates the
     * costliest pixels (the serial tail of a strong-scaled frame). */
    const int32_t* lane_slots;
    int64_t lane_slot_count;
    /* Optional DEVICE uint32 [slots]: per-pixel work of the frame, counted deterministically by the
     * timing variant of the production tracer (its own traversal steps + 3 per big-leaf visit + 1
     * per segment; no clock involved) -- the cost input of rt_lane_plan. */
    uint32_t* lane_cost;
    /* With a lane map: the first priority_waves waves (rt_lane_plan's long waves) issue at raised
     * wave priority, so the frame's serial tail does not queue behind the short waves. */
    int64_t priority_waves;
    /* Refill (production tracer; needs librt_hip_exp.so, rt_experimental_loaded): 0 = off.  n in [1, 64]: the launch holds only as many waves as
     * the GPU runs at once; the rest of the lane order (the lane map, or the sub-tile waves) is a
     * queue, and a wave takes the next n entries as soon as n of its lanes have finished their
     * pixels (waves that start less than half full keep their lanes to themselves). */
    int32_t refill_lanes;
    /* Occupancy of the production tracer: 0 = the default (5 waves per SIMD, 96 registers);
     * 6 = 6 waves per SIMD (80 registers, more spills), 7 = 7 (72 registers) -- faster on some
     * scenes (config 2: 16.2 / 15.3 vs 16.9 ms), slower on others (config 4: 95 vs 90 ms at 6);
     * bench.py picks it per configuration by timing one untimed probe frame of each.  1-4 = the
     * 5-wave build with its residency capped at that many waves per SIMD by dynamic LDS (each
     * wave reserves 160 KB / (4 x cap) of its CU's LDS): fewer co-resident waves for the
     * latency-bound long waves of a strong-scaled shard.  Any other value is an error. */
    int32_t waves_per_simd;
    /* Lone pixels (production tracer; rt_lone.hip, needs librt_hip_exp.so): DEVICE int32 slots (the
     * lane_slots numbering) that the lone-pixel kernel renders one per wave -- all 64 lanes on the
     * pixel's one ray, the BVH read as treelets -- concurrently with the production kernel on a second
     * stream joined back into `stream`.  Requires lane_slots, which must not hold these slots
     * (rt_lone_plan picks them and marks them for rt_lane_plan): a slot in both lists is rendered twice
     * at the same time into the same RNG state and pixel -- UNDEFINED results.  RT_RENDER_VALIDATE
     * checks this (and slot ranges) before launching.  Bit-identical pixels either way; it shortens
     * the chains of a strong-scaled frame's costliest pixels.  lone_count 0 = none. */
    const int32_t* lone_slots;
    int64_t lone_count;
} rt_render_params;

/* Layout rule: with out_shard set, RNG state s and output s are compact in list order
 * (state/slot k*256 + t for thread t of list entry k); without it, RNG states are indexed
 * y*width + x (the reference's layout) and the output goes to the pitched surface, whatever the
 * tile order. */

#define RT_RENDER_STATS 1          /* count traversal work (slower kernel variant) */
#define RT_RENDER_TRACER_REF 2     /* force the reference-layout tracer (A/B, tests) */
#define RT_RENDER_TRACER_FLAT 4    /* force the exact-division flat tracer (A/B, tests) */
#define RT_RENDER_TRACER_WAVEFRONT 8 /* wavefront tracer (needs librt_hip_exp.so): a shade launch and a
                                        persistent trace launch per segment generation, rays refilled
                                        lane by lane (same results; rt_scene_upload scenes, no
                                        statistics / lane_cost / wave_clock / refill / lone frames) */
#define RT_RENDER_VALIDATE 16      /* debug: before launching, check on the device that lone_slots and
                                      lane_slots are disjoint (synchronises; an error if they are not) */

enum {
    RT_STAT_SEGMENTS = 0,   /* GetRayHit calls */
    RT_STAT_NODES = 1,      /* BVH nodes popped (AABB tests) */
    RT_STAT_TRI_TESTS = 2,  /* ray/triangle tests */
    RT_STAT_TRI_ACCEPTS = 3,/* triangle hits accepted as the new closest */
    RT_STAT_SPHERE_ACCEPTS = 4,
    RT_STAT_HITS = 5,       /* segments that hit something */
    RT_STAT_MISSES = 6,     /* segments that sampled the sky */
    /* SIMD-efficiency counters of the fast kernel (wave-level iterations, active lanes) */
    RT_STAT_WAVE_SMALL_ITERS = 8,   /* traversal steps (inner nodes / small leaves) */
    RT_STAT_LANE_SMALL = 9,
    RT_STAT_WAVE_BIG_TRIS = 10,     /* big-leaf triangle iterations */
    RT_STAT_LANE_BIG_TRIS = 11,
    RT_STAT_WAVE_SEGMENT_ITERS = 12,/* segment-loop iterations */
    RT_STAT_LANE_SEGMENTS = 13,
    RT_STAT_TREE_NODES = 14,        /* leaf-tree nodes visited (leaftree.h; statistics frames with RT_TUNE bit 7) */
    RT_STAT_TREE_TRI_TESTS = 15,    /* triangle tests run inside leaf trees */
    RT_STAT_CYCLES_SMALL = 16,      /* RT_TUNE bit 8 timing frames: wave clock cycles in small steps */
    RT_STAT_CYCLES_BIG = 17,        /* ... in big-leaf rounds */
    RT_STAT_CYCLES_TOTAL = 18,      /* ... in the whole kernel */
    RT_STAT_ROUNDS_COOP = 19,       /* cooperative big-leaf rounds */
    RT_STAT_ROUNDS_SHARED = 20,     /* shared-leaf (pair / scalar-load) rounds */
    RT_STAT_COOP_RAYS = 21,         /* rays run through cooperative rounds */
    RT_STAT_CYCLES_TREE_CUT = 7,    /* timing frames, cooperative leaf-tree walk: whole walk (all rounds) */
    RT_STAT_CYCLES_TREE_CLUSTERS = 22, /* ... cluster screening rounds */
    RT_STAT_CYCLES_TREE_TRIS = 23,  /* ... triangle rounds */
    /* timing frames: the production kernel's own big-leaf work with twin records (mirror.h quads / units) */
    RT_STAT_BIG_TESTS = 24,         /* glm tests of a big leaf's unit triangles (quad halves, units), summed over rays */
    RT_STAT_TWIN_DECIDED = 25,      /* twins rejected from their partner's values without a test (rt_fast.h twin_rejected) */
    RT_STAT_TWIN_TESTS = 26,        /* twins tested themselves (too close to call, or a hit) */
    RT_STAT_WAVE_BIG_ITERS = 27,    /* wave iterations of those tests (shared-leaf quads, cooperative unit chunks) */
    /* timing frames of the leaf-tree kernels: deferred big leaves (rt_fast.h defer_leaf) */
    RT_STAT_DEFER_END2 = 28,        /* guard walks (END2: the leaf re-run up to tmin of the hit's own leaf) */
    RT_STAT_DEFER_REDO = 29,        /* lanes redone from the root after END2 found a hit */
    RT_STAT_COUNT = 32
};

/* Render on `stream` (a hipStream_t, NULL = null stream).  Returns 0 or an error code.
 * A GPUScene filled by another host (the reference's own Scene::Upload) is rendered without any
 * host synchronisation: each frame's arrays are fingerprinted on the device, and the frame runs the
 * production tracer when a private mirror built from exactly those arrays is installed, the
 * reference-layout tracer otherwise, while a worker thread (re)builds the mirror in the background. */
int rt_render(const rt_render_params* params, const GPUScene* scene, void* stream);
/* Foreign scenes: block until the background mirror build started by the last rt_render of this
 * scene has finished (the next rt_render installs it).  For tests and benchmarks; 0 or an error. */
int rt_foreign_mirror_wait(const GPUScene* scene);
/* Foreign scenes, for tests: the tracer of the last frame -- 1 production (mirror matched the
 * frame's fingerprint), 0 reference layout (mismatch), -1 no mirror installed yet.  Synchronises. */
int rt_foreign_last_tracer(const GPUScene* scene);

/* 1 when librt_hip_exp.so is loaded: its constructor registers the exact alternatives kept for A/B
 * measurement (wavefront tracer, refill, lone-pixel kernel, RT_TUNE A/B kernel variants) with this
 * library; rt_render refuses frames that ask for them otherwise.  0 otherwise. */
int rt_experimental_loaded(void);

/* ---------------------------------------------------------------------------------------
 * Ray queries: "what does this ray hit?" for batches of rays, on the render kernel's own exact
 * traversal (picking, visibility tests, depth / normal / albedo images, baking).
 *
 * Ray i gets exactly what the reference's GetRayHit(origin, direction) finds
 * (main_raytracing.cu:83-109) with tmax as the initial closest distance (the renderer's own value
 * is 1e30f): nd = normalize(direction); the sphere loop with strict <; BVHRayHit in the
 * reference's right-first DFS order, the slab test on the direction as given, the primitive tests
 * on nd; a triangle accepted when 0 <= t < best.
 *
 * PRECONDITION: direction is finite and not of zero length.  The slab test takes the direction
 * unnormalised, as the reference does: a direction shorter than 1 makes box distances larger
 * than the primitives' and may cull a node early (the reference's behaviour, inherited).
 * rays and hits must be 16-byte aligned device memory; rt_ray.reserved must be 0 (it lives in
 * device memory, so the call cannot check it; the kernel does not read it).
 * ------------------------------------------------------------------------------------- */
typedef struct rt_ray {
    float origin[3];
    float tmax;
    float direction[3];
    uint32_t reserved;
} rt_ray; /* 32 B */

/* kind: 0 miss, 1 sphere, 2 triangle.  id: sphere index or face index.  bx, by: glm's barycentrics
 * (0 for spheres).  position = origin + nd * t.  normal, material: what the renderer shades with --
 * spheres (position - centre) / radius; triangles the normalised v0.normal * bx + v1.normal * by +
 * v2.normal * (1 - bx - by), flipped to face the ray (spheres are not flipped).
 * A miss -- also a hit whose accepted distance is not < tmax, the reference's NaN rule -- has
 * kind 0, t = tmax as passed and every other word 0, so whole buffers compare bytewise. */
typedef struct rt_hit {
    float t;
    uint32_t kind;
    uint32_t id;
    uint32_t material;
    float normal[3];
    float bx;
    float position[3];
    float by;
} rt_hit; /* 48 B */

typedef struct rt_trace_params {
    const rt_ray* rays;     /* DEVICE, count records; NULL = camera mode */
    int64_t count;          /* rays (ignored in camera mode); 0 returns at once; at most 2^31 */
    int32_t width, height;  /* camera mode only */
    rt_hit* hits;           /* DEVICE, one record per ray */
    uint32_t flags;         /* must be 0 */
    int32_t waves_per_simd; /* occupancy build of the query kernel: 5 / 6 / 7, or 0 = the measured default
                               (7; 5 for scenes with leaf trees, whose kernel spills at 6 and 7) */
} rt_trace_params;

#if defined(__cplusplus)
static_assert(sizeof(rt_ray) == 32 && offsetof(rt_ray, tmax) == 12 && offsetof(rt_ray, direction) == 16 &&
              offsetof(rt_ray, reserved) == 28, "rt_ray");
static_assert(sizeof(rt_hit) == 48 && offsetof(rt_hit, kind) == 4 && offsetof(rt_hit, id) == 8 &&
              offsetof(rt_hit, material) == 12 && offsetof(rt_hit, normal) == 16 && offsetof(rt_hit, bx) == 28 &&
              offsetof(rt_hit, position) == 32 && offsetof(rt_hit, by) == 44, "rt_hit");
static_assert(sizeof(rt_trace_params) == 40 && offsetof(rt_trace_params, hits) == 24 &&
              offsetof(rt_trace_params, flags) == 32, "rt_trace_params");
#endif

/* Trace a batch on `stream` (a hipStream_t, NULL = null stream): stream-ordered, no
 * synchronisation, no allocation.  Camera mode (rays == NULL) traces width * height rays from the
 * scene camera's origin through the pixel centres -- ray i is pixel (i % width, i / width),
 * direction ((llc + h * ux) + v * uy) - origin with ux = ((float)x + 0.5f) / (float)width,
 * uy = ((float)y + 0.5f) / (float)height, tmax 1e30f; set the camera with rt_scene_set_viewport
 * before rt_scene_upload.  It reads no RNG state and writes no surface.
 * The scene must have been uploaded by rt_scene_upload (whose rng_state may be NULL for a scene
 * that is only queried); a GPUScene filled by another host is rejected.  Returns 0 or an error
 * code with rt_last_error(). */
int rt_trace_rays(const rt_trace_params* params, const GPUScene* scene, void* stream);

/* ---------------------------------------------------------------------------------------
 * Occlusion queries: "does this ray hit anything before tmax?" (shadow rays, visibility between two
 * points, ambient occlusion, baking).  One byte per ray instead of a 48-byte record, and a traversal
 * that ends at the first accepted primitive where that is proven safe.
 *
 * THE CONTRACT, WITHOUT EXCEPTION: byte i equals (kind != 0) of the record rt_trace_rays writes for
 * ray i.  This holds for every ray and every scene, including the cases at the tmax gates, zero-length
 * and non-finite rays, and scenes outside the filtered range.
 *
 * Why stopping early is safe, and where it is not.  As long as nothing has been accepted, `closest` is
 * still tmax, and the slab test (tmin < closest), the leaf-tree cull and the triangle accept
 * (0 <= t < closest) are all monotone in `closest`: so a first accept of any traversal order exists
 * exactly when the reference's traversal accepts something.  That fails only where a NaN distance can be
 * accepted: the reference's `if (dist >= closest || dist < 0) continue;` lets a NaN through, after which
 * `closest` is NaN, nothing more is accepted, and the final `distance < max_distance` turns an earlier hit
 * into a miss.  So a lane stops at its first accept only inside the gate within which no NaN distance can
 * arise (the filtered range of rt_fast.h, tmax <= 1e30f, the ray's origin and the scene's root box inside
 * +-2^16: every product of the triangle test is then finite); every other lane runs rt_trace_rays' full
 * closest-hit traversal and reports kind != 0 && t < tmax.  The sphere loop runs in order and to the end
 * for every lane, as in rt_trace_rays.
 *
 * rays: as rt_trace_rays (16-byte aligned device memory; there is no camera mode).
 * ------------------------------------------------------------------------------------- */
typedef struct rt_occlusion_params {
    const rt_ray* rays;     /* DEVICE, count records, 16-byte aligned, not NULL */
    int64_t count;          /* 0 returns at once; at most 2^31 */
    uint8_t* occluded;      /* DEVICE, count bytes: 1 = occluded, 0 = not; bytes at and past count untouched */
    uint32_t flags;         /* must be 0 */
    int32_t waves_per_simd; /* occupancy build of the kernel: 5 / 6 / 7, or 0 = the measured default (7; 6 for scenes
                               with leaf trees: profiles/occlusion_timing.txt) */
} rt_occlusion_params;      /* 32 B */

#if defined(__cplusplus)
static_assert(sizeof(rt_occlusion_params) == 32 && offsetof(rt_occlusion_params, rays) == 0 &&
              offsetof(rt_occlusion_params, count) == 8 && offsetof(rt_occlusion_params, occluded) == 16 &&
              offsetof(rt_occlusion_params, flags) == 24 && offsetof(rt_occlusion_params, waves_per_simd) == 28,
              "rt_occlusion_params");
#endif

/* Occlusion of a batch on `stream` (a hipStream_t, NULL = null stream): stream-ordered, no synchronisation,
 * no allocation.  The scene rules are rt_trace_rays': uploaded by rt_scene_upload, a GPUScene filled by
 * another host is rejected.  The arguments that need no device are checked first (NULL params, scene,
 * occluded or rays; flags; waves_per_simd; count < 0 or > 2^31; alignment of rays), then the scene and
 * the buffer sizes.  Returns 0 or an error code with rt_last_error(). */
int rt_occluded(const rt_occlusion_params* params, const GPUScene* scene, void* stream);

/* ---------------------------------------------------------------------------------------
 * Ambient occlusion from the first-hit records of rt_trace_rays' camera mode: per pixel, the fraction
 * of `samples` cosine-weighted rays of length `radius` that reach nothing.  The randomness is the
 * caller's table of unit vectors (a normal plus a uniform point of the unit sphere, normalised, is a
 * cosine-weighted direction), so the library holds no trigonometry and no RNG, and the arithmetic is
 * fixed: fp32, no contraction, only + - * /, comparisons and glm's normalize (v * (1 / sqrt(dot(v, v)))),
 * so that tests/occlusion_ref.py restates it bit for bit.  For pixel index i with rec = hits[i]:
 *
 *   rec.kind == 0: ao[i] = 1.0f.  Otherwise n = rec.normal, P = rec.position, e = bias * rec.t,
 *   o = P + n * e (per component one product, then one sum), and for k = 0 .. samples - 1:
 *     j  = (((uint32_t)i * 0x9E3779B1u + (uint32_t)k * 0x85EBCA6Bu) >> 8) % direction_count
 *     s  = directions[j].xyz;  d0 = n + s;  dd = (d0.x*d0.x + d0.y*d0.y) + d0.z*d0.z
 *     d  = dd > 1e-6f ? normalize(d0) : n
 *     occ += the answer rt_occluded gives for the ray (origin o, tmax radius, direction d)
 *   ao[i] = (float)(samples - occ) / (float)samples.
 * ------------------------------------------------------------------------------------- */
typedef struct rt_ao_params {
    const rt_hit* hits;      /* DEVICE width * height records of rt_trace_rays' camera mode, 16-byte aligned */
    int32_t width, height;   /* > 0, width * height <= 2^30 */
    const float* directions; /* DEVICE float4[direction_count], 16-byte aligned: xyz a unit vector, w ignored */
    int32_t direction_count; /* 1..65536 */
    int32_t samples;         /* 1..64 */
    float radius;            /* > 0 and not NaN (+inf allowed): tmax of every AO ray */
    float bias;              /* >= 0, finite: origin offset along the normal, as a fraction of the hit distance */
    float* ao;               /* DEVICE width * height floats, record order */
    void* scratch;           /* DEVICE, rt_ao_scratch_bytes(width, height, samples); may be NULL when that is 0 */
    uint64_t scratch_bytes;
    uint32_t flags;          /* must be 0 */
    int32_t waves_per_simd;  /* 0 = the measured default, 5 / 6 / 7, as rt_occlusion_params */
} rt_ao_params;              /* 72 B */

#if defined(__cplusplus)
static_assert(sizeof(rt_ao_params) == 72 && offsetof(rt_ao_params, hits) == 0 && offsetof(rt_ao_params, width) == 8 &&
              offsetof(rt_ao_params, height) == 12 && offsetof(rt_ao_params, directions) == 16 &&
              offsetof(rt_ao_params, direction_count) == 24 && offsetof(rt_ao_params, samples) == 28 &&
              offsetof(rt_ao_params, radius) == 32 && offsetof(rt_ao_params, bias) == 36 && offsetof(rt_ao_params, ao) == 40 &&
              offsetof(rt_ao_params, scratch) == 48 && offsetof(rt_ao_params, scratch_bytes) == 56 &&
              offsetof(rt_ao_params, flags) == 64 && offsetof(rt_ao_params, waves_per_simd) == 68,
              "rt_ao_params");
#endif

/* Bytes of scratch rt_ao needs: 0 for every size (one fused kernel loops over a pixel's samples and keeps the
 * count in a register), so also 0 for a size <= 0, and monotone. */
size_t rt_ao_scratch_bytes(int width, int height, int samples);
/* AO on `stream`: stream-ordered, no synchronisation, no allocation, one kernel launch.  Every argument is
 * checked on the host before the launch; the scene rules are rt_occluded's.  Returns 0 or an error code with
 * rt_last_error(). */
int rt_ao(const rt_ao_params* params, const GPUScene* scene, void* stream);

/* ---------------------------------------------------------------------------------------
 * Radiance along caller-given rays: the renderer's path tracing without its camera and its pixel grid
 * (environment probes and panoramas, fisheye or stereo cameras, depth of field, light-map texels,
 * irradiance probes, a second view of the same scene).
 *
 * radiance[i].rgb is the fp32 mean of `samples` evaluations of the reference's
 * ray_color(origin_i, direction_i, rng_i, bounces) (main_raytracing.cu:111-158: emission, the
 * specular / diffuse lobe from 4 draws per hit, Russian roulette, the sky on a miss), accumulated in
 * sample order and divided by (float)samples as the renderer divides by its sample count; w = 1.  State i
 * is read, advances through all the samples (4 draws per hit, none on a miss) and is written back.
 *
 * There is no jitter and no camera: every sample starts along the same ray.  The direction is used as
 * given for the first segment, exactly as the renderer uses its unnormalised camera direction: the
 * traversal and the hit point take normalize(direction), the first hit's reflect() takes the vector as
 * given.  PASS UNIT DIRECTIONS unless you reproduce the reference's camera (a ray that is the renderer's
 * jittered camera ray, with the state advanced past the two jitter draws, gives the renderer's sample bit
 * for bit).  Every segment, the first included, is bounded by the renderer's 1e30f: rt_ray.tmax and
 * rt_ray.reserved are not read.  The sky is the scene's cube map under the renderer's rotation.
 *
 * bounces == 0 gives (0, 0, 0, 1) and leaves the states untouched.  A ray whose normalised direction has
 * a non-finite component (a zero, infinite or NaN direction) is not traced: it gives (0, 0, 0, 1) and its
 * state is unchanged.  A non-finite origin is traced as rt_trace_rays traces it.
 * ------------------------------------------------------------------------------------- */
typedef struct rt_radiance_params {
    const rt_ray* rays;      /* DEVICE, count records, 16-byte aligned; tmax and the reserved word are not read */
    int64_t count;           /* 0 returns at once; at most 2^31 */
    rt_rng_state* rng;       /* DEVICE, count states, 8-byte aligned: state i is read for ray i and written back */
    float* radiance;         /* DEVICE, count float4, 16-byte aligned: rgb, w = 1; rows at and past count untouched */
    int32_t bounces;         /* >= 0 */
    int32_t samples;         /* 1 .. 2^24: paths per ray, along the same ray */
    uint32_t flags;          /* must be 0 */
    int32_t waves_per_simd;  /* occupancy build of the kernel: 5 / 6 / 7, or 0 = the default
                                (profiles/radiance_timing.txt) */
} rt_radiance_params;        /* 48 B */

#if defined(__cplusplus)
static_assert(sizeof(rt_radiance_params) == 48 && offsetof(rt_radiance_params, rays) == 0 &&
              offsetof(rt_radiance_params, count) == 8 && offsetof(rt_radiance_params, rng) == 16 &&
              offsetof(rt_radiance_params, radiance) == 24 && offsetof(rt_radiance_params, bounces) == 32 &&
              offsetof(rt_radiance_params, samples) == 36 && offsetof(rt_radiance_params, flags) == 40 &&
              offsetof(rt_radiance_params, waves_per_simd) == 44,
              "rt_radiance_params");
#endif

/* Radiance of a batch on `stream` (a hipStream_t, NULL = null stream): stream-ordered, no synchronisation, no
 * allocation, one kernel launch.  The scene rules are rt_trace_rays': uploaded by rt_scene_upload (its own
 * rng_state is not used here and may be NULL), a GPUScene filled by another host is rejected.  The arguments
 * that need no device are checked first (NULL params, scene, rays, rng or radiance; flags; waves_per_simd;
 * count < 0 or > 2^31; bounces; samples; alignment), then the scene, then the buffer sizes; `radiance` may not
 * overlap `rays` or `rng`.  Returns 0 or an error code with rt_last_error(). */
int rt_radiance(const rt_radiance_params* params, const GPUScene* scene, void* stream);

/* ---------------------------------------------------------------------------------------
 * Closest-point queries: "which point of the scene's surface is nearest to p, and how far is it?" (distance
 * fields, snapping and picking without a direction, proximity effects, mesh-to-mesh distance, a conservative step
 * for sphere tracing).  The third query beside closest-hit (rt_trace_rays) and any-hit (rt_occluded).
 *
 * THE ANSWER IS DEFINED WITHOUT REFERENCE TO ANY TRAVERSAL, so it is exact, bit for bit.  With r2 = radius * radius,
 * the record of point p is the lexicographic minimum of (d2, kind, id) over all spheres (kind 1, id = the sphere's
 * index) and all faces (kind 2, id = the face's index) whose computed d2 satisfies d2 <= r2; a NaN d2 is never
 * accepted.  Then distance = sqrt(d2) (IEEE), point = q, material = the primitive's, region as below.  If nothing
 * is accepted the record is a miss: distance = radius as passed (its bits) and every other word 0.  The id rule
 * matters on every loaded mesh: each loaded face is in the scene twice, wound both ways, the twin always ties, and
 * the lower face index wins.
 *
 * The arithmetic is fp32 without contraction: + - * /, sqrt and comparisons only, in exactly this order.
 * dot(u, v) = (u.x * v.x + u.y * v.y) + u.z * v.z; vector operations are per component.
 *
 * Sphere (c, rad):
 *   v = p - c;  len = sqrt(dot(v, v));  s = len - rad;  dist = s < 0 ? -s : s;  d2 = dist * dist;
 *   q = len > 0 ? c + v * (rad / len) : c + (rad, 0, 0);  region = 0.
 *
 * Face f:  a = vertices[f.v0].position, ab = vertices[f.v1].position - a, ac = vertices[f.v2].position - a (v1 and
 * v2 read by name: GPUFace above).
 *   ap = p - a;  d1 = dot(ab, ap);  d2_ = dot(ac, ap);  aa = dot(ab, ab);  bb = dot(ab, ac);  cc = dot(ac, ac);
 *   d3 = d1 - aa;  d4 = d2_ - bb;  d5 = d1 - bb;  d6 = d2_ - cc;  ratio(n, d) = d > 0 ? n / d : 0.
 *   The first rule that holds:
 *   1. d1 <= 0 && d2_ <= 0:                                        v = 0, w = 0, region 1
 *   2. d3 >= 0 && d4 <= d3:                                        v = 1, w = 0, region 2
 *   3. vc = d1 * d4 - d3 * d2_;  vc <= 0 && d1 >= 0 && d3 <= 0:    v = ratio(d1, d1 - d3), w = 0, region 4
 *   4. d6 >= 0 && d5 <= d6:                                        v = 0, w = 1, region 3
 *   5. vb = d5 * d2_ - d1 * d6;  vb <= 0 && d2_ >= 0 && d6 <= 0:   v = 0, w = ratio(d2_, d2_ - d6), region 5
 *   6. va = d3 * d6 - d5 * d4;  va <= 0 && (d4 - d3) >= 0 && (d5 - d6) >= 0:
 *                                           w = ratio(d4 - d3, (d4 - d3) + (d5 - d6)), v = 1 - w, region 6
 *   7. otherwise: den = (va + vb) + vc;  v = ratio(vb, den);  w = ratio(vc, den);  then, as selects (a NaN stays a
 *      NaN):  v = v < 0 ? 0 : v;  v = v > 1 ? 1 : v;  w = w < 0 ? 0 : w;  w = w > 1 - v ? 1 - v : w;  region 0
 *   q = (a + ab * v) + ac * w;  e = p - q;  d2 = dot(e, e).
 * Regions: 0 the interior, 1 / 2 / 3 the vertices v0 / v1 / v2, 4 / 5 / 6 the edges v0v1 / v0v2 / v1v2.  A
 * degenerate triangle answers as its vertex or segment (ratio gives 0 for 0 / 0).
 *
 * The distance is UNSIGNED.  Signed distance is out of scope here: with every loaded face present in both windings, the
 * side of the winning triangle says nothing.  (The sign comes from counting crossings under one winding: rt_trace_hits.)
 * ------------------------------------------------------------------------------------- */
typedef struct rt_point {
    float position[3];
    float radius;  /* search radius: only primitives with d2 <= radius * radius answer; +inf = no limit; NaN = a miss */
} rt_point; /* 16 B */

typedef struct rt_nearest {
    float distance;  /* sqrt(d2); on a miss the radius as passed */
    uint32_t kind;   /* 0 miss, 1 sphere, 2 face */
    uint32_t id;     /* sphere index / face index */
    uint32_t material;
    float point[3];  /* q, the nearest point of the surface */
    uint32_t region; /* faces: 0 interior, 1-3 vertex, 4-6 edge; spheres: 0 */
} rt_nearest; /* 32 B */

typedef struct rt_closest_params {
    const rt_point* points; /* DEVICE, count records, 16-byte aligned, not NULL */
    int64_t count;          /* 0 returns at once; at most 2^31 */
    rt_nearest* nearest;    /* DEVICE, 16-byte aligned, one record per point; records at and past count untouched */
    uint32_t flags;         /* must be 0 */
    int32_t waves_per_simd; /* occupancy build of the kernel: 5 / 6 / 7, or 0 = the measured default (7; the three
                               tie: profiles/closest_timing.txt) */
} rt_closest_params;        /* 32 B */

#if defined(__cplusplus)
static_assert(sizeof(rt_point) == 16 && offsetof(rt_point, position) == 0 && offsetof(rt_point, radius) == 12, "rt_point");
static_assert(sizeof(rt_nearest) == 32 && offsetof(rt_nearest, distance) == 0 && offsetof(rt_nearest, kind) == 4 &&
              offsetof(rt_nearest, id) == 8 && offsetof(rt_nearest, material) == 12 && offsetof(rt_nearest, point) == 16 &&
              offsetof(rt_nearest, region) == 28, "rt_nearest");
static_assert(sizeof(rt_closest_params) == 32 && offsetof(rt_closest_params, points) == 0 &&
              offsetof(rt_closest_params, count) == 8 && offsetof(rt_closest_params, nearest) == 16 &&
              offsetof(rt_closest_params, flags) == 24 && offsetof(rt_closest_params, waves_per_simd) == 28,
              "rt_closest_params");
#endif

/* Nearest points of a batch on `stream` (a hipStream_t, NULL = null stream): stream-ordered, no synchronisation,
 * no allocation, one kernel launch.  The scene rules are rt_trace_rays': uploaded by rt_scene_upload, a GPUScene
 * filled by another host is rejected.  The arguments that need no device are checked first, in rt_occluded's order
 * (NULL params, scene, nearest or points; flags; waves_per_simd; count < 0 or > 2^31; alignment), then the scene
 * and the buffer sizes; `nearest` may not overlap `points`.  Every message begins with "rt_closest_point: ".
 * Returns 0 or an error code with rt_last_error(). */
int rt_closest_point(const rt_closest_params* params, const GPUScene* scene, void* stream);

/* ---------------------------------------------------------------------------------------
 * Ordered hits: "what does this ray go through, in order?" (transparency and depth peeling, x-ray and thickness
 * images, picking through a front surface, counting crossings to tell inside from outside).  The fourth query beside
 * closest-hit (rt_trace_rays), any-hit (rt_occluded) and nearest-point (rt_closest_point).  A crossing count under
 * one winding is also the sign rt_closest_point cannot give: see RT_HITS_CULL_BACK below.
 *
 * THE RULE.  rt_trace_hits is the reference's GetRayHit / BVHRayHit (main_raytracing.cu:33-109) with its single
 * closest distance replaced by a list of K = max_hits.  For ray i:
 *
 *   nd = normalize(direction);  list = empty;  total = 0.
 *   bound() = the K-th smallest accepted t once K are held, tmax before that; under RT_HITS_COUNT_ALL tmax throughout.
 *   offer(t, kind, id):  if t is NaN, t < 0 or !(t < bound()): nothing.  Otherwise total += 1; the entry goes in
 *     before the first entry whose t is strictly greater -- an equal t goes behind the ones already there, so arrival
 *     order breaks ties, as the reference's strict < does -- and the list is cut to K.
 *   Spheres k = 0 .. sphere_count - 1: where glm's sphere test hits, offer(dist, 1, k) -- one distance per sphere, as
 *     in the reference.
 *   Then BVHRayHit: right-first DFS, the slab test on the direction as given, exactly as rt_trace_rays runs it, its
 *     clause `tmin < closest` reading `tmin < bound()` at the moment the reference would pop the node.  A leaf's
 *     triangles go in leaf order; where glm's triangle test hits (on nd), offer(t, 2, face).
 *
 * Flags.  RT_HITS_CULL_BACK offers a triangle only when the test's det > 0, RT_HITS_CULL_FRONT only when det < 0
 * (det = dot(v1 - v0, cross(nd, v2 - v0)) with v1 and v2 read by name: det > 0 when the ray runs against
 * cross(v1 - v0, v2 - v0).  GPUFace's field order swaps the two, so for rt_scene_add_triangle(a, b, c) that is a ray
 * running along cross(b - a, c - a): it meets the side on which a, b, c wind clockwise); both at once are refused.  Since |det| > epsilon for every triangle the test accepts, the sign is never
 * in doubt.  Spheres are never culled.  On a loaded mesh, where every face is present in both windings (a twin has
 * det' = -det), either cull flag leaves one record per crossing.  RT_HITS_COUNT_ALL: the bound stays tmax, so every
 * hit in [0, tmax) of every node the walk visits is counted in `total` while the list keeps the first K.
 *
 * Output.  hits[i * max_hits + k] for k < the list's length is a full rt_hit: t, kind, id as offered, and the
 * attributes rt_trace_rays computes for that primitive and t (same arithmetic, same normal flip).  Every remaining row
 * of the ray is rt_trace_rays' miss record (t = tmax as passed, every other word 0), so buffers compare bytewise.
 * counts[i] (counts may be NULL) is the list's length, at most K; under RT_HITS_COUNT_ALL it is `total`, which may
 * exceed K.
 *
 * K = 1 AND THE NaN RULE.  With max_hits 1 and flags 0, row 0 equals rt_trace_rays' record bytewise for every ray
 * whose reference traversal accepts no NaN distance -- every ray inside rt_occluded's gate, for one.  The one
 * deliberate difference from the reference is that a NaN distance is never accepted (the reference lets it through,
 * after which nothing more is accepted and the ray reports a miss).  A NaN tmax gives all misses, as it does there.
 *
 * NO PREFIX GUARANTEE.  The list for K is not promised to be a prefix of the list for K' > K, nor to hold "all
 * geometric hits": the reference's fp32 box test culls against the bound, and with a direction shorter than 1 it
 * culls early -- the precondition rt_trace_rays states and this call inherits.  With unit directions the lists of
 * every scene tried were prefixes of one another; that is an observation, not a contract.
 * ------------------------------------------------------------------------------------- */
#define RT_HITS_MAX 16
enum {
    RT_HITS_CULL_BACK = 1,  /* offer a triangle only when det > 0 */
    RT_HITS_CULL_FRONT = 2, /* ... only when det < 0 */
    RT_HITS_COUNT_ALL = 4,  /* bound() = tmax throughout; counts[i] = total */
};

typedef struct rt_hits_params {
    const rt_ray* rays;     /* DEVICE, count records, 16-byte aligned; NULL = camera mode: the pixel-centre rays exactly as
                               rt_trace_rays forms them */
    int64_t count;          /* rays (ignored in camera mode); 0 returns at once; at most 2^31 */
    int32_t width, height;  /* camera mode only */
    rt_hit* hits;           /* DEVICE, count * max_hits records, 16-byte aligned; rows at and past count * max_hits untouched */
    uint32_t* counts;       /* DEVICE, count words, 4-byte aligned, or NULL: none kept */
    int32_t max_hits;       /* K: 1 .. RT_HITS_MAX */
    uint32_t flags;         /* RT_HITS_* */
    int32_t waves_per_simd; /* occupancy build of the kernel: 5 / 6 / 7, or 0 = the default (7 for max_hits <= 4, else 5:
                               profiles/hits_resources.txt) */
    uint32_t reserved;      /* must be 0 */
} rt_hits_params;           /* 56 B */

#if defined(__cplusplus)
static_assert(sizeof(rt_hits_params) == 56 && offsetof(rt_hits_params, rays) == 0 && offsetof(rt_hits_params, count) == 8 &&
              offsetof(rt_hits_params, width) == 16 && offsetof(rt_hits_params, height) == 20 &&
              offsetof(rt_hits_params, hits) == 24 && offsetof(rt_hits_params, counts) == 32 &&
              offsetof(rt_hits_params, max_hits) == 40 && offsetof(rt_hits_params, flags) == 44 &&
              offsetof(rt_hits_params, waves_per_simd) == 48 && offsetof(rt_hits_params, reserved) == 52,
              "rt_hits_params");
#endif

/* Ordered hits of a batch on `stream` (a hipStream_t, NULL = null stream): stream-ordered, no synchronisation, no
 * allocation, one kernel launch.  The scene rules are rt_trace_rays': uploaded by rt_scene_upload, a GPUScene filled
 * by another host is rejected.  The arguments that need no device are checked first, in this order: NULL params,
 * scene, hits; unknown flag bits or both cull flags; reserved; waves_per_simd; max_hits; the camera size (camera
 * mode); count < 0 or > 2^31; alignment (rays and hits 16, counts 4); count 0 returns 0.  Then the scene, then the
 * buffer sizes, then the overlaps: `hits` may not overlap `rays`, `counts` may overlap neither.  Every message begins
 * with "rt_trace_hits: ".  Returns 0 or an error code with rt_last_error(). */
int rt_trace_hits(const rt_hits_params* params, const GPUScene* scene, void* stream);

/* ---------------------------------------------------------------------------------------
 * Denoising: a viewable image from one low-sample frame and the first-hit records of its camera
 * (render -> rt_trace_rays in camera mode -> rt_denoise).  An edge-avoiding a-trous wavelet filter on
 * the frame divided by the first hit's albedo, guided by normal, position and distance; the albedo
 * is multiplied back in at the end, so texture edges are not blurred.
 *
 * The arithmetic is fixed (fp32, no contraction, IEEE division, only + - * /, fmaxf, fabsf and
 * comparisons), so that tests/denoise_ref.py restates it bit for bit.  With p a pixel, record
 * i = y * width + x of `hits`, valid(p) = hits[p].kind != 0 and dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z:
 *
 *  1. alb = materials[hits[p].material].albedo when valid(p) and material < material_count, else 1;
 *     a = fmaxf(alb, 0.015625f); c = surface.rgb / a.  Alpha passes through untouched.
 *  2. `iterations` passes s = 0.., step = 1 << s, each from the previous pass's colours.  !valid(p)
 *     keeps c_p.  Otherwise for dy = -2..2 (outer), dx = -2..2 (inner), q = (x + dx*step, y + dy*step),
 *     skipping q outside the image, !valid(q) and c_q.rgb not finite:
 *       wn = fmaxf(0, dot(n_p, n_q)), squared normal_power_log2 times;
 *       wz = fmaxf(0, 1 - fabsf(dot(n_p, pos_q - pos_p)) / (sigma_plane * t_p)), squared once
 *            (t_p == 0 gives inf or NaN and so 0);
 *       wc = 1 / (1 + dot(e, e) / (sc*sc)) with e = c_q - c_p, sc = sigma_color * 2^-s, when
 *            sigma_color > 0 and c_p.rgb is finite, else 1;
 *       w = (((h[dy+2] * h[dx+2]) * wn) * wz) * wc, h = {1/16, 1/4, 3/8, 1/4, 1/16};
 *       if w > 0: sum += c_q * w, wsum += w.
 *     out = wsum > 0 ? sum / wsum : c_p.
 *  3. result = c * a.
 *
 * Rational weights instead of exp(): a correctly rounded division is the same on every host, expf is not.
 *
 * PITFALL: give the denoised image its own surface.  Written into rt_render's surface_last_frame it would
 * feed filtered colours into the progressive accumulation.
 * ------------------------------------------------------------------------------------- */
#define RT_DENOISE_DEFAULT (-1)    /* in any of the four filter parameters: the measured default */
#define RT_DENOISE_MAX_HEIGHT 131072      /* 2^17 rows (the launch grids hold a row of blocks per 4 pixel rows) */
#define RT_DENOISE_MAX_PIXELS 1073741824  /* width * height at most 2^30 (64 GiB of scratch) */

typedef struct rt_denoise_params {
    const void* surface;           /* DEVICE pitched float4 frame, as rt_render writes it */
    uint64_t pitch;                /* bytes per row of surface: >= width * 16, a multiple of 16 */
    int32_t width, height;         /* > 0; height <= RT_DENOISE_MAX_HEIGHT, width * height <= RT_DENOISE_MAX_PIXELS */
    const rt_hit* hits;            /* DEVICE width * height records of rt_trace_rays' camera mode */
    const GPUMaterial* materials;  /* DEVICE (GPUScene.gpu_materials); may be NULL when material_count is 0 */
    int32_t material_count;
    int32_t flags;                 /* must be 0 */
    void* out;                     /* DEVICE pitched float4 result; out == surface is allowed (below) */
    uint64_t out_pitch;
    void* scratch;                 /* DEVICE, rt_denoise_scratch_bytes(width, height); contents irrelevant */
    uint64_t scratch_bytes;
    /* Filter parameters.  RT_DENOISE_DEFAULT (-1, -1.0f) selects the default (profiles/denoise_quality.txt);
     * 0 is a value of its own -- normal_power_log2 0 and sigma_color 0 switch their weight off, and
     * iterations 0 and sigma_plane 0 are errors like every other value outside the range. */
    int32_t iterations;            /* 1..6 (5): the last pass reaches 2 << (iterations - 1) pixels */
    int32_t normal_power_log2;     /* 0..8 (5): the normal weight is cos^(2^this) */
    float sigma_plane;             /* > 0 (0.03): tolerated distance from p's tangent plane, as a fraction of t_p */
    float sigma_color;             /* >= 0 (8): colour distance (albedo-divided) that halves a tap at pass 0; 0 = off */
} rt_denoise_params;

#if defined(__cplusplus)
static_assert(sizeof(rt_denoise_params) == 96 &&offsetof(rt_denoise_params, pitch) == 8 &&
              offsetof(rt_denoise_params, width) == 16 && offsetof(rt_denoise_params, hits) == 24 &&
              offsetof(rt_denoise_params, materials) == 32 && offsetof(rt_denoise_params, material_count) == 40 &&
              offsetof(rt_denoise_params, flags) == 44 && offsetof(rt_denoise_params, out) == 48 &&
              offsetof(rt_denoise_params, out_pitch) == 56 && offsetof(rt_denoise_params, scratch) == 64 &&
              offsetof(rt_denoise_params, scratch_bytes) == 72 && offsetof(rt_denoise_params, iterations) == 80 &&
              offsetof(rt_denoise_params, normal_power_log2) == 84 && offsetof(rt_denoise_params, sigma_plane) == 88 &&
              offsetof(rt_denoise_params, sigma_color) == 92,
              "rt_denoise_params");
#endif

/* Bytes of scratch rt_denoise needs for a width x height frame (64 per pixel: the packed guide and two
 * colour buffers); 0 for a size <= 0.  Monotone in both arguments. */
size_t rt_denoise_scratch_bytes(int width, int height);
/* Denoise on `stream` (a hipStream_t, NULL = null stream): stream-ordered, no synchronisation, no
 * allocation; iterations + 1 kernel launches.  Every argument is checked on the host before the first
 * launch (NULL pointers, sizes <= 0 or above the limits, pitches < width * 16, alignment, scratch too small,
 * parameters out of range, flags != 0).  out == surface is safe: the first kernel consumes the whole surface into
 * scratch, and the last pass, the only one that writes `out`, reads scratch and the material table only.
 * `out` must not overlap scratch or hits.  Returns 0 or an error code with rt_last_error(). */
int rt_denoise(const rt_denoise_params* params, void* stream);

/* ---------------------------------------------------------------------------------------
 * Temporal accumulation across camera moves: the samples of earlier frames carried into the new camera's
 * frame (render with frame_index 0 -> rt_trace_rays in camera mode -> rt_reproject -> rt_denoise).  Each
 * call's `out`, `out_history` and `hits` (with its camera) are the next call's prev_*.  The new frame's
 * first-hit points are projected into the previous camera's viewport; the previous image is gathered there
 * bilinearly from the taps whose own first-hit record agrees, and the new frame joins a running mean whose
 * length is kept per pixel.  Static geometry only: there are no motion vectors for objects.
 *
 * The arithmetic is fixed (fp32, no contraction, IEEE division, only + - * /, floorf, fminf, fabsf and
 * comparisons), so that tests/reproject_ref.py restates it bit for bit.  dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z,
 * cross(a, b) = (a.y*b.z - a.z*b.y, a.z*b.x - a.x*b.z, a.x*b.y - a.y*b.x).
 *
 * Per-frame constants (host, fp32) from prev_camera, O, H, V, L = origin, horizontal, vertical, lower_left_corner:
 *   w = L - O, N = cross(H, V), A = cross(V, w), B = cross(w, H), wn = dot(w, N).
 * For a direction d from O the previous viewport coordinates are u = dot(d, A) / dn, v = dot(d, B) / dn with
 * dn = dot(d, N): Cramer's rule on O + s d = L + u H + v V, which needs no orthogonality of H and V.
 *
 * Per pixel p = (x, y), i = y * width + x, rec = hits[i], cur = surface[p]:
 *  1. rec.kind != 0: d = rec.position - O.  rec.kind == 0: d = the current camera's pixel-centre ray direction
 *     exactly as rt_trace_rays' camera mode forms it (above), so sky is reprojected as being at infinity.
 *  2. dn = dot(d, N), s = wn / dn, fx = (dot(d, A) / dn) * (float)width - 0.5f, fy = (dot(d, B) / dn) *
 *     (float)height - 0.5f.  The projection is valid iff dn != 0 && s > 0 && fx > -1 && fx < width && fy > -1 &&
 *     fy < height (NaN fails every comparison).  Only a valid projection is converted to integers:
 *     x0 = (int)floorf(fx), ax = fx - floorf(fx), y0 and ay likewise.
 *  3. Four taps in the order (x0, y0), (x0+1, y0), (x0, y0+1), (x0+1, y0+1), weight w = wx * wy with
 *     wx = 1.0f - ax or ax, wy = 1.0f - ay or ay.  A tap q is taken iff it is inside the image, w > 0,
 *     prev_history[q] >= 1.0f, prev_surface[q].rgb is finite, and
 *       for a miss pixel: prev_hits[q].kind == 0;
 *       for a hit pixel:  prev_hits[q].kind != 0, prev_hits[q].material == rec.material,
 *                         dot(n_p, n_q) >= normal_min and fabsf(dot(n_p, pos_q - rec.position)) <= sigma_plane * rec.t.
 *     Face ids are deliberately not compared: every loaded face exists twice, wound both ways.
 *     A taken tap adds sum += c_q * w, hs += prev_history[q] * w, ws += w.
 *  4. With history (ws > 0): pc = sum / ws, hl = hs / ws.
 *       cur.rgb finite:     n = fminf(hl + 1.0f, (float)max_history), out.rgb = pc + (cur.rgb - pc) * (1.0f / n),
 *                           out_history = n;
 *       cur.rgb not finite: out.rgb = pc, out_history = fminf(hl, (float)max_history)  (the history heals the pixel).
 *  5. Without history (invalid projection, ws == 0, or NULL prev): out.rgb = cur.rgb, out_history = 1, or 0 when
 *     cur.rgb is not finite -- such a pixel is never taken as history, so poison cannot spread.
 *  6. out.a = cur.a always.  Row padding of `out` is never written.
 *
 * PITFALL: render the frames fed to this with frame_index 0 (as the reference's Process() does while its sample
 * flag is dirty); a frame that rt_render has already blended with surface_last_frame would be counted twice.
 * ------------------------------------------------------------------------------------- */
#define RT_REPROJECT_DEFAULT (-1)  /* in any of the three filter parameters: the measured default */
#define RT_REPROJECT_MAX_HEIGHT RT_DENOISE_MAX_HEIGHT  /* the launch grid holds a row of blocks per 4 pixel rows */
#define RT_REPROJECT_MAX_PIXELS RT_DENOISE_MAX_PIXELS

typedef struct rt_reproject_params {
    const void* surface;           /* DEVICE pitched float4: the new frame, rendered with frame_index 0 */
    uint64_t pitch;                /* bytes per row: >= width * 16, a multiple of 16 (all three pitches) */
    const rt_hit* hits;            /* DEVICE width * height records of rt_trace_rays' camera mode for `camera` */
    /* The previous call's results: all three NULL (first frame, no history) or all three non-NULL. */
    const void* prev_surface;      /* DEVICE pitched float4: the previous accumulated image */
    uint64_t prev_pitch;
    const rt_hit* prev_hits;       /* DEVICE: the previous camera's records; prev_hits == hits is allowed */
    const float* prev_history;     /* DEVICE width * height floats: frames the previous image holds per pixel */
    void* out;                     /* DEVICE pitched float4: the new accumulated image; out == surface is allowed */
    uint64_t out_pitch;
    float* out_history;            /* DEVICE width * height floats */
    GPUCamera camera;              /* as rt_scene_camera returns them after the upload of each frame */
    GPUCamera prev_camera;         /* (ignored when prev_* are NULL) */
    int32_t width, height;         /* > 0; height <= RT_REPROJECT_MAX_HEIGHT, width * height <= RT_REPROJECT_MAX_PIXELS */
    /* Filter parameters.  RT_REPROJECT_DEFAULT (-1, -1.0f) selects the default (profiles/reproject_quality.txt);
     * so a normal_min of exactly -1 cannot be asked for -- -0.999999f switches the normal test off just as well. */
    int32_t max_history;           /* 1..65535 (32): the running mean never weighs a new frame below 1 / this */
    float sigma_plane;             /* > 0, finite (0.03): tolerated distance of a tap from p's tangent plane, as a fraction of t_p */
    float normal_min;              /* [-1, 1] (0.9): least cosine between p's normal and a tap's */
    int32_t flags;                 /* must be 0 */
} rt_reproject_params;

#if defined(__cplusplus)
static_assert(sizeof(rt_reproject_params) == 224 && offsetof(rt_reproject_params, surface) == 0 &&
              offsetof(rt_reproject_params, pitch) == 8 && offsetof(rt_reproject_params, hits) == 16 &&
              offsetof(rt_reproject_params, prev_surface) == 24 && offsetof(rt_reproject_params, prev_pitch) == 32 &&
              offsetof(rt_reproject_params, prev_hits) == 40 && offsetof(rt_reproject_params, prev_history) == 48 &&
              offsetof(rt_reproject_params, out) == 56 && offsetof(rt_reproject_params, out_pitch) == 64 &&
              offsetof(rt_reproject_params, out_history) == 72 && offsetof(rt_reproject_params, camera) == 80 &&
              offsetof(rt_reproject_params, prev_camera) == 140 && offsetof(rt_reproject_params, width) == 200 &&
              offsetof(rt_reproject_params, height) == 204 && offsetof(rt_reproject_params, max_history) == 208 &&
              offsetof(rt_reproject_params, sigma_plane) == 212 && offsetof(rt_reproject_params, normal_min) == 216 &&
              offsetof(rt_reproject_params, flags) == 220,
              "rt_reproject_params");
#endif

/* Reproject and accumulate on `stream` (a hipStream_t, NULL = null stream): stream-ordered, no synchronisation, no
 * allocation, no scene, no scratch; one kernel launch.  Every argument is checked on the host before the launch
 * (NULL pointers, prev_* partly NULL, sizes <= 0 or above the limits, pitches, alignment -- 16 bytes for surfaces and
 * records, 4 for the histories --, flags != 0, parameters out of range).  out == surface is safe: a lane reads only its
 * own pixel of `surface` before it writes.  `out` overlapping prev_surface and out_history overlapping prev_history
 * are refused: other lanes gather from them.  Returns 0 or an error code with rt_last_error(). */
int rt_reproject(const rt_reproject_params* params, void* stream);

/* ---------------------------------------------------------------------------------------
 * Variance-steered denoising: rt_denoise's filter with a colour tolerance of its own for every pixel, set by
 * an estimate of the variance of the pixel's luminance as stored -- small where rt_reproject's running mean
 * holds many frames, large where a pixel was just disoccluded -- and filtered along with the colours (the
 * spatial half of SVGF).  Per frame:
 *
 *   render with frame_index 0 -> rt_trace_rays in camera mode
 *     -> rt_reproject (the colour)               -> accumulated image A, history Hc
 *     -> rt_moments (the new frame)              -> moments surface M
 *     -> rt_reproject (M, with its own prev_surface and prev_history, the same hits, prev_hits and cameras)
 *                                                -> accumulated moments AM
 *     -> rt_denoise_variance(A, AM, Hc)          -> the filtered image, and the variance image
 *
 * The temporal accumulation of the moments is rt_reproject itself: its running mean of (l, l*l) is the first and
 * second moment.  There is no second reprojection kernel.
 *
 * The arithmetic is fixed as rt_denoise's is (fp32, no contraction, IEEE division, only + - * /, fmaxf, fabsf and
 * comparisons; no exp and no sqrt: the tolerance is used squared), so that tests/variance_ref.py restates both
 * calls bit for bit.  dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z, lum(c) = (0.2126f*c.x + 0.7152f*c.y) + 0.0722f*c.z.
 * valid(p), the albedo a_p with its 2^-6 floor and the weights wn and wz (with normal_power_log2 and
 * sigma_plane * t_p) are exactly rt_denoise's (steps 1 and 2 of its block above).
 *
 * rt_moments, per pixel p: c = surface.rgb / a_p, l = lum(c), out = (l, l*l, 0, surface.a).  A c that is not finite
 * gives moments that are not finite, on purpose: rt_reproject's rules 4 and 5 then heal or isolate that pixel
 * exactly as they do for the colour.
 *
 * rt_denoise_variance:
 *  1. Prepare.  c_p = surface.rgb / a_p; alpha passes through untouched.  The initial variance v_p estimates the
 *     variance of lum(c_p) as stored, that is, of the accumulated value.  hist = history[p], or 1 when history is
 *     NULL; (m1, m2) = moments[p].xy.
 *       !valid(p) or c_p.rgb not finite: v_p = 0.
 *       else, temporal, when moments != NULL, hist >= min_history (false for a NaN) and m1 and m2 are finite:
 *         v_p = fmaxf(0, m2 - m1*m1) / fmaxf(hist, 1.0f).
 *       else, spatial: s1 = s2 = ws = 0; for dy = -3..3 (outer), dx = -3..3 (inner), q = (x + dx, y + dy) inside
 *         the image with valid(q) and c_q.rgb finite (p itself is one of them): w = wn * wz (no kernel weight);
 *         if w > 0: s1 += lum(c_q) * w, s2 += (lum(c_q) * lum(c_q)) * w, ws += w.
 *         v_p = ws > 0 ? fmaxf(0, s2 / ws - (s1 / ws) * (s1 / ws)) : 0.
 *  2. `iterations` passes s = 0.., step = 1 << s, each from the previous pass's colours and variances.  !valid(p)
 *     keeps c_p and v_p.  Otherwise:
 *       prefilter: vsum = ksum = 0; for dy = -1..1 (outer), dx = -1..1 (inner), q = (x + dx, y + dy) -- stride 1
 *         whatever the pass -- inside the image with valid(q): k = kp[dy+1] * kp[dx+1], kp = {1/4, 1/2, 1/4};
 *         vsum += v_q * k, ksum += k.  vg = vsum / ksum (p itself is always taken).
 *       tol = (sigma_lum * sigma_lum) * vg + 1e-8f.
 *       the 25 taps of rt_denoise's step 2 in its order and with its skips (q outside the image, !valid(q), c_q.rgb
 *         not finite), q = (x + dx*step, y + dy*step):
 *         wl = 1 / (1 + (d * d) / tol) with d = lum(c_q) - lum(c_p) when c_p.rgb is finite, else 1;
 *         w = (((h[dy+2] * h[dx+2]) * wn) * wz) * wl;
 *         if w > 0: sum += c_q * w, vs += v_q * (w * w), wsum += w.
 *       c' = wsum > 0 ? sum / wsum : c_p.   v' = wsum > 0 ? vs / (wsum * wsum) : v_p.
 *  3. out.rgb = c * a_p, out.a = surface.a, out_variance[p] = v_p (0 for !valid(p)).  Row padding of `out` is
 *     never written, nor anything past width * height floats of out_variance.
 *
 * The variance is that of the albedo-divided luminance: multiply by lum(a_p)^2 for an estimate in the image's units.
 *
 * PITFALL: feed rt_denoise_variance the *accumulated* image with the history and moments that belong to it, and
 * render the frames with frame_index 0 (rt_reproject's pitfall): the temporal estimate divides the moments'
 * variance by the history length, which is the variance of the running mean only for the image that mean made.
 * ------------------------------------------------------------------------------------- */
typedef struct rt_moments_params {
    const void* surface;           /* DEVICE pitched float4: the new frame (not the accumulated image) */
    uint64_t pitch;                /* bytes per row: >= width * 16, a multiple of 16 (both pitches) */
    int32_t width, height;         /* > 0; height <= RT_DENOISE_MAX_HEIGHT, width * height <= RT_DENOISE_MAX_PIXELS */
    const rt_hit* hits;            /* DEVICE width * height records of rt_trace_rays' camera mode */
    const GPUMaterial* materials;  /* DEVICE (GPUScene.gpu_materials); may be NULL when material_count is 0 */
    int32_t material_count;
    int32_t flags;                 /* must be 0 */
    void* out;                     /* DEVICE pitched float4 (l, l*l, 0, alpha); must not overlap surface or hits */
    uint64_t out_pitch;
} rt_moments_params;

typedef struct rt_denoise_variance_params {
    const void* surface;           /* DEVICE pitched float4: the accumulated image (rt_reproject's out) */
    uint64_t pitch;                /* bytes per row: >= width * 16, a multiple of 16 (all three pitches) */
    int32_t width, height;         /* > 0; height <= RT_DENOISE_MAX_HEIGHT, width * height <= RT_DENOISE_MAX_PIXELS */
    const rt_hit* hits;            /* DEVICE width * height records of rt_trace_rays' camera mode */
    const GPUMaterial* materials;  /* DEVICE (GPUScene.gpu_materials); may be NULL when material_count is 0 */
    int32_t material_count;
    int32_t flags;                 /* must be 0 */
    const void* moments;           /* DEVICE pitched float4: the accumulated moments; NULL = spatial estimate everywhere */
    uint64_t moments_pitch;        /* (ignored when moments is NULL) */
    const float* history;          /* DEVICE width * height floats: rt_reproject's out_history of the colour; NULL = 1 everywhere */
    void* out;                     /* DEVICE pitched float4 result; out == surface is allowed (below) */
    uint64_t out_pitch;
    float* out_variance;           /* DEVICE width * height floats: the last pass's filtered variance; may be NULL */
    void* scratch;                 /* DEVICE, rt_denoise_variance_scratch_bytes(width, height); contents irrelevant */
    uint64_t scratch_bytes;
    /* Filter parameters.  RT_DENOISE_DEFAULT (-1, -1.0f) selects the default (profiles/variance_quality.txt for
     * sigma_lum and min_history, rt_denoise's for the other three); 0 is an error in all but normal_power_log2. */
    int32_t iterations;            /* 1..6 (5) */
    int32_t normal_power_log2;     /* 0..8 (5) */
    float sigma_plane;             /* > 0, finite (0.03) */
    float sigma_lum;               /* > 0, finite (4): luminance distance, in standard deviations, that halves a tap */
    float min_history;             /* >= 1, finite (4): the shortest history whose temporal moments are trusted */
    int32_t reserved;              /* must be 0 */
} rt_denoise_variance_params;

#if defined(__cplusplus)
static_assert(sizeof(rt_moments_params) == 64 && offsetof(rt_moments_params, surface) == 0 &&
              offsetof(rt_moments_params, pitch) == 8 && offsetof(rt_moments_params, width) == 16 &&
              offsetof(rt_moments_params, height) == 20 && offsetof(rt_moments_params, hits) == 24 &&
              offsetof(rt_moments_params, materials) == 32 && offsetof(rt_moments_params, material_count) == 40 &&
              offsetof(rt_moments_params, flags) == 44 && offsetof(rt_moments_params, out) == 48 &&
              offsetof(rt_moments_params, out_pitch) == 56,
              "rt_moments_params");
static_assert(sizeof(rt_denoise_variance_params) == 136 && offsetof(rt_denoise_variance_params, surface) == 0 &&
              offsetof(rt_denoise_variance_params, pitch) == 8 && offsetof(rt_denoise_variance_params, width) == 16 &&
              offsetof(rt_denoise_variance_params, height) == 20 && offsetof(rt_denoise_variance_params, hits) == 24 &&
              offsetof(rt_denoise_variance_params, materials) == 32 &&
              offsetof(rt_denoise_variance_params, material_count) == 40 && offsetof(rt_denoise_variance_params, flags) == 44 &&
              offsetof(rt_denoise_variance_params, moments) == 48 && offsetof(rt_denoise_variance_params, moments_pitch) == 56 &&
              offsetof(rt_denoise_variance_params, history) == 64 && offsetof(rt_denoise_variance_params, out) == 72 &&
              offsetof(rt_denoise_variance_params, out_pitch) == 80 && offsetof(rt_denoise_variance_params, out_variance) == 88 &&
              offsetof(rt_denoise_variance_params, scratch) == 96 && offsetof(rt_denoise_variance_params, scratch_bytes) == 104 &&
              offsetof(rt_denoise_variance_params, iterations) == 112 &&
              offsetof(rt_denoise_variance_params, normal_power_log2) == 116 &&
              offsetof(rt_denoise_variance_params, sigma_plane) == 120 && offsetof(rt_denoise_variance_params, sigma_lum) == 124 &&
              offsetof(rt_denoise_variance_params, min_history) == 128 && offsetof(rt_denoise_variance_params, reserved) == 132,
              "rt_denoise_variance_params");
#endif

/* The luminance moments of one frame on `stream` (a hipStream_t, NULL = null stream): stream-ordered, no
 * synchronisation, no allocation, no scratch; one kernel launch.  Every argument is checked on the host before the
 * launch (NULL pointers, sizes <= 0 or above the limits, pitches, alignment, flags != 0); `out` overlapping
 * `surface` (out == surface included) or `hits` is refused.  Returns 0 or an error code with rt_last_error(). */
int rt_moments(const rt_moments_params* params, void* stream);
/* Bytes of scratch rt_denoise_variance needs for a width x height frame (68 per pixel: the packed guide, two
 * buffers of colour and variance, one alpha plane; rounded up to 16); 0 for a size <= 0.  Monotone in both arguments. */
size_t rt_denoise_variance_scratch_bytes(int width, int height);
/* Filter on `stream` (a hipStream_t, NULL = null stream): stream-ordered, no synchronisation, no allocation;
 * iterations + 1 kernel launches.  Every argument is checked on the host before the first launch (NULL pointers,
 * sizes <= 0 or above the limits, pitches < width * 16, alignment -- 16 bytes for surfaces, records and scratch, 4 for
 * history and out_variance --, scratch too small, flags or reserved != 0, parameters out of range, overlaps).
 * out == surface is safe: the first kernel consumes the whole surface into scratch, and the last pass, the only one
 * that writes `out` and `out_variance`, reads scratch and the material table only.  `out` must not overlap scratch,
 * hits, moments or history; out_variance must not overlap out or scratch.  Returns 0 or an error code with
 * rt_last_error(). */
int rt_denoise_variance(const rt_denoise_variance_params* params, void* stream);

/* ---------------------------------------------------------------------------------------
 * Upsampling: a frame rendered at 1/scale of the size in each direction (a quarter to a sixteenth of the paths)
 * brought to the full size, guided by the first-hit records at both sizes:
 *
 *   rt_render(low_width, low_height) -> rt_trace_rays camera mode at the low size and at the output size
 *   [-> rt_denoise on the low frame] -> rt_upsample.
 *
 * One camera serves both sizes: GPUCamera depends on the viewport through aspect = width / height only, and
 * (float)(s*w) / (float)(s*h) is the same correctly rounded quotient, so nothing is uploaded again between the calls.
 * A joint-bilateral gather on albedo-divided colour, as rt_denoise's: the low colours are divided by their own first
 * hit's albedo and the result is multiplied by the *output* pixel's, so texture edges come out at the full resolution.
 *
 * The arithmetic is fixed as rt_denoise's is (fp32, no contraction, IEEE division, only + - * /, fmaxf, fabsf and
 * comparisons), so that tests/upsample_ref.py restates it bit for bit.  tag (0 for a miss), the floor-clamped albedo
 * a (1 for a miss), dot and the guide weights wn and wz are rt_denoise's (steps 1 and 2 of its block above), with the
 * *output* pixel as the centre p of wn and wz and the low pixel as the tap q.  Low pixel q has tag_q and colour
 * c_q = low_surface[q].rgb / a_q.  Output pixel P = (X, Y) has record hits[Y * width + X], tag_P and a_P.  With
 * s = scale:
 *
 *  1. Footprint: ix = 2X + 1 - s (an int, may be negative); x0 = floor(ix / 2s) (floor division: -1 for a negative
 *     ix); rx = ix - 2s*x0; tx = (float)rx / (float)(2s); wx = {1.0f - tx, tx}.  The same in y.
 *  2. Guide g(P, q): when tag_P == 0, 1 if tag_q == 0, else 0; when tag_P != 0, 0 if tag_q == 0, else wn * wz
 *     (wn squared normal_power_log2 times, wz squared once; with sigma_plane * t_P in wz).
 *  3. Stage 1: for j = 0..1 (outer), i = 0..1 (inner), q = (x0 + i, y0 + j), skipping q outside the low image and
 *     c_q.rgb not finite: w = (wy[j] * wx[i]) * g; if w > 0: sum += c_q * w, wsum += w.
 *  4. Stage 2, only if wsum > 0 is false after stage 1: for j = 0..3, i = 0..3, q = (x0 - 1 + i, y0 - 1 + j), the
 *     same skips, w = g; if w > 0: sum += c_q * w, wsum += w.
 *  5. c = wsum > 0 ? sum / wsum : c_near with near = (X / s, Y / s) (stage 3; a c_near that is not finite passes
 *     through).  out.rgb = c * a_P, out.w = low_surface[near].w.
 *
 * A tap is added only if w > 0, never as a zero.  Why three stages: stage 1 is bilinear interpolation wherever the
 * guide agrees; an output pixel whose four low neighbours all lie on other surfaces (a thin object, a silhouette)
 * looks for its own surface one ring further out, where the bilinear weights would be extrapolating, hence the guide
 * alone; and a pixel with no usable low pixel nearby at all still gets a colour.
 *
 * Preconditions: both hit buffers come from the same camera (the positions are compared in world space); t_P == 0
 * gives wz = 0 (inf or NaN -> 0) for every tap, and with it stage 3.
 * ------------------------------------------------------------------------------------- */
#define RT_UPSAMPLE_DEFAULT (-1)   /* in either filter parameter: the measured default */
#define RT_UPSAMPLE_MAX_HEIGHT RT_DENOISE_MAX_HEIGHT  /* of the output: the launch grid holds a row of blocks per 4 pixel rows */
#define RT_UPSAMPLE_MAX_PIXELS RT_DENOISE_MAX_PIXELS  /* of the output */

typedef struct rt_upsample_params {
    const void* low_surface;       /* DEVICE pitched float4 frame of low_width x low_height pixels */
    uint64_t low_pitch;            /* bytes per row of low_surface: >= low_width * 16, a multiple of 16 */
    const rt_hit* low_hits;        /* DEVICE low_width * low_height records of rt_trace_rays' camera mode */
    int32_t low_width, low_height; /* > 0 */
    int32_t scale;                 /* 2, 3 or 4: the output is scale * low_width x scale * low_height pixels, height <=
                                      RT_UPSAMPLE_MAX_HEIGHT, width * height <= RT_UPSAMPLE_MAX_PIXELS */
    int32_t material_count;
    const rt_hit* hits;            /* DEVICE width * height records of camera mode at the output size, same camera */
    const GPUMaterial* materials;  /* DEVICE (GPUScene.gpu_materials); may be NULL when material_count is 0 */
    void* out;                     /* DEVICE pitched float4 result at the output size; row padding is never written */
    uint64_t out_pitch;            /* >= width * 16, a multiple of 16 */
    void* scratch;                 /* DEVICE, rt_upsample_scratch_bytes(low_width, low_height); contents irrelevant */
    uint64_t scratch_bytes;
    /* Filter parameters.  RT_UPSAMPLE_DEFAULT (-1, -1.0f) selects the default (profiles/upsample_quality.txt). */
    int32_t normal_power_log2;     /* 0..8 (0): the normal weight is cos^(2^this), cos clamped at 0 */
    float sigma_plane;             /* > 0, finite (0.03): tolerated distance from P's tangent plane, as a fraction of t_P */
    int32_t flags;                 /* must be 0 */
    int32_t reserved;              /* must be 0 */
} rt_upsample_params;

#if defined(__cplusplus)
static_assert(sizeof(rt_upsample_params) == 104 && offsetof(rt_upsample_params, low_surface) == 0 &&
              offsetof(rt_upsample_params, low_pitch) == 8 && offsetof(rt_upsample_params, low_hits) == 16 &&
              offsetof(rt_upsample_params, low_width) == 24 && offsetof(rt_upsample_params, low_height) == 28 &&
              offsetof(rt_upsample_params, scale) == 32 && offsetof(rt_upsample_params, material_count) == 36 &&
              offsetof(rt_upsample_params, hits) == 40 && offsetof(rt_upsample_params, materials) == 48 &&
              offsetof(rt_upsample_params, out) == 56 && offsetof(rt_upsample_params, out_pitch) == 64 &&
              offsetof(rt_upsample_params, scratch) == 72 && offsetof(rt_upsample_params, scratch_bytes) == 80 &&
              offsetof(rt_upsample_params, normal_power_log2) == 88 && offsetof(rt_upsample_params, sigma_plane) == 92 &&
              offsetof(rt_upsample_params, flags) == 96 && offsetof(rt_upsample_params, reserved) == 100,
              "rt_upsample_params");
#endif

/* Bytes of scratch rt_upsample needs for a low frame of low_width x low_height pixels (48 per low pixel: normal,
 * position and tag, albedo-divided colour); 0 for a size <= 0.  Monotone in both arguments. */
size_t rt_upsample_scratch_bytes(int low_width, int low_height);
/* Upsample on `stream` (a hipStream_t, NULL = null stream): stream-ordered, no synchronisation, no allocation; two
 * kernel launches.  Every argument is checked on the host before the first launch, in this order, the first fault
 * reported: NULL pointers (params, low_surface, low_hits, hits, out, scratch); low sizes <= 0 and the scale; the caps,
 * on the output size; materials; pitches; alignment (16 bytes, every buffer); scratch too small; overlaps; flags and
 * reserved != 0; parameters out of range.  `out` must not overlap low_surface, low_hits, hits, scratch or the material
 * table.  Returns 0 or an error code with rt_last_error(). */
int rt_upsample(const rt_upsample_params* params, void* stream);

/* ---------------------------------------------------------------------------------------
 * Adaptive sampling: per-pixel sample budgets.  Four calls, each usable alone:
 *
 *   rt_sample_pixels    trace samples[i] more of the renderer's own samples for pixel pixels[i], into an undivided
 *                       accumulator (sum of colours, sample count), optional luminance moments and the pixel's state
 *   rt_sample_priority  accumulator + moments -> a per-pixel priority (the relative variance of the mean)
 *   rt_sample_plan      any float image of priorities + a budget -> the (pixels, samples) list of the next round
 *   rt_sample_resolve   accumulator -> an image (the mean)
 *
 * The invariant: a pixel that has received N samples in total, in however many calls and in whatever list order, holds
 * exactly the renderer's undivided accumulator after N samples and the renderer's RNG state after N samples.
 *
 * The arithmetic is fp32, no contraction, IEEE division, only + - * /, fmaxf and comparisons, and exact integer
 * arithmetic in the planner, so that tests/adaptive_ref.py restates every call bit for bit.
 *
 * rt_sample_pixels.  The camera is scene->camera (as rt_trace_rays' camera mode), the frame is width x height, pixel
 * index p = y * width + x, state p of `rng` is pixel p's (the renderer's layout, rt_init_rng with one shard).  Per list
 * entry i with n = samples[i] > 0 and p = pixels[i] (or i when pixels is NULL) inside [0, width * height):
 *   1. the state of p is loaded;
 *   2. n times, one of the renderer's samples, exactly as rt_render starts and ends it: draw ru, then rv;
 *      uv = (((float)x + ru) / (float)width, ((float)y + rv) / (float)height); the unnormalised camera direction
 *      ((lower_left_corner + horizontal * uv.x) + vertical * uv.y) - origin from the camera origin; then per segment
 *      the sphere loop, the BVH traversal and ray_color's tail (4 draws per hit, none on a miss), until a miss, Russian
 *      roulette or `bounces` segments.  With bounces == 0 a sample still consumes its two jitter draws and contributes
 *      (0, 0, 0), as the renderer's does;
 *   3. after each sample with colour c, a = accum[p]: a.r = a.r + c.r, a.g = a.g + c.g, a.b = a.b + c.b,
 *      a.w = a.w + 1.0f; with moments, l = (0.2126f*c.r + 0.7152f*c.g) + 0.0722f*c.b (rt_moments' lum),
 *      m.x = m.x + l, m.y = m.y + l*l;
 *   4. the state of p is stored.
 * An entry with samples[i] == 0 reads and writes nothing for its pixel (its pixels[i] is not read either); an entry
 * < 0 or >= width * height renders nothing.  Row padding of accum is never written; pixels the list does not name are
 * never written, in accum, moments or rng.  A pixel named twice in one call gives UNDEFINED values in its accumulator,
 * moments and state, but no fault; rt_sample_plan never produces such a list.
 * ------------------------------------------------------------------------------------- */
typedef struct rt_sample_pixels_params {
    const int32_t* pixels;   /* DEVICE int32[count], 4-byte aligned; NULL: entry i is pixel i, count == width * height */
    const uint16_t* samples; /* DEVICE uint16[count], 2-byte aligned */
    int64_t count;           /* 0 returns at once; at most 2^31 */
    rt_rng_state* rng;       /* DEVICE, width * height states indexed y * width + x, 8-byte aligned */
    void* accum;             /* DEVICE pitched float4 (sum r, sum g, sum b, samples), 16-byte aligned */
    uint64_t accum_pitch;    /* bytes per row: >= width * 16, a multiple of 16 */
    float* moments;          /* DEVICE float[width * height][2] (sum l, sum l*l), 8-byte aligned; may be NULL */
    int32_t width, height;   /* > 0, width * height <= 2^30 */
    int32_t bounces;         /* >= 0 */
    uint32_t flags;          /* must be 0 */
    int32_t waves_per_simd;  /* occupancy build of the kernel: 5 / 6 / 7, or 0 = the default
                                (profiles/adaptive_timing.txt) */
    int32_t reserved;        /* must be 0 */
} rt_sample_pixels_params;   /* 80 B */

/* rt_sample_priority, per pixel p: n = accum[p].w, m = moments[p].
 *   !(n >= 2.0f), or m.x or m.y not finite: priority[p] = +inf (unknown pixels go first);
 *   else m1 = m.x / n, m2 = m.y / n, var = fmaxf(0, m2 - m1*m1) / n, priority[p] = var / (m1*m1 + 1e-4f). */
typedef struct rt_sample_priority_params {
    const void* accum;       /* DEVICE pitched float4, 16-byte aligned */
    uint64_t accum_pitch;    /* >= width * 16, a multiple of 16 */
    const float* moments;    /* DEVICE float[width * height][2], 8-byte aligned */
    float* priority;         /* DEVICE float[width * height], 4-byte aligned; must not overlap accum or moments */
    int32_t width, height;   /* > 0, width * height <= 2^30 */
} rt_sample_priority_params; /* 40 B */

/* rt_sample_plan.  P = width * height; the list always has P entries, so no size is read back.  All exact:
 *   t = priority[p] * scale (fp32);  q_p = !(t < 65535.0f) ? 65535 : (t > 0 ? (uint32_t)t : 0)  (NaN, +inf: 65535);
 *   Q = sum of q_p (uint64);  B = budget - min_samples * P;  extra_p = Q ? (uint64)q_p * B / Q : 0 (the exact
 *   quotient, rounded down);  n_p = min(max_samples, min_samples + extra_p).
 * So the sum of n_p never exceeds budget.  Budget left over by the rounding down and by the cap at max_samples is NOT
 * redistributed.  Order of the list: the pixels enumerated in 8x8 sub-tile order (sub-tiles row-major over
 * ceil(width/8) x ceil(height/8), row-major inside a sub-tile, positions outside the image left out), then sorted
 * stably by n_p descending -- equal counts share waves, neighbours stay together inside a count class, and the
 * zero-sample entries form the tail.  *total, when given, receives the sum of n_p. */
typedef struct rt_sample_plan_params {
    const float* priority;   /* DEVICE float[P], 4-byte aligned (rt_sample_priority's, rt_denoise_variance's out_variance, ...) */
    int32_t width, height;   /* > 0, P <= 2^30 */
    int64_t budget;          /* total samples of the coming round; >= min_samples * P */
    int32_t min_samples;     /* 0 .. max_samples */
    int32_t max_samples;     /* 1 .. 4095 */
    float scale;             /* > 0, finite */
    int32_t reserved;        /* must be 0 */
    int32_t* pixels;         /* DEVICE int32[P], 4-byte aligned */
    uint16_t* samples;       /* DEVICE uint16[P], 2-byte aligned */
    uint64_t* total;         /* DEVICE, 8-byte aligned; may be NULL */
    void* scratch;           /* DEVICE, 16-byte aligned, rt_sample_plan_scratch_bytes(width, height); contents irrelevant */
    uint64_t scratch_bytes;
} rt_sample_plan_params;     /* 80 B */

/* rt_sample_resolve, per pixel: out.rgb = accum.w >= 1.0f ? accum.rgb / accum.w : 0, out.a = 1.  `out` is a surface
 * rt_denoise, rt_tonemap_srgb8 and rt_write_pfm take as is; it must not overlap accum. */
typedef struct rt_sample_resolve_params {
    const void* accum;       /* DEVICE pitched float4, 16-byte aligned */
    uint64_t accum_pitch;    /* >= width * 16, a multiple of 16 (both pitches) */
    void* out;               /* DEVICE pitched float4, 16-byte aligned; row padding is never written */
    uint64_t out_pitch;
    int32_t width, height;   /* > 0, width * height <= 2^30 */
} rt_sample_resolve_params;  /* 40 B */

#if defined(__cplusplus)
static_assert(sizeof(rt_sample_pixels_params) == 80 && offsetof(rt_sample_pixels_params, pixels) == 0 &&
              offsetof(rt_sample_pixels_params, samples) == 8 && offsetof(rt_sample_pixels_params, count) == 16 &&
              offsetof(rt_sample_pixels_params, rng) == 24 && offsetof(rt_sample_pixels_params, accum) == 32 &&
              offsetof(rt_sample_pixels_params, accum_pitch) == 40 && offsetof(rt_sample_pixels_params, moments) == 48 &&
              offsetof(rt_sample_pixels_params, width) == 56 && offsetof(rt_sample_pixels_params, height) == 60 &&
              offsetof(rt_sample_pixels_params, bounces) == 64 && offsetof(rt_sample_pixels_params, flags) == 68 &&
              offsetof(rt_sample_pixels_params, waves_per_simd) == 72 && offsetof(rt_sample_pixels_params, reserved) == 76,
              "rt_sample_pixels_params");
static_assert(sizeof(rt_sample_priority_params) == 40 && offsetof(rt_sample_priority_params, accum) == 0 &&
              offsetof(rt_sample_priority_params, accum_pitch) == 8 && offsetof(rt_sample_priority_params, moments) == 16 &&
              offsetof(rt_sample_priority_params, priority) == 24 && offsetof(rt_sample_priority_params, width) == 32 &&
              offsetof(rt_sample_priority_params, height) == 36,
              "rt_sample_priority_params");
static_assert(sizeof(rt_sample_plan_params) == 80 && offsetof(rt_sample_plan_params, priority) == 0 &&
              offsetof(rt_sample_plan_params, width) == 8 && offsetof(rt_sample_plan_params, height) == 12 &&
              offsetof(rt_sample_plan_params, budget) == 16 && offsetof(rt_sample_plan_params, min_samples) == 24 &&
              offsetof(rt_sample_plan_params, max_samples) == 28 && offsetof(rt_sample_plan_params, scale) == 32 &&
              offsetof(rt_sample_plan_params, reserved) == 36 && offsetof(rt_sample_plan_params, pixels) == 40 &&
              offsetof(rt_sample_plan_params, samples) == 48 && offsetof(rt_sample_plan_params, total) == 56 &&
              offsetof(rt_sample_plan_params, scratch) == 64 && offsetof(rt_sample_plan_params, scratch_bytes) == 72,
              "rt_sample_plan_params");
static_assert(sizeof(rt_sample_resolve_params) == 40 && offsetof(rt_sample_resolve_params, accum) == 0 &&
              offsetof(rt_sample_resolve_params, accum_pitch) == 8 && offsetof(rt_sample_resolve_params, out) == 16 &&
              offsetof(rt_sample_resolve_params, out_pitch) == 24 && offsetof(rt_sample_resolve_params, width) == 32 &&
              offsetof(rt_sample_resolve_params, height) == 36,
              "rt_sample_resolve_params");
#endif

/* All four run on `stream` (a hipStream_t, NULL = null stream): stream-ordered, no synchronisation, no allocation.
 * Each returns 0 or an error code with rt_last_error().
 *
 * rt_sample_pixels: one kernel launch.  The scene rules are rt_radiance's: uploaded by rt_scene_upload (a GPUScene
 * filled by another host is refused), materials required, the sky is the scene's cube map under the renderer's
 * rotation, a BVH deeper than the traversal stack is refused.  Checked in this order, the first fault reported -- no
 * device needed: NULL params, scene, samples, rng, accum; flags; reserved; waves_per_simd; count < 0 or > 2^31;
 * width / height <= 0; width * height > 2^30; pixels == NULL with count != width * height; bounces; accum_pitch;
 * alignment (accum 16, rng and moments 8, pixels 4, samples 2) -- then count == 0 returns 0 -- then the scene, then
 * the buffer sizes (pixels, samples, rng, accum, moments), then overlaps: accum may not overlap rng, moments, pixels
 * or samples. */
int rt_sample_pixels(const rt_sample_pixels_params* params, const GPUScene* scene, void* stream);
/* One kernel launch.  Checked: NULL pointers, sizes, accum_pitch, alignment, priority overlapping accum or moments. */
int rt_sample_priority(const rt_sample_priority_params* params, void* stream);
/* Bytes of scratch rt_sample_plan needs for a width x height frame: 16, + 6 per pixel (the unsorted keys and pixel
 * indices, each array rounded up to 16 bytes), + an upper bound on the radix sort's own storage, whose exact size only
 * a device tells: 6 more per pixel (its second buffers of both) + 16 per pixel (digit counters of its blocks) + 64 KiB.
 * It needs no device; rt_sample_plan checks the sort's real size against it.  0 for a size <= 0; monotone in both
 * arguments. */
size_t rt_sample_plan_scratch_bytes(int width, int height);
/* Three kernels, a memset and a stable radix sort over the bits the largest count needs.  Checked in this order:
 * NULL params, priority, pixels, samples, scratch; width / height <= 0; more than 2^30 pixels; reserved;
 * max_samples outside 1..4095; min_samples outside 0..max_samples; scale; budget < min_samples * P; alignment
 * (scratch 16, total 8, priority and pixels 4, samples 2); scratch_bytes; overlaps among priority, pixels, samples,
 * total and scratch. */
int rt_sample_plan(const rt_sample_plan_params* params, void* stream);
/* One kernel launch.  Checked: NULL pointers, sizes, pitches, alignment, out overlapping accum (out == accum too). */
int rt_sample_resolve(const rt_sample_resolve_params* params, void* stream);

/* init_rng for the pixels of one shard: state index s of shard (shard_index, shard_count)
 * of a width x height frame gets curand_init(seed, pixel_id(s), 0).  With shard_count == 1
 * the states are in y*width + x order (reference layout); otherwise they are compact in the
 * shard's tile order.  Returns 0 or an error code. */
int rt_init_rng(void* rng_states, int width, int height, int shard_index, int shard_count, uint32_t seed,
                void* stream);

/* Number of pixels of a shard (tiles of 16x16, partial edge tiles counted as rendered
 * pixels of the tile: the compact shard always holds whole tiles). */
int64_t rt_shard_tiles(int width, int height, int shard_index, int shard_count);

/* Un-permute gathered compact shards [shard_count][tiles_per_shard_max][256] float4 into a
 * pitched surface.  Returns 0 or an error code. */
int rt_unshard(void* surface, uint64_t pitch, int width, int height, int shard_count, const void* shards,
               int64_t tiles_per_shard_max, void* stream);

/* ---------------------------------------------------------------------------------------
 * Multi-GPU split (the reference renders one frame on one device,
 * RayTracing/RayTracing.cpp:205-234).  Plans deal 16x16 tiles to ranks; each rank renders a
 * compact shard; one gather per frame; the root un-permutes.
 * ------------------------------------------------------------------------------------- */
/* Entries per rank a plan may use (the row length of tile_lists below). */
int64_t rt_shard_plan_capacity(int width, int height, int shard_count);
/* Fill HOST tile_lists [shard_count][capacity] (-1 padded) and counts [shard_count].
 * tile_cost (HOST, one per row-major tile) NULL = round-robin (rank r: tiles r, r+N, ...);
 * otherwise longest-processing-time-first: heaviest tile first, each to the least-loaded rank
 * below capacity; every rank's list comes out heaviest first.  Deterministic.  0 or error. */
int rt_shard_plan(int width, int height, int shard_count, const double* tile_cost, int64_t capacity,
                  int32_t* tile_lists, int64_t* counts);
/* Lane plans (rt_render_params.lane_slots; shard.cpp).  Entries a plan for `slots` slots (a
 * multiple of 64: 256 per list entry) may use. */
int64_t rt_lane_plan_capacity(int64_t slots);
/* Fill HOST lane_slots from HOST per-slot work `cost` (rt_render_params.lane_cost of a probe
 * frame of the same list, zero for slots without a pixel).  A wave's time is modelled as
 * max c x (sum c / max c)^0.34 work units; every 8x8 sub-tile wave above the target
 * slack x max(max c, sum c / parallel_units) is split (first fit, heaviest pixels first) into
 * sub-waves within it.  Waves of at least half the target go first, longest first; the rest keep
 * list order.  Slots whose cost is UINT32_MAX (rt_lone_plan's lone pixels) are left out of the map.  parallel_units <= 0: the identity map.  MI355X: 48000 (bench.py --lane-units; measured
 * best for configs 2 and 3 at N = 2-8).
 * *long_waves (optional) receives the number of those leading waves (rt_render_params.
 * priority_waves).  Returns the entries written (a multiple of 64), or -1 on bad arguments. */
int64_t rt_lane_plan(const uint32_t* cost, int64_t slots, double parallel_units, double slack,
                     int32_t* lane_slots, int64_t capacity, int64_t* long_waves);
/* Measured refinement of a HOST lane map of `entries` entries over `slots` slots: with wave_ticks
 * [entries / 64] the per-wave clocks of a timing frame of that map (rt_render_params.wave_clock),
 * every wave of more than one pixel whose clock is at least theta (0 < theta <= 1) x the longest is
 * split in two (its pixels in decreasing `cost` dealt alternately), and all waves are written to
 * HOST `out` (capacity >= 2 * entries) ordered by expected duration, longest first.  A map is a
 * permutation of the slots, so the frame is bit-identical; the caller keeps the refined map only if
 * a timed frame of it is faster (bench.py refine_lane_map).  *split_waves (optional) receives the
 * number of waves made by splitting.  Returns the entries written, or -1 on bad arguments. */
int64_t rt_lane_refine(const int32_t* lane_slots, int64_t entries, const uint32_t* cost, int64_t slots,
                       const int64_t* wave_ticks, double theta, int32_t* out, int64_t capacity, int64_t* split_waves);
/* Lone-pixel plans: write to HOST lone_slots (up to max_lone entries) the slots whose probe work
 * `cost` is at least min_cost, heaviest first (ties: lower slot first), and mark each of them in
 * `cost` with UINT32_MAX -- the value rt_lane_plan treats as "not in this map".  Returns the number
 * written, or -1 on bad arguments. */
int64_t rt_lone_plan(uint32_t* cost, int64_t slots, int64_t max_lone, uint32_t min_cost, int32_t* lone_slots);
/* rt_init_rng for an explicit tile list (DEVICE int32): state k*256 + t <- curand_init(seed,
 * pixel id of thread t of tile tile_list[k]). */
int rt_init_rng_tiles(void* rng_states, int width, int height, const int32_t* tile_list, int64_t tile_count,
                      uint32_t seed, void* stream);
/* rt_unshard with explicit plans: tile_lists is the DEVICE copy of rt_shard_plan's output. */
int rt_unshard_tiles(void* surface, uint64_t pitch, int width, int height, int shard_count, const void* shards,
                     int64_t tiles_per_shard_max, const int32_t* tile_lists, void* stream);

/* RCCL communicator for the frame-end gather (csrc/comm.hip).  One process per GPU: rank 0 makes
 * an id, the host passes it to every rank by its own means, each rank calls rt_comm_init_rank on
 * its current device.  One process driving N devices: rt_comm_init_all. */
#define RT_COMM_ID_BYTES 128
typedef struct rt_comm rt_comm;
int rt_comm_unique_id(uint8_t id[RT_COMM_ID_BYTES]);
int rt_comm_init_rank(rt_comm** comm, int nranks, int rank, const uint8_t id[RT_COMM_ID_BYTES]);
int rt_comm_init_all(rt_comm** comms, int ndev, const int* devices);
int rt_comm_destroy(rt_comm* comm);
int rt_comm_rank(const rt_comm* comm);
int rt_comm_size(const rt_comm* comm);
/* Bracket the per-device gathers of a one-process, N-device host (RCCL group semantics). */
int rt_comm_group_start(void);
int rt_comm_group_end(void);
/* The frame's gather on `stream`: every rank passes its shard (shard_bytes); the root receives
 * rank r's bytes at gathered + r * stride (recv_bytes[r] bytes, or shard_bytes for every rank
 * when recv_bytes is NULL; the root's own shard is copied on the stream).  Asynchronous. */
int rt_gather_shards(rt_comm* comm, const void* shard, size_t shard_bytes, void* gathered, size_t stride,
                     const size_t* recv_bytes, int root, void* stream);

/* ---------------------------------------------------------------------------------------
 * Frame output (the viewer path: main.cpp:66-94 draws the surface with exposure 0.5 + ACES film
 * into an sRGB back buffer, main.cpp:438).  For looking at frames; not on the render path.
 * ------------------------------------------------------------------------------------- */
/* Tonemap a pitched float4 surface into width*height*3 bytes of DEVICE memory, rows top to
 * bottom (display order): sRGB8(ACESFilm(0.5 * rgb)), IEC sRGB encode.  Returns 0 or nonzero. */
int rt_tonemap_srgb8(const void* surface, uint64_t pitch, int width, int height, uint8_t* out_rgb, void* stream);
/* Host files: PFM of a HOST copy of the surface (linear RGB, rows bottom to top as PFM
 * stores them = the surface's row order), and binary PPM of top-to-bottom RGB8 rows. */
int rt_write_pfm(const char* path, const float* rgba, uint64_t pitch, int width, int height);
int rt_write_ppm(const char* path, const uint8_t* rgb, int width, int height);

/* ---------------------------------------------------------------------------------------
 * Device memory / texture shim (replaces utils/CUDAHelper.h and utils/CUDATexture.*).
 * ------------------------------------------------------------------------------------- */
int rt_set_device(int device);
/* Visible HIP devices (0 when none or on error). */
int rt_device_count(void);
int rt_malloc(void** ptr, size_t bytes);
int rt_malloc_pitch(void** ptr, size_t* pitch, size_t width_bytes, size_t height);
int rt_free(void* ptr);
int rt_memcpy_h2d(void* dst, const void* src, size_t bytes);
int rt_memcpy_d2h(void* dst, const void* src, size_t bytes);
int rt_memcpy_d2d(void* dst, const void* src, size_t bytes);
int rt_memset(void* dst, int value, size_t bytes);
int rt_synchronize(void);
const char* rt_last_error(void);

/* Cube map from level-0 fp32 RGBA faces [6][size][size][4] (host memory), face order
 * +X,-X,+Y,-Y,+Z,-Z.  Sampled in software (bilinear, seamless).  Returns 0 on failure. */
uint64_t rt_cubemap_create(const float* rgba_level0, int size);
int rt_cubemap_destroy(uint64_t handle);

/* ---------------------------------------------------------------------------------------
 * Host scene (C++ mirror of RayTracing::Scene / BVH / Camera, RayTracing/Scene.{h,cpp},
 * RayTracing/BVH.{h,cpp}) exposed for non-C++ hosts.  rt_scene is opaque.
 * ------------------------------------------------------------------------------------- */
typedef struct rt_scene rt_scene;

rt_scene* rt_scene_create(void);
void rt_scene_destroy(rt_scene* scene);
uint32_t rt_scene_add_material(rt_scene* scene, const GPUMaterial* material);
void rt_scene_add_triangle(rt_scene* scene, const float a[3], const float b[3], const float c[3], int material);
void rt_scene_add_quad(rt_scene* scene, const float a[3], const float b[3], const float c[3], const float d[3],
                       int material);
void rt_scene_add_sphere(rt_scene* scene, const float position[3], float radius, int material);
/* Scene::AddLoadedScene with a mesh file -- a Wavefront .obj (imported like the reference's
 * assimp post-processing, objload.cpp) or a mesh asset (assets/bunny_mesh.bin format) -- and a
 * column-major 4x4 transform.  Returns 0 or an error code.
 * PARITY NOTE: a scene built from an .obj is NOT a parity scene.  Positions, vertex order and
 * faces are bit-identical to an assimp 3.3 import, but the smoothed normals differ from it in
 * the last ulps (assimp's summation order over coincident corners follows its SpatialSort's
 * unstable sort, and the reference pins no assimp version: vcpkg.json:4-7), so frames rendered
 * from it can diverge from the reference's.  The parity scenes (rt_scene_setup, the tests and
 * the benchmark) load the mesh asset, which holds the assimp 3.3 import verbatim. */
int rt_scene_add_mesh_file(rt_scene* scene, const char* path, const float transform[16], int material);
/* Environment cube map from an asset (assets/sunset_cube128.bin) or a legacy fp32 DDS. */
int rt_scene_set_environment_file(rt_scene* scene, const char* path);
/* Host view of the scene's level-0 cube texels [6][size][size][4] (NULL / 0 when none). */
int rt_scene_environment(const rt_scene* scene, const float** texels, int* size);
void rt_scene_set_camera(rt_scene* scene, const float position[3], float angle_x_deg, float angle_y_deg);
void rt_scene_set_viewport(rt_scene* scene, int width, int height);
/* Scene::Upload: builds the BVH when dirty, uploads dirty buffers, fills the GPUScene.  0, or 1 with
 * rt_last_error(): a scene without triangles is refused here, before any device state exists (no tracer
 * terminates on the lone root BVH::Calculate gives it). */
int rt_scene_upload(rt_scene* scene, void* rng_state);
const GPUScene* rt_scene_gpu(const rt_scene* scene);
/* The host half of Scene::Upload without any device work: camera basis + BVH build. */
void rt_scene_build(rt_scene* scene);
/* The camera basis as of the last build/upload. */
void rt_scene_camera(const rt_scene* scene, GPUCamera* out);
/* CUDARayTracer::SetupCornellBox + SetupStanfordBunny (RayTracing.cpp:79-203, 33-69);
 * which = 0: Cornell box + bunny (configs 1-3), 1: 4x bunny (config 4), 2: 1M-tri plane
 * (config 5). */
int rt_scene_setup(rt_scene* scene, int which, const char* assets_dir);
/* Config-5 scene with an n x n quad grid (n = 708 for the benchmark). */
int rt_scene_setup_plane(rt_scene* scene, int n, const char* assets_dir);
/* Host views of the scene arrays (valid until the next modification). */
size_t rt_scene_host_arrays(const rt_scene* scene, const GPUBVHNode** nodes, size_t* node_count,
                            const uint32_t** face_indices, size_t* face_count, const GPUVertex** vertices,
                            size_t* vertex_count, const GPUFace** faces);
/* The BVH's depth.  rt_render, rt_trace_rays, rt_occluded, rt_ao and rt_radiance refuse a scene deeper than 62 levels (the
 * traversal stacks hold depth + 2 <= 64 entries; csrc/rt_variant.h kMaxBvhDepth) with an error that names the limit,
 * before anything is launched.  rt_scene_upload refuses a scene without triangles. */
int rt_scene_bvh_max_depth(const rt_scene* scene);
/* Host copy of the scene's GPUMaterial array (what rt_hit.material indexes): *count receives the
 * material count; out (may be NULL) receives the records.  0 or -1 with rt_last_error(). */
int rt_scene_materials(rt_scene* scene, void* out, size_t* count);
/* Host copy of the scene's sphere array (what rt_hit.id indexes on a sphere hit), 32 bytes each: centre[3], radius,
 * material (int32), 12 bytes of padding.  *count receives the sphere count; out (may be NULL) receives the records.
 * 0 or -1 with rt_last_error(). */
int rt_scene_spheres(rt_scene* scene, void* out, size_t* count);

/* Build options (process-wide; affect later rt_scene_upload / mirror builds and
 * rt_bvh_build_device calls).  None of them changes a rendered bit -- the leaf trees and the GPU
 * BVH builder are exact -- only speed; they replace environment knobs so that nothing in the
 * shipped path reads the environment.  rt_get_build_options fills the current values (defaults
 * on first use); rt_set_build_options(NULL) restores the defaults. */
typedef struct rt_build_options {
    uint32_t leaf_tree_min;   /* leaves with at least this many triangles get a leaf tree (1024) */
    uint32_t cut_clusters;    /* leaf trees: clusters per subtree of the flat cut, 1..32 (32) */
    uint32_t cluster_max;     /* leaf trees: triangles per tree leaf, 1..16 (16) */
    float split_angle;        /* leaf trees: split by normals while the cone half-angle exceeds this, rad (0.03) */
    uint32_t bvh_small;       /* GPU BVH builder: nodes this small build their subtree in one thread, 2..64 (16) */
    int32_t host_bvh;         /* 1: rt_scene_upload always builds the BVH on the host (0: GPU from 65,536 faces) */
    int32_t leaf_screens;     /* 1: big leaves whose core can be culled get a screen record (mirror.h pf = 3),
                                 rendered by the screen variants of librt_hip_exp.so (A/B, measured slower) (0) */
    int32_t entry_frontier;   /* 1: the lean render kernels start camera rays from their 8x8 sub-tile's entry record
                                 instead of the BVH root (csrc/entry_frontier.h); read by rt_render at every frame; same
                                 frame bit for bit, a third fewer traversal steps per lane, frame time within noise (0) */
} rt_build_options;
void rt_get_build_options(rt_build_options* out);
int rt_set_build_options(const rt_build_options* options);  /* 0, or an error for out-of-range values */

/* Entry frontier (csrc/entry_frontier.h).  rt_render keeps, per uploaded scene, a device table of entry records
 * -- one per 8x8 sub-tile of the viewport -- and rebuilds it, with one kernel on the render's stream, only when the
 * camera, the viewport or the scene's node array changes.  rt_entry_table_builds counts those rebuilds
 * (process-wide). */
uint64_t rt_entry_table_builds(void);

/* The reference's BVH builder (BVH::Calculate, RayTracing/BVH.cpp:8-124) run on the GPU over
 * device arrays: nodes and face indices byte-identical to the host builder (depth-first node
 * numbering, the swap partition's permutation including failed axes).  nodes_out holds
 * 2 * face_count - 1 nodes; *node_count_out receives nodes_used, *max_depth_out the deepest level.
 * Vertex positions must be finite.  Synchronises `stream`.  Returns 0 or an error code. */
int rt_bvh_build_device(const GPUVertex* vertices, uint32_t vertex_count, const GPUFace* faces, uint32_t face_count,
                        GPUBVHNode* nodes_out, uint32_t* face_indices_out, uint32_t* node_count_out,
                        int* max_depth_out, void* stream);

/* Diagnostics for the tests: the kernel's private triangle mirror (cuda-raytracing_amd/csrc/
   mirror.h: leaf-ordered records, 12 floats; leaf-tree nodes, 16 floats; leaf-tree triangle
   records, 12 floats) built on the host from the scene's host arrays, and the render kernel's
   leaf-tree cull predicate (rt_fast.h cluster_cull) evaluated on the host by the same code.
   Returns 0 (cull: 1 = culled), or -1 with rt_last_error(). */
int rt_scene_mirror_info(rt_scene* scene, size_t* tri_records, size_t* tree_nodes, size_t* tree_tri_records);
int rt_scene_mirror_copy(rt_scene* scene, float* tris, float* tree, float* tree_tris);
int rt_cluster_cull_host(const float origin[3], const float nd[3], float best, const float node[16]);
/* The twin test of the big-leaf quads (rt_fast.h twin_rejected, mirror.h quads) on the host: bit 0
   the twin of triangle record `rec` (v0, e2, e1) is proven rejected from rec's own glm values for the
   ray (origin, nd), bit 1 the twin passes glm's predicate, bit 2 rec does.  For tests. */
int rt_twin_check_host(const float rec[12], const float origin[3], const float nd[3]);
/* The same with the bounds the render kernel uses, formed once per leaf visit (rt_fast.h twin_rejected_pre,
   twin_visit): bounds = (KD, KE, DN) stands for the triangle's own (kd, ke, |origin - v0|_1).  Bits 0-2 as
   above, bit 0 by the hoisted form; bit 3: the packed evaluation of the shared-leaf loop (both halves) and the
   scalar one disagree.  For tests. */
int rt_twin_check_bounds_host(const float rec[12], const float origin[3], const float nd[3], const float bounds[3]);
/* twin_visit on the host: out = (DN, M, M2) for a ray origin, the box [lo, hi] of a leaf's v0 and its KE. */
void rt_twin_visit_host(const float origin[3], const float lo[3], const float hi[3], float ke, float out[3]);
/* The render kernel variant rt_render chooses for a frame (csrc/rt_variant.h choose_variant), on the host and
   without a GPU: in = {tune, stats, lane_cost, refill, has_tree, screens, arrays_complete, depth, want_entry},
   out = {family, mode, stack, needs_plugin, use_entry}.  rt_family_has_mode_host: 1 when the translation unit
   of `family` instantiates `mode` (csrc/rt_render.h, the family table).  For tests. */
void rt_variant_host(const int32_t in[9], int32_t out[5]);
int rt_family_has_mode_host(int family, int mode);
/* The traversal's private node array (mirror.h nodes: GPUBVHNode records, sibling pairs 64-B
   aligned in right-first pre-order), built on the host: *count receives the node count; nodes (may
   be NULL) receives the records.  0 or -1 with rt_last_error(). */
int rt_scene_mirror_nodes(rt_scene* scene, GPUBVHNode* nodes, size_t* count);
/* The big leaves' twin records (mirror.h quads: 28 floats each, units: 16 floats each), built on the
   host: counts first, then the arrays when the pointers are not NULL.  0 or -1. */
int rt_scene_mirror_twins(rt_scene* scene, float* quads, size_t* quad_count, float* units, size_t* unit_count);
/* The twin record (mirror.h pairs: KD, KE, KDD, KDD1, lo.xyz, 0, hi.xyz, 0) of the big leaf whose first
   leaf-ordered record is `first`, built on the host.  0, or -1 when that leaf has no twin records. */
int rt_scene_mirror_leaf_twin(rt_scene* scene, uint32_t first, float rec[12]);
/* Scenes with big leaves: the leaf of every face (mirror.h face_leaf: the private node index, 0xffffffff
   in no leaf, 0xfffffffe in two), which the deferred leaves' guard reads (rt_fast.h).  *count receives
   the face count (0 for scenes without big leaves); leaf (may be NULL) the table.  0 or -1. */
int rt_scene_mirror_face_leaf(rt_scene* scene, uint32_t* leaf, size_t* count);
/* rt_closest_point's answer by brute force on the host, over the scene's host arrays (no BVH, no device): every
   sphere and every face for every point, by the kernel's own source (csrc/closest.h).  The oracle of the GPU tests
   on scenes too large for an interpreter; itself pinned to a numpy restatement of the rules (tests/closest_ref.py).
   0, or -1 with rt_last_error(). */
int rt_closest_point_host(rt_scene* scene, const rt_point* points, int64_t count, rt_nearest* out);
/* closest.h box_bound on the host, for tests: the lower bound of the computed d2 of every face whose vertices lie in
   the box [lo, hi] (-1: no bound), which the kernel's cull compares with the best so far. */
float rt_closest_bound_host(const float p[3], const float lo[3], const float hi[3]);
/* rt_trace_hits' list (csrc/hit_list.h offer, the kernel's own source) on the host, for tests: the n pairs (t[j],
   payload[j]) offered in order to an empty list of max_hits (1 .. RT_HITS_MAX) entries under `tmax`, with the bound
   held at tmax when count_all is not 0.  out_t / out_payload (max_hits each) receive the list, *total (may be NULL)
   the number of offers accepted.  Payloads are opaque here and must not be 0xffffffff.  Returns the list's length,
   or -1 with rt_last_error(). */
int rt_hit_list_host(int max_hits, float tmax, int count_all, int64_t n, const float* t, const uint32_t* payload,
                     float* out_t, uint32_t* out_payload, int64_t* total);

/* Test hook: the private mirror built on the host from raw reference arrays (the foreign-scene path,
   rt_render on a GPUScene not uploaded by rt_scene_upload): words 10-11 of every leaf-ordered record --
   a big leaf's first record (first pair, kind), second and third (its twin quads, its units) -- as
   2 x index_count uint32 in `meta`, and whether twin records were built (0 when big-leaf ranges overlap
   so that their metadata records would collide).  0 or -1 (rt_last_error). */
int rt_mirror_build_check(const GPUBVHNode* nodes, size_t node_count, const uint32_t* face_indices, size_t index_count,
                          const GPUFace* faces, size_t face_count, const GPUVertex* vertices, size_t vertex_count,
                          uint32_t* meta, int* twins);

/* XORWOW jump matrix A^(4^k * 2^67) (k < 32) as 800 uint32 words in rocrand's layout
 * m[i*160 + j*5 + w] (input word i, bit j, output word w).  For tests. */
int rt_xorwow_jump_matrix(int k, uint32_t out[800]);
/* Host-side curand_init(seed, subsequence, 0) for tests. */
void rt_xorwow_init_host(uint32_t seed, uint64_t subsequence, rt_rng_state* out);

#ifdef __cplusplus
}
#endif

#endif /* RT_ABI_H */
