// rt_render.hip -- rt_render (rt_abi.h): one frame, or one shard of it, from the checks of its arguments to the launch
// of the kernel that renders it, as a sequence of stages, each a function below in the order rt_render calls them.
// That order is the order of the refusals (tests/test_render_errors_cpu.py, tests/test_gpu_render_errors.py) and of
// the side effects: a foreign scene's fingerprint kernels are enqueued before the later refusals are made.
// Also here: the launch table of the render families and the plugin's registration (rt_render.h), the lone-pixel
// side streams, the refill counter, and the reference's raytracing_process.
//
// Kernels here
//   mark_slots_kernel, check_lanes_kernel   RT_RENDER_VALIDATE: lone_slots and lane_slots are disjoint.
// The render kernels live in their own translation units (rt_render.h): rt_fast_*.hip (the production tracer,
// rt_fast_body.h + rt_fast.h, per variant family) and rt_ref.hip (the reference-layout and flat tracers).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <string>

#include "rt_abi.h"
#include "rt_host.h"
#include "rt_render.h"
#include "image_entry.h"

using namespace rt_host;
using namespace rtk;
using rt_entry::refuse;

// ---------------------------------------------------------------------------------------
// The launch table of render_fast_body's families (rt_render.h), indexed by Family: the product's rows filled in
// here, the plugin's by register_experimental_kernels (null, and rt_render refuses the frame, until then).
// ---------------------------------------------------------------------------------------
static std::atomic<FastLauncher> g_family[FAM_COUNT] = {{launch_fast_prod}, {launch_fast_lean}, {launch_fast_timing},
                                                        {launch_fast_stats}};
static_assert(FAM_PROD == 0 && FAM_LEAN == 1 && FAM_TIMING == 2 && FAM_STATS == 3 && FAM_AB == 4, "g_family's order");
static std::atomic<const ExperimentalKernels*> g_experimental{nullptr};  // the plugin's table: its lone-pixel and wavefront paths

void rtk::register_experimental_kernels(const rtk::ExperimentalKernels* k, uint32_t abi) {
    if (k && abi != rtk::kExperimentalAbi) {  // a plugin built against another RenderArgs / table layout
        char msg[160];
        std::snprintf(msg, sizeof msg, "librt_hip_exp.so refused: its ABI stamp 0x%08x is not librt_hip.so's 0x%08x "
                      "(rebuild both)", abi, rtk::kExperimentalAbi);
        set_error(msg);
        return;
    }
    g_experimental.store(k);
    for (int f = rtk::FAM_AB; f < rtk::FAM_COUNT; f++) g_family[f].store(k ? k->fast[f] : nullptr);  // the plugin's rows
}
const rtk::ExperimentalKernels* rtk::experimental_kernels() { return g_experimental.load(); }

static hipError_t launch_fast(const Variant& v, const RenderArgs& args, int waves, hipStream_t s) {
    const FastLauncher f = g_family[v.family].load();
    return f ? f(v.stack, v.mode, args, waves, s) : hipErrorNotSupported;  // rt_render refused these frames without the plugin
}

// Per-(device, stream) side stream of the lone-pixel kernel and its fork / join events.
struct LoneStreams {
    hipStream_t side = nullptr;
    hipEvent_t fork = nullptr, join = nullptr;
};
static LoneStreams* lone_streams(hipStream_t s) {
    static std::mutex mu;
    static std::map<std::pair<int, hipStream_t>, LoneStreams> all;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> lock(mu);
    LoneStreams& l = all[std::make_pair(dev, s)];
    if (!l.side && (hipStreamCreateWithFlags(&l.side, hipStreamNonBlocking) != hipSuccess ||
                    hipEventCreateWithFlags(&l.fork, hipEventDisableTiming) != hipSuccess ||
                    hipEventCreateWithFlags(&l.join, hipEventDisableTiming) != hipSuccess)) {
        l = LoneStreams{};
        return nullptr;
    }
    return &l;
}

// Per-(device, stream) queue counter of refill launches, zeroed on the stream before each launch.
static unsigned long long* queue_counter(hipStream_t s) {
    static std::mutex mu;
    static std::map<std::pair<int, hipStream_t>, unsigned long long*> counters;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> lock(mu);
    auto& c = counters[std::make_pair(dev, s)];
    if (!c && hipMalloc(&c, sizeof(unsigned long long)) != hipSuccess) c = nullptr;
    return c;
}

// RT_RENDER_VALIDATE: lone_slots and lane_slots must be disjoint (a slot in both is rendered twice
// at once into the same RNG state and pixel).  Marks the lone slots in a bitmap, then counts lane
// entries that hit a mark or lie outside [0, slots) (< 0 = idle lane, allowed).
__global__ __launch_bounds__(BLOCK) void mark_slots_kernel(const int32_t* list, long long n, long long slots,
                                                           uint32_t* bits, unsigned int* bad) {
    const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const int32_t v = list[i];
    if (v < 0 || v >= slots) {
        atomicAdd(bad, 1u);
        return;
    }
    if (atomicOr(bits + (v >> 5), 1u << (v & 31)) & (1u << (v & 31))) atomicAdd(bad, 1u);  // listed twice
}
__global__ __launch_bounds__(BLOCK) void check_lanes_kernel(const int32_t* lanes, long long n, long long slots,
                                                            const uint32_t* bits, unsigned int* bad) {
    const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const int32_t v = lanes[i];
    if (v < 0) return;
    if (v >= slots || (bits[v >> 5] >> (v & 31) & 1u)) atomicAdd(bad, 1u);
}

static int validate_lone(const int32_t* lone, long long nl, const int32_t* lanes, long long nm, long long slots,
                         hipStream_t s) {
    const char* const who = "rt_render";
    const size_t words = (size_t)(slots + 31) / 32;
    uint32_t* bits = nullptr;
    unsigned int* bad = nullptr;
    if (hipMallocAsync((void**)&bits, words * 4 + 8, s) != hipSuccess) return refuse(who, "validate allocation");
    bad = reinterpret_cast<unsigned int*>(bits + words);
    unsigned int h[2] = {0, 0};
    int rc = 0;
    if (hipMemsetAsync(bits, 0, words * 4 + 8, s) != hipSuccess) rc = refuse(who, "validate memset");
    if (!rc) {
        hipLaunchKernelGGL(mark_slots_kernel, dim3((unsigned)((nl + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, lone, nl, slots, bits, bad);
        hipLaunchKernelGGL(check_lanes_kernel, dim3((unsigned)((nm + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, lanes, nm, slots, bits,
                           bad + 1);
        if (hipMemcpyAsync(h, bad, 8, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
            rc = refuse(who, "validate read-back");
    }
    (void)hipFreeAsync(bits, s);
    if (rc) return rc;
    if (h[0]) return refuse(who, "RT_RENDER_VALIDATE: " + std::to_string(h[0]) + " lone_slots entries out of range or repeated");
    if (h[1]) return refuse(who, "RT_RENDER_VALIDATE: " + std::to_string(h[1]) +
                                     " lane_slots entries are out of range or also in lone_slots");
    return 0;
}

// ---------------------------------------------------------------------------------------
// rt_render's stages.  What one stage works out for the later ones, beside the kernels' RenderArgs:
// ---------------------------------------------------------------------------------------
namespace {
const char* const who = "rt_render";
struct Grid {
    int tiles;  // of the launch's list: the tile list's, or the round-robin deal's share
    int waves;  // the production tracer's grid
};
struct Source {  // where the frame's triangles come from
    MirrorDevice mir;
    int* gate = nullptr;  // foreign scenes: device flag selecting production (1) or reference-layout (0) tracer
};
struct Path {  // which kernels render the frame
    bool stats, flat, wavefront, lone;
    const GPUBVHNode* trav_nodes;  // the node array of the traversal kernels
    Variant v;                     // the production tracer's kernel
};
bool flag(const rt_render_params* p, int f) { return (p->flags & f) != 0; }
}  // namespace

static int arguments_refused(const rt_render_params* p, const GPUScene* scene) {
    if (!p || !scene) return refuse(who, "null argument");
    if (p->width <= 0 || p->height <= 0 || p->spp <= 0 || p->bounces < 0) return refuse(who, "bad frame size / spp / bounces");
    if (p->shard_count <= 0 || p->shard_index < 0 || p->shard_index >= p->shard_count) return refuse(who, "bad shard");
    if (!p->out_shard && (!p->surface || p->pitch < (uint64_t)p->width * 16))
        return refuse(who, "need a surface with pitch >= 16*width, or out_shard");
    if (p->shard_count > 1 && !p->out_shard) return refuse(who, "sharded render needs out_shard");
    if (!scene->rng_state || !scene->gpu_bvh_nodes || !scene->gpu_materials)
        return refuse(who, "scene not uploaded (rng_state / bvh / materials missing)");
    if (flag(p, RT_RENDER_STATS) && !p->stats) return refuse(who, "stats flag without buffer");
    return 0;
}

// the scene, its sky and the frame into `a`
static int fill_frame(const rt_render_params* p, const GPUScene* scene, RenderArgs* a) {
    std::memset(a, 0, sizeof(*a));
    a->spheres = scene->gpu_spheres;
    a->materials = scene->gpu_materials;
    a->nodes = scene->gpu_bvh_nodes;
    a->face_indices = scene->gpu_bvh_face_indices;
    a->vertices = scene->gpu_vertices;
    a->faces = scene->gpu_faces;
    a->rng = (rt_rng_state*)scene->rng_state;
    a->sphere_count = scene->sphere_count;
    a->cam = scene->camera;
    if (fill_sky(who, scene, a) != 0) return 1;
    a->surface = (char*)p->surface;
    a->last = (const char*)p->surface_last_frame;
    a->out_shard = (float4*)p->out_shard;
    a->pitch = p->pitch;
    a->width = p->width, a->height = p->height;
    a->frame_index = p->frame_index, a->spp = p->spp, a->bounces = p->bounces;
    a->shard_index = p->shard_index, a->shard_count = p->shard_count;
    a->tiles_x = (p->width + TILE - 1) / TILE;
    a->stats = (unsigned long long*)p->stats;
    a->seg_counter = (unsigned long long*)p->segment_counter;
    return 0;
}

// The launch's tiles, pixel slots and waves.  g->tiles == 0 on return 0: the shard has no tiles, nothing to render.
static int frame_geometry(const rt_render_params* p, RenderArgs* a, Grid* g) {
    if (p->tile_list && (p->tile_count <= 0 || p->tile_count > (int64_t)1 << 28))
        return refuse(who, "tile_list needs 0 < tile_count < 2^28");
    if (p->tile_list && !p->out_shard && p->shard_count > 1) return refuse(who, "sharded render needs out_shard");
    a->tile_list = p->tile_list;
    a->wave_clock = (unsigned long long*)p->wave_clock;
    g->tiles = p->tile_list ? (int)p->tile_count : tiles_of_shard(p->width, p->height, p->shard_index, p->shard_count);
    if (g->tiles == 0) return 0;
    if (p->lane_slots && (p->lane_slot_count <= 0 || p->lane_slot_count % WAVE != 0 || p->lane_slot_count > (int64_t)1 << 30))
        return refuse(who, "lane_slots needs a positive multiple of 64 entries (< 2^30)");
    a->lane_slots = p->lane_slots;
    a->slot_count = (long long)g->tiles * TILE * TILE;
    if (a->slot_count > (1LL << 32)) return refuse(who, "more than 2^32 pixel slots in one launch");
    a->lane_cost = p->lane_cost;
    a->priority_waves = p->lane_slots ? (int)std::min<int64_t>(std::max<int64_t>(p->priority_waves, 0), 1 << 30) : 0;
    g->waves = p->lane_slots ? (int)(p->lane_slot_count / WAVE) : g->tiles * 4;
    a->entry_count = (long long)g->waves * WAVE;
    return 0;
}

static int knobs_refused(const rt_render_params* p, RenderArgs* a) {
    if (p->refill_lanes < 0 || p->refill_lanes > 64) return refuse(who, "refill_lanes must be in [0, 64]");
    if (p->waves_per_simd < 0 || p->waves_per_simd > 7)
        return refuse(who, "waves_per_simd must be 0 (default), 1-4 (LDS-capped residency), 5, 6 or 7");
    if (((p->tune >> 9) & 3u) == 1u) return refuse(who, "RT_TUNE occupancy override 1 (compiler's choice) is not built");
    a->waves_per_simd = p->waves_per_simd;
    a->refill_lanes = p->refill_lanes;
    return 0;
}

// Every device buffer must cover what the launch touches: a short buffer would fault the GPU.
static int buffers_refused(const rt_render_params* p, const GPUScene* scene, const Grid& g) {
    const bool compact = p->out_shard != nullptr;
    const size_t slots = (size_t)g.tiles * TILE * TILE;
    const size_t frame = (size_t)p->pitch * (size_t)(p->height - 1) + (size_t)p->width * 16;
    const size_t rng_need = (compact ? slots : (size_t)p->width * p->height) * sizeof(rt_rng_state);
    if (bytes_from(scene->rng_state) < rng_need) return refuse(who, "rng_state is smaller than the frame / shard");
    if (compact && bytes_from(p->out_shard) < slots * 16) return refuse(who, "out_shard too small");
    if (compact && p->surface_last_frame && bytes_from(p->surface_last_frame) < slots * 16)
        return refuse(who, "surface_last_frame (shard) too small");
    if (!compact && bytes_from(p->surface) < frame) return refuse(who, "surface too small");
    if (!compact && p->surface_last_frame && bytes_from(p->surface_last_frame) < frame)
        return refuse(who, "surface_last_frame too small");
    if (p->tile_list && bytes_from(p->tile_list) < (size_t)g.tiles * 4) return refuse(who, "tile_list too small");
    if (p->wave_clock && bytes_from(p->wave_clock) < (size_t)g.waves * 8) return refuse(who, "wave_clock too small");
    if (p->lane_slots && bytes_from(p->lane_slots) < (size_t)p->lane_slot_count * 4) return refuse(who, "lane_slots too small");
    if (p->lane_cost && bytes_from(p->lane_cost) < slots * 4) return refuse(who, "lane_cost too small");
    const size_t stats_need = (RT_STAT_COUNT + ((p->tune & 2048u) ? (size_t)g.waves * 8 : 0)) * 8;
    if (p->stats && bytes_from(p->stats) < stats_need) return refuse(who, "stats too small");
    return 0;
}

// The scene's mirror: its own (rt_scene_upload), or a foreign scene's fingerprint-gated private one -- no host sync,
// and none at all until it is built: reference layout, ungated.  The reference-layout tracer asks for neither.
static int resolve_mirror(const rt_render_params* p, const GPUScene* scene, hipStream_t s, Source* src) {
    if ((!rt_internal_lookup_mirror(scene, &src->mir) || !src->mir.owned) && !flag(p, RT_RENDER_TRACER_REF)) {
        bool foreign_fast = false;
        if (foreign_frame(scene, s, &src->mir, &foreign_fast, &src->gate) != 0) return 1;
        if (!foreign_fast) src->gate = nullptr, src->mir = MirrorDevice{};
    }
    return depth_refused(who, src->mir.depth) ? 1 : 0;  // before any launch, the reference-layout tracers' included
}

// the mirror's arrays into `a`, but for those an RT_TUNE A/B knob turns off (0 = the production path)
static void fill_mirror(const rt_render_params* p, const MirrorDevice& mir, RenderArgs* a) {
    a->tune = p->tune;
    a->pairs = (a->tune & 2u) ? nullptr : (const float4*)mir.pairs;
    a->quads = (a->tune & ((1u << 20) | 2u)) ? nullptr : (const float4*)mir.quads;  // RT_TUNE bit 20: no twins
    a->units = (const float4*)mir.units;
    a->tree = (a->tune & 4u) ? nullptr : (const float4*)mir.tree;
    a->ltris = (const float4*)mir.ltris;
    a->spairs = (a->tune & 8u) ? nullptr : (const float4*)mir.spairs;
    a->flat = (const float4*)mir.flat;
    a->face_leaf = (const uint32_t*)mir.face_leaf;
    a->tris = flag(p, RT_RENDER_TRACER_REF) ? nullptr : (const FlatTri*)mir.tris;
}

// Which kernels render the frame, and whether the caller's options go with them.
static int choose_path(const rt_render_params* p, const GPUScene* scene, const Source& src, hipStream_t s, RenderArgs* a,
                       Path* path) {
    const MirrorDevice& mir = src.mir;
    int* const gate = src.gate;
    const bool stats = path->stats = flag(p, RT_RENDER_STATS);
    const bool want_flat = path->flat = flag(p, RT_RENDER_TRACER_FLAT);
    if ((p->lane_slots || p->lane_cost || p->refill_lanes) && (gate || !a->tris || want_flat))
        return refuse(who, "lane_slots / lane_cost / refill_lanes need the production tracer on an rt_scene_upload scene");
    if (p->lane_cost && p->refill_lanes) return refuse(who, "lane_cost probes run without refill");
    const bool want_wf = path->wavefront = flag(p, RT_RENDER_TRACER_WAVEFRONT);
    if (want_wf && (gate || !a->tris || want_flat || stats || p->lane_cost || p->refill_lanes || p->wave_clock ||
                    p->lone_count))
        return refuse(who, "the wavefront tracer needs an rt_scene_upload scene and no statistics / lane_cost / "
                           "wave_clock / refill / lone frames");
    // its pixel state packs the sample count in 16 bits and the bounce in 8; a generation per segment
    if (want_wf && (p->spp > 65535 || p->bounces > 255 || (int64_t)p->spp * p->bounces > 65536))
        return refuse(who, "the wavefront tracer needs spp <= 65535, bounces <= 255, spp x bounces <= 65536");
    a->screens = (mir.screens > 0 && (a->tune & (1u << 28)) == 0 && a->tris && !want_flat) ? 1 : 0;
    // the traversal kernels read the mirror's private node array (mirror.h: 64-B aligned sibling
    // pairs in right-first pre-order; RT_TUNE bit 27: the reference's array instead, A/B); the
    // reference-layout tracers keep the reference's
    path->trav_nodes = (mir.nodes && (a->tune & (1u << 27)) == 0) ? (const GPUBVHNode*)mir.nodes : scene->gpu_bvh_nodes;
    // Camera rays' entry records (entry_frontier.h): scenes with their own mirror inside the filtered range, not the
    // foreign / gated path -- on the frames choose_variant gives a lean kernel
    rt_build_options bo;
    rt_get_build_options(&bo);
    const bool want_entry = bo.entry_frontier && mir.owned && !gate && a->tris && !want_flat && !want_wf && mir.fast &&
                            path->trav_nodes == (const GPUBVHNode*)mir.nodes;
    // the production tracer's kernel for this frame (rt_variant.h; the fields in VariantInput's order); the wavefront
    // tracer and the lone-pixel kernel are paths of their own, in the plugin as well
    const bool arrays_complete = a->nodes && a->tris && a->spairs && a->pairs && a->quads && a->units;
    path->v = choose_variant({a->tune, stats, a->lane_cost != nullptr, a->refill_lanes != 0, a->tree != nullptr, a->screens != 0,
                              arrays_complete, mir.depth, want_entry});
    if (!g_experimental.load() && (want_wf || p->lone_count > 0 || path->v.needs_plugin))
        return refuse(who, "this frame asks for an experimental render path (wavefront tracer, refill, lone-pixel "
                           "kernel or an RT_TUNE A/B variant), which lives in librt_hip_exp.so -- load it first "
                           "(rt.load_experimental())");
    const bool lone = path->lone = p->lone_count > 0;
    if (p->lone_count < 0 || p->lone_count > (int64_t)1 << 28 || (lone && !p->lone_slots))
        return refuse(who, "lone_count must be in [0, 2^28] with lone_slots");
    if (lone && (!p->lane_slots || gate || !a->tris || want_flat || stats || p->lane_cost || p->refill_lanes))
        return refuse(who, "lone_slots need lane_slots and the production tracer on an rt_scene_upload scene "
                           "(no statistics / lane_cost / refill frames)");
    if (lone && (!mir.treelets || mir.depth < 0 || mir.depth > 75))
        return refuse(who, "lone_slots need the scene's treelets (a BVH of depth <= 75 with an inner root)");
    if (lone && bytes_from(p->lone_slots) < (size_t)p->lone_count * 4) return refuse(who, "lone_slots too small");
    if (flag(p, RT_RENDER_VALIDATE) && lone &&
        validate_lone(p->lone_slots, p->lone_count, p->lane_slots, p->lane_slot_count, a->slot_count, s) != 0)
        return 1;
    return 0;
}

// refill: the queue counter, zeroed on the launch stream
static int refill_counter(const rt_render_params* p, hipStream_t s, RenderArgs* a) {
    if (!p->refill_lanes) return 0;
    a->queue_head = queue_counter(s);
    if (!a->queue_head) return refuse(who, "cannot allocate the refill queue counter");
    return check(hipMemsetAsync(a->queue_head, 0, sizeof(unsigned long long), s), "hipMemsetAsync") != 0 ? 1 : 0;
}

// the arguments as they stand at launch, with the traversal's nodes
static RenderArgs traversal_args(const RenderArgs& a, const Path& path, const MirrorDevice& mir) {
    RenderArgs f = a;
    f.nodes = path.trav_nodes;
    // the face -> leaf table holds private-array node indices: with the reference's array (bit 27) the
    // deferral guard must not look them up there -- without a table it walks the leaf up to the entry
    if (path.trav_nodes != (const GPUBVHNode*)mir.nodes) f.face_leaf = nullptr;
    return f;
}

// The frame's kernels on `s`; the lone-pixel kernel, if the frame has one, on `side`.
static hipError_t launch(const rt_render_params* p, const Source& src, const Path& path, const Grid& g, RenderArgs& a,
                         hipStream_t s, hipStream_t side) {
    const int depth = src.mir.depth;
    if (src.gate) {  // foreign scene with a mirror: exactly one of the two runs, by the frame's fingerprint
        a.gate = src.gate, a.gate_value = 1;
        hipError_t e = path.flat ? launch_ref_tracer(true, a, g.tiles * 4, depth, path.stats, s)
                                 : launch_fast(path.v, traversal_args(a, path, src.mir), g.waves, s);
        if (e != hipSuccess) return e;
        RenderArgs r = a;
        r.tris = nullptr, r.gate_value = 0;
        return launch_ref_tracer(false, r, g.tiles * 4, -1, path.stats, s);
    }
    if (!a.tris) return launch_ref_tracer(false, a, g.tiles * 4, depth, path.stats, s);
    if (path.flat) return launch_ref_tracer(true, a, g.tiles * 4, depth, path.stats, s);
    if (path.wavefront) return g_experimental.load()->wavefront(traversal_args(a, path, src.mir), depth, s);
    if (path.lone) {
        const hipError_t e = g_experimental.load()->lone(a, p->lone_slots, (int)p->lone_count, src.mir.treelets, side);
        if (e != hipSuccess) return e;
    }
    return launch_fast(path.v, traversal_args(a, path, src.mir), g.waves, s);
}

extern "C" int rt_render(const rt_render_params* p, const GPUScene* scene, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    RenderArgs a;
    Grid g;
    Source src;
    Path path;
    if (arguments_refused(p, scene) || fill_frame(p, scene, &a) || frame_geometry(p, &a, &g)) return 1;
    if (g.tiles == 0) return 0;
    if (knobs_refused(p, &a) || buffers_refused(p, scene, g) || resolve_mirror(p, scene, s, &src)) return 1;
    fill_mirror(p, src.mir, &a);
    if (choose_path(p, scene, src, s, &a, &path) || refill_counter(p, s, &a)) return 1;
    a.scene_fast = src.mir.fast ? 1 : 0;
    if (path.v.use_entry && !(a.entry = entry_table(src.mir, a.cam, p->width, p->height, s)))
        path.v.use_entry = false, path.v.stack = variant_stack(src.mir.depth);  // no table: every ray from the root
    // the lone-pixel kernel runs on a side stream forked from and joined back into the caller's
    LoneStreams* ls = nullptr;
    if (path.lone) {
        if (!(ls = lone_streams(s))) return refuse(who, "cannot create the lone-pixel stream");
        if (check(hipEventRecord(ls->fork, s), "hipEventRecord") || check(hipStreamWaitEvent(ls->side, ls->fork, 0), "hipStreamWaitEvent"))
            return 1;
    }
    const hipError_t e = launch(p, src, path, g, a, s, ls ? ls->side : nullptr);
    if (ls && (check(hipEventRecord(ls->join, ls->side), "hipEventRecord") || check(hipStreamWaitEvent(s, ls->join, 0), "hipStreamWaitEvent")))
        return 1;
    return check(e, "render_kernel launch");
}

// The reference's entry point (main_raytracing.cu): the whole frame on the null stream, Release's sample count.
extern "C" void raytracing_process(void* surface, void* surface_last_frame, int width, int height, size_t pitch,
                                   int frame_index, GPUScene* scene) {
    rt_render_params p;
    std::memset(&p, 0, sizeof(p));
    p.surface = surface;
    p.surface_last_frame = surface_last_frame;
    p.width = width, p.height = height, p.pitch = pitch;
    p.frame_index = frame_index;
    p.spp = 5;      // main_raytracing.cu:166-170 (Release)
    p.bounces = 6;  // main_raytracing.cu:115
    p.shard_index = 0, p.shard_count = 1;
    if (rt_render(&p, scene, nullptr) != 0)
        std::printf("(raytracing_kernel_main) failed to launch error = %s\n", rt_last_error());
}
