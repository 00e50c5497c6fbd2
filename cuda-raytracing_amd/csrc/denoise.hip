// denoise.hip -- rt_denoise (include/rt_abi.h): an edge-avoiding a-trous wavelet filter for low-sample frames,
// guided by the first-hit records of rt_trace_rays' camera mode (normal, position, distance, material).
//
// The arithmetic is the one rt_abi.h specifies and tests/denoise_ref.py restates in numpy: fp32, no
// contraction, IEEE division (the flags of every unit, build.py), only + - * /, fmaxf, fabsf and comparisons,
// so the GPU and the restatement agree bit for bit.  Three kernels, all one pixel per lane:
//
//   prepare   surface / albedo -> colour buffer A; the guide packed into two float4 per pixel:
//             g0 = (n.xyz, sigma_plane * t), g1 = (pos.xyz, tag) with tag = 0 for a miss, 1 for a hit
//             whose material index is beyond the table (albedo 1), material + 2 otherwise
//   pass      5x5 taps at stride 1 << s from one colour buffer into the other (A -> B -> A ...)
//   the last pass multiplies the albedo back in and writes the pitched output surface.  It reads only
//             scratch and the material table, which is why out == surface is safe: prepare has consumed
//             the whole input surface before, in stream order.
//
// The two shapes of a pass (an LDS tile for step 1 and 2, global memory from step 4 on) are atrous.h's, which
// rt_denoise_variance shares; this unit holds the colour filter's policy: its tap, its result, its arguments.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "atrous.h"
#include "image_entry.h"
#include "rt_abi.h"

namespace {

using namespace atrous;
using namespace rt_entry;

constexpr int DEFAULT_ITERATIONS = 5;
constexpr int DEFAULT_NORMAL_POWER_LOG2 = 5;
constexpr float DEFAULT_SIGMA_PLANE = 0.03f;
constexpr float DEFAULT_SIGMA_COLOR = 8.0f;

__global__ __launch_bounds__(256) void denoise_prepare(const char* surface, uint64_t pitch, int width, int height,
                                                       const float4* hits, const GPUMaterial* materials,
                                                       uint32_t material_count, float sigma_plane, float4* g0, float4* g1,
                                                       float4* colour) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= width || y >= height) return;
    const size_t p = (size_t)y * width + x;
    const float4 h0 = hits[3 * p], h1 = hits[3 * p + 1], h2 = hits[3 * p + 2];  // (t kind id material) (n bx) (pos by)
    const uint32_t tag = tag_of(h0, material_count);
    colour[p] = demodulated(surface, pitch, x, y, tag, materials);
    g0[p] = make_float4(h1.x, h1.y, h1.z, sigma_plane * h0.x);
    g1[p] = make_float4(h2.x, h2.y, h2.z, __uint_as_float(tag));
}

struct PassArgs {
    const float4* g0;
    const float4* g1;
    const float4* cin;
    float4* cout;            // not the last pass
    char* out;               // the last pass: the pitched output surface
    uint64_t out_pitch;
    const GPUMaterial* materials;
    int width, height, step;
    int normal_power_log2;
    float sigma_color, sc2;  // sc2 = (sigma_color * 2^-s)^2, unused when sigma_color == 0
};

// The centre pixel of a pass and its running sums
struct Centre {
    float4 g0, g1, c;  // (n, sigma_plane * t), (pos, tag), colour
    bool use_colour;
    float sx = 0.0f, sy = 0.0f, sz = 0.0f, wsum = 0.0f;
};

// the colour filter as atrous.h's passes see it
struct ColourFilter {
    using Args = PassArgs;
    using Centre = ::Centre;
    static constexpr float EMPTY_W = 0.0f;

    static __device__ __forceinline__ void begin_global(Centre& k, const PassArgs& a, int, int) {
        k.use_colour = a.sigma_color > 0.0f && finite3(k.c);
    }
    template <int HX>
    static __device__ __forceinline__ void begin_lds(Centre& k, const PassArgs& a, const float4*, int) {
        begin_global(k, a, 0, 0);
    }

    static __device__ __forceinline__ void tap(Centre& k, const PassArgs& a, float hw, const float4& gq0, const float4& gq1, const float4& cq) {
        float wz;
        const float wn = guide_weight(k.g0, k.g1, gq0, gq1, a.normal_power_log2, wz);
        float wc = 1.0f;
        if (k.use_colour) {
            const float ex = cq.x - k.c.x, ey = cq.y - k.c.y, ez = cq.z - k.c.z;
            wc = 1.0f / (1.0f + dot3(ex, ey, ez, ex, ey, ez) / a.sc2);
        }
        const float w = ((hw * wn) * wz) * wc;
        if (w > 0.0f) {
            k.sx += cq.x * w, k.sy += cq.y * w, k.sz += cq.z * w;
            k.wsum += w;
        }
    }

    // the pass's result for pixel (x, y): the weighted mean (or the centre's own colour), remodulated by the last pass
    template <bool LAST>
    static __device__ __forceinline__ void finish(const Centre& k, const PassArgs& a, int x, int y, bool filtered) {
        float ox = k.c.x, oy = k.c.y, oz = k.c.z;
        if (filtered && k.wsum > 0.0f) ox = k.sx / k.wsum, oy = k.sy / k.wsum, oz = k.sz / k.wsum;
        if (LAST) {
            float ax, ay, az;
            albedo_of(__float_as_uint(k.g1.w), a.materials, ax, ay, az);
            *reinterpret_cast<float4*>(a.out + (size_t)y * a.out_pitch + (size_t)x * 16) = make_float4(ox * ax, oy * ay, oz * az, k.c.w);
        } else {
            a.cout[(size_t)y * a.width + x] = make_float4(ox, oy, oz, k.c.w);
        }
    }
};

template <bool LAST>
__global__ __launch_bounds__(256) void denoise_pass(const PassArgs a) {
    pass_global<ColourFilter, LAST>(a);
}

template <int STEP, bool LAST>
__global__ __launch_bounds__(256) void denoise_pass_lds(const PassArgs a) {
    pass_lds<ColourFilter, STEP, LAST>(a);
}

struct ColourPasses {  // launch_passes' view of the kernels
    static auto global(bool last) { return last ? denoise_pass<true> : denoise_pass<false>; }
    template <int STEP>
    static auto lds(bool last) { return last ? denoise_pass_lds<STEP, true> : denoise_pass_lds<STEP, false>; }
    static void at_step(PassArgs& a, int s) {
        const float sc = a.sigma_color * (1.0f / (float)(1 << s));  // a power of two: exact
        a.sc2 = sc * sc;
    }
};

}  // namespace

extern "C" size_t rt_denoise_scratch_bytes(int width, int height) {
    if (width <= 0 || height <= 0) return 0;
    return (size_t)width * (size_t)height * 64u;  // g0, g1, colour A, colour B: one float4 each per pixel
}

extern "C" int rt_denoise(const rt_denoise_params* p, void* stream) {
    const char* const who = "rt_denoise";
    if (!p) return refuse(who, "null params");
    if (!p->surface) return refuse(who, "null surface");
    if (!p->hits) return refuse(who, "null hits");
    if (!p->out) return refuse(who, "null out");
    if (!p->scratch) return refuse(who, "null scratch");
    if (size_refused(who, p->width, p->height) || caps_refused(who, p->width, p->height, "DENOISE")) return 1;
    if (materials_refused(who, p->materials, p->material_count)) return 1;
    if (pitch_refused(who, "pitch", p->pitch, p->width) || pitch_refused(who, "out_pitch", p->out_pitch, p->width)) return 1;
    if (pitches_refused(who, {p->pitch, p->out_pitch})) return 1;
    if (misaligned(who, "surface, hits, materials, out and scratch", 16, {p->surface, p->hits, p->out, p->scratch, p->materials}))
        return 1;
    if (p->scratch_bytes < rt_denoise_scratch_bytes(p->width, p->height)) return refuse(who, "scratch too small (rt_denoise_scratch_bytes)");
    if (p->flags != 0) return refuse(who, "flags must be 0");
    const int iterations = or_default(p->iterations, RT_DENOISE_DEFAULT, DEFAULT_ITERATIONS);
    const int npow = or_default(p->normal_power_log2, RT_DENOISE_DEFAULT, DEFAULT_NORMAL_POWER_LOG2);
    const float sigma_plane = or_default(p->sigma_plane, RT_DENOISE_DEFAULT, DEFAULT_SIGMA_PLANE);
    const float sigma_color = or_default(p->sigma_color, RT_DENOISE_DEFAULT, DEFAULT_SIGMA_COLOR);
    if (iterations < 1 || iterations > 6) return refuse(who, "iterations must be 1..6 (or RT_DENOISE_DEFAULT)");
    if (npow < 0 || npow > 8) return refuse(who, "normal_power_log2 must be 0..8 (or RT_DENOISE_DEFAULT)");
    if (!finite_above(sigma_plane, 0.0f)) return refuse(who, "sigma_plane must be > 0 and finite (or RT_DENOISE_DEFAULT)");
    if (!finite_from(sigma_color, 0.0f)) return refuse(who, "sigma_color must be >= 0 and finite (or RT_DENOISE_DEFAULT)");

    hipStream_t st = (hipStream_t)stream;
    const Scratch sc = carve(p->scratch, (size_t)p->width * (size_t)p->height);
    hipLaunchKernelGGL(denoise_prepare, image_grid(p->width, p->height), dim3(256), 0, st,
                       static_cast<const char*>(p->surface), p->pitch, p->width, p->height,
                       static_cast<const float4*>(static_cast<const void*>(p->hits)), p->materials,
                       (uint32_t)p->material_count, sigma_plane, sc.g0, sc.g1, sc.colour[0]);
    PassArgs a;
    a.g0 = sc.g0, a.g1 = sc.g1;
    a.out = static_cast<char*>(p->out), a.out_pitch = p->out_pitch;
    a.materials = p->materials;
    a.width = p->width, a.height = p->height;
    a.normal_power_log2 = npow;
    a.sigma_color = sigma_color;
    launch_passes<ColourPasses>(a, sc.colour, iterations, st);
    return launch_refused(who);
}
