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
// The pass gathers 25 taps x 48 B per pixel.  Its shape is the fastest of those measured
// (profiles/denoise_timing.txt; the slower ones are not kept): the passes of
// step 1 and 2, whose taps neighbouring lanes share, read them from an LDS tile loaded once per block; the
// passes of step 4 and more read global memory, a wave covering 64 x 1 pixels so that a tap's 64 loads are
// 8 whole cache lines per buffer, with the 15 loads of a row of taps issued together before any is tested.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdint>
#include <cstdio>

#include "mirror.h"  // rt_internal_set_error
#include "rt_abi.h"

namespace {

constexpr int DEFAULT_ITERATIONS = 5;
constexpr int DEFAULT_NORMAL_POWER_LOG2 = 5;
constexpr float DEFAULT_SIGMA_PLANE = 0.03f;
constexpr float DEFAULT_SIGMA_COLOR = 8.0f;
constexpr float ALBEDO_FLOOR = 0.015625f;  // 2^-6

__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) {
    return (ax * bx + ay * by) + az * bz;  // rtm::dot's order
}

__device__ __forceinline__ bool finite1(float v) { return fabsf(v) <= FLT_MAX; }
__device__ __forceinline__ bool finite3(const float4& c) { return finite1(c.x) && finite1(c.y) && finite1(c.z); }

// tag -> the albedo floor-clamped as the filter divides and multiplies by it
__device__ __forceinline__ void albedo_of(uint32_t tag, const GPUMaterial* materials, float& ax, float& ay, float& az) {
    float r = 1.0f, g = 1.0f, b = 1.0f;
    if (tag >= 2u) {
        const float4 alb = *reinterpret_cast<const float4*>(materials[tag - 2u].albedo);
        r = alb.x, g = alb.y, b = alb.z;
    }
    ax = fmaxf(r, ALBEDO_FLOOR), ay = fmaxf(g, ALBEDO_FLOOR), az = fmaxf(b, ALBEDO_FLOOR);
}

__global__ __launch_bounds__(256) void denoise_prepare(const char* surface, uint64_t pitch, int width, int height,
                                                       const float4* hits, const GPUMaterial* materials,
                                                       uint32_t material_count, float sigma_plane, float4* g0, float4* g1,
                                                       float4* colour) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= width || y >= height) return;
    const size_t p = (size_t)y * width + x;
    const float4 h0 = hits[3 * p], h1 = hits[3 * p + 1], h2 = hits[3 * p + 2];  // (t kind id material) (n bx) (pos by)
    const uint32_t kind = __float_as_uint(h0.y), material = __float_as_uint(h0.w);
    const uint32_t tag = kind == 0u ? 0u : (material < material_count ? material + 2u : 1u);
    float ax, ay, az;
    albedo_of(tag, materials, ax, ay, az);
    const float4 s = *reinterpret_cast<const float4*>(surface + (size_t)y * pitch + (size_t)x * 16);
    colour[p] = make_float4(s.x / ax, s.y / ay, s.z / az, s.w);
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

// The centre pixel of a pass and its running sums; tap() is the filter's one tap, the same code whichever
// way a kernel fetches the tap's three float4.
struct Centre {
    float4 g0, g1, c;  // (n, sigma_plane * t), (pos, tag), colour
    bool use_colour;
    float sx = 0.0f, sy = 0.0f, sz = 0.0f, wsum = 0.0f;
};

__device__ __forceinline__ void tap(Centre& k, const PassArgs& a, float hw, const float4& gq0, const float4& gq1, const float4& cq) {
    float wn = fmaxf(0.0f, dot3(k.g0.x, k.g0.y, k.g0.z, gq0.x, gq0.y, gq0.z));
    for (int i = 0; i < a.normal_power_log2; ++i) wn = wn * wn;
    const float d = fabsf(dot3(k.g0.x, k.g0.y, k.g0.z, gq1.x - k.g1.x, gq1.y - k.g1.y, gq1.z - k.g1.z));
    float wz = fmaxf(0.0f, 1.0f - d / k.g0.w);  // sigma_plane * t == 0: inf or NaN -> 0
    wz = wz * wz;
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
__device__ __forceinline__ void finish(const Centre& k, const PassArgs& a, int x, int y, bool filtered) {
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

// h[dy + 2] * h[dx + 2], the B3-spline kernel's weight of a tap (exact: the factors are 1, 3 and powers of two)
__device__ __forceinline__ float kernel_weight(int dy, int dx) {
    const float h[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    return h[dy + 2] * h[dx + 2];
}

// Taps straight from global memory, for the passes of step 4 and more.  A wave covers 64 x 1 pixels, so a tap's
// 64 loads are 8 whole cache lines per buffer.  The 15 loads of a row of taps are issued together, from clamped
// coordinates, before any is tested: more bytes for skipped taps, but no load waits for another (measured 20 %
// faster than loading a tap's tag, colour and normal one after the other; profiles/denoise_timing.txt).
template <bool LAST>
__global__ __launch_bounds__(256) void denoise_pass(const PassArgs a) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= a.width || y >= a.height) return;
    const size_t p = (size_t)y * a.width + x;
    Centre k;
    k.g1 = a.g1[p];
    k.c = a.cin[p];
    const bool valid = __float_as_uint(k.g1.w) != 0u;
    if (valid) {
        k.g0 = a.g0[p];
        k.use_colour = a.sigma_color > 0.0f && finite3(k.c);
#pragma unroll
        for (int dy = -2; dy <= 2; ++dy) {
            const int qy = y + dy * a.step;
            if (qy < 0 || qy >= a.height) continue;
            float4 r0[5], r1[5], rc[5];
#pragma unroll
            for (int dx = -2; dx <= 2; ++dx) {
                const int qx = min(max(x + dx * a.step, 0), a.width - 1);
                const size_t q = (size_t)qy * a.width + qx;
                r1[dx + 2] = a.g1[q], rc[dx + 2] = a.cin[q], r0[dx + 2] = a.g0[q];
            }
#pragma unroll
            for (int dx = -2; dx <= 2; ++dx) {
                const int qx = x + dx * a.step;
                if (qx < 0 || qx >= a.width || __float_as_uint(r1[dx + 2].w) == 0u || !finite3(rc[dx + 2])) continue;
                tap(k, a, kernel_weight(dy, dx), r0[dx + 2], r1[dx + 2], rc[dx + 2]);
            }
        }
    }
    finish<LAST>(k, a, x, y, valid);
}

// Taps from an LDS tile, for the passes whose taps neighbouring lanes share (STEP 1 and 2): a block's 32 x 8
// pixels and a halo of 2 * STEP around them are loaded once (1.7 / 2.5 pixels fetched per pixel instead of
// 25); a tile entry outside the image, or a miss, is stored with tag 0 and skipped like a miss.
template <int STEP, bool LAST>
__global__ __launch_bounds__(256) void denoise_pass_lds(const PassArgs a) {
    constexpr int TX = 32, TY = 8, R = 2 * STEP, HX = TX + 2 * R, HY = TY + 2 * R;
    __shared__ float4 s_g0[HX * HY], s_g1[HX * HY], s_c[HX * HY];
    const int x0 = blockIdx.x * TX - R, y0 = blockIdx.y * TY - R;
    for (int i = threadIdx.x; i < HX * HY; i += 256) {
        const int gx = x0 + i % HX, gy = y0 + i / HX;
        float4 v0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), v1 = v0, vc = v0;
        if (gx >= 0 && gx < a.width && gy >= 0 && gy < a.height) {
            const size_t q = (size_t)gy * a.width + gx;
            v1 = a.g1[q];
            if (__float_as_uint(v1.w) != 0u) v0 = a.g0[q], vc = a.cin[q];
        }
        s_g0[i] = v0, s_g1[i] = v1, s_c[i] = vc;
    }
    __syncthreads();
    const int lx = threadIdx.x % TX, ly = threadIdx.x / TX;
    const int x = blockIdx.x * TX + lx, y = blockIdx.y * TY + ly;
    if (x >= a.width || y >= a.height) return;
    const int centre = (ly + R) * HX + lx + R;
    Centre k;
    k.g1 = s_g1[centre];
    k.c = a.cin[(size_t)y * a.width + x];  // a miss's colour is not in the tile
    const bool valid = __float_as_uint(k.g1.w) != 0u;
    if (valid) {
        k.g0 = s_g0[centre];
        k.use_colour = a.sigma_color > 0.0f && finite3(k.c);
#pragma unroll
        for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
            for (int dx = -2; dx <= 2; ++dx) {
                const int q = centre + dy * STEP * HX + dx * STEP;
                const float4 gq1 = s_g1[q];
                if (__float_as_uint(gq1.w) == 0u) continue;
                const float4 cq = s_c[q];
                if (!finite3(cq)) continue;
                tap(k, a, kernel_weight(dy, dx), s_g0[q], gq1, cq);
            }
        }
    }
    finish<LAST>(k, a, x, y, valid);
}

void launch_pass(const PassArgs& a, bool last, hipStream_t st) {
    const dim3 grid((a.width + 63) / 64, (a.height + 3) / 4);
    if (last) hipLaunchKernelGGL(denoise_pass<true>, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(denoise_pass<false>, grid, dim3(256), 0, st, a);
}

template <int STEP>
void launch_pass_lds(const PassArgs& a, bool last, hipStream_t st) {
    const dim3 grid((a.width + 31) / 32, (a.height + 7) / 8);
    if (last) hipLaunchKernelGGL((denoise_pass_lds<STEP, true>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((denoise_pass_lds<STEP, false>), grid, dim3(256), 0, st, a);
}

int fail(const char* msg) {
    rt_internal_set_error(msg);
    return 1;
}

}  // namespace

extern "C" size_t rt_denoise_scratch_bytes(int width, int height) {
    if (width <= 0 || height <= 0) return 0;
    return (size_t)width * (size_t)height * 64u;  // g0, g1, colour A, colour B: one float4 each per pixel
}

extern "C" int rt_denoise(const rt_denoise_params* p, void* stream) {
    if (!p) return fail("rt_denoise: null params");
    if (!p->surface) return fail("rt_denoise: null surface");
    if (!p->hits) return fail("rt_denoise: null hits");
    if (!p->out) return fail("rt_denoise: null out");
    if (!p->scratch) return fail("rt_denoise: null scratch");
    if (p->width <= 0 || p->height <= 0) return fail("rt_denoise: width and height must be > 0");
    // the launch grids: a row of blocks per 4 (8) pixel rows in grid.y, at most 65,535
    if (p->height > RT_DENOISE_MAX_HEIGHT) return fail("rt_denoise: height above RT_DENOISE_MAX_HEIGHT");
    if ((int64_t)p->width * p->height > RT_DENOISE_MAX_PIXELS) return fail("rt_denoise: more than RT_DENOISE_MAX_PIXELS pixels");
    if (p->material_count < 0) return fail("rt_denoise: negative material_count");
    if (p->material_count > 0 && !p->materials) return fail("rt_denoise: null materials with material_count > 0");
    if (p->pitch < (uint64_t)p->width * 16) return fail("rt_denoise: pitch smaller than width * 16");
    if (p->out_pitch < (uint64_t)p->width * 16) return fail("rt_denoise: out_pitch smaller than width * 16");
    if ((p->pitch | p->out_pitch) & 15u) return fail("rt_denoise: pitches must be multiples of 16");
    if (((uintptr_t)p->surface | (uintptr_t)p->hits | (uintptr_t)p->out | (uintptr_t)p->scratch | (uintptr_t)p->materials) & 15u)
        return fail("rt_denoise: surface, hits, materials, out and scratch must be 16-byte aligned");
    if (p->scratch_bytes < rt_denoise_scratch_bytes(p->width, p->height))
        return fail("rt_denoise: scratch too small (rt_denoise_scratch_bytes)");
    if (p->flags != 0) return fail("rt_denoise: flags must be 0");
    const int iterations = p->iterations == RT_DENOISE_DEFAULT ? DEFAULT_ITERATIONS : p->iterations;
    const int npow = p->normal_power_log2 == RT_DENOISE_DEFAULT ? DEFAULT_NORMAL_POWER_LOG2 : p->normal_power_log2;
    const float sigma_plane = p->sigma_plane == (float)RT_DENOISE_DEFAULT ? DEFAULT_SIGMA_PLANE : p->sigma_plane;
    const float sigma_color = p->sigma_color == (float)RT_DENOISE_DEFAULT ? DEFAULT_SIGMA_COLOR : p->sigma_color;
    if (iterations < 1 || iterations > 6) return fail("rt_denoise: iterations must be 1..6 (or RT_DENOISE_DEFAULT)");
    if (npow < 0 || npow > 8) return fail("rt_denoise: normal_power_log2 must be 0..8 (or RT_DENOISE_DEFAULT)");
    if (!(sigma_plane > 0.0f) || !(sigma_plane <= FLT_MAX)) return fail("rt_denoise: sigma_plane must be > 0 and finite (or RT_DENOISE_DEFAULT)");
    if (!(sigma_color >= 0.0f) || !(sigma_color <= FLT_MAX)) return fail("rt_denoise: sigma_color must be >= 0 and finite (or RT_DENOISE_DEFAULT)");

    hipStream_t st = (hipStream_t)stream;
    const size_t n = (size_t)p->width * (size_t)p->height;
    float4* g0 = static_cast<float4*>(p->scratch);
    float4* g1 = g0 + n;
    float4* colour[2] = {g1 + n, g1 + 2 * n};
    hipLaunchKernelGGL(denoise_prepare, dim3((p->width + 63) / 64, (p->height + 3) / 4), dim3(256), 0, st,
                       static_cast<const char*>(p->surface), p->pitch, p->width, p->height,
                       static_cast<const float4*>(static_cast<const void*>(p->hits)), p->materials,
                       (uint32_t)p->material_count, sigma_plane, g0, g1, colour[0]);
    PassArgs a;
    a.g0 = g0, a.g1 = g1;
    a.out = static_cast<char*>(p->out), a.out_pitch = p->out_pitch;
    a.materials = p->materials;
    a.width = p->width, a.height = p->height;
    a.normal_power_log2 = npow;
    a.sigma_color = sigma_color;
    for (int s = 0; s < iterations; ++s) {
        a.cin = colour[s & 1], a.cout = colour[(s + 1) & 1];
        a.step = 1 << s;
        const float sc = sigma_color * (1.0f / (float)(1 << s));  // a power of two: exact
        a.sc2 = sc * sc;
        const bool last = s == iterations - 1;
        if (s == 0) launch_pass_lds<1>(a, last, st);
        else if (s == 1) launch_pass_lds<2>(a, last, st);
        else launch_pass(a, last, st);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        char msg[160];
        snprintf(msg, sizeof msg, "rt_denoise: launch failed: %s", hipGetErrorString(e));
        return fail(msg);
    }
    return 0;
}
