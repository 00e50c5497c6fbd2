// denoise_variance.hip -- rt_moments and rt_denoise_variance (include/rt_abi.h): the a-trous filter of denoise.hip
// with a per-pixel colour tolerance, set by an estimate of the variance of each pixel's luminance (temporal moments
// accumulated by rt_reproject where the history is long enough, a 7x7 spatial estimate elsewhere) that the passes
// filter along with the colours.  The spatial half of SVGF.
//
// The arithmetic is the one rt_abi.h specifies and tests/variance_ref.py restates in numpy: fp32, no contraction,
// IEEE division (the flags of every unit, build.py), only + - * /, fmaxf, fabsf and comparisons, so the GPU and the
// restatement agree bit for bit.  All kernels are one pixel per lane, wave64:
//
//   moments   rt_moments: (l, l*l, 0, alpha) of the albedo-divided colour's luminance, one lane one pixel
//   prepare   surface / albedo and the initial variance -> colour buffer A; the guide packed as denoise.hip packs it;
//             alpha into a plane of its own.  The 7x7 spatial estimate reads a 38 x 14 LDS tile (32 x 8 pixels,
//             halo 3) that a block loads only when one of its lanes needs the estimate (__syncthreads_or): on a
//             warmed-up sequence few blocks do (profiles/variance_timing.txt)
//   pass      25 taps at stride 1 << s and the 3x3 variance prefilter, from one colour buffer into the other
//   the last pass multiplies the albedo back in, writes the pitched output surface and out_variance.  It reads only
//             scratch and the material table, which is why out == surface is safe.
//
// Scratch, 68 B per pixel: g0, g1 (the guide, 2 x 16 B), two colour buffers (2 x 16 B) whose fourth component is the
// variance, not alpha -- -1 for !valid(p), which a valid pixel's variance (fmaxf(0, .), sums of products of
// non-negative numbers, or NaN) never compares below 0 as -- and one alpha plane (4 B).  So a tap is three 16-byte
// loads, exactly rt_denoise's 48 B, the variance riding in the colour's load, and the prefilter's nine taps need no
// second load for validity.  Against colour + alpha and separate variance planes (72 B) it saves a 4-byte load per tap.
//
// The passes are atrous.h's two shapes (an LDS tile for step 1 and 2, global memory from step 4 on) with this unit's
// policy.  The prefilter reaches one pixel and only from the centre, so the LDS tile's halo stays 2 * step; in the
// global passes it is nine 4-byte loads at stride 1, issued together ahead of the taps.
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
constexpr float DEFAULT_SIGMA_LUM = 4.0f;
constexpr float DEFAULT_MIN_HISTORY = 4.0f;
constexpr float TOLERANCE_FLOOR = 1e-8f;
constexpr float INVALID = -1.0f;  // the variance slot of a pixel that is not valid

__global__ __launch_bounds__(256) void moments_kernel(const char* surface, uint64_t pitch, int width, int height,
                                                      const float4* hits, const GPUMaterial* materials,
                                                      uint32_t material_count, char* out, uint64_t out_pitch) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= width || y >= height) return;
    const uint32_t tag = tag_of(hits[3 * ((size_t)y * width + x)], material_count);
    const float4 c = demodulated(surface, pitch, x, y, tag, materials);
    const float l = lum3(c.x, c.y, c.z);
    *reinterpret_cast<float4*>(out + (size_t)y * out_pitch + (size_t)x * 16) = make_float4(l, l * l, 0.0f, c.w);
}

struct PrepareArgs {
    const char* surface;
    uint64_t pitch;
    const char* moments;  // may be null
    uint64_t moments_pitch;
    const float* history;  // may be null: 1 everywhere
    const float4* hits;
    const GPUMaterial* materials;
    uint32_t material_count;
    int width, height;
    int normal_power_log2;
    float sigma_plane, min_history;
    float4 *g0, *g1, *colour;
    float* alpha;
};

__global__ __launch_bounds__(256) void variance_prepare(const PrepareArgs a) {
    constexpr int TX = 32, TY = 8, R = 3, HX = TX + 2 * R, HY = TY + 2 * R;
    __shared__ float4 s_n[HX * HY];  // (n.xyz, lum(c)); read only where s_p.w != 0
    __shared__ float4 s_p[HX * HY];  // (pos.xyz, 1 for a tap to take: inside, valid, c finite; else 0)
    const int lx = threadIdx.x % TX, ly = threadIdx.x / TX;
    const int x = blockIdx.x * TX + lx, y = blockIdx.y * TY + ly;
    const bool inside = x < a.width && y < a.height;
    const size_t p = (size_t)y * a.width + x;
    float4 g0, g1, c;
    float v = INVALID;
    bool spatial = false;
    if (inside) {
        const float4 h0 = a.hits[3 * p], h1 = a.hits[3 * p + 1], h2 = a.hits[3 * p + 2];  // (t kind id material) (n bx) (pos by)
        const uint32_t tag = tag_of(h0, a.material_count);
        c = demodulated(a.surface, a.pitch, x, y, tag, a.materials);
        g0 = make_float4(h1.x, h1.y, h1.z, a.sigma_plane * h0.x);
        g1 = make_float4(h2.x, h2.y, h2.z, __uint_as_float(tag));
        a.g0[p] = g0, a.g1[p] = g1, a.alpha[p] = c.w;
        if (tag != 0u) {
            v = 0.0f;
            if (finite3(c)) {
                spatial = true;
                const float hist = a.history ? a.history[p] : 1.0f;
                if (a.moments && hist >= a.min_history) {
                    const float4 m = *reinterpret_cast<const float4*>(a.moments + (size_t)y * a.moments_pitch + (size_t)x * 16);
                    if (finite1(m.x) && finite1(m.y)) {
                        v = fmaxf(0.0f, m.y - m.x * m.x) / fmaxf(hist, 1.0f);
                        spatial = false;
                    }
                }
            }
        }
    }
    // the 7x7 estimate: the tile is loaded only by a block one of whose lanes needs it
    if (__syncthreads_or(spatial)) {
        const int x0 = blockIdx.x * TX - R, y0 = blockIdx.y * TY - R;
        for (int i = threadIdx.x; i < HX * HY; i += 256) {
            const int gx = x0 + i % HX, gy = y0 + i / HX;
            float4 vn = make_float4(0.0f, 0.0f, 0.0f, 0.0f), vp = vn;
            if (gx >= 0 && gx < a.width && gy >= 0 && gy < a.height) {
                const size_t q = (size_t)gy * a.width + gx;
                const uint32_t tag = tag_of(a.hits[3 * q], a.material_count);
                if (tag != 0u) {
                    const float4 cq = demodulated(a.surface, a.pitch, gx, gy, tag, a.materials);
                    if (finite3(cq)) {
                        const float4 h1 = a.hits[3 * q + 1], h2 = a.hits[3 * q + 2];
                        vn = make_float4(h1.x, h1.y, h1.z, lum3(cq.x, cq.y, cq.z));
                        vp = make_float4(h2.x, h2.y, h2.z, 1.0f);
                    }
                }
            }
            s_n[i] = vn, s_p[i] = vp;
        }
        __syncthreads();
        if (spatial) {
            const int centre = (ly + R) * HX + lx + R;
            float s1 = 0.0f, s2 = 0.0f, ws = 0.0f;
            for (int dy = -R; dy <= R; ++dy) {
#pragma unroll
                for (int dx = -R; dx <= R; ++dx) {
                    const int q = centre + dy * HX + dx;
                    const float4 gq1 = s_p[q];
                    if (gq1.w == 0.0f) continue;
                    const float4 gq0 = s_n[q];
                    float wz;
                    const float wn = guide_weight(g0, g1, gq0, gq1, a.normal_power_log2, wz);
                    const float w = wn * wz;
                    if (w > 0.0f) {
                        s1 += gq0.w * w, s2 += (gq0.w * gq0.w) * w;
                        ws += w;
                    }
                }
            }
            if (ws > 0.0f) {
                const float m1 = s1 / ws;
                v = fmaxf(0.0f, s2 / ws - m1 * m1);
            }
        }
    }
    if (inside) a.colour[p] = make_float4(c.x, c.y, c.z, v);
}

struct PassArgs {
    const float4* g0;
    const float4* g1;
    const float4* cin;       // (c.rgb, variance or INVALID)
    float4* cout;            // not the last pass
    const float* alpha;      // the last pass
    char* out;               // the last pass: the pitched output surface
    uint64_t out_pitch;
    float* out_variance;     // the last pass; may be null
    const GPUMaterial* materials;
    int width, height, step;
    int normal_power_log2;
    float sl2;               // sigma_lum * sigma_lum
};

// The centre pixel of a pass and its running sums
struct Centre {
    float4 g0, g1, c;  // (n, sigma_plane * t), (pos, tag), (colour, variance)
    float l, tol;      // lum(c), the colour tolerance squared
    bool use_lum;
    float sx = 0.0f, sy = 0.0f, sz = 0.0f, vs = 0.0f, wsum = 0.0f;
};

// 1/16 1/8 1/16; 1/8 1/4 1/8; 1/16 1/8 1/16 (exact: powers of two)
__device__ __forceinline__ float prefilter_weight(int dy, int dx) {
    const float k[3] = {0.25f, 0.5f, 0.25f};
    return k[dy + 1] * k[dx + 1];
}

// the variance filter as atrous.h's passes see it
struct VarianceFilter {
    using Args = PassArgs;
    using Centre = ::Centre;
    static constexpr float EMPTY_W = INVALID;

    static __device__ __forceinline__ void start(Centre& k, const PassArgs& a, float vsum, float ksum) {
        k.l = lum3(k.c.x, k.c.y, k.c.z);
        k.use_lum = finite3(k.c);
        k.tol = a.sl2 * (vsum / ksum) + TOLERANCE_FLOOR;
    }

    // the 3x3 prefilter of the variance around (x, y): nine loads issued together, from clamped coordinates
    static __device__ __forceinline__ void begin_global(Centre& k, const PassArgs& a, int x, int y) {
        float pv[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            const int qx = min(max(x + i % 3 - 1, 0), a.width - 1), qy = min(max(y + i / 3 - 1, 0), a.height - 1);
            pv[i] = a.cin[(size_t)qy * a.width + qx].w;
        }
        float vsum = 0.0f, ksum = 0.0f;
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            const int qx = x + i % 3 - 1, qy = y + i / 3 - 1;
            if (qx < 0 || qx >= a.width || qy < 0 || qy >= a.height || pv[i] < 0.0f) continue;
            const float kw = prefilter_weight(i / 3 - 1, i % 3 - 1);
            vsum += pv[i] * kw, ksum += kw;
        }
        start(k, a, vsum, ksum);
    }
    // the same from the colour tile, whose entries outside the image hold INVALID
    template <int HX>
    static __device__ __forceinline__ void begin_lds(Centre& k, const PassArgs& a, const float4* s_c, int centre) {
        float vsum = 0.0f, ksum = 0.0f;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                const float vq = s_c[centre + dy * HX + dx].w;
                if (vq < 0.0f) continue;
                const float kw = prefilter_weight(dy, dx);
                vsum += vq * kw, ksum += kw;
            }
        }
        start(k, a, vsum, ksum);
    }

    static __device__ __forceinline__ void tap(Centre& k, const PassArgs& a, float hw, const float4& gq0, const float4& gq1, const float4& cq) {
        float wz;
        const float wn = guide_weight(k.g0, k.g1, gq0, gq1, a.normal_power_log2, wz);
        float wl = 1.0f;
        if (k.use_lum) {
            const float d = lum3(cq.x, cq.y, cq.z) - k.l;
            wl = 1.0f / (1.0f + (d * d) / k.tol);
        }
        const float w = ((hw * wn) * wz) * wl;
        if (w > 0.0f) {
            k.sx += cq.x * w, k.sy += cq.y * w, k.sz += cq.z * w;
            k.vs += cq.w * (w * w);
            k.wsum += w;
        }
    }

    // the pass's result for pixel (x, y): the weighted mean and its variance (or the centre's own), remodulated by the last pass
    template <bool LAST>
    static __device__ __forceinline__ void finish(const Centre& k, const PassArgs& a, int x, int y, bool filtered) {
        float ox = k.c.x, oy = k.c.y, oz = k.c.z, ov = k.c.w;
        if (filtered && k.wsum > 0.0f) {
            ox = k.sx / k.wsum, oy = k.sy / k.wsum, oz = k.sz / k.wsum;
            ov = k.vs / (k.wsum * k.wsum);
        }
        const size_t p = (size_t)y * a.width + x;
        if (LAST) {
            float ax, ay, az;
            albedo_of(__float_as_uint(k.g1.w), a.materials, ax, ay, az);
            *reinterpret_cast<float4*>(a.out + (size_t)y * a.out_pitch + (size_t)x * 16) = make_float4(ox * ax, oy * ay, oz * az, a.alpha[p]);
            if (a.out_variance) a.out_variance[p] = filtered ? ov : 0.0f;
        } else {
            a.cout[p] = make_float4(ox, oy, oz, ov);
        }
    }
};

template <bool LAST>
__global__ __launch_bounds__(256) void variance_pass(const PassArgs a) {
    pass_global<VarianceFilter, LAST>(a);
}

template <int STEP, bool LAST>
__global__ __launch_bounds__(256) void variance_pass_lds(const PassArgs a) {
    pass_lds<VarianceFilter, STEP, LAST>(a);
}

struct VariancePasses {  // launch_passes' view of the kernels
    static auto global(bool last) { return last ? variance_pass<true> : variance_pass<false>; }
    template <int STEP>
    static auto lds(bool last) { return last ? variance_pass_lds<STEP, true> : variance_pass_lds<STEP, false>; }
    static void at_step(PassArgs&, int) {}
};

}  // namespace

extern "C" int rt_moments(const rt_moments_params* p, void* stream) {
    const char* const who = "rt_moments";
    if (!p) return refuse(who, "null params");
    if (!p->surface) return refuse(who, "null surface");
    if (!p->hits) return refuse(who, "null hits");
    if (!p->out) return refuse(who, "null out");
    if (size_refused(who, p->width, p->height) || caps_refused(who, p->width, p->height, "DENOISE")) return 1;
    if (materials_refused(who, p->materials, p->material_count)) return 1;
    if (pitch_refused(who, "pitch", p->pitch, p->width) || pitch_refused(who, "out_pitch", p->out_pitch, p->width)) return 1;
    if (pitches_refused(who, {p->pitch, p->out_pitch})) return 1;
    if (misaligned(who, "surface, hits, materials and out", 16, {p->surface, p->hits, p->out, p->materials})) return 1;
    if (p->flags != 0) return refuse(who, "flags must be 0");
    const uint64_t n = (uint64_t)p->width * (uint64_t)p->height, row = (uint64_t)p->width * 16;
    const uint64_t out_bytes = surface_bytes(p->height, p->out_pitch, row);
    if (overlap(p->out, out_bytes, p->surface, surface_bytes(p->height, p->pitch, row))) return refuse(who, "out must not overlap surface");
    if (overlap(p->out, out_bytes, p->hits, n * 48)) return refuse(who, "out must not overlap hits");
    hipLaunchKernelGGL(moments_kernel, image_grid(p->width, p->height), dim3(256), 0, (hipStream_t)stream,
                       static_cast<const char*>(p->surface), p->pitch, p->width, p->height,
                       static_cast<const float4*>(static_cast<const void*>(p->hits)), p->materials,
                       (uint32_t)p->material_count, static_cast<char*>(p->out), p->out_pitch);
    return launch_refused(who);
}

extern "C" size_t rt_denoise_variance_scratch_bytes(int width, int height) {
    if (width <= 0 || height <= 0) return 0;
    // g0, g1, colour A, colour B: one float4 each per pixel; the alpha plane: one float, rounded up to 16 bytes
    const size_t n = (size_t)width * (size_t)height;
    return n * 64u + ((n * 4u + 15u) & ~(size_t)15u);
}

extern "C" int rt_denoise_variance(const rt_denoise_variance_params* p, void* stream) {
    const char* const who = "rt_denoise_variance";
    if (!p) return refuse(who, "null params");
    if (!p->surface) return refuse(who, "null surface");
    if (!p->hits) return refuse(who, "null hits");
    if (!p->out) return refuse(who, "null out");
    if (!p->scratch) return refuse(who, "null scratch");
    if (size_refused(who, p->width, p->height) || caps_refused(who, p->width, p->height, "DENOISE")) return 1;
    if (materials_refused(who, p->materials, p->material_count)) return 1;
    if (pitch_refused(who, "pitch", p->pitch, p->width) || pitch_refused(who, "out_pitch", p->out_pitch, p->width)) return 1;
    if (p->moments && pitch_refused(who, "moments_pitch", p->moments_pitch, p->width)) return 1;
    if (pitches_refused(who, {p->pitch, p->out_pitch, p->moments ? p->moments_pitch : 0})) return 1;
    if (misaligned(who, "surface, hits, materials, moments, out and scratch", 16,
                   {p->surface, p->hits, p->out, p->scratch, p->materials, p->moments}))
        return 1;
    if (misaligned(who, "history and out_variance", 4, {p->history, p->out_variance})) return 1;
    const uint64_t need = rt_denoise_variance_scratch_bytes(p->width, p->height);
    if (p->scratch_bytes < need) return refuse(who, "scratch too small (rt_denoise_variance_scratch_bytes)");
    if (p->flags != 0) return refuse(who, "flags must be 0");
    if (p->reserved != 0) return refuse(who, "reserved must be 0");
    const int iterations = or_default(p->iterations, RT_DENOISE_DEFAULT, DEFAULT_ITERATIONS);
    const int npow = or_default(p->normal_power_log2, RT_DENOISE_DEFAULT, DEFAULT_NORMAL_POWER_LOG2);
    const float sigma_plane = or_default(p->sigma_plane, RT_DENOISE_DEFAULT, DEFAULT_SIGMA_PLANE);
    const float sigma_lum = or_default(p->sigma_lum, RT_DENOISE_DEFAULT, DEFAULT_SIGMA_LUM);
    const float min_history = or_default(p->min_history, RT_DENOISE_DEFAULT, DEFAULT_MIN_HISTORY);
    if (iterations < 1 || iterations > 6) return refuse(who, "iterations must be 1..6 (or RT_DENOISE_DEFAULT)");
    if (npow < 0 || npow > 8) return refuse(who, "normal_power_log2 must be 0..8 (or RT_DENOISE_DEFAULT)");
    if (!finite_above(sigma_plane, 0.0f)) return refuse(who, "sigma_plane must be > 0 and finite (or RT_DENOISE_DEFAULT)");
    if (!finite_above(sigma_lum, 0.0f)) return refuse(who, "sigma_lum must be > 0 and finite (or RT_DENOISE_DEFAULT)");
    if (!finite_from(min_history, 1.0f)) return refuse(who, "min_history must be >= 1 and finite (or RT_DENOISE_DEFAULT)");
    const uint64_t n = (uint64_t)p->width * (uint64_t)p->height, row = (uint64_t)p->width * 16;
    const uint64_t out_bytes = surface_bytes(p->height, p->out_pitch, row);
    if (overlap(p->out, out_bytes, p->scratch, need)) return refuse(who, "out must not overlap scratch");
    if (overlap(p->out, out_bytes, p->hits, n * 48)) return refuse(who, "out must not overlap hits");
    if (overlap(p->out, out_bytes, p->moments, surface_bytes(p->height, p->moments_pitch, row))) return refuse(who, "out must not overlap moments");
    if (overlap(p->out, out_bytes, p->history, n * 4)) return refuse(who, "out must not overlap history");
    if (overlap(p->out_variance, n * 4, p->out, out_bytes)) return refuse(who, "out_variance must not overlap out");
    if (overlap(p->out_variance, n * 4, p->scratch, need)) return refuse(who, "out_variance must not overlap scratch");

    hipStream_t st = (hipStream_t)stream;
    const Scratch sc = carve(p->scratch, n);
    float* const alpha = static_cast<float*>(sc.rest);
    PrepareArgs pa;
    pa.surface = static_cast<const char*>(p->surface), pa.pitch = p->pitch;
    pa.moments = static_cast<const char*>(p->moments), pa.moments_pitch = p->moments_pitch;
    pa.history = p->history;
    pa.hits = static_cast<const float4*>(static_cast<const void*>(p->hits));
    pa.materials = p->materials, pa.material_count = (uint32_t)p->material_count;
    pa.width = p->width, pa.height = p->height;
    pa.normal_power_log2 = npow;
    pa.sigma_plane = sigma_plane, pa.min_history = min_history;
    pa.g0 = sc.g0, pa.g1 = sc.g1, pa.colour = sc.colour[0], pa.alpha = alpha;
    hipLaunchKernelGGL(variance_prepare, dim3((p->width + 31) / 32, (p->height + 7) / 8), dim3(256), 0, st, pa);
    PassArgs a;
    a.g0 = sc.g0, a.g1 = sc.g1, a.alpha = alpha;
    a.out = static_cast<char*>(p->out), a.out_pitch = p->out_pitch;
    a.out_variance = p->out_variance;
    a.materials = p->materials;
    a.width = p->width, a.height = p->height;
    a.normal_power_log2 = npow;
    a.sl2 = sigma_lum * sigma_lum;
    launch_passes<VariancePasses>(a, sc.colour, iterations, st);
    return launch_refused(who);
}
