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
// The passes have denoise.hip's access shape (the one it measured fastest, profiles/denoise_timing.txt): an LDS
// tile for step 1 and 2, 64 x 1 waves with a row of taps' loads issued together for step >= 4.  The prefilter reaches
// one pixel and only from the centre, so the LDS tile's halo stays 2 * step; in the global passes it is nine 4-byte
// loads at stride 1, issued together ahead of the taps.
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
constexpr float DEFAULT_SIGMA_LUM = 4.0f;
constexpr float DEFAULT_MIN_HISTORY = 4.0f;
constexpr float ALBEDO_FLOOR = 0.015625f;  // 2^-6
constexpr float TOLERANCE_FLOOR = 1e-8f;
constexpr float INVALID = -1.0f;  // the variance slot of a pixel that is not valid

__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) {
    return (ax * bx + ay * by) + az * bz;  // rtm::dot's order
}

__device__ __forceinline__ float lum3(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

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

__device__ __forceinline__ uint32_t tag_of(const float4& h0, uint32_t material_count) {
    const uint32_t kind = __float_as_uint(h0.y), material = __float_as_uint(h0.w);
    return kind == 0u ? 0u : (material < material_count ? material + 2u : 1u);
}

// surface.rgb / a_p (alpha in w) of pixel (x, y) with the given tag
__device__ __forceinline__ float4 demodulated(const char* surface, uint64_t pitch, int x, int y, uint32_t tag,
                                              const GPUMaterial* materials) {
    float ax, ay, az;
    albedo_of(tag, materials, ax, ay, az);
    const float4 s = *reinterpret_cast<const float4*>(surface + (size_t)y * pitch + (size_t)x * 16);
    return make_float4(s.x / ax, s.y / ay, s.z / az, s.w);
}

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

// the two guide weights of a tap, shared by the spatial estimate and the passes: wn * wz of rt_abi.h
__device__ __forceinline__ float guide_weight(const float4& g0, const float4& g1, const float4& gq0, const float4& gq1,
                                              int normal_power_log2, float& wz_out) {
    float wn = fmaxf(0.0f, dot3(g0.x, g0.y, g0.z, gq0.x, gq0.y, gq0.z));
    for (int i = 0; i < normal_power_log2; ++i) wn = wn * wn;
    const float d = fabsf(dot3(g0.x, g0.y, g0.z, gq1.x - g1.x, gq1.y - g1.y, gq1.z - g1.z));
    float wz = fmaxf(0.0f, 1.0f - d / g0.w);  // sigma_plane * t == 0: inf or NaN -> 0
    wz_out = wz * wz;
    return wn;
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

// The centre pixel of a pass and its running sums; tap() is the filter's one tap, the same code whichever
// way a kernel fetches the tap's three float4.
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

// h[dy + 2] * h[dx + 2], the B3-spline kernel's weight of a tap (exact: the factors are 1, 3 and powers of two)
__device__ __forceinline__ float kernel_weight(int dy, int dx) {
    const float h[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    return h[dy + 2] * h[dx + 2];
}

__device__ __forceinline__ void start(Centre& k, const PassArgs& a, float vsum, float ksum) {
    k.l = lum3(k.c.x, k.c.y, k.c.z);
    k.use_lum = finite3(k.c);
    k.tol = a.sl2 * (vsum / ksum) + TOLERANCE_FLOOR;
}

__device__ __forceinline__ void tap(Centre& k, const PassArgs& a, float hw, const float4& gq0, const float4& gq1, const float4& cq) {
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
__device__ __forceinline__ void finish(const Centre& k, const PassArgs& a, int x, int y, bool filtered) {
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

// Taps straight from global memory, for the passes of step 4 and more: denoise.hip's shape (a wave covers 64 x 1
// pixels, the 15 loads of a row of taps issued together from clamped coordinates before any is tested), with the
// prefilter's nine variance loads issued together ahead of them.
template <bool LAST>
__global__ __launch_bounds__(256) void variance_pass(const PassArgs a) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= a.width || y >= a.height) return;
    const size_t p = (size_t)y * a.width + x;
    Centre k;
    k.g1 = a.g1[p];
    k.c = a.cin[p];
    const bool valid = __float_as_uint(k.g1.w) != 0u;
    if (valid) {
        k.g0 = a.g0[p];
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

// Taps from an LDS tile, for the passes whose taps neighbouring lanes share (STEP 1 and 2): denoise.hip's tile of
// 32 x 8 pixels and a halo of 2 * STEP, the same 48 B per entry (the variance is the colour's fourth component).  A
// tile entry outside the image, or a miss, is stored with tag 0 and variance INVALID and skipped like a miss.
template <int STEP, bool LAST>
__global__ __launch_bounds__(256) void variance_pass_lds(const PassArgs a) {
    constexpr int TX = 32, TY = 8, R = 2 * STEP, HX = TX + 2 * R, HY = TY + 2 * R;
    __shared__ float4 s_g0[HX * HY], s_g1[HX * HY], s_c[HX * HY];
    const int x0 = blockIdx.x * TX - R, y0 = blockIdx.y * TY - R;
    for (int i = threadIdx.x; i < HX * HY; i += 256) {
        const int gx = x0 + i % HX, gy = y0 + i / HX;
        float4 v0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), v1 = v0, vc = make_float4(0.0f, 0.0f, 0.0f, INVALID);
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
    if (last) hipLaunchKernelGGL(variance_pass<true>, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(variance_pass<false>, grid, dim3(256), 0, st, a);
}

template <int STEP>
void launch_pass_lds(const PassArgs& a, bool last, hipStream_t st) {
    const dim3 grid((a.width + 31) / 32, (a.height + 7) / 8);
    if (last) hipLaunchKernelGGL((variance_pass_lds<STEP, true>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((variance_pass_lds<STEP, false>), grid, dim3(256), 0, st, a);
}

int fail(const char* msg) {
    rt_internal_set_error(msg);
    return 1;
}

// [a, a + an) and [b, b + bn) share a byte
bool overlap(const void* a, uint64_t an, const void* b, uint64_t bn) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return a && b && x < y + bn && y < x + an;
}

int launch_error(const char* call) {
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return 0;
    char msg[160];
    snprintf(msg, sizeof msg, "%s: launch failed: %s", call, hipGetErrorString(e));
    return fail(msg);
}

}  // namespace

extern "C" int rt_moments(const rt_moments_params* p, void* stream) {
    if (!p) return fail("rt_moments: null params");
    if (!p->surface) return fail("rt_moments: null surface");
    if (!p->hits) return fail("rt_moments: null hits");
    if (!p->out) return fail("rt_moments: null out");
    if (p->width <= 0 || p->height <= 0) return fail("rt_moments: width and height must be > 0");
    if (p->height > RT_DENOISE_MAX_HEIGHT) return fail("rt_moments: height above RT_DENOISE_MAX_HEIGHT");
    if ((int64_t)p->width * p->height > RT_DENOISE_MAX_PIXELS) return fail("rt_moments: more than RT_DENOISE_MAX_PIXELS pixels");
    if (p->material_count < 0) return fail("rt_moments: negative material_count");
    if (p->material_count > 0 && !p->materials) return fail("rt_moments: null materials with material_count > 0");
    const uint64_t row = (uint64_t)p->width * 16;
    if (p->pitch < row) return fail("rt_moments: pitch smaller than width * 16");
    if (p->out_pitch < row) return fail("rt_moments: out_pitch smaller than width * 16");
    if ((p->pitch | p->out_pitch) & 15u) return fail("rt_moments: pitches must be multiples of 16");
    if (((uintptr_t)p->surface | (uintptr_t)p->hits | (uintptr_t)p->out | (uintptr_t)p->materials) & 15u)
        return fail("rt_moments: surface, hits, materials and out must be 16-byte aligned");
    if (p->flags != 0) return fail("rt_moments: flags must be 0");
    const uint64_t n = (uint64_t)p->width * (uint64_t)p->height;
    const uint64_t out_bytes = (uint64_t)(p->height - 1) * p->out_pitch + row;
    if (overlap(p->out, out_bytes, p->surface, (uint64_t)(p->height - 1) * p->pitch + row))
        return fail("rt_moments: out must not overlap surface");
    if (overlap(p->out, out_bytes, p->hits, n * 48)) return fail("rt_moments: out must not overlap hits");
    hipLaunchKernelGGL(moments_kernel, dim3((p->width + 63) / 64, (p->height + 3) / 4), dim3(256), 0, (hipStream_t)stream,
                       static_cast<const char*>(p->surface), p->pitch, p->width, p->height,
                       static_cast<const float4*>(static_cast<const void*>(p->hits)), p->materials,
                       (uint32_t)p->material_count, static_cast<char*>(p->out), p->out_pitch);
    return launch_error("rt_moments");
}

extern "C" size_t rt_denoise_variance_scratch_bytes(int width, int height) {
    if (width <= 0 || height <= 0) return 0;
    // g0, g1, colour A, colour B: one float4 each per pixel; the alpha plane: one float, rounded up to 16 bytes
    const size_t n = (size_t)width * (size_t)height;
    return n * 64u + ((n * 4u + 15u) & ~(size_t)15u);
}

extern "C" int rt_denoise_variance(const rt_denoise_variance_params* p, void* stream) {
    if (!p) return fail("rt_denoise_variance: null params");
    if (!p->surface) return fail("rt_denoise_variance: null surface");
    if (!p->hits) return fail("rt_denoise_variance: null hits");
    if (!p->out) return fail("rt_denoise_variance: null out");
    if (!p->scratch) return fail("rt_denoise_variance: null scratch");
    if (p->width <= 0 || p->height <= 0) return fail("rt_denoise_variance: width and height must be > 0");
    // the launch grids: a row of blocks per 4 (8) pixel rows in grid.y, at most 65,535
    if (p->height > RT_DENOISE_MAX_HEIGHT) return fail("rt_denoise_variance: height above RT_DENOISE_MAX_HEIGHT");
    if ((int64_t)p->width * p->height > RT_DENOISE_MAX_PIXELS) return fail("rt_denoise_variance: more than RT_DENOISE_MAX_PIXELS pixels");
    if (p->material_count < 0) return fail("rt_denoise_variance: negative material_count");
    if (p->material_count > 0 && !p->materials) return fail("rt_denoise_variance: null materials with material_count > 0");
    const uint64_t row = (uint64_t)p->width * 16;
    if (p->pitch < row) return fail("rt_denoise_variance: pitch smaller than width * 16");
    if (p->out_pitch < row) return fail("rt_denoise_variance: out_pitch smaller than width * 16");
    if (p->moments && p->moments_pitch < row) return fail("rt_denoise_variance: moments_pitch smaller than width * 16");
    if ((p->pitch | p->out_pitch | (p->moments ? p->moments_pitch : 0)) & 15u) return fail("rt_denoise_variance: pitches must be multiples of 16");
    if (((uintptr_t)p->surface | (uintptr_t)p->hits | (uintptr_t)p->out | (uintptr_t)p->scratch | (uintptr_t)p->materials |
         (uintptr_t)p->moments) & 15u)
        return fail("rt_denoise_variance: surface, hits, materials, moments, out and scratch must be 16-byte aligned");
    if (((uintptr_t)p->history | (uintptr_t)p->out_variance) & 3u)
        return fail("rt_denoise_variance: history and out_variance must be 4-byte aligned");
    const uint64_t need = rt_denoise_variance_scratch_bytes(p->width, p->height);
    if (p->scratch_bytes < need) return fail("rt_denoise_variance: scratch too small (rt_denoise_variance_scratch_bytes)");
    if (p->flags != 0) return fail("rt_denoise_variance: flags must be 0");
    if (p->reserved != 0) return fail("rt_denoise_variance: reserved must be 0");
    const int iterations = p->iterations == RT_DENOISE_DEFAULT ? DEFAULT_ITERATIONS : p->iterations;
    const int npow = p->normal_power_log2 == RT_DENOISE_DEFAULT ? DEFAULT_NORMAL_POWER_LOG2 : p->normal_power_log2;
    const float sigma_plane = p->sigma_plane == (float)RT_DENOISE_DEFAULT ? DEFAULT_SIGMA_PLANE : p->sigma_plane;
    const float sigma_lum = p->sigma_lum == (float)RT_DENOISE_DEFAULT ? DEFAULT_SIGMA_LUM : p->sigma_lum;
    const float min_history = p->min_history == (float)RT_DENOISE_DEFAULT ? DEFAULT_MIN_HISTORY : p->min_history;
    if (iterations < 1 || iterations > 6) return fail("rt_denoise_variance: iterations must be 1..6 (or RT_DENOISE_DEFAULT)");
    if (npow < 0 || npow > 8) return fail("rt_denoise_variance: normal_power_log2 must be 0..8 (or RT_DENOISE_DEFAULT)");
    if (!(sigma_plane > 0.0f) || !(sigma_plane <= FLT_MAX)) return fail("rt_denoise_variance: sigma_plane must be > 0 and finite (or RT_DENOISE_DEFAULT)");
    if (!(sigma_lum > 0.0f) || !(sigma_lum <= FLT_MAX)) return fail("rt_denoise_variance: sigma_lum must be > 0 and finite (or RT_DENOISE_DEFAULT)");
    if (!(min_history >= 1.0f) || !(min_history <= FLT_MAX)) return fail("rt_denoise_variance: min_history must be >= 1 and finite (or RT_DENOISE_DEFAULT)");
    const uint64_t n = (uint64_t)p->width * (uint64_t)p->height;
    const uint64_t out_bytes = (uint64_t)(p->height - 1) * p->out_pitch + row;
    if (overlap(p->out, out_bytes, p->scratch, need)) return fail("rt_denoise_variance: out must not overlap scratch");
    if (overlap(p->out, out_bytes, p->hits, n * 48)) return fail("rt_denoise_variance: out must not overlap hits");
    if (overlap(p->out, out_bytes, p->moments, (uint64_t)(p->height - 1) * p->moments_pitch + row))
        return fail("rt_denoise_variance: out must not overlap moments");
    if (overlap(p->out, out_bytes, p->history, n * 4)) return fail("rt_denoise_variance: out must not overlap history");
    if (overlap(p->out_variance, n * 4, p->out, out_bytes)) return fail("rt_denoise_variance: out_variance must not overlap out");
    if (overlap(p->out_variance, n * 4, p->scratch, need)) return fail("rt_denoise_variance: out_variance must not overlap scratch");

    hipStream_t st = (hipStream_t)stream;
    float4* g0 = static_cast<float4*>(p->scratch);
    float4* g1 = g0 + n;
    float4* colour[2] = {g1 + n, g1 + 2 * n};
    float* alpha = reinterpret_cast<float*>(g1 + 3 * n);
    PrepareArgs pa;
    pa.surface = static_cast<const char*>(p->surface), pa.pitch = p->pitch;
    pa.moments = static_cast<const char*>(p->moments), pa.moments_pitch = p->moments_pitch;
    pa.history = p->history;
    pa.hits = static_cast<const float4*>(static_cast<const void*>(p->hits));
    pa.materials = p->materials, pa.material_count = (uint32_t)p->material_count;
    pa.width = p->width, pa.height = p->height;
    pa.normal_power_log2 = npow;
    pa.sigma_plane = sigma_plane, pa.min_history = min_history;
    pa.g0 = g0, pa.g1 = g1, pa.colour = colour[0], pa.alpha = alpha;
    hipLaunchKernelGGL(variance_prepare, dim3((p->width + 31) / 32, (p->height + 7) / 8), dim3(256), 0, st, pa);
    PassArgs a;
    a.g0 = g0, a.g1 = g1, a.alpha = alpha;
    a.out = static_cast<char*>(p->out), a.out_pitch = p->out_pitch;
    a.out_variance = p->out_variance;
    a.materials = p->materials;
    a.width = p->width, a.height = p->height;
    a.normal_power_log2 = npow;
    a.sl2 = sigma_lum * sigma_lum;
    for (int s = 0; s < iterations; ++s) {
        a.cin = colour[s & 1], a.cout = colour[(s + 1) & 1];
        a.step = 1 << s;
        const bool last = s == iterations - 1;
        if (s == 0) launch_pass_lds<1>(a, last, st);
        else if (s == 1) launch_pass_lds<2>(a, last, st);
        else launch_pass(a, last, st);
    }
    return launch_error("rt_denoise_variance");
}
