// atrous.h -- the core the a-trous filters share (denoise.hip: rt_denoise; denoise_variance.hip: rt_denoise_variance):
// the small device helpers of the image-space units, the two shapes of a filter pass as templates over a filter
// policy, the ladder that launches a call's passes and the head of the scratch both filters carve alike.
//
// A pass gathers 25 taps x 48 B per pixel (the guide's two float4 and the colour), one pixel per lane.  Its shape is
// the fastest of those measured (profiles/denoise_timing.txt; the slower ones are not kept): the
// passes of step 1 and 2, whose taps neighbouring lanes share, read them from an LDS tile loaded once per block
// (pass_lds); the passes of step 4 and more read global memory (pass_global).
//
// A policy F supplies what differs between the filters:
//   F::Args, F::Centre            the kernel's argument block (g0, g1, cin, width, height, step and the filter's own)
//                                 and the centre pixel with its running sums (g0, g1, c and the filter's own)
//   F::EMPTY_W                    the colour's fourth component in an LDS tile entry that holds no pixel
//   F::begin_global(k, a, x, y)   run once the centre's guide is loaded, before the first tap: the global pass's
//   F::begin_lds<HX>(k, a, s_c, centre)   form and the LDS pass's, which may read the colour tile around `centre`
//   F::tap(k, a, hw, gq0, gq1, cq)        one tap of kernel weight hw: the same code whichever way it was fetched
//   F::finish<LAST>(k, a, x, y, filtered) the pixel's result; the last pass remodulates and writes the output
// Every function is forced inline into the unit's own __global__ kernels, which keep the names the profiles and the
// static comparisons know them by.
#pragma once

#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdint>

#include "rt_abi.h"

namespace atrous {

constexpr float ALBEDO_FLOOR = 0.015625f;  // 2^-6

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

// the first float4 of a hit record (t kind id material) -> 0 for a miss, 1 for a hit whose material index is beyond
// the table (albedo 1), material + 2 otherwise
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

// the two guide weights of a tap, wn and (through wz_out) wz of rt_abi.h, between a centre's guide (g0, g1) =
// ((n, sigma_plane * t), (pos, tag)) and a tap's
__device__ __forceinline__ float guide_weight(const float4& g0, const float4& g1, const float4& gq0, const float4& gq1,
                                              int normal_power_log2, float& wz_out) {
    float wn = fmaxf(0.0f, dot3(g0.x, g0.y, g0.z, gq0.x, gq0.y, gq0.z));
    for (int i = 0; i < normal_power_log2; ++i) wn = wn * wn;
    const float d = fabsf(dot3(g0.x, g0.y, g0.z, gq1.x - g1.x, gq1.y - g1.y, gq1.z - g1.z));
    float wz = fmaxf(0.0f, 1.0f - d / g0.w);  // sigma_plane * t == 0: inf or NaN -> 0
    wz_out = wz * wz;
    return wn;
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
template <class F, bool LAST>
__device__ __forceinline__ void pass_global(const typename F::Args& a) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= a.width || y >= a.height) return;
    const size_t p = (size_t)y * a.width + x;
    typename F::Centre k;
    k.g1 = a.g1[p];
    k.c = a.cin[p];
    const bool valid = __float_as_uint(k.g1.w) != 0u;
    if (valid) {
        k.g0 = a.g0[p];
        F::begin_global(k, a, x, y);
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
                F::tap(k, a, kernel_weight(dy, dx), r0[dx + 2], r1[dx + 2], rc[dx + 2]);
            }
        }
    }
    F::template finish<LAST>(k, a, x, y, valid);
}

// Taps from an LDS tile, for the passes whose taps neighbouring lanes share (STEP 1 and 2): a block's 32 x 8
// pixels and a halo of 2 * STEP around them are loaded once (1.7 / 2.5 pixels fetched per pixel instead of
// 25); a tile entry outside the image, or a miss, is stored with tag 0 (and F::EMPTY_W) and skipped like a miss.
// The halo stays 2 * STEP whatever begin_lds reads: it reaches from the centre only, never from a tap.
template <class F, int STEP, bool LAST>
__device__ __forceinline__ void pass_lds(const typename F::Args& a) {
    constexpr int TX = 32, TY = 8, R = 2 * STEP, HX = TX + 2 * R, HY = TY + 2 * R;
    __shared__ float4 s_g0[HX * HY], s_g1[HX * HY], s_c[HX * HY];
    const int x0 = blockIdx.x * TX - R, y0 = blockIdx.y * TY - R;
    for (int i = threadIdx.x; i < HX * HY; i += 256) {
        const int gx = x0 + i % HX, gy = y0 + i / HX;
        float4 v0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), v1 = v0, vc = make_float4(0.0f, 0.0f, 0.0f, F::EMPTY_W);
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
    typename F::Centre k;
    k.g1 = s_g1[centre];
    k.c = a.cin[(size_t)y * a.width + x];  // a miss's colour is not in the tile
    const bool valid = __float_as_uint(k.g1.w) != 0u;
    if (valid) {
        k.g0 = s_g0[centre];
        F::template begin_lds<HX>(k, a, s_c, centre);
#pragma unroll
        for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
            for (int dx = -2; dx <= 2; ++dx) {
                const int q = centre + dy * STEP * HX + dx * STEP;
                const float4 gq1 = s_g1[q];
                if (__float_as_uint(gq1.w) == 0u) continue;
                const float4 cq = s_c[q];
                if (!finite3(cq)) continue;
                F::tap(k, a, kernel_weight(dy, dx), s_g0[q], gq1, cq);
            }
        }
    }
    F::template finish<LAST>(k, a, x, y, valid);
}

// The head of both filters' scratch: g0, g1, colour A, colour B, one float4 each per pixel; `rest` is what follows.
struct Scratch {
    float4 *g0, *g1, *colour[2];
    void* rest;
};
inline Scratch carve(void* scratch, size_t n) {
    float4* const g0 = static_cast<float4*>(scratch);
    return Scratch{g0, g0 + n, {g0 + 2 * n, g0 + 3 * n}, g0 + 4 * n};
}

// A call's passes, A -> B -> A ...: pass s has step 1 << s, the last one writes the output.  K names the unit's
// kernels: K::lds<STEP>(last) and K::global(last) return the __global__ function, K::at_step(a, s) sets what else
// of the arguments depends on the pass.  The grids: 32 x 8 pixels a block from the LDS tile, 64 x 4 from global memory.
template <class K, class A>
void launch_passes(A& a, float4* const colour[2], int iterations, hipStream_t st) {
    const dim3 lds_grid((a.width + 31) / 32, (a.height + 7) / 8), grid((a.width + 63) / 64, (a.height + 3) / 4);
    for (int s = 0; s < iterations; ++s) {
        a.cin = colour[s & 1], a.cout = colour[(s + 1) & 1];
        a.step = 1 << s;
        K::at_step(a, s);
        const bool last = s == iterations - 1;
        if (s == 0) hipLaunchKernelGGL(K::template lds<1>(last), lds_grid, dim3(256), 0, st, a);
        else if (s == 1) hipLaunchKernelGGL(K::template lds<2>(last), lds_grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL(K::global(last), grid, dim3(256), 0, st, a);
    }
}

}  // namespace atrous
