// upsample.hip -- rt_upsample (include/rt_abi.h): a joint-bilateral upsampler that turns a frame rendered at
// 1/scale of the size in each direction into a full-size one, guided by the first-hit records of rt_trace_rays'
// camera mode at both sizes.  It works on albedo-divided colour, as rt_denoise does, and multiplies the output
// pixel's own albedo back in, so texture edges come out at the full resolution.
//
// The arithmetic is the one rt_abi.h specifies and tests/upsample_ref.py restates in numpy: fp32, no contraction,
// IEEE division (the flags of every unit, build.py), only + - * /, fmaxf, fabsf and comparisons, so the GPU and the
// restatement agree bit for bit.  Two kernels, both one pixel per lane, a block 64 x 4 pixels (image_grid):
//
//   prepare   at the low size: the low records and colours packed into three float4 per low pixel (48 B, the whole
//             scratch): (n.xyz, 0), (pos.xyz, tag), (low_surface.rgb / a_q, alpha)
//   gather    at the output size: the block's 4 x 4 footprints staged in an LDS tile loaded once per block
//             (scale 2: 36 x 6 low pixels for 256 output pixels, 10,368 B; an entry outside the low image is marked
//             EMPTY), then stage 1 (the 2 x 2 bilinear footprint), stage 2 (the 4 x 4 footprint, guide weights only)
//             under a wave ballot, so that a wave none of whose pixels needs it does not enter it, and stage 3 (the
//             nearest low pixel)
//
// The gather's shape is the faster of the two measured (profiles/upsample_timing.txt; the other, taps
// read straight from global memory, is not kept: 6 to 22 % slower at 1920x1080, 27 to 49 % slower at 3840x2160).
//
// The host checks, in this order, the first fault reported: null pointers (params, low_surface, low_hits, hits, out,
// scratch); sizes and scale; caps (on the output size); materials; pitches; alignment; scratch size; overlaps (out
// against low_surface, low_hits, hits, scratch, materials); flags and reserved; parameters.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "atrous.h"
#include "image_entry.h"
#include "rt_abi.h"

namespace {

using namespace atrous;
using namespace rt_entry;

constexpr int DEFAULT_NORMAL_POWER_LOG2 = 0;  // profiles/upsample_quality.txt
constexpr float DEFAULT_SIGMA_PLANE = 0.03f;
constexpr uint32_t EMPTY = 0xFFFFFFFFu;  // the tag of a tile entry that holds no low pixel (a miss is 0: a tap of misses)

__global__ __launch_bounds__(256) void upsample_prepare(const char* low_surface, uint64_t low_pitch, int low_width,
                                                        int low_height, const float4* low_hits, const GPUMaterial* materials,
                                                        uint32_t material_count, float4* gn, float4* g1, float4* colour) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= low_width || y >= low_height) return;
    const size_t q = (size_t)y * low_width + x;
    const float4 h0 = low_hits[3 * q], h1 = low_hits[3 * q + 1], h2 = low_hits[3 * q + 2];  // (t kind id material) (n bx) (pos by)
    const uint32_t tag = tag_of(h0, material_count);
    colour[q] = demodulated(low_surface, low_pitch, x, y, tag, materials);
    gn[q] = make_float4(h1.x, h1.y, h1.z, 0.0f);
    g1[q] = make_float4(h2.x, h2.y, h2.z, __uint_as_float(tag));
}

struct GatherArgs {
    const float4* hits;  // the output size's records
    const GPUMaterial* materials;
    const float4 *gn, *g1, *colour;  // prepare's, at the low size
    char* out;
    uint64_t out_pitch;
    uint32_t material_count;
    int width, height, low_width, low_height;
    int normal_power_log2;
    float sigma_plane;
};

// floor((2 * X + 1 - S) / (2 * S)): the first low column (row) of output column (row) X's bilinear footprint; -1 when
// the numerator is negative, which is above -2 * S
template <int S>
__device__ __forceinline__ int footprint(int X, int& r) {
    const int i = 2 * X + 1 - S;
    const int f = i < 0 ? -1 : i / (2 * S);
    r = i - 2 * S * f;
    return f;
}

// the tile of a block: columns tx0 .. tx0 + TW - 1 and rows ty0 .. ty0 + TH - 1 of the low image.  A block's 64
// columns span 126 in the numerator above, so their footprints start in at most 126 / 2S + 1 columns; one more on
// the left and two on the right for stage 2.  Likewise 4 rows span 6.
template <int S>
struct Tile {
    static constexpr int TW = 126 / (2 * S) + 5, TH = 6 / (2 * S) + 5;
    const float4 *n, *g1, *c;
    int tx0, ty0;
    // low pixel (qx, qy) of the block's footprints -> whether it exists, and its three float4
    __device__ __forceinline__ bool fetch(int qx, int qy, float4& qn, float4& q1, float4& qc) const {
        const int i = (qy - ty0) * TW + (qx - tx0);
        q1 = g1[i], qn = n[i], qc = c[i];
        return __float_as_uint(q1.w) != EMPTY;
    }
};

// One output pixel (x, y) inside the image, its taps read from the block's tile.
template <int S>
__device__ __forceinline__ void gather_pixel(const GatherArgs& a, const Tile<S>& taps, int x, int y) {
    const size_t p = (size_t)y * a.width + x;
    const float4 h0 = a.hits[3 * p], h1 = a.hits[3 * p + 1], h2 = a.hits[3 * p + 2];
    const uint32_t tag = tag_of(h0, a.material_count);
    const float4 g0 = make_float4(h1.x, h1.y, h1.z, a.sigma_plane * h0.x), g1 = make_float4(h2.x, h2.y, h2.z, 0.0f);
    int rx, ry;
    const int x0 = footprint<S>(x, rx), y0 = footprint<S>(y, ry);
    const float tx = (float)rx / (float)(2 * S), ty = (float)ry / (float)(2 * S);
    const float wx[2] = {1.0f - tx, tx}, wy[2] = {1.0f - ty, ty};
    float sx = 0.0f, sy = 0.0f, sz = 0.0f, wsum = 0.0f;

    // the guide g(P, q) of a fetched tap, 0 for one that is skipped
    auto guide = [&](bool exists, const float4& qn, const float4& q1, const float4& qc) -> float {
        if (!exists || !finite3(qc)) return 0.0f;
        const uint32_t tq = __float_as_uint(q1.w);
        if (tag == 0u) return tq == 0u ? 1.0f : 0.0f;
        if (tq == 0u) return 0.0f;
        float wz;
        const float wn = guide_weight(g0, g1, qn, q1, a.normal_power_log2, wz);
        return wn * wz;
    };
    auto add = [&](const float4& qc, float w) {
        if (w > 0.0f) {
            sx += qc.x * w, sy += qc.y * w, sz += qc.z * w;
            wsum += w;
        }
    };

    // stage 1: the bilinear footprint.  `near`, the low pixel the output pixel lies in, is one of its four taps.
    const int nx = x / S, ny = y / S;
    float4 cnear = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            float4 qn, q1, qc;
            const bool exists = taps.fetch(x0 + i, y0 + j, qn, q1, qc);
            if (x0 + i == nx && y0 + j == ny) cnear = qc;
            add(qc, (wy[j] * wx[i]) * guide(exists, qn, q1, qc));  // a skipped tap: w = 0, not added
        }
    }
    // stage 2: the 4 x 4 footprint with the guide alone, for the pixels whose footprint held nothing usable; a wave
    // with no such pixel skips it on a scalar branch
    const bool more = !(wsum > 0.0f);
    if (__ballot(more) != 0ull) {
        if (more) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    float4 qn, q1, qc;
                    const bool exists = taps.fetch(x0 - 1 + i, y0 - 1 + j, qn, q1, qc);
                    add(qc, guide(exists, qn, q1, qc));
                }
            }
        }
    }
    // stage 3: the nearest low pixel, finite or not
    float ox = cnear.x, oy = cnear.y, oz = cnear.z;
    if (wsum > 0.0f) ox = sx / wsum, oy = sy / wsum, oz = sz / wsum;
    float ax, ay, az;
    albedo_of(tag, a.materials, ax, ay, az);
    *reinterpret_cast<float4*>(a.out + (size_t)y * a.out_pitch + (size_t)x * 16) = make_float4(ox * ax, oy * ay, oz * az, cnear.w);
}

template <int S>
__global__ __launch_bounds__(256) void upsample_gather(const GatherArgs a) {
    using T = Tile<S>;
    __shared__ float4 s_n[T::TW * T::TH], s_g1[T::TW * T::TH], s_c[T::TW * T::TH];
    int r;
    const int tx0 = footprint<S>(blockIdx.x * 64, r) - 1, ty0 = footprint<S>(blockIdx.y * 4, r) - 1;
    for (int i = threadIdx.x; i < T::TW * T::TH; i += 256) {
        const int qx = tx0 + i % T::TW, qy = ty0 + i / T::TW;
        float4 vn = make_float4(0.0f, 0.0f, 0.0f, 0.0f), v1 = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(EMPTY)), vc = vn;
        if (qx >= 0 && qx < a.low_width && qy >= 0 && qy < a.low_height) {
            const size_t q = (size_t)qy * a.low_width + qx;
            vn = a.gn[q], v1 = a.g1[q], vc = a.colour[q];
        }
        s_n[i] = vn, s_g1[i] = v1, s_c[i] = vc;
    }
    __syncthreads();
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= a.width || y >= a.height) return;
    gather_pixel<S>(a, T{s_n, s_g1, s_c, tx0, ty0}, x, y);
}

}  // namespace

extern "C" size_t rt_upsample_scratch_bytes(int low_width, int low_height) {
    if (low_width <= 0 || low_height <= 0) return 0;
    return (size_t)low_width * (size_t)low_height * 48u;  // normal, position and tag, colour: one float4 each per low pixel
}

extern "C" int rt_upsample(const rt_upsample_params* p, void* stream) {
    const char* const who = "rt_upsample";
    if (!p) return refuse(who, "null params");
    if (!p->low_surface) return refuse(who, "null low_surface");
    if (!p->low_hits) return refuse(who, "null low_hits");
    if (!p->hits) return refuse(who, "null hits");
    if (!p->out) return refuse(who, "null out");
    if (!p->scratch) return refuse(who, "null scratch");
    if (p->low_width <= 0 || p->low_height <= 0) return refuse(who, "low_width and low_height must be > 0");
    if (p->scale < 2 || p->scale > 4) return refuse(who, "scale must be 2, 3 or 4");
    const int64_t width = (int64_t)p->low_width * p->scale, height = (int64_t)p->low_height * p->scale;
    if (caps_refused(who, width, height, "UPSAMPLE")) return 1;
    if (materials_refused(who, p->materials, p->material_count)) return 1;
    if (p->low_pitch < (uint64_t)p->low_width * 16) return refuse(who, "low_pitch smaller than low_width * 16");
    if (pitch_refused(who, "out_pitch", p->out_pitch, (int)width)) return 1;
    if (pitches_refused(who, {p->low_pitch, p->out_pitch})) return 1;
    if (misaligned(who, "low_surface, low_hits, hits, materials, out and scratch", 16,
                   {p->low_surface, p->low_hits, p->hits, p->materials, p->out, p->scratch}))
        return 1;
    const uint64_t need = rt_upsample_scratch_bytes(p->low_width, p->low_height);
    if (p->scratch_bytes < need) return refuse(who, "scratch too small (rt_upsample_scratch_bytes)");
    const uint64_t low_n = (uint64_t)p->low_width * (uint64_t)p->low_height, n = (uint64_t)width * (uint64_t)height;
    const uint64_t out_bytes = surface_bytes((int)height, p->out_pitch, (uint64_t)width * 16);
    if (overlap(p->out, out_bytes, p->low_surface, surface_bytes(p->low_height, p->low_pitch, (uint64_t)p->low_width * 16)))
        return refuse(who, "out must not overlap low_surface");
    if (overlap(p->out, out_bytes, p->low_hits, low_n * 48)) return refuse(who, "out must not overlap low_hits");
    if (overlap(p->out, out_bytes, p->hits, n * 48)) return refuse(who, "out must not overlap hits");
    if (overlap(p->out, out_bytes, p->scratch, need)) return refuse(who, "out must not overlap scratch");
    if (overlap(p->out, out_bytes, p->materials, (uint64_t)p->material_count * sizeof(GPUMaterial)))
        return refuse(who, "out must not overlap materials");
    if (p->flags != 0) return refuse(who, "flags must be 0");
    if (p->reserved != 0) return refuse(who, "reserved must be 0");
    const int npow = or_default(p->normal_power_log2, RT_UPSAMPLE_DEFAULT, DEFAULT_NORMAL_POWER_LOG2);
    const float sigma_plane = or_default(p->sigma_plane, RT_UPSAMPLE_DEFAULT, DEFAULT_SIGMA_PLANE);
    if (npow < 0 || npow > 8) return refuse(who, "normal_power_log2 must be 0..8 (or RT_UPSAMPLE_DEFAULT)");
    if (!finite_above(sigma_plane, 0.0f)) return refuse(who, "sigma_plane must be > 0 and finite (or RT_UPSAMPLE_DEFAULT)");

    hipStream_t st = (hipStream_t)stream;
    float4* const gn = static_cast<float4*>(p->scratch);
    GatherArgs a;
    a.hits = static_cast<const float4*>(static_cast<const void*>(p->hits));
    a.materials = p->materials, a.material_count = (uint32_t)p->material_count;
    a.gn = gn, a.g1 = gn + low_n, a.colour = gn + 2 * low_n;
    a.out = static_cast<char*>(p->out), a.out_pitch = p->out_pitch;
    a.width = (int)width, a.height = (int)height, a.low_width = p->low_width, a.low_height = p->low_height;
    a.normal_power_log2 = npow, a.sigma_plane = sigma_plane;
    hipLaunchKernelGGL(upsample_prepare, image_grid(p->low_width, p->low_height), dim3(256), 0, st,
                       static_cast<const char*>(p->low_surface), p->low_pitch, p->low_width, p->low_height,
                       static_cast<const float4*>(static_cast<const void*>(p->low_hits)), p->materials,
                       (uint32_t)p->material_count, gn, gn + low_n, gn + 2 * low_n);
    const dim3 grid = image_grid(a.width, a.height);
    if (p->scale == 2) hipLaunchKernelGGL(upsample_gather<2>, grid, dim3(256), 0, st, a);
    else if (p->scale == 3) hipLaunchKernelGGL(upsample_gather<3>, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(upsample_gather<4>, grid, dim3(256), 0, st, a);
    return launch_refused(who);
}
