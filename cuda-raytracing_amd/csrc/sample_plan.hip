// sample_plan.hip -- the pixel kernels of adaptive sampling (include/rt_abi.h): rt_sample_priority (accumulator and
// moments -> priority), rt_sample_plan (priorities and a budget -> the list of the next round) and rt_sample_resolve
// (accumulator -> image).  No scene.  The arithmetic is the header's: fp32 without contraction and IEEE division
// (build.py's flags), exact integers in the planner; tests/adaptive_ref.py restates all three.
//
// The planner, in stream order:
//   memset          the two 64-bit cells at the head of scratch (Q, and the total when the caller keeps none)
//   quantise_sum    q_p per pixel, Q = sum q_p (integer atomics: exact in any order)
//   plan_keys       n_p per pixel; key max_samples - n_p and value p at the pixel's place in the 8x8 sub-tile
//                   enumeration; total = sum n_p
//   hipcub          stable radix sort of (key, value) over the bits max_samples needs: keys into `samples`, values
//                   into `pixels`
//   keys_to_counts  samples[i] = max_samples - samples[i]
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <cstdint>

#include "image_entry.h"
#include "rt_abi.h"

namespace {

using namespace rt_entry;

constexpr int64_t kMaxPixels = (int64_t)1 << 30;

__device__ __forceinline__ bool is_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

__global__ __launch_bounds__(256) void priority_kernel(const char* accum, uint64_t pitch, const float2* moments,
                                                       float* priority, int width, int height) {
    const int x = (int)(blockIdx.x * 64u + (threadIdx.x & 63u)), y = (int)(blockIdx.y * 4u + (threadIdx.x >> 6));
    if (x >= width || y >= height) return;
    const size_t p = (size_t)y * (size_t)width + (size_t)x;
    const float n = reinterpret_cast<const float4*>(accum + (size_t)y * pitch)[x].w;
    const float2 m = moments[p];
    float pr = __uint_as_float(0x7f800000u);  // +inf: unknown pixels go first
    if (n >= 2.0f && is_finite(m.x) && is_finite(m.y)) {
        const float m1 = m.x / n, m2 = m.y / n;
        const float var = fmaxf(0.0f, m2 - m1 * m1) / n;
        pr = var / (m1 * m1 + 1e-4f);
    }
    priority[p] = pr;
}

__global__ __launch_bounds__(256) void resolve_kernel(const char* accum, uint64_t pitch, char* out, uint64_t out_pitch,
                                                      int width, int height) {
    const int x = (int)(blockIdx.x * 64u + (threadIdx.x & 63u)), y = (int)(blockIdx.y * 4u + (threadIdx.x >> 6));
    if (x >= width || y >= height) return;
    const float4 a = reinterpret_cast<const float4*>(accum + (size_t)y * pitch)[x];
    float4 o = make_float4(0.0f, 0.0f, 0.0f, 1.0f);
    if (a.w >= 1.0f) o.x = a.x / a.w, o.y = a.y / a.w, o.z = a.z / a.w;
    reinterpret_cast<float4*>(out + (size_t)y * out_pitch)[x] = o;
}

__device__ __forceinline__ uint32_t quantise(float priority, float scale) {
    const float t = priority * scale;
    return !(t < 65535.0f) ? 65535u : (t > 0.0f ? (uint32_t)t : 0u);
}

// The sum of v over the block into *cell: wave shuffles, then one atomic per wave.
__device__ __forceinline__ void block_add(unsigned long long v, unsigned long long* cell) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if ((threadIdx.x & 63u) == 0 && v) atomicAdd(cell, v);
}

__global__ __launch_bounds__(256) void quantise_sum(const float* priority, uint32_t pixels, float scale,
                                                    unsigned long long* q_sum) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    block_add(p < pixels ? quantise(priority[p], scale) : 0u, q_sum);
}

// floor(q * B / Q) for q < 2^16, Q < 2^46, capped at 4096 q (every cap the planner applies is below): with
// B = k Q + r, q B / Q = q k + q r / Q, and q r < 2^62.
__device__ __forceinline__ unsigned long long share(unsigned long long q, unsigned long long B, unsigned long long Q) {
    unsigned long long k = B / Q;
    const unsigned long long r = B % Q;
    if (k > 4096ull) k = 4096ull;
    return q * k + q * r / Q;
}

__global__ __launch_bounds__(256) void plan_keys(const float* priority, int width, int height, float scale,
                                                 unsigned long long budget_extra, uint32_t min_samples, uint32_t max_samples,
                                                 const unsigned long long* q_sum, uint16_t* keys, int32_t* values,
                                                 unsigned long long* total) {
    const uint32_t pixels = (uint32_t)width * (uint32_t)height, p = blockIdx.x * 256u + threadIdx.x;
    uint32_t n = 0;
    if (p < pixels) {
        const unsigned long long Q = *q_sum;
        const uint32_t q = quantise(priority[p], scale);
        const unsigned long long extra = Q ? share(q, budget_extra, Q) : 0ull;
        n = extra >= (unsigned long long)(max_samples - min_samples) ? max_samples : min_samples + (uint32_t)extra;
        // the pixel's place in the sub-tile enumeration: the full tile rows above, the tiles to the left, inside the tile
        const uint32_t w = (uint32_t)width, x = p % w, y = p / w, tx = x >> 3, ty = y >> 3;
        const uint32_t tw = min(8u, w - 8u * tx), th = min(8u, (uint32_t)height - 8u * ty);
        const uint32_t e = ty * 8u * w + tx * 8u * th + (y & 7u) * tw + (x & 7u);
        keys[e] = (uint16_t)(max_samples - n);
        values[e] = (int32_t)p;
    }
    block_add(n, total);
}

__global__ __launch_bounds__(256) void keys_to_counts(uint16_t* samples, uint32_t pixels, uint32_t max_samples) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < pixels) samples[i] = (uint16_t)(max_samples - samples[i]);
}

size_t round16(size_t n) { return (n + 15u) & ~(size_t)15u; }

// scratch: [0, 16) the cells, then the unsorted keys, the unsorted values, the sort's storage
struct PlanLayout {
    size_t keys, values, sort, sort_bound, end;
};
PlanLayout plan_layout(size_t n) {
    PlanLayout l;
    l.keys = 16;
    l.values = l.keys + round16(n * 2);
    l.sort = l.values + round16(n * 4);
    l.sort_bound = round16(n * 2) + round16(n * 4) + n * 16 + 65536;  // rt_abi.h rt_sample_plan_scratch_bytes
    l.end = l.sort + l.sort_bound;
    return l;
}

// the checks the pitched-accumulator calls share
int accum_refused(const char* who, int width, int height, const void* accum, uint64_t pitch) {
    if (size_refused(who, width, height)) return 1;
    if ((int64_t)width * height > kMaxPixels) return refuse(who, "more than 2^30 pixels");
    if (pitch_refused(who, "accum_pitch", pitch, width)) return 1;
    if (pitch & 15u) return refuse(who, "accum_pitch must be a multiple of 16");
    return misaligned(who, "accum", 16, {accum});
}

}  // namespace

extern "C" int rt_sample_priority(const rt_sample_priority_params* p, void* stream) {
    const char* const who = "rt_sample_priority";
    if (!p) return refuse(who, "null params");
    if (!p->accum) return refuse(who, "null accum");
    if (!p->moments) return refuse(who, "null moments");
    if (!p->priority) return refuse(who, "null priority");
    if (accum_refused(who, p->width, p->height, p->accum, p->accum_pitch)) return 1;
    if (misaligned(who, "moments", 8, {p->moments}) || misaligned(who, "priority", 4, {p->priority})) return 1;
    const uint64_t n = (uint64_t)p->width * (uint64_t)p->height;
    const uint64_t accum_bytes = surface_bytes(p->height, p->accum_pitch, (uint64_t)p->width * 16);
    if (overlap(p->priority, n * 4, p->accum, accum_bytes)) return refuse(who, "priority must not overlap accum");
    if (overlap(p->priority, n * 4, p->moments, n * 8)) return refuse(who, "priority must not overlap moments");
    hipLaunchKernelGGL(priority_kernel, image_grid(p->width, p->height), dim3(256), 0, (hipStream_t)stream,
                       static_cast<const char*>(p->accum), p->accum_pitch, reinterpret_cast<const float2*>(p->moments),
                       p->priority, p->width, p->height);
    return launch_refused(who);
}

extern "C" int rt_sample_resolve(const rt_sample_resolve_params* p, void* stream) {
    const char* const who = "rt_sample_resolve";
    if (!p) return refuse(who, "null params");
    if (!p->accum) return refuse(who, "null accum");
    if (!p->out) return refuse(who, "null out");
    if (accum_refused(who, p->width, p->height, p->accum, p->accum_pitch)) return 1;
    if (pitch_refused(who, "out_pitch", p->out_pitch, p->width)) return 1;
    if (p->out_pitch & 15u) return refuse(who, "out_pitch must be a multiple of 16");
    if (misaligned(who, "out", 16, {p->out})) return 1;
    const uint64_t row = (uint64_t)p->width * 16;
    if (overlap(p->out, surface_bytes(p->height, p->out_pitch, row), p->accum, surface_bytes(p->height, p->accum_pitch, row)))
        return refuse(who, "out must not overlap accum");
    hipLaunchKernelGGL(resolve_kernel, image_grid(p->width, p->height), dim3(256), 0, (hipStream_t)stream,
                       static_cast<const char*>(p->accum), p->accum_pitch, static_cast<char*>(p->out), p->out_pitch, p->width,
                       p->height);
    return launch_refused(who);
}

extern "C" size_t rt_sample_plan_scratch_bytes(int width, int height) {
    if (width <= 0 || height <= 0) return 0;
    return plan_layout((size_t)width * (size_t)height).end;
}

extern "C" int rt_sample_plan(const rt_sample_plan_params* p, void* stream) {
    const char* const who = "rt_sample_plan";
    if (!p) return refuse(who, "null params");
    if (!p->priority) return refuse(who, "null priority");
    if (!p->pixels) return refuse(who, "null pixels");
    if (!p->samples) return refuse(who, "null samples");
    if (!p->scratch) return refuse(who, "null scratch");
    if (size_refused(who, p->width, p->height)) return 1;
    const int64_t P = (int64_t)p->width * p->height;
    if (P > kMaxPixels) return refuse(who, "more than 2^30 pixels");
    if (p->reserved != 0) return refuse(who, "reserved must be 0");
    if (p->max_samples < 1 || p->max_samples > 4095) return refuse(who, "max_samples must be 1..4095");
    if (p->min_samples < 0 || p->min_samples > p->max_samples) return refuse(who, "min_samples must be 0..max_samples");
    if (!finite_above(p->scale, 0.0f)) return refuse(who, "scale must be > 0 and finite");
    if (p->budget < (int64_t)p->min_samples * P) return refuse(who, "budget smaller than min_samples * width * height");
    if (misaligned(who, "scratch", 16, {p->scratch}) || misaligned(who, "total", 8, {p->total}) ||
        misaligned(who, "priority and pixels", 4, {p->priority, p->pixels}) || misaligned(who, "samples", 2, {p->samples}))
        return 1;
    const size_t n = (size_t)P;
    const PlanLayout l = plan_layout(n);
    if (p->scratch_bytes < l.end) return refuse(who, "scratch too small (rt_sample_plan_scratch_bytes)");
    const struct {
        const char* name;
        const void* ptr;
        uint64_t bytes;
    } bufs[5] = {{"priority", p->priority, n * 4}, {"pixels", p->pixels, n * 4}, {"samples", p->samples, n * 2},
                 {"total", p->total, 8},           {"scratch", p->scratch, l.end}};
    for (int i = 0; i < 5; i++)
        for (int j = i + 1; j < 5; j++)
            if (overlap(bufs[i].ptr, bufs[i].bytes, bufs[j].ptr, bufs[j].bytes))
                return refuse(who, std::string(bufs[i].name) + " must not overlap " + bufs[j].name);

    const hipStream_t st = (hipStream_t)stream;
    char* const scratch = static_cast<char*>(p->scratch);
    unsigned long long* const cells = reinterpret_cast<unsigned long long*>(scratch);
    uint16_t* const keys = reinterpret_cast<uint16_t*>(scratch + l.keys);
    int32_t* const values = reinterpret_cast<int32_t*>(scratch + l.values);
    unsigned long long* const total = p->total ? reinterpret_cast<unsigned long long*>(p->total) : cells + 1;
    int end_bit = 0;  // the key max_samples - n_p is at most max_samples
    while ((p->max_samples >> end_bit) != 0) end_bit++;
    size_t sort_bytes = 0;
    if (hip_refused(who, "radix sort size query",
                  hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, keys, p->samples, values, p->pixels, (int)n, 0, end_bit, st)))
        return 1;
    if (sort_bytes > l.sort_bound) return refuse(who, "the radix sort asks for more storage than rt_sample_plan_scratch_bytes bounds");

    if (hip_refused(who, "hipMemsetAsync", hipMemsetAsync(cells, 0, 16, st))) return 1;
    if (p->total && hip_refused(who, "hipMemsetAsync", hipMemsetAsync(p->total, 0, 8, st))) return 1;
    const dim3 grid((unsigned)((n + 255) / 256));
    hipLaunchKernelGGL(quantise_sum, grid, dim3(256), 0, st, p->priority, (uint32_t)n, p->scale, cells);
    if (hip_refused(who, "quantise_sum launch", hipGetLastError())) return 1;
    hipLaunchKernelGGL(plan_keys, grid, dim3(256), 0, st, p->priority, p->width, p->height, p->scale,
                       (unsigned long long)(p->budget - (int64_t)p->min_samples * P), (uint32_t)p->min_samples,
                       (uint32_t)p->max_samples, cells, keys, values, total);
    if (hip_refused(who, "plan_keys launch", hipGetLastError())) return 1;
    if (hip_refused(who, "radix sort",
                  hipcub::DeviceRadixSort::SortPairs(scratch + l.sort, sort_bytes, keys, p->samples, values, p->pixels, (int)n, 0,
                                                     end_bit, st)))
        return 1;
    hipLaunchKernelGGL(keys_to_counts, grid, dim3(256), 0, st, p->samples, (uint32_t)n, (uint32_t)p->max_samples);
    return hip_refused(who, "keys_to_counts launch", hipGetLastError());
}
