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

#include <cfloat>
#include <cstdint>
#include <cstdio>

#include "rt_abi.h"
#include "mirror.h"  // rt_internal_set_error

namespace {

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

int fail(const char* msg) {
    rt_internal_set_error(msg);
    return 1;
}

int hip_error(const char* call, const char* what, hipError_t e) {
    if (e == hipSuccess) return 0;
    char msg[200];
    snprintf(msg, sizeof msg, "%s: %s: %s", call, what, hipGetErrorString(e));
    return fail(msg);
}

// [a, a + an) and [b, b + bn) share a byte
bool overlap(const void* a, uint64_t an, const void* b, uint64_t bn) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return a && b && x < y + bn && y < x + an;
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

dim3 image_grid(int width, int height) { return dim3((unsigned)((width + 63) / 64), (unsigned)((height + 3) / 4)); }

// the checks the pitched-accumulator calls share; `row` = width * 16
int image_refused(const char* who, int width, int height, const void* accum, uint64_t pitch) {
    char msg[160];
    const char* what = nullptr;
    if (width <= 0 || height <= 0) what = "width and height must be > 0";
    else if ((int64_t)width * height > kMaxPixels) what = "more than 2^30 pixels";
    else if (pitch < (uint64_t)width * 16) what = "accum_pitch smaller than width * 16";
    else if (pitch & 15u) what = "accum_pitch must be a multiple of 16";
    else if ((uintptr_t)accum & 15u) what = "accum must be 16-byte aligned";
    if (!what) return 0;
    snprintf(msg, sizeof msg, "%s: %s", who, what);
    return fail(msg);
}

}  // namespace

extern "C" int rt_sample_priority(const rt_sample_priority_params* p, void* stream) {
    if (!p) return fail("rt_sample_priority: null params");
    if (!p->accum) return fail("rt_sample_priority: null accum");
    if (!p->moments) return fail("rt_sample_priority: null moments");
    if (!p->priority) return fail("rt_sample_priority: null priority");
    if (image_refused("rt_sample_priority", p->width, p->height, p->accum, p->accum_pitch)) return 1;
    if ((uintptr_t)p->moments & 7u) return fail("rt_sample_priority: moments must be 8-byte aligned");
    if ((uintptr_t)p->priority & 3u) return fail("rt_sample_priority: priority must be 4-byte aligned");
    const uint64_t n = (uint64_t)p->width * (uint64_t)p->height;
    const uint64_t accum_bytes = (uint64_t)(p->height - 1) * p->accum_pitch + (uint64_t)p->width * 16;
    if (overlap(p->priority, n * 4, p->accum, accum_bytes)) return fail("rt_sample_priority: priority must not overlap accum");
    if (overlap(p->priority, n * 4, p->moments, n * 8)) return fail("rt_sample_priority: priority must not overlap moments");
    hipLaunchKernelGGL(priority_kernel, image_grid(p->width, p->height), dim3(256), 0, (hipStream_t)stream,
                       static_cast<const char*>(p->accum), p->accum_pitch, reinterpret_cast<const float2*>(p->moments),
                       p->priority, p->width, p->height);
    return hip_error("rt_sample_priority", "launch failed", hipGetLastError());
}

extern "C" int rt_sample_resolve(const rt_sample_resolve_params* p, void* stream) {
    if (!p) return fail("rt_sample_resolve: null params");
    if (!p->accum) return fail("rt_sample_resolve: null accum");
    if (!p->out) return fail("rt_sample_resolve: null out");
    if (image_refused("rt_sample_resolve", p->width, p->height, p->accum, p->accum_pitch)) return 1;
    const uint64_t row = (uint64_t)p->width * 16;
    if (p->out_pitch < row) return fail("rt_sample_resolve: out_pitch smaller than width * 16");
    if (p->out_pitch & 15u) return fail("rt_sample_resolve: out_pitch must be a multiple of 16");
    if ((uintptr_t)p->out & 15u) return fail("rt_sample_resolve: out must be 16-byte aligned");
    if (overlap(p->out, (uint64_t)(p->height - 1) * p->out_pitch + row, p->accum, (uint64_t)(p->height - 1) * p->accum_pitch + row))
        return fail("rt_sample_resolve: out must not overlap accum");
    hipLaunchKernelGGL(resolve_kernel, image_grid(p->width, p->height), dim3(256), 0, (hipStream_t)stream,
                       static_cast<const char*>(p->accum), p->accum_pitch, static_cast<char*>(p->out), p->out_pitch, p->width,
                       p->height);
    return hip_error("rt_sample_resolve", "launch failed", hipGetLastError());
}

extern "C" size_t rt_sample_plan_scratch_bytes(int width, int height) {
    if (width <= 0 || height <= 0) return 0;
    return plan_layout((size_t)width * (size_t)height).end;
}

extern "C" int rt_sample_plan(const rt_sample_plan_params* p, void* stream) {
    const char* const who = "rt_sample_plan";
    if (!p) return fail("rt_sample_plan: null params");
    if (!p->priority) return fail("rt_sample_plan: null priority");
    if (!p->pixels) return fail("rt_sample_plan: null pixels");
    if (!p->samples) return fail("rt_sample_plan: null samples");
    if (!p->scratch) return fail("rt_sample_plan: null scratch");
    if (p->width <= 0 || p->height <= 0) return fail("rt_sample_plan: width and height must be > 0");
    const int64_t P = (int64_t)p->width * p->height;
    if (P > kMaxPixels) return fail("rt_sample_plan: more than 2^30 pixels");
    if (p->reserved != 0) return fail("rt_sample_plan: reserved must be 0");
    if (p->max_samples < 1 || p->max_samples > 4095) return fail("rt_sample_plan: max_samples must be 1..4095");
    if (p->min_samples < 0 || p->min_samples > p->max_samples) return fail("rt_sample_plan: min_samples must be 0..max_samples");
    if (!(p->scale > 0.0f) || !(p->scale <= FLT_MAX)) return fail("rt_sample_plan: scale must be > 0 and finite");
    if (p->budget < (int64_t)p->min_samples * P) return fail("rt_sample_plan: budget smaller than min_samples * width * height");
    if ((uintptr_t)p->scratch & 15u) return fail("rt_sample_plan: scratch must be 16-byte aligned");
    if ((uintptr_t)p->total & 7u) return fail("rt_sample_plan: total must be 8-byte aligned");
    if (((uintptr_t)p->priority | (uintptr_t)p->pixels) & 3u) return fail("rt_sample_plan: priority and pixels must be 4-byte aligned");
    if ((uintptr_t)p->samples & 1u) return fail("rt_sample_plan: samples must be 2-byte aligned");
    const size_t n = (size_t)P;
    const PlanLayout l = plan_layout(n);
    if (p->scratch_bytes < l.end) return fail("rt_sample_plan: scratch too small (rt_sample_plan_scratch_bytes)");
    const struct {
        const char* name;
        const void* ptr;
        uint64_t bytes;
    } bufs[5] = {{"priority", p->priority, n * 4}, {"pixels", p->pixels, n * 4}, {"samples", p->samples, n * 2},
                 {"total", p->total, 8},           {"scratch", p->scratch, l.end}};
    for (int i = 0; i < 5; i++)
        for (int j = i + 1; j < 5; j++)
            if (overlap(bufs[i].ptr, bufs[i].bytes, bufs[j].ptr, bufs[j].bytes)) {
                char msg[120];
                snprintf(msg, sizeof msg, "rt_sample_plan: %s must not overlap %s", bufs[i].name, bufs[j].name);
                return fail(msg);
            }

    const hipStream_t st = (hipStream_t)stream;
    char* const scratch = static_cast<char*>(p->scratch);
    unsigned long long* const cells = reinterpret_cast<unsigned long long*>(scratch);
    uint16_t* const keys = reinterpret_cast<uint16_t*>(scratch + l.keys);
    int32_t* const values = reinterpret_cast<int32_t*>(scratch + l.values);
    unsigned long long* const total = p->total ? reinterpret_cast<unsigned long long*>(p->total) : cells + 1;
    int end_bit = 0;  // the key max_samples - n_p is at most max_samples
    while ((p->max_samples >> end_bit) != 0) end_bit++;
    size_t sort_bytes = 0;
    if (hip_error(who, "radix sort size query",
                  hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, keys, p->samples, values, p->pixels, (int)n, 0, end_bit, st)))
        return 1;
    if (sort_bytes > l.sort_bound) return fail("rt_sample_plan: the radix sort asks for more storage than rt_sample_plan_scratch_bytes bounds");

    if (hip_error(who, "hipMemsetAsync", hipMemsetAsync(cells, 0, 16, st))) return 1;
    if (p->total && hip_error(who, "hipMemsetAsync", hipMemsetAsync(p->total, 0, 8, st))) return 1;
    const dim3 grid((unsigned)((n + 255) / 256));
    hipLaunchKernelGGL(quantise_sum, grid, dim3(256), 0, st, p->priority, (uint32_t)n, p->scale, cells);
    if (hip_error(who, "quantise_sum launch", hipGetLastError())) return 1;
    hipLaunchKernelGGL(plan_keys, grid, dim3(256), 0, st, p->priority, p->width, p->height, p->scale,
                       (unsigned long long)(p->budget - (int64_t)p->min_samples * P), (uint32_t)p->min_samples,
                       (uint32_t)p->max_samples, cells, keys, values, total);
    if (hip_error(who, "plan_keys launch", hipGetLastError())) return 1;
    if (hip_error(who, "radix sort",
                  hipcub::DeviceRadixSort::SortPairs(scratch + l.sort, sort_bytes, keys, p->samples, values, p->pixels, (int)n, 0,
                                                     end_bit, st)))
        return 1;
    hipLaunchKernelGGL(keys_to_counts, grid, dim3(256), 0, st, p->samples, (uint32_t)n, (uint32_t)p->max_samples);
    return hip_error(who, "keys_to_counts launch", hipGetLastError());
}
