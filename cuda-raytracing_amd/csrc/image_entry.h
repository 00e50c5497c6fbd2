// image_entry.h -- what the entry points share on the host: how a call refuses ("who: what" through
// rt_internal_set_error, return value 1) and the checks of a pitched float4 image, each written once.  Used by the
// image-space calls (denoise.hip, denoise_variance.hip, reproject.hip, sample_plan.hip, upsample.hip, image.hip) and by the
// ray-batch calls (rt_batch_calls.hip), rt_render.hip and rng_shard.hip.  A check whose wording belongs to one call stays a line of that call.
#pragma once

#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdint>
#include <initializer_list>
#include <string>

#include "mirror.h"  // rt_internal_set_error
#include "rt_abi.h"

namespace rt_entry {

// "who: what" as the last error; 1, the refusing call's return value
inline int refuse(const char* who, const std::string& what) {
    rt_internal_set_error((std::string(who) + ": " + what).c_str());
    return 1;
}

// "who: what: <HIP's text>" unless e is hipSuccess
inline int hip_refused(const char* who, const char* what, hipError_t e) {
    return e == hipSuccess ? 0 : refuse(who, std::string(what) + ": " + hipGetErrorString(e));
}
// after the launches of a call: whether any of them failed
inline int launch_refused(const char* who, const char* what = "launch failed") { return hip_refused(who, what, hipGetLastError()); }

inline int misaligned(const char* who, const char* names, unsigned align, std::initializer_list<const void*> ptrs) {
    uintptr_t bits = 0;
    for (const void* p : ptrs) bits |= (uintptr_t)p;
    return (bits & (align - 1)) ? refuse(who, std::string(names) + " must be " + std::to_string(align) + "-byte aligned") : 0;
}

// [a, a + an) and [b, b + bn) share a byte; a null buffer overlaps nothing
inline bool overlap(const void* a, uint64_t an, const void* b, uint64_t bn) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return a && b && x < y + bn && y < x + an;
}

// v unless it is the call's RT_*_DEFAULT, which selects the measured default
template <class T>
T or_default(T v, int sentinel, T measured) {
    return v == (T)sentinel ? measured : v;
}

// v in (lo, FLT_MAX], or in [lo, FLT_MAX]; a NaN is in neither
inline bool finite_above(float v, float lo) { return v > lo && v <= FLT_MAX; }
inline bool finite_from(float v, float lo) { return v >= lo && v <= FLT_MAX; }

// one lane per pixel, a wave 64 x 1 pixels, a block 64 x 4
inline dim3 image_grid(int width, int height) { return dim3((unsigned)((width + 63) / 64), (unsigned)((height + 3) / 4)); }

// bytes from the first to the last pixel of a pitched image whose rows hold `row` bytes
inline uint64_t surface_bytes(int height, uint64_t pitch, uint64_t row) { return (uint64_t)(height - 1) * pitch + row; }

inline int size_refused(const char* who, int width, int height) {
    return (width <= 0 || height <= 0) ? refuse(who, "width and height must be > 0") : 0;
}
// The caps of the filters' launch grids (a row of blocks per 4 or 8 pixel rows in grid.y, at most 65,535) and scratch;
// `family` names the constants the message quotes: "DENOISE", "REPROJECT" or "UPSAMPLE", which rt_abi.h defines alike.
// The sizes are 64 bits wide for rt_upsample, whose capped size is a product (scale * low size, below 2^34).
inline int caps_refused(const char* who, int64_t width, int64_t height, const char* family) {
    static_assert(RT_REPROJECT_MAX_HEIGHT == RT_DENOISE_MAX_HEIGHT && RT_REPROJECT_MAX_PIXELS == RT_DENOISE_MAX_PIXELS &&
                      RT_UPSAMPLE_MAX_HEIGHT == RT_DENOISE_MAX_HEIGHT && RT_UPSAMPLE_MAX_PIXELS == RT_DENOISE_MAX_PIXELS,
                  "one set of caps");
    if (height > RT_DENOISE_MAX_HEIGHT) return refuse(who, std::string("height above RT_") + family + "_MAX_HEIGHT");
    if (width * height > RT_DENOISE_MAX_PIXELS) return refuse(who, std::string("more than RT_") + family + "_MAX_PIXELS pixels");
    return 0;
}
// a row of float4 pixels must fit the pitch called `name`
inline int pitch_refused(const char* who, const char* name, uint64_t pitch, int width) {
    return pitch < (uint64_t)width * 16 ? refuse(who, std::string(name) + " smaller than width * 16") : 0;
}
inline int pitches_refused(const char* who, std::initializer_list<uint64_t> pitches) {
    uint64_t bits = 0;
    for (const uint64_t p : pitches) bits |= p;
    return (bits & 15u) ? refuse(who, "pitches must be multiples of 16") : 0;
}
inline int materials_refused(const char* who, const GPUMaterial* materials, int material_count) {
    if (material_count < 0) return refuse(who, "negative material_count");
    return (material_count > 0 && !materials) ? refuse(who, "null materials with material_count > 0") : 0;
}

}  // namespace rt_entry
