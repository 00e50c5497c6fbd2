// rt_batch.h -- the scaffold of the one-item-per-lane units, wave w owning items [64w, 64w + 64).
//
// A ray-batch unit (rt_query.hip, rt_occlude.hip, rt_radiance.hip, rt_adaptive.hip) goes through rtfast::trace.  It
// writes its body
//     template <int STACK, int MODE> void body(const Args&, const rtfast::Stack<RT_BATCH_SL(STACK)>&, uint32_t* scratch)
// names its kernels with RT_BATCH_KERNELS and launches them with launch_batch.  The variants are the ones a
// production frame runs at RT_TUNE 0 (rt_variant.h choose_variant): MODE_PROD = 17 or its lean form 17 | 128 for
// scenes without leaf trees, 21 with them; stacks of 30 / 40 / 64 entries; 5, 6 and 7 waves per SIMD.
//
// A walk unit (rt_closest.hip, rt_hits.hip) never calls trace: each lane walks the mirror's private nodes itself, so
// its frame is the stack's LDS rows alone and it has no MODE -- whether a leaf has a tree is read from its lead
// record.  It writes its body
//     template <int STACK, int V> void body(const Args&, const rtfast::Stack<RT_BATCH_SL(STACK)>&)
// with V a build integer of its own (0 where it has none), names its kernels with RT_WALK_KERNELS and launches them
// with launch_walk.
//
// Compiled with the flags of every other unit (rt_fast_body.h RT_FAST_FAMILY, build.py).
#pragma once

#include <hip/hip_runtime.h>

#include "rt_abi.h"
#include "rt_device.h"
#include "rt_math.h"
#include "rt_common.h"
#include "leaftree.h"
#include "rt_fast.h"
#include "rt_render.h"

#ifndef RT_LDS_SL
#define RT_LDS_SL 16  // stack entries in LDS, as in rt_fast_body.h
#endif
#define RT_BATCH_SL(STACK) ((STACK) < RT_LDS_SL ? (STACK) : RT_LDS_SL)

// NAME_w5, NAME_w6, NAME_w7<STACK, MODE>(ARGS): BODY in the render kernel's frame (rt_fast.h RT_TRACE_FRAME) at 5 / 6 /
// 7 waves per SIMD, and NAME_set (RT_KERNEL_SET), which hands the launcher the one of them a launch asks for.
#define RT_BATCH_KERNEL(NAME, W, ARGS, BODY) \
    template <int STACK, int MODE> \
    __global__ __launch_bounds__(WAVE) __attribute__((amdgpu_waves_per_eu(W))) void NAME(ARGS a) { \
        RT_TRACE_FRAME(STACK, MODE) \
        BODY<STACK, MODE>(a, rtfast::Stack<SL>{stack_lds, ovf}, scratch_lds); \
    }
#define RT_KERNEL_SET(NAME) \
    struct NAME##_set { \
        template <int STACK, int V> \
        static auto get(int w) { \
            if (w == 7) return NAME##_w7<STACK, V>; \
            if (w == 6) return NAME##_w6<STACK, V>; \
            return NAME##_w5<STACK, V>; \
        } \
    };
#define RT_BATCH_KERNELS(NAME, ARGS, BODY) \
    RT_BATCH_KERNEL(NAME##_w5, 5, ARGS, BODY) \
    RT_BATCH_KERNEL(NAME##_w6, 6, ARGS, BODY) \
    RT_BATCH_KERNEL(NAME##_w7, 7, ARGS, BODY) \
    RT_KERNEL_SET(NAME)

// NAME_w5, NAME_w6, NAME_w7<STACK, V>(ARGS) and NAME_set for a walk unit: BODY in the stack-only frame -- the LDS rows
// of rtfast::Stack and the private overflow entries, no scratch_lds.
#define RT_WALK_KERNEL(NAME, W, ARGS, BODY) \
    template <int STACK, int V> \
    __global__ __launch_bounds__(WAVE) __attribute__((amdgpu_waves_per_eu(W))) void NAME(ARGS a) { \
        constexpr int SL = RT_BATCH_SL(STACK); \
        __shared__ uint32_t stack_lds[(SL + rtfast::STACK_PAD_ROWS) * WAVE]; \
        uint32_t ovf[STACK > SL ? STACK - SL : 1]; \
        BODY<STACK, V>(a, rtfast::Stack<SL>{stack_lds, ovf}); \
    }
#define RT_WALK_KERNELS(NAME, ARGS, BODY) \
    RT_WALK_KERNEL(NAME##_w5, 5, ARGS, BODY) \
    RT_WALK_KERNEL(NAME##_w6, 6, ARGS, BODY) \
    RT_WALK_KERNEL(NAME##_w7, 7, ARGS, BODY) \
    RT_KERNEL_SET(NAME)

namespace rtk {

// Ray i of a launch whose Args name rays, width, height and cam as QueryArgs does (rt_query.hip, rt_hits.hip): the
// caller's record as two 16-byte loads (adjacent lanes, adjacent records), or -- rays null -- the camera ray through
// the centre of pixel (i % width, i / width) in the operation order of render_fast_body's sample start.  Called again
// after the traversal, so that only the index is carried across it.
template <class Args>
__device__ __forceinline__ void query_ray(const Args& q, long long i, rtm::f3& ro, rtm::f3& rd, float& tmax) {
    if (q.rays) {
        const float4* const r = reinterpret_cast<const float4*>(q.rays + i);
        const float4 a = r[0], b = r[1];
        ro = rtm::mk(a.x, a.y, a.z);
        tmax = a.w;
        rd = rtm::mk(b.x, b.y, b.z);
    } else {
        const int x = (int)(i % q.width), y = (int)(i / q.width);
        const float uvx = ((float)x + 0.5f) / (float)q.width;
        const float uvy = ((float)y + 0.5f) / (float)q.height;
        const rtm::f3 co = ld3(q.cam.origin), ch = ld3(q.cam.horizontal), cv = ld3(q.cam.vertical),
                      cl = ld3(q.cam.lower_left_corner);
        ro = co;
        rd = rtm::sub(rtm::add(rtm::add(cl, rtm::muls(ch, uvx)), rtm::muls(cv, uvy)), co);
        tmax = 1e30f;
    }
}

// GetRayHit's sphere loop (main_raytracing.cu:87-101) on a Hit whose `best` starts at the ray's tmax: in order and to
// the end, since a later sphere overrides an earlier one whenever `dist >= best` is false.
__device__ __forceinline__ rtfast::Hit sphere_loop(const QueryArgs& q, rtm::f3 ro, rtm::f3 nd, rtfast::Hit h) {
    for (int k = 0; k < q.sphere_count; k++) {
        const GeometrySphere& sp = q.spheres[k];
        float dist;
        if (rtd::intersect_sphere(ro, nd, ld3(sp.position), sp.radius * sp.radius, &dist)) {
            if (dist >= h.best) continue;
            h.best = dist;
            h.kind = 1;
            h.id = (uint32_t)k;
        }
    }
    return h;
}

// One rt_hit record (rt_trace_rays' and every row of rt_trace_hits', bytewise alike): three 16-byte stores, adjacent
// lanes to adjacent records.  A hit at distance t along the normalised nd, of sphere (kind 1) or face (kind 2) `id`
// with the barycentrics (bx, by) -- 0 for a sphere: the attributes of shade_segment (rt_fast_body.h), same arithmetic.
__device__ __forceinline__ void store_hit(float4* out, rtm::f3 ro, rtm::f3 nd, float t, uint32_t kind, uint32_t id, float bx,
                                          float by, const GeometrySphere* spheres, const GPUFace* faces, const GPUVertex* vertices) {
    const rtm::f3 pos = rtm::add(ro, rtm::muls(nd, t));
    rtm::f3 nrm;
    uint32_t mat;
    if (kind == 1) {
        const GeometrySphere& sp = spheres[id];
        nrm = rtm::divs(rtm::sub(pos, ld3(sp.position)), sp.radius);
        mat = (uint32_t)sp.material;
    } else {
        const GPUFace f = faces[id];
        const float bz = (1.0f - bx) - by;
        nrm = rtm::normalize(rtm::add(rtm::add(rtm::muls(ld3(vertices[f.v0].normal), bx), rtm::muls(ld3(vertices[f.v1].normal), by)),
                                      rtm::muls(ld3(vertices[f.v2].normal), bz)));
        if (rtm::dot(nd, nrm) >= 0.0f) nrm = rtm::neg(nrm);
        mat = f.material;
    }
    out[0] = make_float4(t, __uint_as_float(kind), __uint_as_float(id), __uint_as_float(mat));
    out[1] = make_float4(nrm.x, nrm.y, nrm.z, bx);
    out[2] = make_float4(pos.x, pos.y, pos.z, by);
}
// ... and the miss record: the ray's tmax, zeros.
__device__ __forceinline__ void store_miss(float4* out, float tmax) {
    out[0] = make_float4(tmax, 0.0f, 0.0f, 0.0f);
    out[1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    out[2] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

template <class K, int STACK, class A>
auto batch_kernel(int mode, int w) -> void (*)(A) {
    using namespace rtfast;
    switch (mode) {
        case MODE_PROD: return K::template get<STACK, MODE_PROD>(w);
        case MODE_PROD | LEAN_BIT: return K::template get<STACK, MODE_PROD | LEAN_BIT>(w);
        case MODE_PROD | TREE_BIT: return K::template get<STACK, MODE_PROD | TREE_BIT>(w);
    }
    return nullptr;  // a mode the batch kernels are not built in
}

// One wave per 64 of `count` items.  An empty batch, or one past the 32-bit item index (2^31), is refused, as is a
// kernel the set was not built with.
template <class A>
hipError_t launch_items(void (*k)(A), long long count, const A& a, hipStream_t s) {
    if (!k || count <= 0 || count > (1LL << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k, dim3((unsigned)((count + WAVE - 1) / WAVE)), dim3(WAVE), 0, s, a);
    return hipGetLastError();
}

// Kernel set K (RT_BATCH_KERNELS' NAME_set): stack 30 / 40 / 64, then the mode, then the occupancy.
template <class K, class A>
hipError_t launch_batch(int stack, int mode, int w, long long count, const A& a, hipStream_t s) {
    return launch_items<A>(stack == 30   ? batch_kernel<K, 30, A>(mode, w)
                           : stack == 40 ? batch_kernel<K, 40, A>(mode, w)
                                         : batch_kernel<K, 64, A>(mode, w),
                           count, a, s);
}

// Kernel set K (RT_WALK_KERNELS' NAME_set) in the unit's build V: stack 30 / 40 / 64, then the occupancy.
template <class K, int V, class A>
hipError_t launch_walk(int stack, int w, long long count, const A& a, hipStream_t s) {
    return launch_items<A>(stack == 30   ? K::template get<30, V>(w)
                           : stack == 40 ? K::template get<40, V>(w)
                                         : K::template get<64, V>(w),
                           count, a, s);
}

}  // namespace rtk
