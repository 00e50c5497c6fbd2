// rt_batch.h -- the scaffold of a ray-batch unit (rt_query.hip, rt_occlude.hip, rt_radiance.hip): one ray (or pixel)
// per lane, wave w owning items [64w, 64w + 64), through rtfast::trace.  A unit writes its body
//     template <int STACK, int MODE> void body(const Args&, const rtfast::Stack<RT_BATCH_SL(STACK)>&, uint32_t* scratch)
// names its kernels with RT_BATCH_KERNELS and launches them with launch_batch.  The variants are the ones a
// production frame runs at RT_TUNE 0 (rt_variant.h choose_variant): MODE_PROD = 17 or its lean form 17 | 128 for
// scenes without leaf trees, 21 with them; stacks of 30 / 40 / 64 entries; 5, 6 and 7 waves per SIMD.  Compiled with
// the flags of every other unit (rt_fast_body.h RT_FAST_FAMILY, build.py).
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
// 7 waves per SIMD, and NAME_set, which hands launch_batch the one of them a launch asks for.
#define RT_BATCH_KERNEL(NAME, W, ARGS, BODY) \
    template <int STACK, int MODE> \
    __global__ __launch_bounds__(WAVE) __attribute__((amdgpu_waves_per_eu(W))) void NAME(ARGS a) { \
        RT_TRACE_FRAME(STACK, MODE) \
        BODY<STACK, MODE>(a, rtfast::Stack<SL>{stack_lds, ovf}, scratch_lds); \
    }
#define RT_BATCH_KERNELS(NAME, ARGS, BODY) \
    RT_BATCH_KERNEL(NAME##_w5, 5, ARGS, BODY) \
    RT_BATCH_KERNEL(NAME##_w6, 6, ARGS, BODY) \
    RT_BATCH_KERNEL(NAME##_w7, 7, ARGS, BODY) \
    struct NAME##_set { \
        template <int STACK, int MODE> \
        static auto get(int w) { \
            if (w == 7) return NAME##_w7<STACK, MODE>; \
            if (w == 6) return NAME##_w6<STACK, MODE>; \
            return NAME##_w5<STACK, MODE>; \
        } \
    };

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

// One wave per 64 of `count` items with kernel set K (RT_BATCH_KERNELS' NAME_set): stack 30 / 40 / 64, then the mode,
// then the occupancy.  An empty batch, or one past the 32-bit item index (2^31), is refused.
template <class K, class A>
hipError_t launch_batch(int stack, int mode, int w, long long count, const A& a, hipStream_t s) {
    if (count <= 0 || count > (1LL << 31)) return hipErrorInvalidValue;
    void (*const k)(A) = stack == 30 ? batch_kernel<K, 30, A>(mode, w)
                         : stack == 40 ? batch_kernel<K, 40, A>(mode, w)
                                       : batch_kernel<K, 64, A>(mode, w);
    if (!k) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k, dim3((unsigned)((count + WAVE - 1) / WAVE)), dim3(WAVE), 0, s, a);
    return hipGetLastError();
}

}  // namespace rtk
