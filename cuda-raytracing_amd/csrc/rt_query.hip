// rt_query.hip -- the ray-query kernel behind rt_trace_rays (include/rt_abi.h): a second, thin body on the
// render kernel's traversal.  One ray per lane, wave w owning rays [64w, 64w + 64): the lane reads its ray (or
// forms the camera ray of its pixel centre), runs GetRayHit's sphere loop and rtfast::trace exactly as
// render_fast_body does (rt_fast_body.h), and writes one 48-byte hit record with the attributes shade_segment
// computes -- no RNG, no shading, no sky, no surface.  The variants are the ones a production frame runs at
// RT_TUNE 0 (rt_variant.h choose_variant): MODE_PROD = 17 or its lean form 17 | 128 for scenes without leaf
// trees, 21 with them; stacks of 30 / 40 / 64 entries; 5, 6 and 7 waves per SIMD.  rt_kernel.hip picks one
// (rt_trace_rays).  Compiled with the flags of every other unit (rt_fast_body.h RT_FAST_FAMILY, build.py).
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

namespace rtk {
namespace {

// Ray i of the launch: the caller's record as two 16-byte loads (adjacent lanes, adjacent records), or the
// camera ray through the centre of pixel (i % width, i / width) in the operation order of render_fast_body's
// sample start.  Called again after the traversal, so that only the index is carried across it.
__device__ __forceinline__ void query_ray(const QueryArgs& q, long long i, rtm::f3& ro, rtm::f3& rd, float& tmax) {
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

template <int STACK, int MODE>
__device__ __forceinline__ void query_body(const QueryArgs& q,
                                           const rtfast::Stack<(STACK < RT_LDS_SL ? STACK : RT_LDS_SL)>& stk,
                                           uint32_t* const scratch) {
    const long long i = (long long)blockIdx.x * WAVE + (long long)(threadIdx.x & 63u);
    const bool live = i < q.count;  // lanes past the batch still call trace: its big-leaf rounds are wave-cooperative
    rtm::f3 ro = rtm::mk(0, 0, 0), rd = rtm::mk(0, 0, 1);
    float tmax = 0.0f;
    if (live) query_ray(q, i, ro, rd, tmax);

    // GetRayHit (main_raytracing.cu:83-109) with the closest distance starting at the ray's tmax
    rtfast::Hit h;
    h.best = tmax, h.kind = 0, h.id = 0, h.bx = h.by = 0.0f;
    rtm::f3 nd = rtm::normalize(rd);
    if (live) {
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
    }
    rtfast::Ray R = rtfast::make_ray(ro, rd, nd, q.scene_fast != 0);
    Counters c;
    rtfast::trace<false, MODE>(reinterpret_cast<const float4*>(q.nodes), reinterpret_cast<const float4*>(q.tris), q.pairs,
                               q.tree, q.ltris, q.flat, q.spairs, 0u, stk, scratch, R, h, live, c, q.quads, q.units,
                               q.face_leaf);
    if (!live) return;

    // the record: three 16-byte stores, adjacent lanes to adjacent records
    query_ray(q, i, ro, rd, tmax);
    nd = rtm::normalize(rd);
    float4* const out = reinterpret_cast<float4*>(q.hits + i);
    // `result.distance < max_distance` (main_raytracing.cu:108): a NaN distance is a miss
    if (h.kind != 0 && h.best < tmax) {
        // the attributes of shade_segment (rt_fast_body.h), same arithmetic
        const rtm::f3 pos = rtm::add(ro, rtm::muls(nd, h.best));
        rtm::f3 nrm;
        uint32_t mat;
        if (h.kind == 1) {
            const GeometrySphere& sp = q.spheres[h.id];
            nrm = rtm::divs(rtm::sub(pos, ld3(sp.position)), sp.radius);
            mat = (uint32_t)sp.material;
        } else {
            const GPUFace f = q.faces[h.id];
            const float bz = (1.0f - h.bx) - h.by;
            nrm = rtm::normalize(rtm::add(rtm::add(rtm::muls(ld3(q.vertices[f.v0].normal), h.bx),
                                                   rtm::muls(ld3(q.vertices[f.v1].normal), h.by)),
                                          rtm::muls(ld3(q.vertices[f.v2].normal), bz)));
            if (rtm::dot(nd, nrm) >= 0.0f) nrm = rtm::neg(nrm);
            mat = f.material;
        }
        out[0] = make_float4(h.best, __uint_as_float((uint32_t)h.kind), __uint_as_float(h.id), __uint_as_float(mat));
        out[1] = make_float4(nrm.x, nrm.y, nrm.z, h.bx);
        out[2] = make_float4(pos.x, pos.y, pos.z, h.by);
    } else {
        out[0] = make_float4(tmax, 0.0f, 0.0f, 0.0f);
        out[1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        out[2] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
}

// The LDS stack and scratch of render_fast_kernel (rt_fast_body.h), at 5 / 6 / 7 waves per SIMD.
#define RT_QUERY_KERNEL(NAME, W) \
    template <int STACK, int MODE> \
    __global__ __launch_bounds__(WAVE) __attribute__((amdgpu_waves_per_eu(W))) void NAME(QueryArgs q) { \
        constexpr int SL = STACK < RT_LDS_SL ? STACK : RT_LDS_SL; \
        __shared__ uint32_t stack_lds[(SL + rtfast::STACK_PAD_ROWS) * WAVE]; \
        __shared__ uint32_t scratch_lds[((MODE & rtfast::TREE_BIT) ? 64 : 0) + rtfast::DEFER_WORDS]; \
        uint32_t ovf[STACK > SL ? STACK - SL : 1]; \
        query_body<STACK, MODE>(q, rtfast::Stack<SL>{stack_lds, ovf}, scratch_lds); \
    }
RT_QUERY_KERNEL(query_kernel_w5, 5)
RT_QUERY_KERNEL(query_kernel_w6, 6)
RT_QUERY_KERNEL(query_kernel_w7, 7)
#undef RT_QUERY_KERNEL

template <int STACK, int MODE>
hipError_t launch_occ(int w, const QueryArgs& q, hipStream_t s) {
    const dim3 grid((unsigned)((q.count + WAVE - 1) / WAVE)), block(WAVE);
    if (w == 7) hipLaunchKernelGGL((query_kernel_w7<STACK, MODE>), grid, block, 0, s, q);
    else if (w == 6) hipLaunchKernelGGL((query_kernel_w6<STACK, MODE>), grid, block, 0, s, q);
    else hipLaunchKernelGGL((query_kernel_w5<STACK, MODE>), grid, block, 0, s, q);
    return hipGetLastError();
}

template <int STACK>
hipError_t dispatch(int mode, int w, const QueryArgs& q, hipStream_t s) {
    using namespace rtfast;
    switch (mode) {
        case MODE_PROD: return launch_occ<STACK, MODE_PROD>(w, q, s);
        case MODE_PROD | LEAN_BIT: return launch_occ<STACK, MODE_PROD | LEAN_BIT>(w, q, s);
        case MODE_PROD | TREE_BIT: return launch_occ<STACK, MODE_PROD | TREE_BIT>(w, q, s);
    }
    return hipErrorInvalidValue;
}

}  // namespace

hipError_t launch_query(int stack, int mode, int waves_per_simd, const QueryArgs& q, hipStream_t s) {
    if (q.count <= 0 || q.count > (1LL << 31)) return hipErrorInvalidValue;
    switch (stack) {
        case 30: return dispatch<30>(mode, waves_per_simd, q, s);
        case 40: return dispatch<40>(mode, waves_per_simd, q, s);
        default: return dispatch<64>(mode, waves_per_simd, q, s);
    }
}

}  // namespace rtk
