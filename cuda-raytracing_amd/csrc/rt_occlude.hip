// rt_occlude.hip -- the any-hit kernels behind rt_occluded and rt_ao (include/rt_abi.h): "does this ray hit
// anything before tmax?".  One ray per lane, wave w owning rays [64w, 64w + 64), as the query kernel
// (rt_query.hip): the lane reads its ray, runs GetRayHit's sphere loop in order and to the end, and calls
// rtfast::trace<.., ANY>, in which a lane inside any_gate (rt_fast.h) stops at its first accept and every other
// lane runs the closest-hit traversal.  The answer of both is one predicate, `kind != 0 && best < tmax` -- the
// query kernel's own test for writing a hit record -- so byte i is (kind != 0) of rt_trace_rays' record i for
// every input.  The AO kernel runs the same predicate over `samples` rays per pixel, formed from the pixel's
// first-hit record by the fixed arithmetic rt_abi.h spells out.  The kernel frame, the variants and the launch
// are the ray-batch scaffold's (rt_batch.h), as the query kernel's.
#include "rt_batch.h"

namespace rtk {
namespace {

// Whether ray (ro, rd, tmax) is occluded: what rt_trace_rays reports as kind != 0.  Every lane of the wave
// calls it (`live` false: no ray on this lane; trace's big-leaf rounds are wave-cooperative).
template <int STACK, int MODE>
__device__ __forceinline__ bool occluded(const QueryArgs& q, const rtfast::Stack<RT_BATCH_SL(STACK)>& stk,
                                         uint32_t* const scratch, rtm::f3 ro, rtm::f3 rd, float tmax, bool live) {
    // GetRayHit's sphere loop as in query_body
    rtfast::Hit h;
    h.best = tmax, h.kind = 0, h.id = 0, h.bx = h.by = 0.0f;
    const rtm::f3 nd = rtm::normalize(rd);
    if (live) h = sphere_loop(q, ro, nd, h);
    rtfast::Ray R = rtfast::make_ray(ro, rd, nd, q.scene_fast != 0);
    // a sphere's hit below tmax inside the gate is final: the traversal could only replace it by a closer one.
    // (A sphere's hit that is not below tmax -- tmax NaN -- traverses as a closest-hit lane: trace stops only
    // lanes that enter without a hit.)
    const bool by_sphere = live && h.kind != 0 && h.best < tmax && rtfast::any_gate(reinterpret_cast<const float4*>(q.nodes), R, tmax);
    Counters c;
    rtfast::trace<false, MODE, false, true>(reinterpret_cast<const float4*>(q.nodes), reinterpret_cast<const float4*>(q.tris),
                                            q.pairs, q.tree, q.ltris, q.flat, q.spairs, 0u, stk, scratch, R, h,
                                            live && !by_sphere, c, q.quads, q.units, q.face_leaf);
    // `result.distance < max_distance` (main_raytracing.cu:108): a NaN distance, or tmax, is a miss
    return live && h.kind != 0 && h.best < tmax;
}

template <int STACK, int MODE>
__device__ __forceinline__ void occlusion_body(const OcclusionArgs& a,
                                               const rtfast::Stack<RT_BATCH_SL(STACK)>& stk,
                                               uint32_t* const scratch) {
    const long long i = (long long)blockIdx.x * WAVE + (long long)(threadIdx.x & 63u);
    const bool live = i < a.q.count;
    rtm::f3 ro = rtm::mk(0, 0, 0), rd = rtm::mk(0, 0, 1);
    float tmax = 0.0f;
    if (live) {  // the record as two 16-byte loads (adjacent lanes, adjacent records)
        const float4* const r = reinterpret_cast<const float4*>(a.q.rays + i);
        const float4 u = r[0], v = r[1];
        ro = rtm::mk(u.x, u.y, u.z), tmax = u.w, rd = rtm::mk(v.x, v.y, v.z);
    }
    const bool occ = occluded<STACK, MODE>(a.q, stk, scratch, ro, rd, tmax, live);
    if (live) a.occluded[i] = occ ? 1 : 0;  // the lane's own byte: adjacent lanes, adjacent bytes
}

// rt_ao (rt_abi.h spells the arithmetic out): pixel i on lane i, its samples one after the other.
template <int STACK, int MODE>
__device__ __forceinline__ void ao_body(const AoArgs& a, const rtfast::Stack<RT_BATCH_SL(STACK)>& stk,
                                        uint32_t* const scratch) {
    const long long i = (long long)blockIdx.x * WAVE + (long long)(threadIdx.x & 63u);
    const bool inside = i < a.q.count;
    bool valid = false;
    rtm::f3 n = rtm::mk(0, 0, 1), o = rtm::mk(0, 0, 0);
    if (inside) {
        const float4* const rec = reinterpret_cast<const float4*>(a.q.hits + i);
        const float4 r0 = rec[0], r1 = rec[1], r2 = rec[2];
        valid = __float_as_uint(r0.y) != 0u;
        if (valid) {
            n = rtm::mk(r1.x, r1.y, r1.z);
            const float e = a.bias * r0.x;
            o = rtm::add(rtm::mk(r2.x, r2.y, r2.z), rtm::muls(n, e));
        }
    }
    int occ = 0;
    for (int k = 0; k < a.samples; k++) {  // uniform trip count: every lane calls the traversal
        const uint32_t j = (((uint32_t)i * 0x9E3779B1u + (uint32_t)k * 0x85EBCA6Bu) >> 8) % (uint32_t)a.direction_count;
        rtm::f3 d = n;
        if (valid) {
            const float4 s = a.directions[j];
            const rtm::f3 d0 = rtm::add(n, rtm::mk(s.x, s.y, s.z));
            const float dd = (d0.x * d0.x + d0.y * d0.y) + d0.z * d0.z;
            if (dd > 1e-6f) d = rtm::normalize(d0);
        }
        occ += occluded<STACK, MODE>(a.q, stk, scratch, o, d, a.radius, valid) ? 1 : 0;
    }
    if (inside) a.ao[i] = valid ? (float)(a.samples - occ) / (float)a.samples : 1.0f;
}

RT_BATCH_KERNELS(occlusion_kernel, OcclusionArgs, occlusion_body)
RT_BATCH_KERNELS(ao_kernel, AoArgs, ao_body)

}  // namespace

hipError_t launch_occlusion(int stack, int mode, int waves_per_simd, const OcclusionArgs& a, hipStream_t s) {
    return launch_batch<occlusion_kernel_set>(stack, mode, waves_per_simd, a.q.count, a, s);
}
hipError_t launch_ao(int stack, int mode, int waves_per_simd, const AoArgs& a, hipStream_t s) {
    return launch_batch<ao_kernel_set>(stack, mode, waves_per_simd, a.q.count, a, s);
}

}  // namespace rtk
