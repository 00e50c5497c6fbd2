// rt_query.hip -- the ray-query kernel behind rt_trace_rays (include/rt_abi.h): a second, thin body on the
// render kernel's traversal.  One ray per lane, wave w owning rays [64w, 64w + 64): the lane reads its ray (or
// forms the camera ray of its pixel centre), runs GetRayHit's sphere loop and rtfast::trace exactly as
// render_fast_body does (rt_fast_body.h), and writes one 48-byte hit record with the attributes shade_segment
// computes -- no RNG, no shading, no sky, no surface.  The kernel frame, the variants and the launch are the
// ray-batch scaffold's (rt_batch.h); rt_batch_calls.hip picks the variant (rt_trace_rays).
#include "rt_batch.h"

namespace rtk {
namespace {

template <int STACK, int MODE>
__device__ __forceinline__ void query_body(const QueryArgs& q, const rtfast::Stack<RT_BATCH_SL(STACK)>& stk,
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

RT_BATCH_KERNELS(query_kernel, QueryArgs, query_body)

}  // namespace

hipError_t launch_query(int stack, int mode, int waves_per_simd, const QueryArgs& q, hipStream_t s) {
    return launch_batch<query_kernel_set>(stack, mode, waves_per_simd, q.count, q, s);
}

}  // namespace rtk
