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
    if (live) h = sphere_loop(q, ro, nd, h);
    rtfast::Ray R = rtfast::make_ray(ro, rd, nd, q.scene_fast != 0);
    Counters c;
    rtfast::trace<false, MODE>(reinterpret_cast<const float4*>(q.nodes), reinterpret_cast<const float4*>(q.tris), q.pairs,
                               q.tree, q.ltris, q.flat, q.spairs, 0u, stk, scratch, R, h, live, c, q.quads, q.units,
                               q.face_leaf);
    if (!live) return;

    // the record (rt_batch.h store_hit)
    query_ray(q, i, ro, rd, tmax);
    nd = rtm::normalize(rd);
    float4* const out = reinterpret_cast<float4*>(q.hits + i);
    // `result.distance < max_distance` (main_raytracing.cu:108): a NaN distance is a miss
    if (h.kind != 0 && h.best < tmax)
        store_hit(out, ro, nd, h.best, (uint32_t)h.kind, h.id, h.bx, h.by, q.spheres, q.faces, q.vertices);
    else
        store_miss(out, tmax);
}

RT_BATCH_KERNELS(query_kernel, QueryArgs, query_body)

}  // namespace

hipError_t launch_query(int stack, int mode, int waves_per_simd, const QueryArgs& q, hipStream_t s) {
    return launch_batch<query_kernel_set>(stack, mode, waves_per_simd, q.count, q, s);
}

}  // namespace rtk
