// rt_hits.hip -- the kernel behind rt_trace_hits (include/rt_abi.h): "what does this ray go through, in order?".
// GetRayHit / BVHRayHit (main_raytracing.cu:33-109) with the single closest distance replaced by a list of the K
// smallest accepted distances (hit_list.h), whose bound() -- the K-th once K are held, tmax before, tmax throughout
// under RT_HITS_COUNT_ALL -- stands wherever the reference reads `closest`.
//
// One ray per lane, wave w owning rays [64w, 64w + 64) as the ray-batch units (rt_batch.h); lanes past `count` leave at
// once and nothing here is wave-cooperative, so the frame is the stack's LDS rows alone (as rt_closest.hip: no
// RT_TRACE_FRAME, no MODE).  The walk is rt_fast.h's own pieces on the mirror's private nodes: make_ray, the root as
// trav_begin tests it, inner_step and pop with `best` = the list's bound at that moment -- so every node decision is
// the reference's, the IEEE quotients outside the filtered range included.  Leaves of every size read the contiguous
// 48-byte `tris` records with the branch-free predicate (tri_ok); only an accepted triangle pays the division.  A
// leaf with a leaf tree (mirror.h pf == 2) is walked through `tree` / `ltris` in pre-order by its skip links, culling
// with cluster_cull against the bound, which drops as the walk fills the list.
//
// Why order within a leaf is free.  After K offers the list holds the K smallest of everything offered so far under
// the order (t, arrival), and an offer that is refused would have been cut anyway -- so the list after a leaf depends
// on the SET of that leaf's accepted triangles and on their relative order among equal t only, not on when each was
// offered.  Entries of earlier leaves arrived earlier and win every tie; among one leaf's triangles arrival order is
// position in the leaf.  So a leaf walked out of order offers its candidates under (t, position in leaf) --
// hit_list.h's `leaf_end` -- and leaves exactly the list the sequential loop leaves, provided nothing it skips could
// have entered: cluster_cull excludes a node only when no triangle under it passes the fp32 test with 0 <= t <= best
// (its segment reaches Et past `best`, so a distance equal to the bound, which an earlier position could still win
// with, is not excluded), and the bound it is given is never below the final one of the leaf.  Under COUNT_ALL the
// bound is tmax and the total counts a set.  Between leaves the bound is the sequential one, so the nodes popped are
// the reference's.  A NaN distance is never offered (the one deliberate difference from the reference, rt_abi.h).
//
// The list is two words an entry -- t and a `tris` record index, or SPHERE | index -- in registers that only unrolled,
// statically indexed code touches.  What a record needs beyond that (bx, by, face, material, normal, position) is
// re-derived for the K survivors after the walk by running the test on their records again: the same operations in
// the same order give the same bits, and nothing of it is carried through the traversal.
//
// Builds: list capacity 4 / 8 / 16 (max_hits rounded up; a shorter list sits in the last slots), stack 30 / 40 / 64
// (rtfast::Stack: 16 entries in LDS, deeper ones private -- the only scratch), 5 / 6 / 7 waves per SIMD
// (profiles/hits_resources.txt).
#include "rt_batch.h"
#include "hit_list.h"

namespace rtk {
namespace {

using rtfast::ldo;
using rtm::f3;

// glm::intersectRayTriangle's quantities for one record (test_triangle's operation order).
struct TriEval {
    float det, u, v, uv;
    f3 e2, perp;
};
__device__ __forceinline__ TriEval tri_eval(const rtfast::Ray& R, float4 A, float4 B, float4 Cc) {
    TriEval E;
    const f3 e1 = rtm::mk(A.w, B.x, B.y);
    E.e2 = rtm::mk(B.z, B.w, Cc.x);
    const f3 p = rtm::cross(R.nd, E.e2);
    E.det = rtm::dot(e1, p);
    const f3 dist = rtm::sub(R.o, rtm::mk(A.x, A.y, A.z));
    E.u = rtm::dot(dist, p);
    E.perp = rtm::cross(dist, e1);
    E.v = rtm::dot(R.nd, E.perp);
    E.uv = E.u + E.v;
    return E;
}

struct Walk {
    rtfast::Ray R;
    uint32_t cull;  // RT_HITS_CULL_BACK / RT_HITS_CULL_FRONT, or 0
    bool all;       // RT_HITS_COUNT_ALL
};

// Record `idx` (its three float4 given) offered when glm's test hits and the winding passes; leaf_end as hit_list.h.
template <int CAP>
__device__ __forceinline__ void offer_record(const Walk& w, rth::List<CAP>& L, float4 A, float4 B, float4 Cc, uint32_t idx,
                                             uint32_t leaf_end) {
    const TriEval E = tri_eval(w.R, A, B, Cc);
    // |det| > eps for every triangle the test accepts: the sign is never in doubt
    const bool wound = w.cull == 0u || ((E.det > 0.0f) == (w.cull == RT_HITS_CULL_BACK));
    if (rtfast::tri_ok(E.det, E.u, E.v, E.uv) && wound) {
        const float inv_det = 1.0f / E.det;
        rth::offer(L, w.all, rtm::dot(E.e2, E.perp) * inv_det, idx, leaf_end);
    }
}

// Leaf [f0, f0 + c0) through its tree (leaftree.h: pre-order, `skip` = the node after the subtree; ltris field-major,
// C.z = the record's position in the leaf).
template <int CAP>
__device__ __forceinline__ void tree_leaf(const Walk& w, rth::List<CAP>& L, const float4* tree, const float4* ltris,
                                          uint32_t root, uint32_t f0, uint32_t c0) {
    const bool cull_ok = w.R.fast;
    const f3 rnd = cull_ok ? rtm::mk(1.0f / w.R.nd.x, 1.0f / w.R.nd.y, 1.0f / w.R.nd.z) : rtm::mk(0.0f, 0.0f, 0.0f);
    const float4 KR = ldo(tree, 4 * root + 3);
    const uint32_t end = __float_as_uint(KR.y), ln = __float_as_uint(KR.x);
    uint32_t k = root;
    while (k < end) {
        const float4 K3 = ldo(tree, 4 * k + 3);
        const uint32_t skip = __float_as_uint(K3.y), begin = __float_as_uint(K3.z), info = __float_as_uint(K3.w);
        if (cull_ok && (info & 1u) &&
            rtfast::cluster_cull(w.R, rnd, rth::bound(L, w.all), ldo(tree, 4 * k), ldo(tree, 4 * k + 1), ldo(tree, 4 * k + 2), K3)) {
            k = skip;
        } else if (begin != 0xffffffffu) {
            const uint32_t n = info >> 8;
            for (uint32_t i = begin; i < begin + n; i++) {
                const float4 Cc = ldo(ltris, 2 * ln + i);
                offer_record(w, L, ldo(ltris, i), ldo(ltris, ln + i), Cc, f0 + __float_as_uint(Cc.z), f0 + c0);
            }
            k = skip;
        } else {
            k++;
        }
    }
}

// One row of the output: three 16-byte stores.
__device__ __forceinline__ void store_row(float4* out, float4 a, float4 b, float4 c) {
    out[0] = a, out[1] = b, out[2] = c;
}

template <int CAP, int STACK>
__device__ __forceinline__ void hits_body(const HitsArgs& a, const rtfast::Stack<RT_BATCH_SL(STACK)>& stk) {
    using S = rtfast::Stack<RT_BATCH_SL(STACK)>;
    const long long i = (long long)blockIdx.x * WAVE + (long long)(threadIdx.x & 63u);
    if (i >= a.count) return;
    f3 ro, rd;
    float tmax;
    query_ray(a, i, ro, rd, tmax);
    const f3 nd = rtm::normalize(rd);
    Walk w;
    w.R = rtfast::make_ray(ro, rd, nd, a.scene_fast != 0);
    w.cull = a.flags & (RT_HITS_CULL_BACK | RT_HITS_CULL_FRONT);
    w.all = (a.flags & RT_HITS_COUNT_ALL) != 0;
    const int K = a.max_hits;
    rth::List<CAP> L;
    rth::init(L, K, tmax);

    // GetRayHit's sphere loop (main_raytracing.cu:87-101): one distance per sphere, never culled
    for (int k = 0; k < a.sphere_count; k++) {
        const GeometrySphere& sp = a.spheres[k];
        float dist;
        if (rtd::intersect_sphere(ro, nd, ld3(sp.position), sp.radius * sp.radius, &dist)) rth::offer(L, w.all, dist, rth::SPHERE | (uint32_t)k);
    }

    // BVHRayHit: the root as trav_begin tests it, then inner_step / pop against the list's bound
    const float4* const nodes4 = reinterpret_cast<const float4*>(a.nodes);
    const float4* const tris = reinterpret_cast<const float4*>(a.tris);
    int sp = S::empty((int)(threadIdx.x & 63u));
    uint32_t first, count;
    bool go;
    {
        const float4 lo = ldo(nodes4, 0), hi = ldo(nodes4, 1);
        float te, tx;
        rtfast::slab_exact(w.R, lo, hi, &te, &tx);
        first = __float_as_uint(hi.z), count = __float_as_uint(hi.w);
        go = tx >= te && te < rth::bound(L, w.all) && tx > 0.0f;
    }
    Counters c;  // inner_step's statistics argument (unused: STATS false)
    while (go) {
        bool step = false;
        if (count > 0) {
            bool walked = false;
            if (count > (uint32_t)rtfast::BIG && a.tree) {  // a big leaf's lead record says whether it has a tree
                const float4 lead = ldo(tris, 3 * first + 2);
                if (__float_as_uint(lead.w) == 2u) {
                    tree_leaf(w, L, a.tree, a.ltris, __float_as_uint(lead.z), first, count);
                    walked = true;
                }
            }
            if (!walked)  // leaf order is arrival order
                for (uint32_t t = first; t < first + count; t++) offer_record(w, L, ldo(tris, 3 * t), ldo(tris, 3 * t + 1), ldo(tris, 3 * t + 2), t, 0u);
        } else {
            step = rtfast::inner_step<false>(nodes4, stk, sp, w.R, rth::bound(L, w.all), first, count, c);
        }
        go = step || rtfast::pop(nodes4, stk, sp, w.R, rth::bound(L, w.all), first, count);
    }

    // The rows: the list's slots in turn (rotate: no runtime index), the first CAP - K of which hold no entry.  An
    // entry becomes the record rt_trace_rays writes for that primitive and t (rt_query.hip: same arithmetic, same
    // flip); every other row is its miss record.
    float4* const out = reinterpret_cast<float4*>(a.hits) + 3 * ((size_t)i * (size_t)K);
    uint32_t held = 0;
#pragma unroll 1
    for (int s = 0; s < CAP; s++) {
        float t;
        uint32_t p;
        rth::rotate(L, &t, &p);
        if (s < CAP - K) continue;
        float4* const row = out + 3 * (s - (CAP - K));
        if (p == rth::EMPTY) {
            store_row(row, make_float4(tmax, 0.0f, 0.0f, 0.0f), make_float4(0.0f, 0.0f, 0.0f, 0.0f), make_float4(0.0f, 0.0f, 0.0f, 0.0f));
            continue;
        }
        held++;
        const f3 pos = rtm::add(ro, rtm::muls(nd, t));
        if (p & rth::SPHERE) {
            const uint32_t id = p & ~rth::SPHERE;
            const GeometrySphere& sph = a.spheres[id];
            const f3 nrm = rtm::divs(rtm::sub(pos, ld3(sph.position)), sph.radius);
            store_row(row, make_float4(t, __uint_as_float(1u), __uint_as_float(id), __uint_as_float((uint32_t)sph.material)),
                      make_float4(nrm.x, nrm.y, nrm.z, 0.0f), make_float4(pos.x, pos.y, pos.z, 0.0f));
        } else {
            const float4 Cc = ldo(tris, 3 * p + 2);
            const TriEval E = tri_eval(w.R, ldo(tris, 3 * p), ldo(tris, 3 * p + 1), Cc);
            const float inv_det = 1.0f / E.det;
            const float bx = E.u * inv_det, by = E.v * inv_det;
            const uint32_t id = __float_as_uint(Cc.y);
            const GPUFace f = a.faces[id];
            const float bz = (1.0f - bx) - by;
            f3 nrm = rtm::normalize(rtm::add(rtm::add(rtm::muls(ld3(a.vertices[f.v0].normal), bx), rtm::muls(ld3(a.vertices[f.v1].normal), by)),
                                             rtm::muls(ld3(a.vertices[f.v2].normal), bz)));
            if (rtm::dot(nd, nrm) >= 0.0f) nrm = rtm::neg(nrm);
            store_row(row, make_float4(t, __uint_as_float(2u), __uint_as_float(id), __uint_as_float(f.material)),
                      make_float4(nrm.x, nrm.y, nrm.z, bx), make_float4(pos.x, pos.y, pos.z, by));
        }
    }
    if (a.counts) a.counts[i] = w.all ? L.total : held;
}

#define RT_HITS_KERNEL(W) \
    template <int CAP, int STACK> \
    __global__ __launch_bounds__(WAVE) __attribute__((amdgpu_waves_per_eu(W))) void hits_kernel_w##W(HitsArgs a) { \
        constexpr int SL = RT_BATCH_SL(STACK); \
        __shared__ uint32_t stack_lds[(SL + rtfast::STACK_PAD_ROWS) * WAVE]; \
        uint32_t ovf[STACK > SL ? STACK - SL : 1]; \
        hits_body<CAP, STACK>(a, rtfast::Stack<SL>{stack_lds, ovf}); \
    }
RT_HITS_KERNEL(5)
RT_HITS_KERNEL(6)
RT_HITS_KERNEL(7)
#undef RT_HITS_KERNEL

template <int CAP, int STACK>
auto hits_kernel(int w) -> void (*)(HitsArgs) {
    return w == 7 ? hits_kernel_w7<CAP, STACK> : w == 6 ? hits_kernel_w6<CAP, STACK> : hits_kernel_w5<CAP, STACK>;
}
template <int CAP>
auto hits_kernel(int stack, int w) -> void (*)(HitsArgs) {
    return stack == 30 ? hits_kernel<CAP, 30>(w) : stack == 40 ? hits_kernel<CAP, 40>(w) : hits_kernel<CAP, 64>(w);
}

}  // namespace

// One wave per 64 of a.count rays: the list capacity that holds max_hits, then the stack (rt_variant.h variant_stack),
// then the occupancy.
hipError_t launch_hits(int stack, int waves_per_simd, const HitsArgs& a, hipStream_t s) {
    if (a.count <= 0 || a.count > (1LL << 31) || a.max_hits < 1 || a.max_hits > rth::MAX_HITS) return hipErrorInvalidValue;
    void (*const k)(HitsArgs) = a.max_hits <= 4   ? hits_kernel<4>(stack, waves_per_simd)
                                : a.max_hits <= 8 ? hits_kernel<8>(stack, waves_per_simd)
                                                  : hits_kernel<16>(stack, waves_per_simd);
    hipLaunchKernelGGL(k, dim3((unsigned)((a.count + WAVE - 1) / WAVE)), dim3(WAVE), 0, s, a);
    return hipGetLastError();
}

}  // namespace rtk
