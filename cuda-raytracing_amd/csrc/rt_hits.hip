// rt_hits.hip -- the kernel behind rt_trace_hits (include/rt_abi.h): "what does this ray go through, in order?".
// GetRayHit / BVHRayHit (main_raytracing.cu:33-109) with the single closest distance replaced by a list of the K
// smallest accepted distances (hit_list.h), whose bound() -- the K-th once K are held, tmax before, tmax throughout
// under RT_HITS_COUNT_ALL -- stands wherever the reference reads `closest`.
//
// One ray per lane, wave w owning rays [64w, 64w + 64) as the ray-batch units (rt_batch.h); lanes past `count` leave at
// once and nothing here is wave-cooperative, so the kernels are a walk unit's (rt_batch.h RT_WALK_KERNELS, their build
// integer the list's capacity).  The walk is rt_fast.h's own pieces on the mirror's private nodes: make_ray, the root as
// trav_begin tests it, inner_step and pop with `best` = the list's bound at that moment -- so every node decision is
// the reference's, the IEEE quotients outside the filtered range included.  Leaves of every size read the contiguous
// 48-byte `tris` records with the branch-free predicate (tri_eval, tri_ok); only an accepted triangle pays the
// division.  A leaf with a leaf tree (mirror.h pf == 2) is walked through `tree` / `ltris` in pre-order by its skip
// links, culling with cluster_cull against the bound, which drops as the walk fills the list.
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

struct Walk {
    rtfast::Ray R;
    uint32_t cull;  // RT_HITS_CULL_BACK / RT_HITS_CULL_FRONT, or 0
    bool all;       // RT_HITS_COUNT_ALL
};

// Record `idx` (its three float4 given) offered when glm's test hits and the winding passes; leaf_end as hit_list.h.
template <int CAP>
__device__ __forceinline__ void offer_record(const Walk& w, rth::List<CAP>& L, float4 A, float4 B, float4 Cc, uint32_t idx,
                                             uint32_t leaf_end) {
    const rtfast::TriEval E = rtfast::tri_eval(w.R.o, w.R.nd, A, B, Cc);
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

template <int STACK, int CAP>
__device__ __forceinline__ void hits_body(const HitsArgs& a, const rtfast::Stack<RT_BATCH_SL(STACK)>& stk) {
    using S = rtfast::Stack<RT_BATCH_SL(STACK)>;
    const long long i = (long long)blockIdx.x * WAVE + (long long)(threadIdx.x & 63u);
    if (i >= a.count) return;
    f3 ro, rd;
    float tmax;
    query_ray(a, i, ro, rd, tmax);
    const f3 nd = rtm::normalize(rd);
    Walk w;
    w.R = rtfast::make_ray(ro, rd, nd, a.s.scene_fast != 0);
    w.cull = a.flags & (RT_HITS_CULL_BACK | RT_HITS_CULL_FRONT);
    w.all = (a.flags & RT_HITS_COUNT_ALL) != 0;
    const int K = a.max_hits;
    rth::List<CAP> L;
    rth::init(L, K, tmax);

    // GetRayHit's sphere loop (main_raytracing.cu:87-101): one distance per sphere, never culled
    for (int k = 0; k < a.s.sphere_count; k++) {
        const GeometrySphere& sp = a.s.spheres[k];
        float dist;
        if (rtd::intersect_sphere(ro, nd, ld3(sp.position), sp.radius * sp.radius, &dist)) rth::offer(L, w.all, dist, rth::SPHERE | (uint32_t)k);
    }

    // BVHRayHit: the root as trav_begin tests it, then inner_step / pop against the list's bound
    const float4* const nodes4 = reinterpret_cast<const float4*>(a.s.nodes);
    const float4* const tris = reinterpret_cast<const float4*>(a.s.tris);
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
            if (count > (uint32_t)rtfast::BIG && a.s.tree) {  // a big leaf's lead record says whether it has a tree
                const float4 lead = ldo(tris, 3 * first + 2);
                if (__float_as_uint(lead.w) == 2u) {
                    tree_leaf(w, L, a.s.tree, a.s.ltris, __float_as_uint(lead.z), first, count);
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
    // entry becomes the record rt_trace_rays writes for that primitive and t (rt_batch.h store_hit); every other row
    // is its miss record.
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
            store_miss(row, tmax);
            continue;
        }
        held++;
        if (p & rth::SPHERE) {
            store_hit(row, ro, nd, t, 1u, p & ~rth::SPHERE, 0.0f, 0.0f, a.s.spheres, a.s.faces, a.s.vertices);
        } else {  // the test on the record again: the same operations give the same bits
            const float4 Cc = ldo(tris, 3 * p + 2);
            const rtfast::TriEval E = rtfast::tri_eval(w.R.o, w.R.nd, ldo(tris, 3 * p), ldo(tris, 3 * p + 1), Cc);
            const float inv_det = 1.0f / E.det;
            store_hit(row, ro, nd, t, 2u, __float_as_uint(Cc.y), E.u * inv_det, E.v * inv_det, a.s.spheres, a.s.faces, a.s.vertices);
        }
    }
    if (a.counts) a.counts[i] = w.all ? L.total : held;
}

RT_WALK_KERNELS(hits_kernel, HitsArgs, hits_body)

}  // namespace

// The list capacity that holds max_hits, then launch_walk's choices.
hipError_t launch_hits(int stack, int waves_per_simd, const HitsArgs& a, hipStream_t s) {
    if (a.max_hits < 1 || a.max_hits > rth::MAX_HITS) return hipErrorInvalidValue;
    return a.max_hits <= 4   ? launch_walk<hits_kernel_set, 4>(stack, waves_per_simd, a.count, a, s)
           : a.max_hits <= 8 ? launch_walk<hits_kernel_set, 8>(stack, waves_per_simd, a.count, a, s)
                             : launch_walk<hits_kernel_set, 16>(stack, waves_per_simd, a.count, a, s);
}

}  // namespace rtk
