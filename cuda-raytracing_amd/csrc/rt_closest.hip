// rt_closest.hip -- the kernel behind rt_closest_point (include/rt_abi.h): "which point of the scene's surface is
// nearest to p, within radius?".  One point per lane, wave w owning points [64w, 64w + 64) as the ray-batch units
// (rt_batch.h); the point is one 16-byte load, the record two 16-byte stores; lanes past `count` leave at once and
// nothing here is wave-cooperative.  The answer is defined without a traversal -- the (d2, kind, id) minimum of
// closest.h over every sphere and face within radius -- and the kernel computes it exactly: the sphere loop in order,
// then the private node mirror (mirror.h nodes: one sibling pair = one 64-byte line) nearer child first, skipping a
// subtree only where closest.h box_bound PROVES every face under it farther than the best so far.  The other child's
// slot goes onto the lane's stack and is tested again when popped, against the best as it is then (no bound is kept
// in the entry).  Leaves read the mirror's contiguous 48-byte `tris` records, which hold (v0, e1, e2, face) -- no
// vertex is gathered; a leaf with a leaf tree (mirror.h pf == 2) walks the tree in pre-order by its skip links,
// culling on the nodes' outward-rounded boxes with the same bound, and reads the field-major `ltris`.
//
// Where the bound's premises fail -- the point outside +-2^60 or not finite, or a scene whose node bounds leave the
// mirror's `fast` range -- the lane walks everything and culls nothing: the same answer, slowly.  A NaN radius accepts
// nothing (d2 <= NaN is false), so such a lane skips the walk.
//
// The kernels are a walk unit's (rt_batch.h RT_WALK_KERNELS, no build integer of their own).  The stack is
// rtfast::Stack (16 entries in LDS, deeper ones private), its 30 / 40 / 64 size chosen from the mirror's depth as for
// the ray kernels: near-first descent pushes one entry per level at most.  5 / 6 / 7 waves per SIMD as the other batch
// units (profiles/closest_resources.txt).
#include "rt_batch.h"
#include "closest.h"

namespace rtk {
namespace {

using rtc::Best;
using rtfast::ldo;

struct Walk {
    rtm::f3 p;
    bool cull;  // the gate: box_bound's premises hold for this lane
    Best best;
};

// > best.d2 only when the box is proven out of reach; -1 (never above) without the gate
__device__ __forceinline__ float node_bound(const Walk& w, float4 lo, float4 hi) {
    const float b = rtc::box_bound(w.p, rtm::mk(lo.x, lo.y, lo.z), rtm::mk(lo.w, hi.x, hi.y));
    return w.cull ? b : -1.0f;
}

// one triangle record: A = (v0.xyz, e1.x), B = (e1.yz, e2.xy), C = (e2.z, face, ..)
__device__ __forceinline__ void offer_record(Walk& w, float4 A, float4 B, float4 C) {
    const rtc::Candidate c = rtc::closest_on_triangle(w.p, rtm::mk(A.x, A.y, A.z), rtm::mk(A.w, B.x, B.y), rtm::mk(B.z, B.w, C.x));
    rtc::offer(w.best, c, 2u, __float_as_uint(C.y));
}

// Leaf [first, first + count) through its tree (leaftree.h: pre-order, `skip` = the node after the subtree).
__device__ __forceinline__ void tree_leaf(Walk& w, const float4* tree, const float4* ltris, uint32_t root) {
    const float4 KR = ldo(tree, 4 * root + 3);
    const uint32_t end = __float_as_uint(KR.y), ln = __float_as_uint(KR.x);  // ltris is field-major over ln records
    uint32_t k = root;
    while (k < end) {
        const float4 K0 = ldo(tree, 4 * k), K1 = ldo(tree, 4 * k + 1), K3 = ldo(tree, 4 * k + 3);
        const uint32_t skip = __float_as_uint(K3.y), begin = __float_as_uint(K3.z), n = __float_as_uint(K3.w) >> 8;
        const float b = rtc::box_bound(w.p, rtm::mk(K0.x, K0.y, K0.z), rtm::mk(K1.x, K1.y, K1.z));
        if (w.cull && b > w.best.d2) {
            k = skip;
        } else if (begin != 0xffffffffu) {
            for (uint32_t i = begin; i < begin + n; i++) offer_record(w, ldo(ltris, i), ldo(ltris, ln + i), ldo(ltris, 2 * ln + i));
            k = skip;
        } else {
            k++;
        }
    }
}

template <int STACK, int>
__device__ __forceinline__ void closest_body(const ClosestArgs& a, const rtfast::Stack<RT_BATCH_SL(STACK)>& stk) {
    using S = rtfast::Stack<RT_BATCH_SL(STACK)>;
    const long long i = (long long)blockIdx.x * WAVE + (long long)(threadIdx.x & 63u);
    if (i >= a.count) return;
    const float4 P = reinterpret_cast<const float4*>(a.points)[i];
    Walk w;
    w.p = rtm::mk(P.x, P.y, P.z);
    w.cull = a.s.scene_fast != 0 && rtc::point_in_cull_range(w.p);
    const float r2 = P.w * P.w;
    w.best = rtc::best_start(r2);
    if (r2 == r2) {
        for (int k = 0; k < a.s.sphere_count; k++) {
            const GeometrySphere& sp = a.s.spheres[k];
            rtc::offer(w.best, rtc::closest_on_sphere(w.p, ld3(sp.position), sp.radius), 1u, (uint32_t)k);
        }
        const float4* const nodes4 = reinterpret_cast<const float4*>(a.s.nodes);
        const float4* const tris = reinterpret_cast<const float4*>(a.s.tris);
        int sp = S::empty((int)(threadIdx.x & 63u));
        const float4 rlo = ldo(nodes4, 0), rhi = ldo(nodes4, 1);
        uint32_t first = __float_as_uint(rhi.z), count = __float_as_uint(rhi.w);
        bool go = !(node_bound(w, rlo, rhi) > w.best.d2);
        while (go) {
            bool step = false;  // whether (first, count) names the next node
            if (count > 0) {
                bool walked = false;
                if (count > (uint32_t)rtfast::BIG && a.s.tree) {  // a big leaf's lead record says whether it has a tree
                    const float4 lead = ldo(tris, 3 * first + 2);
                    if (__float_as_uint(lead.w) == 2u) {
                        tree_leaf(w, a.s.tree, a.s.ltris, __float_as_uint(lead.z));
                        walked = true;
                    }
                }
                if (!walked)
                    for (uint32_t t = first; t < first + count; t++) offer_record(w, ldo(tris, 3 * t), ldo(tris, 3 * t + 1), ldo(tris, 3 * t + 2));
            } else {
                const float4 l0 = ldo(nodes4, 2 * first), l1 = ldo(nodes4, 2 * first + 1);
                const float4 r0 = ldo(nodes4, 2 * first + 2), r1 = ldo(nodes4, 2 * first + 3);
                const float bl = node_bound(w, l0, l1), br = node_bound(w, r0, r1);
                const bool tl = !(bl > w.best.d2), tr = !(br > w.best.d2);
                if (tl || tr) {
                    const bool left = tl && (!tr || bl <= br);  // the nearer child first
                    if (tl && tr) {
                        stk.put(sp, left ? first + 1 : first);
                        sp += S::STEP;
                    }
                    const float4 n1 = left ? l1 : r1;
                    first = __float_as_uint(n1.z), count = __float_as_uint(n1.w);
                    step = true;
                }
            }
            while (!step && sp >= S::STEP) {  // pop: the entry's own box against the best as it is now
                sp -= S::STEP;
                const uint32_t idx = stk.get(sp);
                const float4 lo = ldo(nodes4, 2 * idx), hi = ldo(nodes4, 2 * idx + 1);
                if (!(node_bound(w, lo, hi) > w.best.d2)) {
                    first = __float_as_uint(hi.z), count = __float_as_uint(hi.w);
                    step = true;
                }
            }
            go = step;
        }
    }
    // the record: a miss is (radius as passed, 0 ...), so buffers compare bytewise
    const Best& b = w.best;
    float4 o0 = make_float4(P.w, 0.0f, 0.0f, 0.0f), o1 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (b.kind != 0u) {
        const uint32_t material = b.kind == 1u ? (uint32_t)a.s.spheres[b.id].material : a.s.faces[b.id].material;
        o0 = make_float4(sqrtf(b.d2), __uint_as_float(b.kind), __uint_as_float(b.id), __uint_as_float(material));
        o1 = make_float4(b.q.x, b.q.y, b.q.z, __uint_as_float(b.region));
    }
    float4* const out = reinterpret_cast<float4*>(a.nearest + i);
    out[0] = o0;
    out[1] = o1;
}

RT_WALK_KERNELS(closest_kernel, ClosestArgs, closest_body)

}  // namespace

hipError_t launch_closest(int stack, int waves_per_simd, const ClosestArgs& a, hipStream_t s) {
    return launch_walk<closest_kernel_set, 0>(stack, waves_per_simd, a.count, a, s);
}

}  // namespace rtk
