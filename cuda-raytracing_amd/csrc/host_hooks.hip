// host_hooks.hip -- device code's decisions evaluated on the host by the same source, for the tests: the twin test and
// the leaf-tree cull predicate of rt_fast.h, the hit list of hit_list.h, the variant chooser of rt_variant.h and the
// family table of rt_render.h.
#include <hip/hip_runtime.h>

#include "rt_abi.h"
#include "rt_device.h"
#include "rt_math.h"
#include "rt_common.h"
#include "leaftree.h"
#include "rt_fast.h"
#include "mirror.h"
#include "rt_render.h"
#include "hit_list.h"

static_assert(RT_HITS_MAX == rth::MAX_HITS, "hit_list.h holds at most RT_HITS_MAX entries");
static_assert(MIRROR_BIG_LEAF == (uint32_t)rtfast::BIG, "pair records exist for exactly the big leaves");

// 1 when librt_hip_exp.so's render paths are registered (rt_render.h ExperimentalKernels).
extern "C" int rt_experimental_loaded() { return rtk::experimental_kernels() ? 1 : 0; }

// The twin test (rt_fast.h twin_rejected) on the host, for tests/test_scene.py: triangle record `rec`
// (mirror.h tris) and its twin (v0, e2, e1) under glm's test (test_triangle's operation order) for the
// ray (o, nd); bit 0: twin_rejected, bit 1: the twin passes glm's predicate, bit 2: A passes it.
// With `bounds` = (KD, KE, DN) the hoisted form decides instead (twin_rejected_pre on those bounds, as the
// kernels call it), and bit 3 says that the packed evaluation of the shared-leaf loop (quad_test's sequence on
// an f2 holding this triangle in either half) and the scalar one disagree.
static int twin_check(const float rec[12], const float o[3], const float nd[3], const float* bounds) {
    using rtm::f3;
    using namespace rtfast;
    const f3 O = rtm::mk(o[0], o[1], o[2]), N = rtm::mk(nd[0], nd[1], nd[2]), v0 = rtm::mk(rec[0], rec[1], rec[2]);
    const f3 e1 = rtm::mk(rec[3], rec[4], rec[5]), e2 = rtm::mk(rec[6], rec[7], rec[8]);
    auto glm = [&](f3 a, f3 b, float* det, float* u, float* v, float* uv) {  // (e1, e2) = (a, b)
        const f3 p = rtm::cross(N, b);
        *det = rtm::dot(a, p);
        const f3 dist = rtm::sub(O, v0);
        *u = rtm::dot(dist, p);
        *v = rtm::dot(N, rtm::cross(dist, a));
        *uv = *u + *v;
    };
    auto ok = [](float det, float u, float v, float uv) {
        const bool neg = signbit(det);
        const float ad = fabsf(det), su = neg ? -u : u, sv = neg ? -v : v, suv = neg ? -uv : uv;
        return ad > 1.1920928955078125e-07f && !(su < 0.0f || su > ad) && !(sv < 0.0f || suv > ad);
    };
    float d, u, v, uv, d2, u2, v2, uv2;
    glm(e1, e2, &d, &u, &v, &uv);
    glm(e2, e1, &d2, &u2, &v2, &uv2);
    const int glm_bits = (ok(d2, u2, v2, uv2) ? 2 : 0) | (ok(d, u, v, uv) ? 4 : 0);
    if (!bounds) {
        const f3 dist = rtm::sub(O, v0);
        const float dn = (fabsf(dist.x) + fabsf(dist.y)) + fabsf(dist.z);
        float kd, ke;
        rt_twin_bounds(rec, &kd, &ke);
        return (twin_rejected(d, u, v, uv, dn, kd, ke) ? 1 : 0) | glm_bits;
    }
    const float dn = bounds[2], m = bounds[1] * dn + 0x1p-90f, m2 = 2.001f * m;
    const float kdd = bounds[0] + 0x1p-90f, kdd1 = kdd * (1.0f + 0x1p-20f);
    const bool scalar = twin_rejected_pre(d, u, v, uv, dn, m, m2, kdd, kdd1);
    // quad_test's sequence, this triangle beside a degenerate one in the other half
    bool same = true;
    for (int half = 0; half < 2; half++) {
        auto two = [&](float x) { return half ? f2{0.0f, x} : f2{x, 0.0f}; };
        const f2 D = two(d);
        const TwinFold<f2> F = twin_fold<f2>(D, two(u), two(v), two(uv), f2{copysignf(1.0f, D.x), copysignf(1.0f, D.y)});
        const TwinLimits<f2> L = twin_limits<f2>(F.ad, F.suv, m, m2, kdd);
        const bool packed = half ? twin_decide(F.ad.y, F.su.y, F.sv.y, dn, m, kdd1, L.top.y, L.lim_v.y, L.lim_uv.y, L.suv_lo.y)
                                 : twin_decide(F.ad.x, F.su.x, F.sv.x, dn, m, kdd1, L.top.x, L.lim_v.x, L.lim_uv.x, L.suv_lo.x);
        same = same && packed == scalar;
        const bool okp = half ? tri_ok_folded(F.ad.y, F.su.y, F.sv.y, F.suv.y) : tri_ok_folded(F.ad.x, F.su.x, F.sv.x, F.suv.x);
        same = same && okp == ok(d, u, v, uv);
    }
    return (scalar ? 1 : 0) | glm_bits | (same ? 0 : 8);
}
extern "C" int rt_twin_check_host(const float rec[12], const float o[3], const float nd[3]) {
    return twin_check(rec, o, nd, nullptr);
}
extern "C" int rt_twin_check_bounds_host(const float rec[12], const float o[3], const float nd[3], const float bounds[3]) {
    return twin_check(rec, o, nd, bounds);
}
// twin_visit (rt_fast.h) on the host: out = (DN, M, M2).
extern "C" void rt_twin_visit_host(const float o[3], const float lo[3], const float hi[3], float ke, float out[3]) {
    const rtfast::TwinVisit V = rtfast::twin_visit(rtm::mk(o[0], o[1], o[2]), rtm::mk(lo[0], lo[1], lo[2]), rtm::mk(hi[0], hi[1], hi[2]), ke);
    out[0] = V.dn, out[1] = V.m, out[2] = V.m2;
}

// choose_variant (rt_variant.h) for tests/test_variant_cpu.py: in = {tune, stats, lane_cost, refill, has_tree, screens,
// arrays_complete, depth, want_entry}, out = {family, mode, stack, needs_plugin, use_entry}.
extern "C" void rt_variant_host(const int32_t in[9], int32_t out[5]) {
    const rtk::VariantInput vi{(uint32_t)in[0], in[1] != 0, in[2] != 0, in[3] != 0, in[4] != 0,
                               in[5] != 0, in[6] != 0, in[7], in[8] != 0};
    const rtk::Variant v = rtk::choose_variant(vi);
    out[0] = v.family, out[1] = v.mode, out[2] = v.stack, out[3] = v.needs_plugin, out[4] = v.use_entry;
}

// Whether the unit of `family` instantiates `mode`, from the rows its launcher is built from (rt_render.h).
template <int... MODES>
static bool one_of(int mode) { return ((mode == MODES) || ...); }
extern "C" int rt_family_has_mode_host(int family, int mode) {
    switch (family) {
#define RT_FAMILY_CASE(FAM, NAME, STATS, ...) case rtk::FAM: return one_of<__VA_ARGS__>(mode);
        RT_FAST_FAMILIES(RT_FAMILY_CASE)
#undef RT_FAMILY_CASE
    }
    return 0;
}

// rt_trace_hits' list (hit_list.h) on the host, for tests/test_hits_cpu.py: the offers in order, arrival breaking ties.
extern "C" int rt_hit_list_host(int max_hits, float tmax, int count_all, int64_t n, const float* t, const uint32_t* payload,
                                float* out_t, uint32_t* out_payload, int64_t* total) {
    if (max_hits < 1 || max_hits > rth::MAX_HITS || n < 0 || (n > 0 && (!t || !payload)) || !out_t || !out_payload) {
        rt_internal_set_error("rt_hit_list_host: max_hits outside 1..16, negative n or a null array");
        return -1;
    }
    rth::List<rth::MAX_HITS> L;
    rth::init(L, max_hits, tmax);
    for (int64_t j = 0; j < n; j++) rth::offer(L, count_all != 0, t[j], payload[j]);
    int held = 0;
    for (int s = rth::MAX_HITS - max_hits; s < rth::MAX_HITS; s++) {
        if (L.p[s] == rth::EMPTY) break;
        out_t[held] = L.t[s], out_payload[held] = L.p[s];
        held++;
    }
    if (total) *total = (int64_t)L.total;
    return held;
}

// The leaf-tree cull predicate of the render kernel (rt_fast.h cluster_cull), for tests/test_leaf_tree.py.
extern "C" int rt_cluster_cull_host(const float origin[3], const float nd[3], float best, const float node[16]) {
    rtfast::Ray R;
    R.o = rtm::mk(origin[0], origin[1], origin[2]);
    R.nd = rtm::mk(nd[0], nd[1], nd[2]);
    R.d = R.nd;
    R.r = rtm::mk(1.0f / nd[0], 1.0f / nd[1], 1.0f / nd[2]);
    R.fast = true;
    const float4 K0 = make_float4(node[0], node[1], node[2], node[3]);
    const float4 K1 = make_float4(node[4], node[5], node[6], node[7]);
    const float4 K2 = make_float4(node[8], node[9], node[10], node[11]);
    const float4 K3 = make_float4(node[12], node[13], node[14], node[15]);
    return rtfast::cluster_cull(R, R.r, best, K0, K1, K2, K3) ? 1 : 0;
}
