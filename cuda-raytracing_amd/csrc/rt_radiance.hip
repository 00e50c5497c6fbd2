// rt_radiance.hip -- the kernel behind rt_radiance (include/rt_abi.h): the reference's ray_color along the caller's
// rays.  One ray per lane, wave w owning rays [64w, 64w + 64), as the query kernel (rt_query.hip); each lane runs
// render_fast_body's sample state machine (rt_fast_body.h) with the pixel replaced by a ray -- start sample k along
// the ray, GetRayHit's sphere loop, rtfast::trace, shade_segment, end the path on a miss / Russian roulette / the
// bounce limit, start the next sample -- so a lane idles only once all its `samples` are done.  Lanes past `count`
// and lanes that are done keep calling trace with live = false: its big-leaf rounds are wave-cooperative.
// shade_segment is the renderer's own, on the RenderArgs the argument struct begins with (rt_render.h RadianceArgs),
// so a ray that is a jittered camera ray gets the renderer's sample bit for bit.  The kernel frame, the variants and
// the launch are the ray-batch scaffold's (rt_batch.h), as the query kernel's.
#include "rt_fast_body.h"
#include "rt_batch.h"

namespace rtk {
namespace {

// A field of the RadianceArgs behind its RenderArgs, read as arg() reads the RenderArgs' own (rt_fast_body.h).
template <bool COLD, class T>
__device__ __forceinline__ T xarg(const RadianceArgs& a, T RadianceArgs::*m) {
    typedef const volatile __attribute__((address_space(4))) RadianceArgs* KernelArgs;
    if constexpr (COLD) return ((KernelArgs)__builtin_amdgcn_kernarg_segment_ptr())->*m;
    else return a.*m;
}

__device__ __forceinline__ bool is_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

template <int STACK, int MODE>
__device__ __forceinline__ void radiance_body(const RadianceArgs& a, const rtfast::Stack<RT_BATCH_SL(STACK)>& stk,
                                              uint32_t* const scratch) {
    constexpr bool COLD = (MODE & rtfast::LEAN_BIT) != 0;  // as render_fast_body: the lean variants read cold fields in place
    auto A = [&](auto member) { return arg<COLD>(a.r, member); };
    auto X = [&](auto member) { return xarg<COLD>(a, member); };
    // Path state is kept as small as the render body's: the 32-bit ray index (count <= 2^31), from which the ray, the
    // state and the output row are addressed again where they are needed
    const uint32_t i = blockIdx.x * (uint32_t)WAVE + (threadIdx.x & 63u);
    auto ray = [&](rtm::f3& o, rtm::f3& d) {  // two 16-byte loads (adjacent lanes, adjacent records); tmax is not used
        const float4* const r = reinterpret_cast<const float4*>(X(&RadianceArgs::rays) + i);
        const float4 u = r[0], v = r[1];
        o = rtm::mk(u.x, u.y, u.z), d = rtm::mk(v.x, v.y, v.z);
    };
    bool ready = (long long)i < a.count;  // samples left to start
    rtm::Xorwow rng{0, 0, 0, 0, 0, 0};
    rtm::f3 ro = rtm::mk(0, 0, 0), rd = rtm::mk(0, 0, 1);
    if (ready) {
        ray(ro, rd);
        const rtm::f3 n0 = rtm::normalize(rd);
        // nothing to trace: an empty bounce loop, or a direction normalize() cannot make a ray of (zero, infinite,
        // NaN) -- decided here, before any access that depends on the direction; the state is not touched
        if (a.r.bounces == 0 || !(is_finite(n0.x) && is_finite(n0.y) && is_finite(n0.z))) {
            X(&RadianceArgs::radiance)[i] = make_float4(0.0f, 0.0f, 0.0f, 1.0f);
            ready = false;
        } else {
            const rt_rng_state* const rs = X(&RadianceArgs::rng) + i;
            rng = rtm::Xorwow{rs->d, rs->v[0], rs->v[1], rs->v[2], rs->v[3], rs->v[4]};
        }
    }
    Counters c;
    float acc_r = 0.0f, acc_g = 0.0f, acc_b = 0.0f;
    int sample = 0, bounce = 0;
    bool path = false;
    rtm::f3 color = rtm::mk(0, 0, 0), thr = rtm::mk(1, 1, 1);
    for (;;) {
        if (ready && !path) {
            if (sample < X(&RadianceArgs::samples)) {
                ray(ro, rd);  // read again, not carried across the traversal
                color = rtm::mk(0, 0, 0);
                thr = rtm::mk(1, 1, 1);
                bounce = 0;
                path = true;
            } else {
                ready = false;
                const float fs = (float)X(&RadianceArgs::samples);  // the renderer's acc / spp
                X(&RadianceArgs::radiance)[i] = make_float4(acc_r / fs, acc_g / fs, acc_b / fs, 1.0f);
                rt_rng_state* const rs = X(&RadianceArgs::rng) + i;
                rs->d = rng.d;
                rs->v[0] = rng.v0;
                rs->v[1] = rng.v1;
                rs->v[2] = rng.v2;
                rs->v[3] = rng.v3;
                rs->v[4] = rng.v4;
            }
        }
        if (!__ballot(path)) break;

        // GetRayHit (main_raytracing.cu:83-109), every segment bounded by the renderer's 1e30
        rtfast::Hit h;
        h.best = 1e30f, h.kind = 0, h.id = 0, h.bx = h.by = 0.0f;
        const rtm::f3 nd = rtm::normalize(rd);
        if (path) {
            const int sphere_count = A(&RenderArgs::sphere_count);
            const GeometrySphere* const spheres = A(&RenderArgs::spheres);
            for (int k = 0; k < sphere_count; k++) {
                const GeometrySphere& sp = spheres[k];
                float dist;
                if (rtd::intersect_sphere(ro, nd, ld3(sp.position), sp.radius * sp.radius, &dist)) {
                    if (dist >= h.best) continue;
                    h.best = dist;
                    h.kind = 1;
                    h.id = (uint32_t)k;
                }
            }
        }
        rtfast::Ray R = rtfast::make_ray(ro, rd, nd, A(&RenderArgs::scene_fast) != 0);
        // `tune` is the argument (always 0 here), as in render_fast_body, not a literal 0: with the literal the MODE 21
        // build issued 16 % more vector and 83 % more LDS instructions on the same paths
        rtfast::trace<false, MODE>(reinterpret_cast<const float4*>(a.r.nodes), reinterpret_cast<const float4*>(a.r.tris),
                                   a.r.pairs, a.r.tree, a.r.ltris, a.r.flat, a.r.spairs, a.r.tune, stk, scratch, R, h, path, c,
                                   a.r.quads, a.r.units, a.r.face_leaf);
        if (!path) continue;

        bool end = shade_segment<false, COLD>(a.r, h, ro, rd, nd, rng, color, thr, c);
        if (++bounce >= A(&RenderArgs::bounces)) end = true;
        if (end) {
            acc_r += color.x;
            acc_g += color.y;
            acc_b += color.z;
            sample++;
            path = false;
        }
    }
}

RT_BATCH_KERNELS(radiance_kernel, RadianceArgs, radiance_body)

}  // namespace

hipError_t launch_radiance(int stack, int mode, int waves_per_simd, const RadianceArgs& a, hipStream_t s) {
    if (a.samples < 1 || a.r.bounces < 0) return hipErrorInvalidValue;
    return launch_batch<radiance_kernel_set>(stack, mode, waves_per_simd, a.count, a, s);
}

}  // namespace rtk
