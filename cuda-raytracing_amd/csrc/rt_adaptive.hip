// rt_adaptive.hip -- the kernel behind rt_sample_pixels (include/rt_abi.h): more of the renderer's own samples for
// the pixels of a list.  One list entry per lane, wave w owning entries [64w, 64w + 64), as the radiance kernel
// (rt_radiance.hip); each lane runs render_fast_body's sample state machine (rt_fast_body.h) on its entry's pixel --
// start a camera sample from two jitter draws, GetRayHit's sphere loop, rtfast::trace, shade_segment, end the path on a
// miss / Russian roulette / the bounce limit, add the sample to the pixel's accumulator, start the next -- so a lane
// idles only once all its samples are done.  Lanes past `count`, lanes whose entry asks for nothing and lanes that are
// done keep calling trace with live = false: its big-leaf rounds are wave-cooperative.  No entry frontier: the lanes
// of a wave belong to any pixels.  shade_segment is the renderer's own, on the RenderArgs the argument struct begins
// with (rt_render.h SampleArgs).  The kernel frame, the variants and the launch are the ray-batch scaffold's
// (rt_batch.h).
#include "rt_fast_body.h"
#include "rt_batch.h"

namespace rtk {
namespace {

// A field of the SampleArgs behind its RenderArgs, read as arg() reads the RenderArgs' own (rt_fast_body.h).
template <bool COLD, class T>
__device__ __forceinline__ T sarg(const SampleArgs& a, T SampleArgs::*m) {
    typedef const volatile __attribute__((address_space(4))) SampleArgs* KernelArgs;
    if constexpr (COLD) return ((KernelArgs)__builtin_amdgcn_kernarg_segment_ptr())->*m;
    else return a.*m;
}

template <int STACK, int MODE>
__device__ __forceinline__ void sample_body(const SampleArgs& a, const rtfast::Stack<RT_BATCH_SL(STACK)>& stk,
                                            uint32_t* const scratch) {
    constexpr bool COLD = (MODE & rtfast::LEAN_BIT) != 0;  // as render_fast_body: the lean variants read cold fields in place
    auto A = [&](auto member) { return arg<COLD>(a.r, member); };
    auto X = [&](auto member) { return sarg<COLD>(a, member); };
    // Path state is kept as small as the radiance body's: the 32-bit pixel index (width * height <= 2^30) and the
    // samples left; x, y, the accumulator's, the moments' and the state's addresses are computed again where they are
    // used, and the accumulator lives in memory between samples (one 16-byte load and store per sample)
    const uint32_t i = blockIdx.x * (uint32_t)WAVE + (threadIdx.x & 63u);
    uint32_t p = 0, left = 0;
    rtm::Xorwow rng{0, 0, 0, 0, 0, 0};
    if ((long long)i < a.count) {
        const uint32_t n = X(&SampleArgs::samples)[i];  // a wave of zeros ends after this load
        if (n) {
            const int32_t* const pixels = X(&SampleArgs::pixels);
            const long long q = pixels ? (long long)pixels[i] : (long long)i;
            if (q >= 0 && q < (long long)a.r.width * a.r.height) {
                p = (uint32_t)q, left = n;
                const rt_rng_state* const rs = A(&RenderArgs::rng) + p;
                rng = rtm::Xorwow{rs->d, rs->v[0], rs->v[1], rs->v[2], rs->v[3], rs->v[4]};
            }
        }
    }
    Counters c;
    int bounce = 0;
    bool path = false;
    rtm::f3 ro = rtm::mk(0, 0, 0), rd = rtm::mk(0, 0, 1), color = rtm::mk(0, 0, 0), thr = rtm::mk(1, 1, 1);
    // the end of a sample of colour `col`: into the accumulator and the moments, in rt_sample_pixels' order of
    // operations (rt_abi.h); after the last one the state goes back
    auto finish = [&](const rtm::f3 col) {
        const uint32_t w = (uint32_t)A(&RenderArgs::width);
        float4* const at =
            reinterpret_cast<float4*>(A(&RenderArgs::surface) + (size_t)(p / w) * A(&RenderArgs::pitch) + (size_t)(p % w) * 16);
        float4 s = *at;
        s.x = s.x + col.x, s.y = s.y + col.y, s.z = s.z + col.z, s.w = s.w + 1.0f;
        *at = s;
        if (float2* const moments = X(&SampleArgs::moments)) {
            const float l = (0.2126f * col.x + 0.7152f * col.y) + 0.0722f * col.z;
            float2 m = moments[p];
            m.x = m.x + l, m.y = m.y + l * l;
            moments[p] = m;
        }
        path = false;
        if (--left == 0) {
            rt_rng_state* const rs = A(&RenderArgs::rng) + p;
            rs->d = rng.d;
            rs->v[0] = rng.v0;
            rs->v[1] = rng.v1;
            rs->v[2] = rng.v2;
            rs->v[3] = rng.v3;
            rs->v[4] = rng.v4;
        }
    };
    for (;;) {
        if (left && !path) {
            // main_raytracing.cu:190: uv = (pixel + vec2(rng(), rng())) / vec2(W, H), u first
            const float ru = rng.uniform();
            const float rv = rng.uniform();
            const int w = A(&RenderArgs::width);
            const float uvx = ((float)(int)(p % (uint32_t)w) + ru) / (float)w;
            const float uvy = ((float)(int)(p / (uint32_t)w) + rv) / (float)A(&RenderArgs::height);
            const rtm::f3 co = arg3<COLD>(a.r, offsetof(RenderArgs, cam) + offsetof(GPUCamera, origin)),
                          ch = arg3<COLD>(a.r, offsetof(RenderArgs, cam) + offsetof(GPUCamera, horizontal)),
                          cv = arg3<COLD>(a.r, offsetof(RenderArgs, cam) + offsetof(GPUCamera, vertical)),
                          cl = arg3<COLD>(a.r, offsetof(RenderArgs, cam) + offsetof(GPUCamera, lower_left_corner));
            ro = co;  // GPUCamera::GetRay (GPUScene.h:13), not normalized
            rd = rtm::sub(rtm::add(rtm::add(cl, rtm::muls(ch, uvx)), rtm::muls(cv, uvy)), co);
            color = rtm::mk(0, 0, 0);
            thr = rtm::mk(1, 1, 1);
            bounce = 0;
            path = true;
            if (A(&RenderArgs::bounces) == 0) {  // an empty bounce loop: the sample contributes (0, 0, 0)
                finish(color);
                continue;
            }
        }
        if (!__ballot(path)) break;

        // GetRayHit (main_raytracing.cu:83-109)
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
        // `tune` is the argument (always 0 here), not a literal 0, as in the radiance body
        rtfast::trace<false, MODE>(reinterpret_cast<const float4*>(a.r.nodes), reinterpret_cast<const float4*>(a.r.tris),
                                   a.r.pairs, a.r.tree, a.r.ltris, a.r.flat, a.r.spairs, a.r.tune, stk, scratch, R, h, path, c,
                                   a.r.quads, a.r.units, a.r.face_leaf);
        if (!path) continue;

        bool end = shade_segment<false, COLD>(a.r, h, ro, rd, nd, rng, color, thr, c);
        if (++bounce >= A(&RenderArgs::bounces)) end = true;
        if (end) finish(color);
    }
}

RT_BATCH_KERNELS(sample_kernel, SampleArgs, sample_body)

}  // namespace

hipError_t launch_sample_pixels(int stack, int mode, int waves_per_simd, const SampleArgs& a, hipStream_t s) {
    if (a.r.bounces < 0 || a.r.width <= 0 || a.r.height <= 0) return hipErrorInvalidValue;
    return launch_batch<sample_kernel_set>(stack, mode, waves_per_simd, a.count, a, s);
}

}  // namespace rtk
