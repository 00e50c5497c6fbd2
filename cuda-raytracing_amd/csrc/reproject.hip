// reproject.hip -- rt_reproject (include/rt_abi.h): temporal accumulation across camera moves.  The new frame's
// first-hit points (rt_trace_rays' camera mode) are projected into the previous camera's viewport, the previous
// accumulated image and its per-pixel history length are gathered there bilinearly from the taps whose own
// first-hit record agrees (material, normal, tangent plane), and the new frame is blended in as a running mean.
//
// The arithmetic is the one rt_abi.h specifies and tests/reproject_ref.py restates in numpy: fp32, no contraction,
// IEEE division (the flags of every unit, build.py), only + - * /, floorf, fminf, fabsf and comparisons, so the
// GPU and the restatement agree bit for bit.  One kernel, one pixel per lane, the 64 x 4-pixel block of
// denoise_pass: a wave covers 64 x 1 pixels, so its own pixel's loads and stores are whole cache lines, and under
// a small camera move its taps are a nearly contiguous row of the previous buffers as well.  The loads of all four
// taps (3 float4 of the record, the colour, the history: 68 B each) are issued together from clamped coordinates
// before any tap is tested, as denoise_pass measured for its taps.  A lane moves 16 + 48 B in and 16 + 4 B out for
// itself and gathers 4 x 68 B, most of which its neighbours gather too (profiles/reproject_timing.txt).  This is
// the fastest of the shapes measured (profiles/reproject_variants.txt; the others are not kept):
// loading a tap's normal and position only after its cheap tests passed is 24 % slower, a 32 x 8-pixel block 1 %.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "atrous.h"  // finite1, finite3
#include "image_entry.h"
#include "rt_abi.h"

namespace {

using atrous::finite3;
using namespace rt_entry;

// the defaults RT_REPROJECT_DEFAULT selects, chosen from profiles/reproject_quality.txt: the error
// is flat beyond a history of 32 frames and does not depend on sigma_plane there; normal_min 0.99 loses history
constexpr int DEFAULT_MAX_HISTORY = 32;
constexpr float DEFAULT_SIGMA_PLANE = 0.03f;
constexpr float DEFAULT_NORMAL_MIN = 0.9f;

struct V3 {
    float x, y, z;
};

__host__ __device__ __forceinline__ float dot3(const V3& a, const V3& b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__host__ __device__ __forceinline__ V3 cross3(const V3& a, const V3& b) {
    return V3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
__host__ __device__ __forceinline__ V3 sub3(const V3& a, const V3& b) { return V3{a.x - b.x, a.y - b.y, a.z - b.z}; }

struct ReprojectArgs {
    const char* surface;
    uint64_t pitch;
    const float4* hits;
    const char* prev_surface;  // NULL: no history at all
    uint64_t prev_pitch;
    const float4* prev_hits;
    const float* prev_history;
    char* out;
    uint64_t out_pitch;
    float* out_history;
    V3 co, ch, cv, cl;     // the current camera: origin, horizontal, vertical, lower-left corner (sky directions)
    V3 po, pn, pa, pb;     // the previous camera: origin O and the per-frame constants N, A, B
    float wn;
    int width, height;
    float max_history, sigma_plane, normal_min;
};

__global__ __launch_bounds__(256) void reproject_kernel(const ReprojectArgs a) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= a.width || y >= a.height) return;
    const size_t p = (size_t)y * a.width + x;
    const float4 cur = *reinterpret_cast<const float4*>(a.surface + (size_t)y * a.pitch + (size_t)x * 16);
    const bool cur_finite = finite3(cur);
    float ox = cur.x, oy = cur.y, oz = cur.z, oh = cur_finite ? 1.0f : 0.0f;  // without history
    if (a.prev_surface) {
        const float4 h0 = a.hits[3 * p], h1 = a.hits[3 * p + 1], h2 = a.hits[3 * p + 2];  // (t kind id material) (n bx) (pos by)
        const bool hit = __float_as_uint(h0.y) != 0u;
        const V3 np{h1.x, h1.y, h1.z}, pp{h2.x, h2.y, h2.z};
        V3 d;
        if (hit) {
            d = sub3(pp, a.po);
        } else {  // sky is at infinity: the pixel-centre direction, formed as rt_trace_rays' camera mode forms it
            const float ux = ((float)x + 0.5f) / (float)a.width, uy = ((float)y + 0.5f) / (float)a.height;
            d = V3{((a.cl.x + a.ch.x * ux) + a.cv.x * uy) - a.co.x, ((a.cl.y + a.ch.y * ux) + a.cv.y * uy) - a.co.y,
                   ((a.cl.z + a.ch.z * ux) + a.cv.z * uy) - a.co.z};
        }
        const float dn = dot3(d, a.pn), s = a.wn / dn;
        const float fx = (dot3(d, a.pa) / dn) * (float)a.width - 0.5f;
        const float fy = (dot3(d, a.pb) / dn) * (float)a.height - 0.5f;
        // NaN fails every comparison; only a projection that passed them reaches the int conversion below
        if (dn != 0.0f && s > 0.0f && fx > -1.0f && fx < (float)a.width && fy > -1.0f && fy < (float)a.height) {
            const float flx = floorf(fx), fly = floorf(fy);
            const int x0 = (int)flx, y0 = (int)fly;  // in [-1, width - 1] x [-1, height - 1]
            const float ax = fx - flx, ay = fy - fly;
            const float wx[2] = {1.0f - ax, ax}, wy[2] = {1.0f - ay, ay};
            float4 q0[4], q1[4], q2[4], qc[4];
            float qh[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {  // every load of every tap, from clamped coordinates, before any test
                const int qx = min(max(x0 + (k & 1), 0), a.width - 1), qy = min(max(y0 + (k >> 1), 0), a.height - 1);
                const size_t q = (size_t)qy * a.width + qx;
                q0[k] = a.prev_hits[3 * q], q1[k] = a.prev_hits[3 * q + 1], q2[k] = a.prev_hits[3 * q + 2];
                qc[k] = *reinterpret_cast<const float4*>(a.prev_surface + (size_t)qy * a.prev_pitch + (size_t)qx * 16);
                qh[k] = a.prev_history[q];
            }
            const float plane = a.sigma_plane * h0.x;
            float sx = 0.0f, sy = 0.0f, sz = 0.0f, hs = 0.0f, ws = 0.0f;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int qx = x0 + (k & 1), qy = y0 + (k >> 1);
                const float w = wx[k & 1] * wy[k >> 1];
                if (qx < 0 || qx >= a.width || qy < 0 || qy >= a.height || !(w > 0.0f) || !(qh[k] >= 1.0f) || !finite3(qc[k]))
                    continue;
                const bool qhit = __float_as_uint(q0[k].y) != 0u;
                if (hit) {
                    if (!qhit || __float_as_uint(q0[k].w) != __float_as_uint(h0.w)) continue;
                    const V3 nq{q1[k].x, q1[k].y, q1[k].z}, pq{q2[k].x, q2[k].y, q2[k].z};
                    if (!(dot3(np, nq) >= a.normal_min) || !(fabsf(dot3(np, sub3(pq, pp))) <= plane)) continue;
                } else if (qhit) {
                    continue;
                }
                sx += qc[k].x * w, sy += qc[k].y * w, sz += qc[k].z * w;
                hs += qh[k] * w;
                ws += w;
            }
            if (ws > 0.0f) {
                const float px = sx / ws, py = sy / ws, pz = sz / ws, hl = hs / ws;
                if (cur_finite) {
                    const float n = fminf(hl + 1.0f, a.max_history), r = 1.0f / n;
                    ox = px + (cur.x - px) * r, oy = py + (cur.y - py) * r, oz = pz + (cur.z - pz) * r;
                    oh = n;
                } else {  // the history heals the pixel
                    ox = px, oy = py, oz = pz;
                    oh = fminf(hl, a.max_history);
                }
            }
        }
    }
    *reinterpret_cast<float4*>(a.out + (size_t)y * a.out_pitch + (size_t)x * 16) = make_float4(ox, oy, oz, cur.w);
    a.out_history[p] = oh;
}

V3 ld3(const float v[3]) { return V3{v[0], v[1], v[2]}; }

}  // namespace

extern "C" int rt_reproject(const rt_reproject_params* p, void* stream) {
    const char* const who = "rt_reproject";
    if (!p) return refuse(who, "null params");
    if (!p->surface) return refuse(who, "null surface");
    if (!p->hits) return refuse(who, "null hits");
    if (!p->out) return refuse(who, "null out");
    if (!p->out_history) return refuse(who, "null out_history");
    const int prevs = (p->prev_surface != nullptr) + (p->prev_hits != nullptr) + (p->prev_history != nullptr);
    if (prevs != 0 && prevs != 3) return refuse(who, "prev_surface, prev_hits and prev_history must be all NULL or all non-NULL");
    const bool has_prev = prevs == 3;
    if (size_refused(who, p->width, p->height) || caps_refused(who, p->width, p->height, "REPROJECT")) return 1;
    if (pitch_refused(who, "pitch", p->pitch, p->width) || pitch_refused(who, "out_pitch", p->out_pitch, p->width)) return 1;
    if (has_prev && pitch_refused(who, "prev_pitch", p->prev_pitch, p->width)) return 1;
    if (pitches_refused(who, {p->pitch, p->out_pitch, has_prev ? p->prev_pitch : 0})) return 1;
    if (misaligned(who, "surface, hits, prev_surface, prev_hits and out", 16, {p->surface, p->hits, p->out, p->prev_surface, p->prev_hits}))
        return 1;
    if (misaligned(who, "prev_history and out_history", 4, {p->out_history, p->prev_history})) return 1;
    if (p->flags != 0) return refuse(who, "flags must be 0");
    const int max_history = or_default(p->max_history, RT_REPROJECT_DEFAULT, DEFAULT_MAX_HISTORY);
    const float sigma_plane = or_default(p->sigma_plane, RT_REPROJECT_DEFAULT, DEFAULT_SIGMA_PLANE);
    const float normal_min = or_default(p->normal_min, RT_REPROJECT_DEFAULT, DEFAULT_NORMAL_MIN);
    if (max_history < 1 || max_history > 65535) return refuse(who, "max_history must be 1..65535 (or RT_REPROJECT_DEFAULT)");
    if (!finite_above(sigma_plane, 0.0f)) return refuse(who, "sigma_plane must be > 0 and finite (or RT_REPROJECT_DEFAULT)");
    if (!(normal_min >= -1.0f) || !(normal_min <= 1.0f)) return refuse(who, "normal_min must be in [-1, 1] (or RT_REPROJECT_DEFAULT)");
    const uint64_t n = (uint64_t)p->width * (uint64_t)p->height, row = (uint64_t)p->width * 16;
    if (has_prev) {
        // other lanes gather from the previous image and history while this one writes
        if (overlap(p->out, surface_bytes(p->height, p->out_pitch, row), p->prev_surface, surface_bytes(p->height, p->prev_pitch, row)))
            return refuse(who, "out must not overlap prev_surface");
        if (overlap(p->out_history, n * 4, p->prev_history, n * 4)) return refuse(who, "out_history must not overlap prev_history");
    }

    ReprojectArgs a;
    a.surface = static_cast<const char*>(p->surface), a.pitch = p->pitch;
    a.hits = static_cast<const float4*>(static_cast<const void*>(p->hits));
    a.prev_surface = has_prev ? static_cast<const char*>(p->prev_surface) : nullptr, a.prev_pitch = p->prev_pitch;
    a.prev_hits = static_cast<const float4*>(static_cast<const void*>(p->prev_hits));
    a.prev_history = p->prev_history;
    a.out = static_cast<char*>(p->out), a.out_pitch = p->out_pitch;
    a.out_history = p->out_history;
    a.co = ld3(p->camera.origin), a.ch = ld3(p->camera.horizontal), a.cv = ld3(p->camera.vertical);
    a.cl = ld3(p->camera.lower_left_corner);
    // the per-frame constants of the previous camera (rt_abi.h): Cramer's rule on O + s d = L + u H + v V
    const V3 O = ld3(p->prev_camera.origin), H = ld3(p->prev_camera.horizontal), V = ld3(p->prev_camera.vertical);
    const V3 w = sub3(ld3(p->prev_camera.lower_left_corner), O);
    a.po = O;
    a.pn = cross3(H, V), a.pa = cross3(V, w), a.pb = cross3(w, H);
    a.wn = dot3(w, a.pn);
    a.width = p->width, a.height = p->height;
    a.max_history = (float)max_history, a.sigma_plane = sigma_plane, a.normal_min = normal_min;
    hipLaunchKernelGGL(reproject_kernel, image_grid(p->width, p->height), dim3(256), 0, (hipStream_t)stream, a);
    return launch_refused(who);
}
