// entry_frontier.h -- per-sub-tile entry records for camera rays (DESIGN.md 4.1 "Entry frontier").
//
// Every camera ray of a frame leaves one origin through a pixel known before the ray exists, and walks down
// from the BVH root.  For each 8x8 sub-tile of the viewport this header builds a record: up to EF_K nodes of
// the mirror's private node array (mirror.h), in the reference's visit order, such that the reference DFS
// (main_raytracing.cu:33-81) of any camera ray of the sub-tile visits, below the root, only subtrees of
// those nodes.  The lean render kernels (rt_fast.h trav_begin_entry) start a camera ray from its record
// instead of the root.  The same code runs on the host (tests: entry_host.cpp; tools/entry_probe.cpp) and in the builder
// kernel (entry_table.hip entry_table_kernel), one lane per sub-tile.
//
// A record is built from [root] by replacing an inner node by its children, right child first (the
// reference pops first + 1 first), leaving out a child that is PROVEN missed:
//
//  * Expansion goes only through a node whose children's boxes lie inside its own (compared as floats, all
//    finite).  Then a child that passes the reference's fp32 IntersectAABB for some ray and `closest` has
//    every ancestor passing it earlier (rounded slab quantities are monotone in the bounds and `closest`
//    only falls), so testing the child alone at its turn decides what the reference decides.
//  * A child is left out only if fp32 IntersectAABB (Math.h:50-61: tmax >= tmin && tmax > 0) is false for
//    every ray the kernel can generate for the sub-tile, for any `closest` (ef_box_missed).
//
// The miss proof.  Ranges: the camera origin and every node bound in {0} u [2^-60, 2^62] (the mirror's
// `fast` flag, ef_camera_ok), direction components in [2^-40, 2^20] (the kernel starts any other ray at the
// root: rt_fast.h make_ray's R.fast).  In these ranges no quotient of the slab test overflows or underflows
// (|b - o| is 0 or >= 2^-83), so each computed quotient is ((b - o) / d)(1 + e), |e| < 2^-22.9, or exactly
// 0 when b == o.  The computed per-axis interval therefore lies inside the real interval of the box B+ whose
// faces are moved to o + (b - o)(1 +- 2^-21), outward; fmin / fmax are monotone, so if the fp32 test
// passes, t* = min_i tmax'_i > 0 lies in all three real intervals: the real ray o + t d (d the fp32
// direction, taken as a real vector) meets B+ at t* > 0.  ef_box_missed shows that no such ray exists: it
// finds a plane through o with normal n such that n . d >= 0 for every direction of the sub-tile and
// n . (p - o) < 0 for every p in B+.  The directions: the kernel computes uvx = RN(RN(x + ru) / W) with
// ru in [0, 1], which lies in [x0 / W (1 - 2^-22), x1 / W (1 + 2^-22)] for the sub-tile's columns
// [x0, x1), likewise uvy; d = RN(RN(RN(ll + RN(h uvx)) + RN(v uvy)) - o) differs from the real
// ll + h uvx + v uvy - o by at most E_i = 2^-21 (|ll_i| + |h_i| umax + |v_i| vmax + |o_i|) + 2^-100 per
// component (four roundings of at most 2^-24 of partial sums below that total, doubled).  The real
// expression is affine in (uvx, uvy), so every direction is a convex combination of the four corner
// directions plus a vector of the box [-E, E]: n . d >= min_k n . c_k - sum_i |n_i| E_i.  The candidate
// planes are the four side planes of the sub-tile's frustum widened by 1/64 of its size and the plane
// normal to its axis; each is USED only when that lower bound, evaluated in double with a 2^-40 relative
// slack for the double roundings, is >= 0 (ef_tile_setup), so the widening is a matter of yield, not of
// correctness.  All of it is evaluated in double, each sum again with a 2^-40 slack.
//
// Fallbacks: a camera outside the ranges, a camera origin lying in a face plane of an examined box (b == o:
// nothing is wrong with the proof there, but such scenes are degenerate and cheap to leave alone), or a
// non-finite box give the record {1, root}, which is the reference's walk.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define EF_HD __host__ __device__ inline
#else
#define EF_HD inline
#endif

// nodes per record: count + 15 indices = one 64-B line, 2 MB at 1920x1080.  K = 8 visits 10.4 instead of 8.0 nodes per
// camera ray on the CPU (profiles/entry_pricing.txt) and measured slower than no table at all (profiles/entry_ab.txt).
// RT_EF_K / RT_EF_TILE: other sizes for the pricing tool only (tools/entry_probe.cpp); the kernels assert the defaults.
#ifndef RT_EF_K
#define RT_EF_K 15
#endif
#ifndef RT_EF_TILE
#define RT_EF_TILE 8
#endif
constexpr int EF_K = RT_EF_K;
constexpr int EF_TILE = RT_EF_TILE;  // sub-tile edge in pixels: 8 = the 8x8 pixels of one wave in plain lane order
constexpr int EF_WORDS = (EF_K + 16) / 16 * 16;  // uint32 words per record: [0] count, [1..count] node indices in visit order
constexpr int EF_MAX_PASSES = 64;

struct EfCamera {  // GPUCamera's four vectors (rt_abi.h), as the kernel's arguments hold them
    float origin[3], lower_left[3], horizontal[3], vertical[3];
};

struct EfTile {
    double n[5][3];  // plane normals: four frustum sides, then the axis
    bool use[5];     // the plane is proven to have every direction of the sub-tile on its non-negative side
    double o[3];
    bool ok;  // camera inside the proven ranges
};

EF_HD bool ef_in_range_or_zero(float v) {
    const float a = fabsf(v);
    return v == 0.0f || (a >= 0x1p-60f && a <= 0x1p62f);
}

// The camera side of the ranges: origin in {0} u [2^-60, 2^62], the other vectors finite and below 2^60.
EF_HD bool ef_camera_ok(const EfCamera& c, int width, int height) {
    if (width <= 0 || height <= 0 || width > (1 << 20) || height > (1 << 20)) return false;
    for (int i = 0; i < 3; i++) {
        if (!ef_in_range_or_zero(c.origin[i])) return false;
        if (!(fabsf(c.lower_left[i]) < 0x1p60f && fabsf(c.horizontal[i]) < 0x1p60f && fabsf(c.vertical[i]) < 0x1p60f)) return false;
    }
    return true;
}

// Number of sub-tiles across / down a viewport; record of pixel (x, y) = (y / EF_TILE) * ef_tiles_x + x / EF_TILE.
EF_HD int ef_tiles_x(int width) { return (width + EF_TILE - 1) / EF_TILE; }
EF_HD int ef_tiles_y(int height) { return (height + EF_TILE - 1) / EF_TILE; }

// The planes of sub-tile (tx, ty) and which of them are proven (see the header comment).
EF_HD void ef_tile_setup(const EfCamera& c, int width, int height, int tx, int ty, EfTile* T) {
    T->ok = ef_camera_ok(c, width, height);
    for (int i = 0; i < 3; i++) T->o[i] = c.origin[i];
    for (int k = 0; k < 5; k++) T->use[k] = false;
    if (!T->ok) return;
    const int x0 = tx * EF_TILE, y0 = ty * EF_TILE;
    const int x1 = x0 + EF_TILE < width ? x0 + EF_TILE : width, y1 = y0 + EF_TILE < height ? y0 + EF_TILE : height;
    // the range of uvx, uvy the kernel can compute for these pixels
    const double ulo = (double)x0 / width * (1.0 - 0x1p-22), uhi = (double)x1 / width * (1.0 + 0x1p-22);
    const double vlo = (double)y0 / height * (1.0 - 0x1p-22), vhi = (double)y1 / height * (1.0 + 0x1p-22);
    const double du = (uhi - ulo) * (1.0 / 64), dv = (vhi - vlo) * (1.0 / 64);
    double E[3], cr[4][3], g[4][3];  // direction error bound, true corners, widened corners
    const double us[4] = {ulo, uhi, uhi, ulo}, vs[4] = {vlo, vlo, vhi, vhi};
    const double gu[4] = {ulo - du, uhi + du, uhi + du, ulo - du}, gv[4] = {vlo - dv, vlo - dv, vhi + dv, vhi + dv};
    for (int i = 0; i < 3; i++) {
        const double ll = c.lower_left[i], h = c.horizontal[i], v = c.vertical[i], o = c.origin[i];
        E[i] = 0x1p-21 * (fabs(ll) + fabs(h) * uhi + fabs(v) * vhi + fabs(o)) + 0x1p-100;
        for (int k = 0; k < 4; k++) {
            cr[k][i] = ((ll + h * us[k]) + v * vs[k]) - o;
            g[k][i] = ((ll + h * gu[k]) + v * gv[k]) - o;
        }
    }
    // side plane k through widened corners k, k + 1, oriented towards the opposite corner; the axis plane last
    for (int k = 0; k < 5; k++) {
        double* n = T->n[k];
        if (k < 4) {
            const double* a = g[k];
            const double* b = g[(k + 1) & 3];
            n[0] = a[1] * b[2] - a[2] * b[1], n[1] = a[2] * b[0] - a[0] * b[2], n[2] = a[0] * b[1] - a[1] * b[0];
            const double* op = g[(k + 2) & 3];
            if (n[0] * op[0] + n[1] * op[1] + n[2] * op[2] < 0.0) n[0] = -n[0], n[1] = -n[1], n[2] = -n[2];
        } else {
            for (int i = 0; i < 3; i++) n[i] = (g[0][i] + g[1][i]) + (g[2][i] + g[3][i]);
        }
        bool good = true;
        for (int j = 0; j < 4 && good; j++) {
            double dot = 0.0, mag = 0.0, err = 0.0;
            for (int i = 0; i < 3; i++) {
                dot += n[i] * cr[j][i];
                mag += fabs(n[i]) * fabs(cr[j][i]);
                err += fabs(n[i]) * E[i];
            }
            // every direction d of the sub-tile then has n . d >= 0; !(>=) also refuses NaN and infinities
            good = (dot - err * (1.0 + 0x1p-30) - 0x1p-40 * mag >= 0.0) && mag < 0x1p900;
        }
        T->use[k] = good;
    }
}

// Whether the fp32 IntersectAABB of box [lo, hi] is proven false for every camera ray of the sub-tile.
EF_HD bool ef_box_missed(const EfTile& T, const float* lo, const float* hi) {
    if (!T.ok) return false;
    double a[3], b[3];  // B+ relative to the origin
    for (int i = 0; i < 3; i++) {
        const double l = (double)lo[i] - T.o[i], h = (double)hi[i] - T.o[i];
        a[i] = l - 0x1p-21 * fabs(l);
        b[i] = h + 0x1p-21 * fabs(h);
    }
    for (int k = 0; k < 5; k++) {
        if (!T.use[k]) continue;
        double top = 0.0, mag = 0.0;  // max of n . (p - o) over B+
        for (int i = 0; i < 3; i++) {
            const double pa = T.n[k][i] * a[i], pb = T.n[k][i] * b[i];
            top += pa > pb ? pa : pb;
            mag += fabs(pa) > fabs(pb) ? fabs(pa) : fabs(pb);
        }
        if (top + 0x1p-40 * mag < 0.0) return true;
    }
    return false;
}

// nodes: the mirror's private node array, 8 floats a node: bmin.xyz, bmax.xyz, first, count (uint bits).
EF_HD uint32_t ef_bits(float f) {
    union { float f; uint32_t u; } v;
    v.f = f;
    return v.u;
}
EF_HD bool ef_finite3(const float* p) { return fabsf(p[0]) < INFINITY && fabsf(p[1]) < INFINITY && fabsf(p[2]) < INFINITY; }

// Whether node `p` (inner) may be expanded: both children's boxes finite and inside its own.
EF_HD bool ef_contains_children(const float* nodes, uint32_t p, uint32_t left) {
    const float* P = nodes + 8 * (size_t)p;
    if (!ef_finite3(P) || !ef_finite3(P + 3)) return false;
    for (uint32_t c = left; c < left + 2; c++) {
        const float* C = nodes + 8 * (size_t)c;
        if (!ef_finite3(C) || !ef_finite3(C + 3)) return false;
        for (int i = 0; i < 3; i++)
            if (!(C[i] >= P[i] && C[3 + i] <= P[3 + i] && C[i] <= C[3 + i])) return false;
    }
    return true;
}

EF_HD bool ef_on_face_plane(const float* N, const float* origin) {
    for (int i = 0; i < 3; i++)
        if (N[i] == origin[i] || N[3 + i] == origin[i]) return true;
    return false;
}

// The record of sub-tile (tx, ty): rec[0] = count, rec[1..count] = nodes in visit order.  node_count bounds
// every index read (a malformed array gives the fallback).  `dropped` (host tests; may be null) receives up
// to `dropped_cap` indices of the nodes left out, *dropped_n how many there are.
EF_HD void ef_build_record(const float* nodes, uint32_t node_count, const EfCamera& cam, int width, int height, int tx,
                           int ty, uint32_t* rec, uint32_t* dropped = nullptr, int dropped_cap = 0,
                           int* dropped_n = nullptr) {
    EfTile T;
    ef_tile_setup(cam, width, height, tx, ty, &T);
    uint32_t list[EF_K];
    int n = 1, nd = 0;
    list[0] = 0;
    bool fallback = !T.ok || node_count == 0;
    for (int pass = 0; pass < EF_MAX_PASSES && !fallback; pass++) {
        bool changed = false;
        for (int i = 0; i < n && !fallback; i++) {
            const uint32_t p = list[i];
            const float* P = nodes + 8 * (size_t)p;
            if (ef_bits(P[7]) != 0) continue;  // a leaf stays
            const uint32_t left = ef_bits(P[6]);
            if (left >= node_count || left + 1 >= node_count || left == 0) {
                fallback = true;
                break;
            }
            if (!ef_contains_children(nodes, p, left)) continue;
            const float* L = nodes + 8 * (size_t)left;
            const float* R = L + 8;
            if (ef_on_face_plane(P, cam.origin) || ef_on_face_plane(L, cam.origin) || ef_on_face_plane(R, cam.origin)) {
                fallback = true;
                break;
            }
            const bool kr = !ef_box_missed(T, R, R + 3), kl = !ef_box_missed(T, L, L + 3);
            if (kr && kl) {
                if (n == EF_K) continue;  // no slot for the second child
                for (int j = n; j > i + 1; j--) list[j] = list[j - 1];
                list[i] = left + 1, list[i + 1] = left;
                n++;
                i++;  // the children are looked at in the next pass (breadth first)
            } else if (kr || kl) {
                list[i] = kr ? left + 1 : left;
                if (dropped && nd < dropped_cap) dropped[nd] = kr ? left : left + 1;
                nd++;
            } else {
                if (dropped && nd < dropped_cap) dropped[nd] = left + 1;
                if (dropped && nd + 1 < dropped_cap) dropped[nd + 1] = left;
                nd += 2;
                for (int j = i; j + 1 < n; j++) list[j] = list[j + 1];
                n--;
                i--;
            }
            changed = true;
        }
        if (!changed) break;
    }
    if (fallback) {
        n = 1, nd = 0;
        list[0] = 0;
    }
    rec[0] = (uint32_t)n;
    for (int i = 0; i < EF_K; i++) rec[1 + i] = i < n ? list[i] : 0u;
    if (dropped_n) *dropped_n = nd;  // the true number: above dropped_cap the list is cut short
}

// The ray side of the ranges, as rt_fast.h make_ray decides R.fast for a scene inside its own range: every
// direction component in [2^-40, 2^20], the origin in {0} u [2^-60, 2^62].  Any other ray starts at the root.
EF_HD bool ef_ray_ok(const float* o, const float* d) {
    for (int i = 0; i < 3; i++) {
        if (!(fabsf(d[i]) >= 0x1p-40f && fabsf(d[i]) <= 0x1p20f)) return false;
        if (!ef_in_range_or_zero(o[i])) return false;
    }
    return true;
}

// What a table was built from.  A table is rebuilt only when its key changes: the camera's bytes, the viewport,
// the node array (its address and the mirror's generation: an address can be reused) or the record size.
struct EfKey {
    EfCamera cam;
    int width, height;
    const void* nodes;
    uint64_t generation;
    int k;
};
inline EfKey ef_make_key(const EfCamera& cam, int width, int height, const void* nodes, uint64_t generation) {
    EfKey key{};
    key.cam = cam, key.width = width, key.height = height, key.nodes = nodes, key.generation = generation, key.k = EF_K;
    return key;
}
inline bool ef_key_same(const EfKey& a, const EfKey& b) {
    // the camera by bytes: -0 and +0, or two NaNs, are different cameras here, which only costs a rebuild
    return memcmp(&a.cam, &b.cam, sizeof(EfCamera)) == 0 && a.width == b.width && a.height == b.height && a.nodes == b.nodes &&
           a.generation == b.generation && a.k == b.k;
}
