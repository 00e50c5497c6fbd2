// entry_host.cpp -- the entry table on the host (entry_host.h, librt_entry_host.so: a test helper beside the
// product library, not part of it): the same builder as the device kernel (entry_frontier.h) over a mirror built
// from host arrays, the same key rule as rt_render's cache, and a plain fp32 replay of the reference's walk
// (main_raytracing.cu:33-81) from the root and from a record, for tests/test_entry_frontier.py.
#include "entry_frontier.h"

#include <cstring>
#include <exception>
#include <stdexcept>
#include <vector>

#include "entry_host.h"
#include "mirror.h"

struct rt_entry_host {
    EfKey key{};
    bool valid = false;
    uint64_t builds = 0;
    MirrorHost mirror;
    const void* mirror_of = nullptr;  // the reference node array the mirror was built from
    size_t mirror_nodes = 0;
    uint64_t generation = 0;
    std::vector<uint32_t> records;
    std::vector<std::vector<uint32_t>> dropped;  // per record: the nodes left out
};
namespace {
constexpr int kDroppedCap = 4096;  // far above any record's (a record leaves out a few nodes per level)

EfCamera ef_camera(const GPUCamera& c) {
    EfCamera e;
    for (int i = 0; i < 3; i++) {
        e.origin[i] = c.origin[i], e.lower_left[i] = c.lower_left_corner[i];
        e.horizontal[i] = c.horizontal[i], e.vertical[i] = c.vertical[i];
    }
    return e;
}

// Math.h:50-61, the reference's arithmetic (IEEE quotients, fminf / fmaxf)
bool aabb_hit(const float* o, const float* d, const float* n, float len) {
    const float tx1 = (n[0] - o[0]) / d[0], tx2 = (n[3] - o[0]) / d[0];
    float tmin = fminf(tx1, tx2), tmax = fmaxf(tx1, tx2);
    const float ty1 = (n[1] - o[1]) / d[1], ty2 = (n[4] - o[1]) / d[1];
    tmin = fmaxf(tmin, fminf(ty1, ty2)), tmax = fminf(tmax, fmaxf(ty1, ty2));
    const float tz1 = (n[2] - o[2]) / d[2], tz2 = (n[5] - o[2]) / d[2];
    tmin = fmaxf(tmin, fminf(tz1, tz2)), tmax = fminf(tmax, fmaxf(tz1, tz2));
    return tmax >= tmin && tmin < len && tmax > 0;
}

struct V3 {
    float x, y, z;
};
V3 cross(V3 a, V3 b) { return V3{a.y * b.z - b.y * a.z, a.z * b.x - b.z * a.x, a.x * b.y - b.x * a.y}; }
float dot(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }

// glm::intersectRayTriangle (gtx/intersect.inl:29-94) on a mirror record (v0, e1, e2)
bool tri_hit(V3 o, V3 d, const float* r, float* dist) {
    const float eps = 1.1920928955078125e-07f;
    const V3 a{r[0], r[1], r[2]}, e1{r[3], r[4], r[5]}, e2{r[6], r[7], r[8]};
    const V3 p = cross(d, e2);
    const float det = dot(e1, p);
    const V3 t{o.x - a.x, o.y - a.y, o.z - a.z};
    V3 q;
    if (det > eps) {
        const float u = dot(t, p);
        if (u < 0.0f || u > det) return false;
        q = cross(t, e1);
        const float v = dot(d, q);
        if (v < 0.0f || u + v > det) return false;
    } else if (det < -eps) {
        const float u = dot(t, p);
        if (u > 0.0f || u < det) return false;
        q = cross(t, e1);
        const float v = dot(d, q);
        if (v > 0.0f || u + v < det) return false;
    } else {
        return false;
    }
    *dist = dot(e2, q) * (1.0f / det);
    return true;
}

// BVHRayHit from the given start stack (top = last element)
// *depth: the most entries the kernel's stack holds on this walk.  The kernel pushes a node only when it passes
// IntersectAABB's own conditions (inner_step, trav_begin_entry), and continues into the right child without
// pushing it, so at any point it holds at most the entries of this stack that pass them.
void walk(const MirrorHost& m, const float* o, const float* d, std::vector<uint32_t> stack, uint32_t* face, float* best,
          uint32_t* visits, uint32_t* depth) {
    std::vector<char> held;
    uint32_t nheld = 0;
    for (uint32_t i : stack) {
        held.push_back(aabb_hit(o, d, &m.nodes[8 * (size_t)i], INFINITY));
        nheld += held.back();
    }
    *depth = nheld;
    const float len = sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
    const V3 nd{d[0] / len, d[1] / len, d[2] / len}, ro{o[0], o[1], o[2]};
    *face = 0xffffffffu, *best = 1e30f, *visits = 0;
    while (!stack.empty()) {
        const uint32_t i = stack.back();
        stack.pop_back();
        nheld -= held.back();
        held.pop_back();
        const float* n = &m.nodes[8 * (size_t)i];
        ++*visits;
        if (!aabb_hit(o, d, n, *best)) continue;
        uint32_t first, count;
        std::memcpy(&first, n + 6, 4), std::memcpy(&count, n + 7, 4);
        if (count > 0) {
            for (uint32_t k = first; k < first + count; k++) {
                float dist;
                if (tri_hit(ro, nd, &m.tris[12 * (size_t)k], &dist)) {
                    if (dist >= *best || dist < 0.0f) continue;
                    *best = dist;
                    std::memcpy(face, &m.tris[12 * (size_t)k + 9], 4);
                }
            }
        } else {
            stack.push_back(first);
            stack.push_back(first + 1);
            held.push_back(aabb_hit(o, d, &m.nodes[8 * (size_t)first], INFINITY));
            nheld += held.back();
            if (nheld > *depth) *depth = nheld;  // the left child waits while the right one is walked
            held.push_back(0);                    // the right child is continued, never pushed
        }
    }
}
}  // namespace

extern "C" rt_entry_host* rt_entry_host_create(void) { return new rt_entry_host(); }
extern "C" void rt_entry_host_destroy(rt_entry_host* t) { delete t; }

extern "C" int rt_entry_host_update(rt_entry_host* t, const GPUBVHNode* nodes, size_t node_count, const uint32_t* face_indices,
                                    size_t index_count, const GPUFace* faces, size_t face_count, const GPUVertex* vertices,
                                    size_t vertex_count, const GPUCamera* cam, int width, int height) {
    if (!t || !nodes || !cam || width <= 0 || height <= 0) {
        rt_internal_set_error("rt_entry_host_update: bad argument");
        return -1;
    }
    try {
        if (t->mirror_of != nodes || t->mirror_nodes != node_count) {  // another node array: a new mirror generation
            t->mirror = MirrorHost{};
            rt_build_mirror(nodes, node_count, face_indices, index_count, faces, face_count, vertices, vertex_count, &t->mirror);
            t->mirror_of = nodes, t->mirror_nodes = node_count;
            t->generation++;
        }
        const EfKey now = ef_make_key(ef_camera(*cam), width, height, nodes, t->generation);
        if (t->valid && ef_key_same(t->key, now)) return 0;
        const int tx = ef_tiles_x(width), ty = ef_tiles_y(height);
        t->records.assign((size_t)tx * ty * EF_WORDS, 0u);
        t->dropped.assign((size_t)tx * ty, std::vector<uint32_t>());
        std::vector<uint32_t> out(kDroppedCap);
        const uint32_t nn = (uint32_t)(t->mirror.nodes.size() / 8);
        for (int y = 0; y < ty; y++)
            for (int x = 0; x < tx; x++) {
                const size_t i = (size_t)y * tx + x;
                if (t->mirror.fast) {
                    int nd = 0;
                    ef_build_record(t->mirror.nodes.data(), nn, now.cam, width, height, x, y, &t->records[i * EF_WORDS],
                                    out.data(), kDroppedCap, &nd);
                    if (nd > kDroppedCap) throw std::runtime_error("rt_entry_host_update: more nodes left out than the list holds");
                    t->dropped[i].assign(out.begin(), out.begin() + nd);
                } else {
                    t->records[i * EF_WORDS] = 1;  // outside the proven range: {1, root}
                }
            }
        t->key = now, t->valid = true;
        t->builds++;
        return 1;
    } catch (const std::exception& e) {
        rt_internal_set_error(e.what());
        return -1;
    }
}

extern "C" uint64_t rt_entry_host_builds(const rt_entry_host* t) { return t ? t->builds : 0; }

extern "C" const uint32_t* rt_entry_host_records(const rt_entry_host* t, size_t* count) {
    if (count) *count = t ? t->records.size() / EF_WORDS : 0;
    return t && !t->records.empty() ? t->records.data() : nullptr;
}

extern "C" const float* rt_entry_host_nodes(const rt_entry_host* t, size_t* count) {
    if (count) *count = t ? t->mirror.nodes.size() / 8 : 0;
    return t && !t->mirror.nodes.empty() ? t->mirror.nodes.data() : nullptr;
}

extern "C" int rt_entry_host_dropped(const rt_entry_host* t, int tx, int ty, uint32_t* out, int cap) {
    if (!t || !t->valid || tx < 0 || ty < 0 || tx >= ef_tiles_x(t->key.width) || ty >= ef_tiles_y(t->key.height)) return -1;
    const size_t i = (size_t)ty * ef_tiles_x(t->key.width) + tx;
    const int n = (int)t->dropped[i].size();
    for (int k = 0; k < n && k < cap; k++) out[k] = t->dropped[i][k];
    return n;  // all of them: call again with a larger list when n > cap
}

extern "C" int rt_entry_host_replay(const rt_entry_host* t, size_t n, const int32_t* px, const int32_t* py, const float* ru,
                                    const float* rv, rt_entry_replay* out) {
    if (!t || !t->valid || !px || !py || !ru || !rv || !out) {
        rt_internal_set_error("rt_entry_host_replay: bad argument");
        return -1;
    }
    const EfCamera& c = t->key.cam;
    const int W = t->key.width, H = t->key.height, tiles_x = ef_tiles_x(W);
    for (size_t r = 0; r < n; r++) {
        const int x = px[r], y = py[r];
        if (x < 0 || y < 0 || x >= W || y >= H) {
            rt_internal_set_error("rt_entry_host_replay: pixel outside the viewport");
            return -1;
        }
        // render_fast_body's camera ray (main_raytracing.cu:190, GPUCamera::GetRay), in fp32
        const float uvx = ((float)x + ru[r]) / (float)W, uvy = ((float)y + rv[r]) / (float)H;
        float d[3];
        for (int i = 0; i < 3; i++) d[i] = ((c.lower_left[i] + c.horizontal[i] * uvx) + c.vertical[i] * uvy) - c.origin[i];
        rt_entry_replay& o = out[r];
        std::memset(&o, 0, sizeof(o));
        o.direction[0] = d[0], o.direction[1] = d[1], o.direction[2] = d[2];
        walk(t->mirror, c.origin, d, std::vector<uint32_t>{0u}, &o.face_root, &o.t_root, &o.visits_root, &o.stack_root);
        const size_t rec = ((size_t)(y / EF_TILE) * tiles_x + x / EF_TILE);
        o.qualifies = t->mirror.fast && ef_ray_ok(c.origin, d) ? 1 : 0;
        std::vector<uint32_t> start{0u};
        if (o.qualifies) {
            const uint32_t* R = &t->records[rec * EF_WORDS];
            start.assign(R + 1, R + 1 + R[0]);
            for (size_t a = 0, b = start.size(); a + 1 < b; a++, b--) std::swap(start[a], start[b - 1]);  // first visited on top
        }
        walk(t->mirror, c.origin, d, start, &o.face_entry, &o.t_entry, &o.visits_entry, &o.stack_entry);
        // no node left out of the record may pass IntersectAABB for this ray, whatever `closest`
        for (uint32_t k : t->dropped[rec])
            if (aabb_hit(c.origin, d, &t->mirror.nodes[8 * (size_t)k], INFINITY)) o.dropped_hit++;
    }
    return 0;
}
