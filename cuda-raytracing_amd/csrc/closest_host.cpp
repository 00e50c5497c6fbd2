// closest_host.cpp -- rt_closest_point_host (rt_abi.h): rt_closest_point's answer by brute force over the scene's host
// arrays -- every sphere in order, then every face in order, no BVH -- by the kernel's own source (closest.h), compiled
// with the same numerics flags (build.py FP_FLAGS).  The points are dealt to a few threads; each record depends on
// its own point only.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <thread>
#include <vector>

#include "rt_abi.h"
#include "closest.h"
#include "mirror.h"  // rt_internal_set_error

static rtm::f3 v3(const float* p) { return rtm::f3{p[0], p[1], p[2]}; }

extern "C" int rt_closest_point_host(rt_scene* scene, const rt_point* points, int64_t count, rt_nearest* out) {
    if (!scene || count < 0 || (count > 0 && (!points || !out))) {
        rt_internal_set_error("rt_closest_point_host: null argument or negative count");
        return -1;
    }
    const GPUVertex* vertices = nullptr;
    const GPUFace* faces = nullptr;
    size_t face_count = 0, vertex_count = 0, sphere_count = 0;
    rt_scene_host_arrays(scene, nullptr, nullptr, nullptr, &face_count, &vertices, &vertex_count, &faces);
    rt_scene_spheres(scene, nullptr, &sphere_count);
    std::vector<GeometrySphere> spheres(sphere_count);
    if (sphere_count) rt_scene_spheres(scene, spheres.data(), &sphere_count);
    // the mirror's records: (v0, v1 - v0, v2 - v0), v1 and v2 by name
    struct Rec {
        rtm::f3 a, ab, ac;
    };
    std::vector<Rec> recs(face_count);
    for (size_t f = 0; f < face_count; f++) {
        const GPUFace& fc = faces[f];
        if (fc.v0 >= vertex_count || fc.v1 >= vertex_count || fc.v2 >= vertex_count) {
            rt_internal_set_error("rt_closest_point_host: a face names a vertex out of range");
            return -1;
        }
        const rtm::f3 a = v3(vertices[fc.v0].position);
        recs[f] = Rec{a, rtm::sub(v3(vertices[fc.v1].position), a), rtm::sub(v3(vertices[fc.v2].position), a)};
    }
    auto run = [&](int64_t i0, int64_t i1) {
        for (int64_t i = i0; i < i1; i++) {
            const rtm::f3 p = v3(points[i].position);
            const float radius = points[i].radius;
            rtc::Best b = rtc::best_start(radius * radius);
            for (size_t k = 0; k < sphere_count; k++)
                rtc::offer(b, rtc::closest_on_sphere(p, v3(spheres[k].position), spheres[k].radius), 1u, (uint32_t)k);
            for (size_t f = 0; f < face_count; f++)
                rtc::offer(b, rtc::closest_on_triangle(p, recs[f].a, recs[f].ab, recs[f].ac), 2u, (uint32_t)f);
            rt_nearest r;
            std::memset(&r, 0, sizeof(r));
            r.distance = radius;
            if (b.kind != 0u) {
                r.distance = sqrtf(b.d2);
                r.kind = b.kind, r.id = b.id;
                r.material = b.kind == 1u ? (uint32_t)spheres[b.id].material : faces[b.id].material;
                r.point[0] = b.q.x, r.point[1] = b.q.y, r.point[2] = b.q.z;
                r.region = b.region;
            }
            std::memcpy(&out[i], &r, sizeof(r));  // the radius' bits as passed, a NaN's payload included
        }
    };
    const int64_t work = count * (int64_t)(face_count + sphere_count);
    const int threads = (int)std::max<int64_t>(1, std::min<int64_t>({16, (int64_t)std::thread::hardware_concurrency(), work >> 22}));
    if (threads == 1) {
        run(0, count);
        return 0;
    }
    std::vector<std::thread> pool;
    for (int t = 0; t < threads; t++) pool.emplace_back(run, count * t / threads, count * (t + 1) / threads);
    for (auto& th : pool) th.join();
    return 0;
}

extern "C" float rt_closest_bound_host(const float p[3], const float lo[3], const float hi[3]) {
    return rtc::point_in_cull_range(v3(p)) ? rtc::box_bound(v3(p), v3(lo), v3(hi)) : -1.0f;
}
