/* entry_probe.cpp -- analysis tool (test infrastructure, includes the oracle): what starting camera rays from a
 * per-sub-tile entry record (csrc/entry_frontier.h) instead of the BVH root saves, priced on the oracle's own node
 * array with the oracle's own aabb_hit / tri_hit.  C++ only because it shares the builder's header with the kernels;
 * the oracle's C source is included as it is.
 *
 * Config 2's camera, every sub-tile of the viewport, 8 jittered primary rays per sub-tile: BVHRayHit
 * (main_raytracing.cu:33-81) from the root against the same loop started from the sub-tile's record.  Prints node
 * visits per primary ray both ways, the mean record size and the rays whose hit differs (face or distance bits).
 *
 *   g++ -O2 -fopenmp -ffp-contract=off -fpermissive -w -x c++ -DRT_EF_K=15 -DRT_EF_TILE=8 \
 *       -I cuda-raytracing_amd/csrc -o /tmp/entry_probe tools/entry_probe.cpp -lm
 *   /tmp/entry_probe assets [width height]        (one build per K / sub-tile size: profiles/entry_pricing.txt)
 */
#include "../oracle/rt_oracle.c"

#include "entry_frontier.h"

struct Res { uint32_t face; float t; uint64_t visits; };

/* BVHRayHit from a start stack (top = last element), the oracle's arithmetic; no spheres: `closest` starts at 1e30 */
static Res walk(const OScene* s, v3 ro, v3 rd, const uint32_t* start, int n) {
    uint32_t stack[96];
    int top = 0;
    for (int i = 0; i < n; i++) stack[top++] = start[i];
    const v3 nd = vnorm(rd);
    Res r = {0xffffffffu, 1e30f, 0};
    while (top) {
        const ONode* nd_ = &s->nodes[stack[--top]];
        r.visits++;
        if (!aabb_hit(ro, rd, nd_, r.t)) continue;
        if (nd_->count > 0) {
            for (uint32_t i = 0; i < nd_->count; i++) {
                const uint32_t fi = s->face_idx[nd_->first + i];
                const OFace* f = &s->faces[fi];
                const OVertex *v0 = &s->verts[f->v0], *v1 = &s->verts[f->v1], *v2 = &s->verts[f->v2];
                float bx, by, dist;
                if (tri_hit(ro, nd, V(v0->p[0], v0->p[1], v0->p[2]), V(v1->p[0], v1->p[1], v1->p[2]), V(v2->p[0], v2->p[1], v2->p[2]),
                            &bx, &by, &dist)) {
                    if (dist >= r.t || dist < 0.0f) continue;
                    r.t = dist, r.face = fi;
                }
            }
        } else {
            stack[top++] = nd_->first;
            stack[top++] = nd_->first + 1;
        }
    }
    return r;
}

int main(int argc, char** argv) {
    if (argc < 2) return fprintf(stderr, "usage: entry_probe assets [width height]\n"), 2;
    const int W = argc > 3 ? atoi(argv[2]) : 1920, H = argc > 3 ? atoi(argv[3]) : 1080;
    OScene* s = oracle_scene_create(0, argv[1], 0);
    if (!s) return fprintf(stderr, "oracle_scene_create failed\n"), 1;
    OCamera oc;
    o_camera(s, W, H, &oc);
    EfCamera cam;
    for (int i = 0; i < 3; i++)
        cam.origin[i] = oc.origin[i], cam.lower_left[i] = oc.llc[i], cam.horizontal[i] = oc.horizontal[i], cam.vertical[i] = oc.vertical[i];
    const int tx = ef_tiles_x(W), ty = ef_tiles_y(H);
    uint64_t v_root = 0, v_rec = 0, rays = 0, diff = 0, size = 0, root_started = 0;
    /* the oracle's node array has the layout the builder reads: 8 words a node, children adjacent, first = the left one */
    const float* nodes = (const float*)s->nodes;
#pragma omp parallel for schedule(dynamic, 16) reduction(+ : v_root, v_rec, rays, diff, size, root_started)
    for (int t = 0; t < tx * ty; t++) {
        uint32_t rec[EF_WORDS];
        ef_build_record(nodes, (uint32_t)s->nnodes, cam, W, H, t % tx, t / tx, rec);
        size += rec[0];
        uint32_t start[EF_K], root = 0;
        for (uint32_t i = 0; i < rec[0]; i++) start[i] = rec[rec[0] - i];  /* first visited on top */
        ORng g;
        rng_init(0xDEADBEEFu, (uint64_t)t, &g);
        for (int k = 0; k < 8; k++) {
            const int x0 = (t % tx) * EF_TILE, y0 = (t / tx) * EF_TILE;
            int x = x0 + (int)(rng_next(&g) % EF_TILE), y = y0 + (int)(rng_next(&g) % EF_TILE);
            x = x < W ? x : W - 1, y = y < H ? y : H - 1;
            const float uvx = ((float)x + rng_uniform(&g)) / (float)W, uvy = ((float)y + rng_uniform(&g)) / (float)H;
            const v3 ro = V(oc.origin[0], oc.origin[1], oc.origin[2]);
            float d[3];
            for (int i = 0; i < 3; i++) d[i] = ((oc.llc[i] + oc.horizontal[i] * uvx) + oc.vertical[i] * uvy) - oc.origin[i];
            const v3 rd = V(d[0], d[1], d[2]);
            const Res a = walk(s, ro, rd, &root, 1);
            const bool ok = ef_ray_ok(oc.origin, d);  /* any other ray starts at the root in the kernel too */
            const Res b = ok ? walk(s, ro, rd, start, (int)rec[0]) : a;
            uint32_t ta, tb;
            memcpy(&ta, &a.t, 4), memcpy(&tb, &b.t, 4);
            v_root += a.visits, v_rec += b.visits, rays++, root_started += !ok;
            diff += a.face != b.face || ta != tb;
        }
    }
    printf("%dx%d sub-tiles, K = %2d | node visits per primary ray, root -> record: %.1f -> %.1f | mean record size %.1f | "
           "rays with a different hit: %llu of %llu | started at the root: %llu\n", EF_TILE, EF_TILE, EF_K, (double)v_root / rays,
           (double)v_rec / rays, (double)size / (tx * ty), (unsigned long long)diff, (unsigned long long)rays,
           (unsigned long long)root_started);
    oracle_scene_destroy(s);
    return 0;
}
