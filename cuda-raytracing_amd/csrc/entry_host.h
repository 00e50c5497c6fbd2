/* entry_host.h -- the tests' view of the entry-record builder on the host (librt_entry_host.so, built by build() from
 * entry_host.cpp and linked against librt_hip.so; not part of the product's ABI).  The same builder and key rule as
 * rt_render's cache (entry_frontier.h): update builds the mirror of the given reference arrays when they change and
 * the table when its key does (returns 1 when it rebuilt the table, 0 when the key was unchanged, -1 on error, text
 * in rt_last_error); records are 16 words (count, then node indices of the private node array in visit order);
 * replay walks the reference's DFS in plain fp32 for camera rays of pixel (px, py) with jitter (ru, rv), from the
 * root and from the pixel's record. */
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "rt_abi.h"

#ifdef __cplusplus
extern "C" {
#endif
typedef struct rt_entry_host rt_entry_host;
typedef struct rt_entry_replay {
    uint32_t face_root, face_entry;     /* face hit (0xffffffff: none) walking from the root / from the record */
    float t_root, t_entry;              /* its distance (1e30: none) */
    uint32_t visits_root, visits_entry; /* nodes popped */
    int32_t qualifies;                  /* the ray is one the kernel starts from its record (else both walks start at the root) */
    int32_t dropped_hit;                /* nodes left out of the record that pass IntersectAABB with len = inf (must be 0) */
    float direction[3];
    uint32_t stack_root, stack_entry;   /* most stack entries the kernel's walk holds (entries that pass IntersectAABB's own
                                           conditions: the others it never pushes), from the root / from the record */
    uint32_t reserved;
} rt_entry_replay;
rt_entry_host* rt_entry_host_create(void);
void rt_entry_host_destroy(rt_entry_host* table);
int rt_entry_host_update(rt_entry_host* table, const GPUBVHNode* nodes, size_t node_count, const uint32_t* face_indices,
                         size_t index_count, const GPUFace* faces, size_t face_count, const GPUVertex* vertices,
                         size_t vertex_count, const GPUCamera* camera, int width, int height);
uint64_t rt_entry_host_builds(const rt_entry_host* table);
const uint32_t* rt_entry_host_records(const rt_entry_host* table, size_t* record_count);
const float* rt_entry_host_nodes(const rt_entry_host* table, size_t* node_count);  /* 8 floats a node */
int rt_entry_host_dropped(const rt_entry_host* table, int tile_x, int tile_y, uint32_t* out, int cap);
int rt_entry_host_replay(const rt_entry_host* table, size_t count, const int32_t* px, const int32_t* py, const float* ru,
                         const float* rv, rt_entry_replay* out);

#ifdef __cplusplus
}
#endif
