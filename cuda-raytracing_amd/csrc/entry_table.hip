// entry_table.hip -- the camera rays' entry frontier (entry_frontier.h): per mirror, the device table of the entry
// records and the key it was built from.  entry_table returns the table for this frame's camera and viewport,
// rebuilding it on `s` -- entry_table_kernel, one lane per 8x8 sub-tile -- only when the key changed: a still camera
// pays nothing per frame, a moving one the builder (2.7 ms at 1080p as it stands: profiles/entry_ab.txt) and never a
// host round trip (a new viewport SIZE reallocates, which synchronises).  One table per scene: frames of one scene
// rendered from different cameras on different streams at once would race for it, as they would for the scene's RNG
// states.  A frame of the same key on another stream than the one the table was built on waits for the build's event
// first.
#include <hip/hip_runtime.h>

#include <atomic>
#include <map>
#include <mutex>

#include "rt_abi.h"
#include "rt_host.h"
#include "rt_variant.h"
#include "entry_frontier.h"

namespace {

static_assert(EF_K == 15 && EF_TILE == 8 && EF_WORDS == 16, "the lean kernels read 16-word records of 8x8 sub-tiles (rt_fast.h)");
static_assert(rtk::kEntryStackExtra == EF_K - 1, "rt_variant.h sizes the stack of a frame with entry records");

__global__ __launch_bounds__(64) void entry_table_kernel(const float* nodes, uint32_t node_count, EfCamera cam, int width,
                                                         int height, int tiles_x, int tiles, uint32_t* out) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= tiles) return;
    uint32_t rec[EF_WORDS];
    ef_build_record(nodes, node_count, cam, width, height, i % tiles_x, i / tiles_x, rec);
    uint4* o = reinterpret_cast<uint4*>(out + (size_t)EF_WORDS * i);
    for (int k = 0; k < EF_WORDS / 4; k++) o[k] = make_uint4(rec[4 * k], rec[4 * k + 1], rec[4 * k + 2], rec[4 * k + 3]);
}

struct EntryTable {
    EfKey key{};
    bool valid = false;
    uint32_t* dev = nullptr;
    size_t bytes = 0;
    hipEvent_t built = nullptr;  // recorded behind the builder on `built_on`
    hipStream_t built_on = nullptr;
};
std::mutex g_entry_mutex;
std::map<const void*, EntryTable> g_entry;  // keyed by the mirror's private node array
std::atomic<uint64_t> g_entry_builds{0};

}  // namespace

const uint32_t* rt_host::entry_table(const MirrorDevice& mir, const GPUCamera& c, int width, int height, hipStream_t s) {
    EfCamera cam;
    for (int i = 0; i < 3; i++) {
        cam.origin[i] = c.origin[i], cam.lower_left[i] = c.lower_left_corner[i];
        cam.horizontal[i] = c.horizontal[i], cam.vertical[i] = c.vertical[i];
    }
    const EfKey now = ef_make_key(cam, width, height, mir.nodes, mir.generation);
    const int tiles_x = ef_tiles_x(width), tiles = tiles_x * ef_tiles_y(height);
    const size_t bytes = (size_t)tiles * EF_WORDS * 4;
    std::lock_guard<std::mutex> lock(g_entry_mutex);
    EntryTable& t = g_entry[mir.nodes];
    if (t.valid && ef_key_same(t.key, now)) {
        if (s != t.built_on && hipStreamWaitEvent(s, t.built, 0) != hipSuccess) return nullptr;
        return t.dev;
    }
    t.valid = false;
    if (t.bytes != bytes) {
        if (t.dev) (void)hipFree(t.dev);  // synchronises: no earlier frame still reads it
        t.dev = nullptr, t.bytes = 0;
        if (hipMalloc((void**)&t.dev, bytes) != hipSuccess) {
            (void)hipGetLastError();
            t.dev = nullptr;
            return nullptr;
        }
        t.bytes = bytes;
    }
    hipLaunchKernelGGL(entry_table_kernel, dim3((unsigned)((tiles + 63) / 64)), dim3(64), 0, s, (const float*)mir.nodes,
                       mir.node_count, cam, width, height, tiles_x, tiles, t.dev);
    if (hipGetLastError() != hipSuccess) return nullptr;
    if (!t.built && hipEventCreateWithFlags(&t.built, hipEventDisableTiming) != hipSuccess) return nullptr;
    if (hipEventRecord(t.built, s) != hipSuccess) return nullptr;
    t.built_on = s;
    t.key = now, t.valid = true;
    g_entry_builds++;
    return t.dev;
}

extern "C" uint64_t rt_entry_table_builds(void) { return g_entry_builds.load(); }

void rt_internal_forget_entry_table(const void* mirror_nodes) {
    std::lock_guard<std::mutex> lock(g_entry_mutex);
    auto it = g_entry.find(mirror_nodes);
    if (it == g_entry.end()) return;
    if (it->second.dev) (void)hipFree(it->second.dev);
    if (it->second.built) (void)hipEventDestroy(it->second.built);
    g_entry.erase(it);
}
