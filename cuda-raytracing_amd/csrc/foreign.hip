// foreign.hip -- foreign scenes.  A GPUScene filled by another host (the reference's own Scene::Upload,
// Scene.cpp:182-234) never registers a mirror.  raytracing_process keeps the reference's
// asynchronous contract (main_raytracing.cu:202-220): no call waits for the device.
//
//   * Every frame enqueues, on the render stream, a content fingerprint of the four arrays the
//     mirror derives from (~15 MB read, a few microseconds) and a one-thread kernel that sets a
//     device flag: 1 when it equals the fingerprint of the installed mirror.  The production
//     kernel is launched gated on flag == 1 and the reference-layout tracer (which reads the AoS
//     arrays directly, no mirror) gated on flag == 0: exactly one of them renders the frame, and
//     the other's waves exit at their first instruction.
//   * The fingerprint is also copied (async) to pinned host memory.  A later call that finds it
//     different from the installed mirror's -- or a first call, with no mirror yet -- starts a
//     rebuild: async copies of the arrays to pinned host buffers, then a worker thread waits for
//     them, builds the mirror as rt_scene_upload does (mirror.h MirrorLayout), uploads it on its own
//     stream and hands it over; the next call installs it.  Until then frames render through the
//     reference layout, bit-identical by construction.
//   * A replaced mirror is freed stream-ordered after the frames that may still read it.
//
// Kernels here
//   fingerprint_kernel (+ gate)  content fingerprint of a foreign scene's arrays, per frame.
#include <hip/hip_runtime.h>

#include <atomic>
#include <map>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "rt_abi.h"
#include "rt_host.h"
#include "image_entry.h"

using namespace rt_host;
using rt_entry::refuse;
using rtk::BLOCK;

__host__ __device__ __forceinline__ unsigned long long mix64(unsigned long long x) {
    x ^= x >> 30;
    x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27;
    x *= 0x94d049bb133111ebull;
    x ^= x >> 31;
    return x;
}

struct HashArrays {
    const uint32_t* w[4];
    unsigned long long n[4];  // words
};
// what a fingerprint of arrays of these sizes is xor-ed with
static unsigned long long fingerprint_salt(const size_t bytes[4]) {
    return (unsigned long long)bytes[0] << 1 ^ (unsigned long long)bytes[3] << 33;
}

__global__ __launch_bounds__(BLOCK) void fingerprint_kernel(HashArrays h, unsigned long long* out) {
    unsigned long long acc = 0;
    const unsigned long long stride = (unsigned long long)gridDim.x * BLOCK;
    for (int k = 0; k < 4; k++) {
        for (unsigned long long i = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x; i < h.n[k]; i += stride)
            acc += mix64(((unsigned long long)k << 60) ^ (i << 32) ^ h.w[k][i]);
    }
    // one atomic per workgroup (the per-wave atomics on one word serialised: 55 us per frame)
    __shared__ unsigned long long part[BLOCK / 64];
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
        for (int w = 0; w < BLOCK / 64; w++) t += part[w];
        atomicAdd(out, t);
    }
}

// flag = (fingerprint == expected) for the gated launches; then clears the accumulator for the
// next frame (kernels on one stream run in order).
__global__ void fingerprint_gate_kernel(unsigned long long* acc, unsigned long long salt, unsigned long long expected,
                                        int have, int* flag, unsigned long long* out) {
    const unsigned long long fp = *acc ^ salt;
    *flag = (have && fp == expected) ? 1 : 0;
    *out = fp;
    *acc = 0;
}

// the same fingerprint of host copies of the arrays
static uint64_t host_fingerprint(const HashArrays& h, unsigned long long salt) {
    unsigned long long acc = 0;
    for (int k = 0; k < 4; k++)
        for (unsigned long long i = 0; i < h.n[k]; i++) acc += mix64(((unsigned long long)k << 60) ^ (i << 32) ^ h.w[k][i]);
    return acc ^ salt;
}

namespace {
struct ForeignBuild {  // one background rebuild
    std::thread worker;
    std::atomic<int> state{0};  // 1 running, 2 done (ok), 3 failed
    std::vector<char> host[4];
    char* pinned[4] = {nullptr, nullptr, nullptr, nullptr};
    size_t bytes[4] = {0, 0, 0, 0};
    hipEvent_t copied = nullptr;
    uint64_t fingerprint = 0;
    void* block = nullptr;
    MirrorDevice dev;
    std::string error;
    ~ForeignBuild() {
        if (worker.joinable()) worker.join();
    }
};

struct ForeignEntry {
    int device = 0;
    unsigned long long* d_acc = nullptr;  // fingerprint accumulator, fingerprint of the frame
    unsigned long long* d_fp = nullptr;
    int* d_flag = nullptr;
    unsigned long long* h_fp = nullptr;   // pinned copy of the last fingerprint
    hipEvent_t fp_ready = nullptr;
    bool fp_pending = false;
    bool have = false;      // a mirror is installed
    uint64_t fp_mirror = 0;  // fingerprint of the arrays it was built from
    MirrorDevice dev;
    void* block = nullptr;
    std::unique_ptr<ForeignBuild> build;
    std::vector<void*> retired;  // freed stream-ordered at the next call
};

std::mutex g_foreign_mutex;
std::map<const void*, std::unique_ptr<ForeignEntry>> g_foreign;  // keyed by the BVH node array

void upload_mirror(ForeignBuild* b) {
    try {
        const GPUBVHNode* nodes = reinterpret_cast<const GPUBVHNode*>(b->pinned[0]);
        const uint32_t* fi = reinterpret_cast<const uint32_t*>(b->pinned[1]);
        const GPUFace* faces = reinterpret_cast<const GPUFace*>(b->pinned[2]);
        const GPUVertex* verts = reinterpret_cast<const GPUVertex*>(b->pinned[3]);
        if (hipEventSynchronize(b->copied) != hipSuccess) throw std::runtime_error("array read-back failed");
        HashArrays h;
        for (int k = 0; k < 4; k++) h.w[k] = reinterpret_cast<const uint32_t*>(b->pinned[k]), h.n[k] = b->bytes[k] / 4;
        b->fingerprint = host_fingerprint(h, fingerprint_salt(b->bytes));
        MirrorHost mh;
        rt_build_mirror(nodes, b->bytes[0] / sizeof(GPUBVHNode), fi, b->bytes[1] / 4, faces, b->bytes[2] / sizeof(GPUFace),
                        verts, b->bytes[3] / sizeof(GPUVertex), &mh);
        const MirrorLayout lay(mh);
        hipStream_t st;
        if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) throw std::runtime_error("stream");
        void* block = nullptr;
        if (hipMallocAsync(&block, lay.bytes, st) != hipSuccess) throw std::runtime_error("mirror allocation failed");
        for (int i = 0; i < 11; i++)
            if (lay.size[i] && hipMemcpyAsync(static_cast<char*>(block) + lay.offset[i], lay.part[i], lay.size[i],
                                              hipMemcpyHostToDevice, st) != hipSuccess)
                throw std::runtime_error("mirror upload failed");
        const hipError_t e = hipStreamSynchronize(st);  // this worker thread only
        hipStreamDestroy(st);
        if (e != hipSuccess) throw std::runtime_error("mirror upload failed");
        b->block = block;
        b->dev = lay.at(block);
        b->dev.owned = false, b->dev.fingerprint = b->fingerprint;
        b->state = 2;
    } catch (const std::exception& e) {
        b->error = e.what();
        b->state = 3;
    }
}

void free_build(ForeignBuild* b) {
    if (b->worker.joinable()) b->worker.join();
    for (auto* p : b->pinned)
        if (p) hipHostFree(p);
    if (b->copied) hipEventDestroy(b->copied);
}

// Start a rebuild from the arrays as they are on `st` now.
int start_build(ForeignEntry& fe, const GPUScene* scene, hipStream_t st, const size_t bytes[4]) {
    auto b = std::make_unique<ForeignBuild>();
    const void* src[4] = {scene->gpu_bvh_nodes, scene->gpu_bvh_face_indices, scene->gpu_faces, scene->gpu_vertices};
    for (int i = 0; i < 4; i++) {
        b->bytes[i] = bytes[i];
        if (hipHostMalloc((void**)&b->pinned[i], bytes[i] ? bytes[i] : 16) != hipSuccess ||
            hipMemcpyAsync(b->pinned[i], src[i], bytes[i], hipMemcpyDeviceToHost, st) != hipSuccess) {
            free_build(b.get());
            return refuse("rt_render", "foreign scene read-back failed");
        }
    }
    if (hipEventCreateWithFlags(&b->copied, hipEventDisableTiming) != hipSuccess || hipEventRecord(b->copied, st) != hipSuccess) {
        free_build(b.get());
        return refuse("rt_render", "foreign scene event");
    }
    b->state = 1;
    ForeignBuild* raw = b.get();
    b->worker = std::thread([raw, dev = fe.device]() {
        hipSetDevice(dev);
        upload_mirror(raw);
    });
    fe.build = std::move(b);
    return 0;
}

ForeignEntry* foreign_entry(const GPUScene* scene) {
    std::lock_guard<std::mutex> lock(g_foreign_mutex);
    auto& slot = g_foreign[scene->gpu_bvh_nodes];
    if (!slot) {
        auto fe = std::make_unique<ForeignEntry>();
        hipGetDevice(&fe->device);
        if (hipMalloc(&fe->d_acc, 16) != hipSuccess || hipMalloc(&fe->d_fp, 8) != hipSuccess ||
            hipMalloc(&fe->d_flag, 4) != hipSuccess || hipMemset(fe->d_acc, 0, 16) != hipSuccess ||
            hipHostMalloc((void**)&fe->h_fp, 8) != hipSuccess ||
            hipEventCreateWithFlags(&fe->fp_ready, hipEventDisableTiming) != hipSuccess) {
            refuse("rt_render", "foreign scene state");
            return nullptr;
        }
        slot = std::move(fe);
    }
    return slot.get();
}

// the entry of a scene that rt_render has seen, or null
ForeignEntry* find_entry(const GPUScene* scene) {
    std::lock_guard<std::mutex> lock(g_foreign_mutex);
    auto it = g_foreign.find(scene->gpu_bvh_nodes);
    return it == g_foreign.end() ? nullptr : it->second.get();
}
}  // namespace

int rt_host::foreign_frame(const GPUScene* scene, hipStream_t st, MirrorDevice* mir, bool* have, int** gate) {
    const size_t bytes[4] = {bytes_from(scene->gpu_bvh_nodes), bytes_from(scene->gpu_bvh_face_indices),
                             bytes_from(scene->gpu_faces), bytes_from(scene->gpu_vertices)};
    if (!bytes[0] || !bytes[1] || !bytes[2] || !bytes[3]) return refuse("rt_render", "scene arrays are not device allocations");
    ForeignEntry* fe = foreign_entry(scene);
    if (!fe) return 1;
    for (void* p : fe->retired) hipFreeAsync(p, st);  // after every frame already enqueued
    fe->retired.clear();
    if (fe->build && fe->build->state >= 2) {
        ForeignBuild* b = fe->build.get();
        if (b->worker.joinable()) b->worker.join();
        if (b->state == 2) {
            if (fe->block) fe->retired.push_back(fe->block);
            fe->block = b->block;
            fe->dev = b->dev;
            fe->fp_mirror = b->fingerprint;
            fe->have = true;
        }
        free_build(b);
        fe->build.reset();
    }
    // the previous frame's fingerprint, if it has landed: a mismatch starts a rebuild
    bool stale = !fe->have;
    if (fe->fp_pending && hipEventQuery(fe->fp_ready) == hipSuccess) {
        fe->fp_pending = false;
        stale = stale || *fe->h_fp != fe->fp_mirror;
    }
    if (stale && !fe->build && start_build(*fe, scene, st, bytes) != 0) return 1;
    HashArrays h;
    h.w[0] = (const uint32_t*)scene->gpu_bvh_nodes, h.n[0] = bytes[0] / 4;
    h.w[1] = scene->gpu_bvh_face_indices, h.n[1] = bytes[1] / 4;
    h.w[2] = (const uint32_t*)scene->gpu_faces, h.n[2] = bytes[2] / 4;
    h.w[3] = (const uint32_t*)scene->gpu_vertices, h.n[3] = bytes[3] / 4;
    hipLaunchKernelGGL(fingerprint_kernel, dim3(512), dim3(BLOCK), 0, st, h, fe->d_acc);
    hipLaunchKernelGGL(fingerprint_gate_kernel, dim3(1), dim3(1), 0, st, fe->d_acc, fingerprint_salt(bytes),
                       (unsigned long long)fe->fp_mirror, fe->have ? 1 : 0, fe->d_flag, fe->d_fp);
    if (!fe->fp_pending) {
        if (hipMemcpyAsync(fe->h_fp, fe->d_fp, 8, hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipEventRecord(fe->fp_ready, st) != hipSuccess)
            return refuse("rt_render", "fingerprint read-back");
        fe->fp_pending = true;
    }
    if (hipGetLastError() != hipSuccess) return refuse("rt_render", "fingerprint launch");
    *have = fe->have;
    *mir = fe->dev;
    *gate = fe->d_flag;
    return 0;
}

// Tests: which tracer rendered this foreign scene's last frame -- 1 the production tracer (its
// mirror matched the frame's fingerprint), 0 the reference layout (mismatch), -1 no mirror was
// installed (reference layout, ungated).  Synchronises the device.
extern "C" int rt_foreign_last_tracer(const GPUScene* scene) {
    ForeignEntry* fe = find_entry(scene);
    if (!fe) return -2;
    if (!fe->have) return -1;
    int flag = -3;
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(&flag, fe->d_flag, 4, hipMemcpyDeviceToHost) != hipSuccess) return -3;
    return flag;
}

// Tests and benchmarks: wait (host) until a rebuild for this foreign scene has finished, then let
// the next frame install it.  Returns 0 when a mirror is or will be installed, 1 on failure.
extern "C" int rt_foreign_mirror_wait(const GPUScene* scene) {
    const char* const who = "rt_foreign_mirror_wait";
    ForeignEntry* fe = find_entry(scene);
    if (!fe) return refuse(who, "scene never rendered");
    if (fe->build) {
        if (fe->build->worker.joinable()) fe->build->worker.join();
        return fe->build->state != 2 ? refuse(who, fe->build->error) : 0;
    }
    return fe->have ? 0 : refuse(who, "no mirror");
}
