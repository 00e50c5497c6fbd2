// rt_kernel.hip -- the base of the host side behind the C-ABI of include/rt_abi.h: the error state, the memory shim,
// the cube-map registry and the two checks every entry point shares (rt_host.h).  No kernel lives here: rt_render is
// rt_render.hip, the ray-batch calls rt_batch_calls.hip, the RNG set-up and the multi-GPU unshard rng_shard.hip,
// foreign scenes foreign.hip, the entry table entry_table.hip, the tests' host hooks host_hooks.hip.
//
// Numerics: every unit is compiled with -ffp-contract=off and IEEE fp32 division/sqrt, so every value
// matches the CPU oracle bit for bit ("Parity").
#include <hip/hip_runtime.h>

#include <map>
#include <mutex>
#include <string>

#include "rt_abi.h"
#include "rt_host.h"
#include "rt_variant.h"
#include "image_entry.h"

// ---------------------------------------------------------------------------------------
// error state
// ---------------------------------------------------------------------------------------
static thread_local std::string g_last_error;

int rt_host::set_error(const std::string& msg, int code) {
    g_last_error = msg;
    return code;
}
int rt_host::check(hipError_t e, const char* what) {
    if (e == hipSuccess) return 0;
    return set_error(std::string(what) + ": " + hipGetErrorString(e), (int)e);
}
using namespace rt_host;

extern "C" const char* rt_last_error(void) { return g_last_error.c_str(); }
void rt_internal_set_error(const char* msg) { set_error(msg); }

bool rt_host::depth_refused(const char* who, int depth) {
    if (depth <= rtk::kMaxBvhDepth) return false;
    set_error(std::string(who) + ": the scene's BVH is " + std::to_string(depth) + " levels deep; the traversal stack holds depth <= " +
              std::to_string(rtk::kMaxBvhDepth) + " (rebuild the scene with fewer nested triangles)");
    return true;
}

size_t rt_host::bytes_from(const void* p) {
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (!p || hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) != hipSuccess) return 0;
    return size - (size_t)((const char*)p - (const char*)base);
}

// ---------------------------------------------------------------------------------------
// memory shim (utils/CUDAHelper.h:114-156)
// ---------------------------------------------------------------------------------------
extern "C" int rt_set_device(int device) { return check(hipSetDevice(device), "hipSetDevice"); }
extern "C" int rt_device_count(void) {
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}
extern "C" int rt_malloc(void** ptr, size_t bytes) { return check(hipMalloc(ptr, bytes), "hipMalloc"); }
extern "C" int rt_malloc_pitch(void** ptr, size_t* pitch, size_t width_bytes, size_t height) {
    return check(hipMallocPitch(ptr, pitch, width_bytes, height), "hipMallocPitch");
}
extern "C" int rt_free(void* ptr) { return check(hipFree(ptr), "hipFree"); }
extern "C" int rt_memcpy_h2d(void* dst, const void* src, size_t n) {
    return check(hipMemcpy(dst, src, n, hipMemcpyHostToDevice), "hipMemcpy H2D");
}
extern "C" int rt_memcpy_d2h(void* dst, const void* src, size_t n) {
    return check(hipMemcpy(dst, src, n, hipMemcpyDeviceToHost), "hipMemcpy D2H");
}
extern "C" int rt_memcpy_d2d(void* dst, const void* src, size_t n) {
    return check(hipMemcpy(dst, src, n, hipMemcpyDeviceToDevice), "hipMemcpy D2D");
}
extern "C" int rt_memset(void* dst, int value, size_t n) { return check(hipMemset(dst, value, n), "hipMemset"); }
extern "C" int rt_synchronize(void) { return check(hipDeviceSynchronize(), "hipDeviceSynchronize"); }

// ---------------------------------------------------------------------------------------
// cube maps (utils/CUDATexture.cpp): a handle is the device address of float4[6][n][n]
// ---------------------------------------------------------------------------------------
static std::mutex g_cube_mutex;
static std::map<uint64_t, int> g_cube_size;

extern "C" uint64_t rt_cubemap_create(const float* rgba, int size) {
    if (!rgba || size <= 0) {
        set_error("rt_cubemap_create: bad arguments");
        return 0;
    }
    void* p = nullptr;
    const size_t bytes = (size_t)6 * size * size * 16;
    if (rt_malloc(&p, bytes) || rt_memcpy_h2d(p, rgba, bytes)) return 0;
    std::lock_guard<std::mutex> lock(g_cube_mutex);
    g_cube_size[(uint64_t)p] = size;
    return (uint64_t)p;
}

extern "C" int rt_cubemap_destroy(uint64_t handle) {
    {
        std::lock_guard<std::mutex> lock(g_cube_mutex);
        if (!g_cube_size.erase(handle)) return set_error("rt_cubemap_destroy: unknown handle");
    }
    return rt_free((void*)handle);
}

int rt_host::cube_size(uint64_t handle) {
    std::lock_guard<std::mutex> lock(g_cube_mutex);
    auto it = g_cube_size.find(handle);
    return it == g_cube_size.end() ? -1 : it->second;
}

// quat(vec3(0, PI, 0)) with PI = 3.1415926536f (main_raytracing.cu:7,151), glm
// qua(eulerAngle) (type_quat.inl:204-213) using the RT deterministic sin/cos.
static void sky_quat(float* w, float* x, float* y, float* z) {
    const float ex = 0.0f, ey = 3.1415926536f, ez = 0.0f;
    const float cx = rtm::rt_cosf(ex * 0.5f), cy = rtm::rt_cosf(ey * 0.5f), cz = rtm::rt_cosf(ez * 0.5f);
    const float sx = rtm::rt_sinf(ex * 0.5f), sy = rtm::rt_sinf(ey * 0.5f), sz = rtm::rt_sinf(ez * 0.5f);
    *w = cx * cy * cz + sx * sy * sz;
    *x = sx * cy * cz - cx * sy * sz;
    *y = cx * sy * cz + sx * cy * sz;
    *z = cx * cy * sz - sx * sy * cz;
}

int rt_host::fill_sky(const char* who, const GPUScene* scene, rtk::RenderArgs* a) {
    if (scene->environment_cubemap_tex) {
        const int n = cube_size(scene->environment_cubemap_tex);
        if (n <= 0) return rt_entry::refuse(who, "unknown environment cube map handle");
        a->sky = (const float*)scene->environment_cubemap_tex;
        a->sky_n = n;
    }
    sky_quat(&a->qw, &a->qx, &a->qy, &a->qz);
    return 0;
}
