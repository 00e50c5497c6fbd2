// rng_shard.hip -- what sets a frame's RNG states up and puts a sharded frame together (rt_abi.h): rt_init_rng,
// rt_init_rng_tiles, rt_shard_tiles, rt_unshard, rt_unshard_tiles and the reference's init_rng.
//
// Kernels here
//   init_rng_kernel   curand_init(seed, pixel, 0) with GF(2) jump matrices.
//   unshard_kernel    scatter gathered tile shards back into a pitched surface.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <map>
#include <mutex>

#include "rt_abi.h"
#include "rt_host.h"
#include "xorwow.h"
#include "image_entry.h"

using namespace rt_host;
using namespace rtk;
using rt_entry::refuse;

namespace {

// ---------------------------------------------------------------------------------------
// init_rng (Random.cu:3-13): state s <- curand_init(seed, pixel(s), 0)
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void init_rng_kernel(rt_rng_state* states, const uint32_t* __restrict__ jump,
                                                         uint32_t seed, int64_t count, int width, int height,
                                                         int shard_index, int shard_count, int tiles_x,
                                                         const int32_t* __restrict__ tile_list) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= count) return;
    uint64_t sub;
    if (shard_count <= 0) {
        sub = (uint64_t)s;  // reference layout: thread id == state index
    } else {
        const int64_t k = s / BLOCK;
        const int tile = tile_list ? tile_list[k] : shard_index + (int)k * shard_count;
        if (tile < 0 || tile >= tiles_x * ((height + TILE - 1) / TILE)) return;
        int lx, ly;
        tile_pixel((int)(s % BLOCK), &lx, &ly);
        const int x = (tile % tiles_x) * TILE + lx, y = (tile / tiles_x) * TILE + ly;
        if (x >= width || y >= height) return;
        sub = (uint64_t)y * (uint64_t)width + (uint64_t)x;
    }
    uint32_t st[6];
    rt_xorwow_seed(seed, st);
    uint32_t v[5] = {st[1], st[2], st[3], st[4], st[5]};
    for (int k = 0; sub && k < RT_XORWOW_JUMPS; k++, sub >>= 2) {
        const uint32_t reps = (uint32_t)(sub & 3u);
        const uint32_t* m = jump + (size_t)k * 800;
        for (uint32_t r = 0; r < reps; r++) {
            uint32_t o[5] = {0, 0, 0, 0, 0};
            for (int i = 0; i < 5; i++) {
                const uint32_t word = v[i];
                for (int j = 0; j < 32; j++) {
                    const uint32_t mask = 0u - ((word >> j) & 1u);
                    const uint32_t* row = m + i * 160 + j * 5;
                    o[0] ^= row[0] & mask;
                    o[1] ^= row[1] & mask;
                    o[2] ^= row[2] & mask;
                    o[3] ^= row[3] & mask;
                    o[4] ^= row[4] & mask;
                }
            }
            for (int w = 0; w < 5; w++) v[w] = o[w];
        }
    }
    rt_rng_state* out = states + s;
    out->d = st[0];
    for (int i = 0; i < 5; i++) out->v[i] = v[i];
    for (int i = 0; i < 6; i++) out->unused[i] = 0;
}

__global__ __launch_bounds__(BLOCK) void unshard_kernel(char* surface, uint64_t pitch, int width, int height,
                                                        int shard_count, const float4* shards, int64_t per_shard,
                                                        int tiles_x, const int32_t* __restrict__ tile_lists) {
    const int rank = blockIdx.y;
    const int64_t k = blockIdx.x;
    const int tile = tile_lists ? tile_lists[(size_t)rank * per_shard + k] : rank + (int)k * shard_count;
    int lx, ly;
    tile_pixel(threadIdx.x, &lx, &ly);
    const int x = (tile % tiles_x) * TILE + lx, y = (tile / tiles_x) * TILE + ly;
    if (tile < 0 || tile >= tiles_x * ((height + TILE - 1) / TILE) || x >= width || y >= height) return;
    const float4 v = shards[((size_t)rank * per_shard + k) * BLOCK + threadIdx.x];
    *reinterpret_cast<float4*>(surface + (size_t)y * pitch + (size_t)x * 16) = v;
}

}  // namespace

const uint32_t* rt_host::device_jump_table() {
    static std::mutex mu;
    static std::map<int, uint32_t*> per_device;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> lock(mu);
    auto it = per_device.find(dev);
    if (it != per_device.end()) return it->second;
    uint32_t* d = nullptr;
    const size_t bytes = (size_t)RT_XORWOW_JUMPS * 800 * 4;
    if (hipMalloc(&d, bytes) != hipSuccess) return nullptr;
    if (hipMemcpy(d, rt_xorwow_jump_table(), bytes, hipMemcpyHostToDevice) != hipSuccess) return nullptr;
    per_device[dev] = d;
    return d;
}

int rt_host::tiles_of_shard(int width, int height, int shard_index, int shard_count) {
    const int tiles = ((width + TILE - 1) / TILE) * ((height + TILE - 1) / TILE);
    if (shard_index >= tiles) return 0;
    return (tiles - shard_index + shard_count - 1) / shard_count;
}

extern "C" int64_t rt_shard_tiles(int width, int height, int shard_index, int shard_count) {
    if (width <= 0 || height <= 0 || shard_count <= 0 || shard_index < 0 || shard_index >= shard_count) return 0;
    return tiles_of_shard(width, height, shard_index, shard_count);
}

extern "C" int rt_init_rng(void* states, int width, int height, int shard_index, int shard_count, uint32_t seed,
                           void* stream) {
    const char* const who = "rt_init_rng";
    if (!states || width <= 0 || height <= 0 || shard_count <= 0 || shard_index < 0 || shard_index >= shard_count)
        return refuse(who, "bad arguments");
    const uint32_t* jump = device_jump_table();
    if (!jump) return refuse(who, "jump table upload failed");
    const int tiles_x = (width + TILE - 1) / TILE;
    int64_t count;
    int sc;
    if (shard_count == 1) {
        count = (int64_t)width * height;
        sc = 0;
    } else {
        count = (int64_t)tiles_of_shard(width, height, shard_index, shard_count) * BLOCK;
        sc = shard_count;
    }
    if (count == 0) return 0;
    if (bytes_from(states) < (size_t)count * sizeof(rt_rng_state)) return refuse(who, "rng_states too small");
    const int blocks = (int)((count + BLOCK - 1) / BLOCK);
    hipLaunchKernelGGL(init_rng_kernel, dim3(blocks), dim3(BLOCK), 0, (hipStream_t)stream, (rt_rng_state*)states, jump,
                       seed, count, width, height, shard_index, sc, tiles_x, (const int32_t*)nullptr);
    return check(hipGetLastError(), "init_rng_kernel launch");
}

extern "C" int rt_init_rng_tiles(void* states, int width, int height, const int32_t* tile_list, int64_t tile_count,
                                 uint32_t seed, void* stream) {
    const char* const who = "rt_init_rng_tiles";
    if (!states || !tile_list || width <= 0 || height <= 0 || tile_count <= 0 || tile_count > ((int64_t)1 << 28))
        return refuse(who, "bad arguments");
    const uint32_t* jump = device_jump_table();
    if (!jump) return refuse(who, "jump table upload failed");
    const int64_t count = tile_count * BLOCK;
    if (bytes_from(states) < (size_t)count * sizeof(rt_rng_state) || bytes_from(tile_list) < (size_t)tile_count * 4)
        return refuse(who, "rng_states or tile_list too small");
    hipLaunchKernelGGL(init_rng_kernel, dim3((unsigned)tile_count), dim3(BLOCK), 0, (hipStream_t)stream,
                       (rt_rng_state*)states, jump, seed, count, width, height, 0, 1, (width + TILE - 1) / TILE,
                       tile_list);
    return check(hipGetLastError(), "init_rng_kernel launch");
}

extern "C" int rt_unshard(void* surface, uint64_t pitch, int width, int height, int shard_count, const void* shards,
                          int64_t per_shard, void* stream) {
    const char* const who = "rt_unshard";
    if (!surface || !shards || shard_count <= 0 || per_shard <= 0 || width <= 0 || height <= 0)
        return refuse(who, "bad arguments");
    if (bytes_from(shards) < (size_t)shard_count * per_shard * BLOCK * 16 ||
        bytes_from(surface) < pitch * (size_t)(height - 1) + (size_t)width * 16)
        return refuse(who, "shards or surface too small");
    const int tiles_x = (width + TILE - 1) / TILE;
    hipLaunchKernelGGL(unshard_kernel, dim3((unsigned)per_shard, shard_count), dim3(BLOCK), 0, (hipStream_t)stream,
                       (char*)surface, pitch, width, height, shard_count, (const float4*)shards, per_shard, tiles_x,
                       (const int32_t*)nullptr);
    return check(hipGetLastError(), "unshard_kernel launch");
}

extern "C" int rt_unshard_tiles(void* surface, uint64_t pitch, int width, int height, int shard_count,
                                const void* shards, int64_t per_shard, const int32_t* tile_lists, void* stream) {
    const char* const who = "rt_unshard_tiles";
    if (!surface || !shards || !tile_lists || shard_count <= 0 || per_shard <= 0 || width <= 0 || height <= 0)
        return refuse(who, "bad arguments");
    if (bytes_from(shards) < (size_t)shard_count * per_shard * BLOCK * 16 ||
        bytes_from(tile_lists) < (size_t)shard_count * per_shard * 4 ||
        bytes_from(surface) < pitch * (size_t)(height - 1) + (size_t)width * 16)
        return refuse(who, "shards, tile_lists or surface too small");
    hipLaunchKernelGGL(unshard_kernel, dim3((unsigned)per_shard, shard_count), dim3(BLOCK), 0, (hipStream_t)stream,
                       (char*)surface, pitch, width, height, shard_count, (const float4*)shards, per_shard,
                       (width + TILE - 1) / TILE, tile_lists);
    return check(hipGetLastError(), "unshard_kernel launch");
}

// The reference's entry point (Random.cu): thread id == state index, on the null stream.
extern "C" void init_rng(uint32_t thread_block_count, uint32_t thread_block_size, void* states, unsigned int seed) {
    const uint32_t* jump = device_jump_table();
    const int64_t count = (int64_t)thread_block_count * thread_block_size;
    if (bytes_from(states) < (size_t)count * sizeof(rt_rng_state)) {
        set_error("init_rng: rngStates is smaller than thread_block_count * thread_block_size states");
        std::printf("(init_rng) failed: %s\n", rt_last_error());
        return;
    }
    if (!jump || count == 0) {
        set_error("init_rng: jump table upload failed");
        std::printf("(init_rng) failed: %s\n", rt_last_error());
        return;
    }
    hipLaunchKernelGGL(init_rng_kernel, dim3(thread_block_count), dim3(thread_block_size), 0, nullptr,
                       (rt_rng_state*)states, jump, seed, count, 0, 0, 0, 0, 0, (const int32_t*)nullptr);
    if (check(hipGetLastError(), "init_rng_kernel launch")) std::printf("(init_rng) failed: %s\n", rt_last_error());
}
