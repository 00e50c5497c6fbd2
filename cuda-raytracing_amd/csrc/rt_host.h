// rt_host.h -- what the host units behind the C-ABI of include/rt_abi.h share, each defined once in the unit named:
// declarations only.  How a call words a refusal is image_entry.h's (rt_entry::refuse, "who: what", return value 1).
#pragma once

#include <hip/hip_runtime.h>

#include <string>

#include "mirror.h"
#include "rt_common.h"

namespace rt_host {

// rt_kernel.hip -- the last error of this thread (rt_last_error): set_error returns `code`; check returns 0 for
// hipSuccess, else sets "what: <HIP's text>" and returns the HIP error code
int set_error(const std::string& msg, int code = 1);
int check(hipError_t e, const char* what);
// bytes of the device allocation holding p from p to its end (0 if p is not device memory)
size_t bytes_from(const void* p);
// a BVH deeper than the largest traversal stack holds (rt_variant.h kMaxBvhDepth) reaches no kernel: `who` refuses it
bool depth_refused(const char* who, int depth);
// edge length of a cube map made by rt_cubemap_create, -1 for any other handle
int cube_size(uint64_t handle);
// the sky of a launch of `who` (rt_render, rt_radiance, rt_sample_pixels): the scene's cube map, if it has one, and
// the sky rotation
int fill_sky(const char* who, const GPUScene* scene, rtk::RenderArgs* a);

// rng_shard.hip -- tiles of the round-robin deal's shard; this device's copy of the XORWOW jump matrices (null: failed)
int tiles_of_shard(int width, int height, int shard_index, int shard_count);
const uint32_t* device_jump_table();

// entry_table.hip -- the camera rays' entry records for this frame's camera and viewport, rebuilt on `s` when they
// changed; null (and the frame starts every ray at the root) when the table cannot be had
const uint32_t* entry_table(const MirrorDevice& mir, const GPUCamera& c, int width, int height, hipStream_t s);

// foreign.hip -- per frame for a GPUScene another host filled: install a finished rebuild, enqueue the fingerprint
// gate, start a rebuild when the arrays no longer match.  *mir receives the installed mirror (if *have); *gate the
// device flag the two launches are gated on
int foreign_frame(const GPUScene* scene, hipStream_t st, MirrorDevice* mir, bool* have, int** gate);

}  // namespace rt_host
