"""Python host binding of the MI355X ray tracer (librt_hip.so, C-ABI in include/rt_abi.h).

Mirrors the reference's host interface so a host written against it reads the same:

* ``Scene``      -- RayTracing::Scene (RayTracing/Scene.h:87-129): AddTriangle/AddQuad/
                    AddSphere/AddMaterial/AddLoadedScene, the camera, ``upload``.
* ``RayTracer``  -- CUDARayTracer (RayTracing/RayTracing.{h,cpp}): owns the scene, the
                    per-pixel RNG state and the progressive frame index; ``process()``
                    renders one frame (RayTracing.cpp:205-234).
* ``raytracing_process`` / ``init_rng`` -- the two extern "C" entry points
                    (main_raytracing.cu:202, Random.cu:10).

Device buffers are torch tensors on the current HIP device (torch is plumbing here: memory,
streams, torch.distributed); every kernel is in librt_hip.so.  There is no CPU fallback: if
the native library is missing or fails to load this module raises.

This file only re-exports the names of the private modules, each of which imports only from those before it: _abi,
_args, _scene, _render, _queries, _image, _adaptive, _tracer.
"""
from . import sharding
from ._abi import (ASSETS_DIR, DENOISE_DEFAULT, DENOISE_DEFAULTS, DENOISE_VARIANCE_DEFAULTS, EXP_LIB_PATH, HIT_MISS,
                   HIT_SPHERE, HIT_TRIANGLE, HITS_MAX, LIB_PATH, NEAREST_FACE, NEAREST_MISS, NEAREST_SPHERE, PKG_DIR,
                   RAY_TMAX, REFERENCE_BOUNCES, REFERENCE_SPP, REPROJECT_DEFAULT, REPROJECT_DEFAULTS, RNG_STATE_BYTES,
                   ROOT_DIR, RT_HITS_COUNT_ALL, RT_HITS_CULL_BACK, RT_HITS_CULL_FRONT, RT_RENDER_STATS,
                   RT_RENDER_VALIDATE, SAMPLE_SCALE_DEFAULT, SCENES, SIGNATURES, STAT_COUNT, STAT_NAMES, TRACERS,
                   UPSAMPLE_DEFAULT, UPSAMPLE_DEFAULTS, AoParams, BuildOptions, ClosestParams, DenoiseParams,
                   DenoiseVarianceParams, GPUCamera, GPUMaterial, GPUScene, Hit, HitsParams, MomentsParams, Nearest,
                   OcclusionParams, Point, RadianceParams, Ray, RenderParams, ReprojectParams, RTError,
                   SamplePixelsParams, SamplePlanParams, SamplePriorityParams, SampleResolveParams, TraceParams,
                   UpsampleParams, lib, load_experimental)
from ._adaptive import (AdaptiveSampler, sample_pixels, sample_plan, sample_plan_scratch_bytes, sample_priority,
                        sample_resolve)
from ._args import alloc_rng, alloc_surface, surface_view
from ._image import (TemporalAccumulator, VarianceAccumulator, camera_floats, denoise, denoise_raw, denoise_scratch_bytes,
                     denoise_variance, denoise_variance_raw, denoise_variance_scratch_bytes, moments, reproject_raw,
                     upsample, upsample_raw, upsample_scratch_bytes)
from ._queries import (CONTAINS_DIRECTIONS, ambient_occlusion, ao_directions, ao_scratch_bytes, closest_bound_host,
                       closest_points, closest_points_host, contains, distance_grid, gbuffer, hit_fields, hit_list_host,
                       nearest_fields, occluded, panorama, panorama_rays, radiance, ray_rng, signed_distance_grid,
                       trace_camera, trace_hits, trace_hits_camera, trace_rays)
from ._render import (Comm, init_rng, init_rng_states, init_rng_tiles, lane_plan, lane_refine, lone_plan,
                      raytracing_process, render, shard_plan, shard_tiles, tiles_of, tonemap, unshard, unshard_tiles,
                      write_pfm, write_ppm)
from ._scene import (Scene, build_options, bvh_build_device, cluster_cull_host, entry_table_builds, foreign_last_tracer,
                     foreign_mirror_wait, mirror_build_check, set_build_options)
from ._tracer import RayTracer

# the private names the tests reach for
from ._abi import _check  # isort: skip
from ._args import _as_camera, _scene_ptr  # isort: skip
from ._queries import _ao_default_directions  # isort: skip
