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
"""
import contextlib
import ctypes
import os

import numpy as np
import torch  # imported before the library so librt_hip.so binds to the HIP runtime torch already loaded

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
ROOT_DIR = os.path.dirname(PKG_DIR)
LIB_PATH = os.path.join(PKG_DIR, "librt_hip.so")
EXP_LIB_PATH = os.path.join(PKG_DIR, "librt_hip_exp.so")  # experimental render paths (A/B + their tests)
ASSETS_DIR = os.path.join(ROOT_DIR, "assets")

RT_RENDER_STATS = 1
RT_RENDER_VALIDATE = 16
TRACERS = {"fast": 0, "ref": 2, "flat": 4, "wavefront": 8}  # rt_render_params.flags
STAT_NAMES = ("segments", "nodes", "tri_tests", "tri_accepts", "sphere_accepts", "hits", "misses", "cycles_tree_cut",
              "wave_small_iters", "lane_small", "wave_big_tris", "lane_big_tris", "wave_segment_iters",
              "lane_segments", "tree_nodes", "tree_tri_tests", "cycles_small", "cycles_big", "cycles_total",
              "rounds_coop", "rounds_shared", "coop_rays", "cycles_tree_clusters", "cycles_tree_tris",
              "big_tests", "twin_decided", "twin_tests", "wave_big_iters", "defer_end2", "defer_redo", None, None)
STAT_COUNT = len(STAT_NAMES)  # RT_STAT_COUNT (include/rt_abi.h): per-wave records of RT_TUNE bit 11 follow
SCENES = {"bunny": 0, "bunny4": 1, "plane1m": 2}

REFERENCE_SPP = 5      # main_raytracing.cu:166-170 (Release)
REFERENCE_BOUNCES = 6  # main_raytracing.cu:115
RNG_STATE_BYTES = 48   # sizeof(curandState)


class GPUCamera(ctypes.Structure):
    _fields_ = [("origin", ctypes.c_float * 3), ("viewport_worldspace_size", ctypes.c_float * 2),
                ("aspect", ctypes.c_float), ("horizontal", ctypes.c_float * 3),
                ("vertical", ctypes.c_float * 3), ("lower_left_corner", ctypes.c_float * 3)]


class GPUScene(ctypes.Structure):
    _fields_ = [("gpu_spheres", ctypes.c_void_p), ("gpu_materials", ctypes.c_void_p),
                ("gpu_bvh_nodes", ctypes.c_void_p), ("gpu_bvh_face_indices", ctypes.c_void_p),
                ("gpu_vertices", ctypes.c_void_p), ("gpu_faces", ctypes.c_void_p),
                ("sphere_count", ctypes.c_int32), ("material_count", ctypes.c_int32),
                ("rng_state", ctypes.c_void_p), ("environment_cubemap_tex", ctypes.c_uint64),
                ("camera", GPUCamera)]


class GPUMaterial(ctypes.Structure):
    _fields_ = [("albedo", ctypes.c_float * 4), ("emissive", ctypes.c_float * 4), ("specular", ctypes.c_float * 4),
                ("roughness", ctypes.c_float), ("specular_percent", ctypes.c_float), ("IOR", ctypes.c_float),
                ("_pad", ctypes.c_float)]


class BuildOptions(ctypes.Structure):
    """rt_build_options (rt_abi.h): exact-preserving speed knobs of the mirror / BVH builders."""
    _fields_ = [("leaf_tree_min", ctypes.c_uint32), ("cut_clusters", ctypes.c_uint32), ("cluster_max", ctypes.c_uint32),
                ("split_angle", ctypes.c_float), ("bvh_small", ctypes.c_uint32), ("host_bvh", ctypes.c_int32),
                ("leaf_screens", ctypes.c_int32), ("entry_frontier", ctypes.c_int32)]


class RenderParams(ctypes.Structure):
    _fields_ = [("surface", ctypes.c_void_p), ("surface_last_frame", ctypes.c_void_p),
                ("width", ctypes.c_int32), ("height", ctypes.c_int32), ("pitch", ctypes.c_uint64),
                ("frame_index", ctypes.c_int32), ("spp", ctypes.c_int32), ("bounces", ctypes.c_int32),
                ("shard_index", ctypes.c_int32), ("shard_count", ctypes.c_int32), ("flags", ctypes.c_int32),
                ("out_shard", ctypes.c_void_p), ("stats", ctypes.c_void_p), ("segment_counter", ctypes.c_void_p),
                ("tile_list", ctypes.c_void_p), ("tile_count", ctypes.c_int64), ("wave_clock", ctypes.c_void_p),
                ("tune", ctypes.c_uint32), ("lane_slots", ctypes.c_void_p), ("lane_slot_count", ctypes.c_int64),
                ("lane_cost", ctypes.c_void_p), ("priority_waves", ctypes.c_int64), ("refill_lanes", ctypes.c_int32),
                ("waves_per_simd", ctypes.c_int32), ("lone_slots", ctypes.c_void_p), ("lone_count", ctypes.c_int64)]


class Ray(ctypes.Structure):
    """rt_ray (rt_abi.h): one row of a float32 [N, 8] ray tensor."""
    _fields_ = [("origin", ctypes.c_float * 3), ("tmax", ctypes.c_float), ("direction", ctypes.c_float * 3),
                ("reserved", ctypes.c_uint32)]


class Hit(ctypes.Structure):
    """rt_hit (rt_abi.h): one row of a float32 [N, 12] hit tensor (hit_fields gives typed views)."""
    _fields_ = [("t", ctypes.c_float), ("kind", ctypes.c_uint32), ("id", ctypes.c_uint32), ("material", ctypes.c_uint32),
                ("normal", ctypes.c_float * 3), ("bx", ctypes.c_float), ("position", ctypes.c_float * 3),
                ("by", ctypes.c_float)]


class TraceParams(ctypes.Structure):
    _fields_ = [("rays", ctypes.c_void_p), ("count", ctypes.c_int64), ("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("hits", ctypes.c_void_p), ("flags", ctypes.c_uint32), ("waves_per_simd", ctypes.c_int32)]


class OcclusionParams(ctypes.Structure):
    """rt_occlusion_params (rt_abi.h)."""
    _fields_ = [("rays", ctypes.c_void_p), ("count", ctypes.c_int64), ("occluded", ctypes.c_void_p),
                ("flags", ctypes.c_uint32), ("waves_per_simd", ctypes.c_int32)]


class Point(ctypes.Structure):
    """rt_point (rt_abi.h): one row of a float32 [N, 4] point tensor."""
    _fields_ = [("position", ctypes.c_float * 3), ("radius", ctypes.c_float)]


class Nearest(ctypes.Structure):
    """rt_nearest (rt_abi.h): one row of a float32 [N, 8] record tensor (nearest_fields gives typed views)."""
    _fields_ = [("distance", ctypes.c_float), ("kind", ctypes.c_uint32), ("id", ctypes.c_uint32),
                ("material", ctypes.c_uint32), ("point", ctypes.c_float * 3), ("region", ctypes.c_uint32)]


class ClosestParams(ctypes.Structure):
    """rt_closest_params (rt_abi.h)."""
    _fields_ = [("points", ctypes.c_void_p), ("count", ctypes.c_int64), ("nearest", ctypes.c_void_p),
                ("flags", ctypes.c_uint32), ("waves_per_simd", ctypes.c_int32)]


class HitsParams(ctypes.Structure):
    """rt_hits_params (rt_abi.h)."""
    _fields_ = [("rays", ctypes.c_void_p), ("count", ctypes.c_int64), ("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("hits", ctypes.c_void_p), ("counts", ctypes.c_void_p), ("max_hits", ctypes.c_int32), ("flags", ctypes.c_uint32),
                ("waves_per_simd", ctypes.c_int32), ("reserved", ctypes.c_uint32)]


class AoParams(ctypes.Structure):
    """rt_ao_params (rt_abi.h)."""
    _fields_ = [("hits", ctypes.c_void_p), ("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("directions", ctypes.c_void_p), ("direction_count", ctypes.c_int32), ("samples", ctypes.c_int32),
                ("radius", ctypes.c_float), ("bias", ctypes.c_float), ("ao", ctypes.c_void_p), ("scratch", ctypes.c_void_p),
                ("scratch_bytes", ctypes.c_uint64), ("flags", ctypes.c_uint32), ("waves_per_simd", ctypes.c_int32)]


class RadianceParams(ctypes.Structure):
    """rt_radiance_params (rt_abi.h)."""
    _fields_ = [("rays", ctypes.c_void_p), ("count", ctypes.c_int64), ("rng", ctypes.c_void_p), ("radiance", ctypes.c_void_p),
                ("bounces", ctypes.c_int32), ("samples", ctypes.c_int32), ("flags", ctypes.c_uint32),
                ("waves_per_simd", ctypes.c_int32)]


class DenoiseParams(ctypes.Structure):
    """rt_denoise_params (rt_abi.h)."""
    _fields_ = [("surface", ctypes.c_void_p), ("pitch", ctypes.c_uint64), ("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("hits", ctypes.c_void_p), ("materials", ctypes.c_void_p), ("material_count", ctypes.c_int32),
                ("flags", ctypes.c_int32), ("out", ctypes.c_void_p), ("out_pitch", ctypes.c_uint64),
                ("scratch", ctypes.c_void_p), ("scratch_bytes", ctypes.c_uint64), ("iterations", ctypes.c_int32),
                ("normal_power_log2", ctypes.c_int32), ("sigma_plane", ctypes.c_float), ("sigma_color", ctypes.c_float)]


class ReprojectParams(ctypes.Structure):
    """rt_reproject_params (rt_abi.h)."""
    _fields_ = [("surface", ctypes.c_void_p), ("pitch", ctypes.c_uint64), ("hits", ctypes.c_void_p),
                ("prev_surface", ctypes.c_void_p), ("prev_pitch", ctypes.c_uint64), ("prev_hits", ctypes.c_void_p),
                ("prev_history", ctypes.c_void_p), ("out", ctypes.c_void_p), ("out_pitch", ctypes.c_uint64),
                ("out_history", ctypes.c_void_p), ("camera", GPUCamera), ("prev_camera", GPUCamera),
                ("width", ctypes.c_int32), ("height", ctypes.c_int32), ("max_history", ctypes.c_int32),
                ("sigma_plane", ctypes.c_float), ("normal_min", ctypes.c_float), ("flags", ctypes.c_int32)]


class MomentsParams(ctypes.Structure):
    """rt_moments_params (rt_abi.h)."""
    _fields_ = [("surface", ctypes.c_void_p), ("pitch", ctypes.c_uint64), ("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("hits", ctypes.c_void_p), ("materials", ctypes.c_void_p), ("material_count", ctypes.c_int32),
                ("flags", ctypes.c_int32), ("out", ctypes.c_void_p), ("out_pitch", ctypes.c_uint64)]


class DenoiseVarianceParams(ctypes.Structure):
    """rt_denoise_variance_params (rt_abi.h)."""
    _fields_ = [("surface", ctypes.c_void_p), ("pitch", ctypes.c_uint64), ("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("hits", ctypes.c_void_p), ("materials", ctypes.c_void_p), ("material_count", ctypes.c_int32),
                ("flags", ctypes.c_int32), ("moments", ctypes.c_void_p), ("moments_pitch", ctypes.c_uint64),
                ("history", ctypes.c_void_p), ("out", ctypes.c_void_p), ("out_pitch", ctypes.c_uint64),
                ("out_variance", ctypes.c_void_p), ("scratch", ctypes.c_void_p), ("scratch_bytes", ctypes.c_uint64),
                ("iterations", ctypes.c_int32), ("normal_power_log2", ctypes.c_int32), ("sigma_plane", ctypes.c_float),
                ("sigma_lum", ctypes.c_float), ("min_history", ctypes.c_float), ("reserved", ctypes.c_int32)]


class UpsampleParams(ctypes.Structure):
    """rt_upsample_params (rt_abi.h)."""
    _fields_ = [("low_surface", ctypes.c_void_p), ("low_pitch", ctypes.c_uint64), ("low_hits", ctypes.c_void_p),
                ("low_width", ctypes.c_int32), ("low_height", ctypes.c_int32), ("scale", ctypes.c_int32),
                ("material_count", ctypes.c_int32), ("hits", ctypes.c_void_p), ("materials", ctypes.c_void_p),
                ("out", ctypes.c_void_p), ("out_pitch", ctypes.c_uint64), ("scratch", ctypes.c_void_p),
                ("scratch_bytes", ctypes.c_uint64), ("normal_power_log2", ctypes.c_int32), ("sigma_plane", ctypes.c_float),
                ("flags", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class SamplePixelsParams(ctypes.Structure):
    """rt_sample_pixels_params (rt_abi.h)."""
    _fields_ = [("pixels", ctypes.c_void_p), ("samples", ctypes.c_void_p), ("count", ctypes.c_int64), ("rng", ctypes.c_void_p),
                ("accum", ctypes.c_void_p), ("accum_pitch", ctypes.c_uint64), ("moments", ctypes.c_void_p),
                ("width", ctypes.c_int32), ("height", ctypes.c_int32), ("bounces", ctypes.c_int32), ("flags", ctypes.c_uint32),
                ("waves_per_simd", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class SamplePriorityParams(ctypes.Structure):
    """rt_sample_priority_params (rt_abi.h)."""
    _fields_ = [("accum", ctypes.c_void_p), ("accum_pitch", ctypes.c_uint64), ("moments", ctypes.c_void_p),
                ("priority", ctypes.c_void_p), ("width", ctypes.c_int32), ("height", ctypes.c_int32)]


class SamplePlanParams(ctypes.Structure):
    """rt_sample_plan_params (rt_abi.h)."""
    _fields_ = [("priority", ctypes.c_void_p), ("width", ctypes.c_int32), ("height", ctypes.c_int32), ("budget", ctypes.c_int64),
                ("min_samples", ctypes.c_int32), ("max_samples", ctypes.c_int32), ("scale", ctypes.c_float),
                ("reserved", ctypes.c_int32), ("pixels", ctypes.c_void_p), ("samples", ctypes.c_void_p),
                ("total", ctypes.c_void_p), ("scratch", ctypes.c_void_p), ("scratch_bytes", ctypes.c_uint64)]


class SampleResolveParams(ctypes.Structure):
    """rt_sample_resolve_params (rt_abi.h)."""
    _fields_ = [("accum", ctypes.c_void_p), ("accum_pitch", ctypes.c_uint64), ("out", ctypes.c_void_p),
                ("out_pitch", ctypes.c_uint64), ("width", ctypes.c_int32), ("height", ctypes.c_int32)]


assert ctypes.sizeof(SamplePixelsParams) == 80 and ctypes.sizeof(SamplePriorityParams) == 40
assert ctypes.sizeof(SamplePlanParams) == 80 and ctypes.sizeof(SampleResolveParams) == 40
# AdaptiveSampler.step's scale: priorities are relative variances of the mean, quantised to 0..65535 after the
# scaling.  The best point of profiles/adaptive_quality.txt's grid (tools/adaptive_quality.py) on both of its scenes:
# 2^28 saturates every pixel whose relative variance is above 2^-12, so a round is shared almost evenly among the
# pixels that have not converged, and the few below that get in proportion less.
SAMPLE_SCALE_DEFAULT = 268435456.0

HIT_MISS, HIT_SPHERE, HIT_TRIANGLE = 0, 1, 2  # rt_hit.kind
RAY_TMAX = 1e30  # the renderer's own initial closest distance (main_raytracing.cu:85)
DENOISE_DEFAULT = -1  # RT_DENOISE_DEFAULT: in a filter parameter of rt_denoise, the measured default
# the defaults rt_denoise substitutes (csrc/denoise.hip; profiles/denoise_quality.txt)
DENOISE_DEFAULTS = {"iterations": 5, "normal_power_log2": 5, "sigma_plane": 0.03, "sigma_color": 8.0}

assert ctypes.sizeof(GPUScene) == 136 and ctypes.sizeof(GPUMaterial) == 64
assert ctypes.sizeof(Ray) == 32 and ctypes.sizeof(Hit) == 48 and ctypes.sizeof(TraceParams) == 40
assert ctypes.sizeof(DenoiseParams) == 96 and ctypes.sizeof(OcclusionParams) == 32 and ctypes.sizeof(AoParams) == 72
REPROJECT_DEFAULT = -1  # RT_REPROJECT_DEFAULT: in a filter parameter of rt_reproject, the measured default
# the defaults rt_reproject substitutes (csrc/reproject.hip; profiles/reproject_quality.txt)
REPROJECT_DEFAULTS = {"max_history": 32, "sigma_plane": 0.03, "normal_min": 0.9}
assert ctypes.sizeof(ReprojectParams) == 224 and ctypes.sizeof(GPUCamera) == 60
assert ctypes.sizeof(RadianceParams) == 48
assert ctypes.sizeof(Point) == 16 and ctypes.sizeof(Nearest) == 32 and ctypes.sizeof(ClosestParams) == 32
# the defaults rt_denoise_variance substitutes (csrc/denoise_variance.hip; profiles/variance_quality.txt)
DENOISE_VARIANCE_DEFAULTS = {"iterations": 5, "normal_power_log2": 5, "sigma_plane": 0.03, "sigma_lum": 4.0, "min_history": 4.0}
assert ctypes.sizeof(MomentsParams) == 64 and ctypes.sizeof(DenoiseVarianceParams) == 136
UPSAMPLE_DEFAULT = -1  # RT_UPSAMPLE_DEFAULT: in a filter parameter of rt_upsample, the measured default
# the defaults rt_upsample substitutes (csrc/upsample.hip; profiles/upsample_quality.txt)
UPSAMPLE_DEFAULTS = {"normal_power_log2": 0, "sigma_plane": 0.03}
assert ctypes.sizeof(UpsampleParams) == 104

# name -> (restype, argtypes); every symbol include/rt_abi.h declares.
_P, _I, _U32, _U64, _F, _SZ = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_float, ctypes.c_size_t
_FP = ctypes.POINTER(ctypes.c_float)
SIGNATURES = {
    "raytracing_process": (None, [_P, _P, _I, _I, _SZ, _I, _P]),
    "init_rng": (None, [_U32, _U32, _P, ctypes.c_uint]),
    "rt_render": (_I, [ctypes.POINTER(RenderParams), _P, _P]),
    "rt_trace_rays": (_I, [ctypes.POINTER(TraceParams), _P, _P]),
    "rt_occluded": (_I, [ctypes.POINTER(OcclusionParams), _P, _P]),
    "rt_closest_point": (_I, [ctypes.POINTER(ClosestParams), _P, _P]),
    "rt_closest_point_host": (_I, [_P, _P, ctypes.c_int64, _P]),
    "rt_closest_bound_host": (_F, [_P, _P, _P]),
    "rt_trace_hits": (_I, [ctypes.POINTER(HitsParams), _P, _P]),
    "rt_hit_list_host": (_I, [_I, _F, _I, ctypes.c_int64, _P, _P, _P, _P, ctypes.POINTER(ctypes.c_int64)]),
    "rt_ao_scratch_bytes": (_SZ, [_I, _I, _I]),
    "rt_ao": (_I, [ctypes.POINTER(AoParams), _P, _P]),
    "rt_radiance": (_I, [ctypes.POINTER(RadianceParams), _P, _P]),
    "rt_denoise_scratch_bytes": (_SZ, [_I, _I]),
    "rt_denoise": (_I, [ctypes.POINTER(DenoiseParams), _P]),
    "rt_reproject": (_I, [ctypes.POINTER(ReprojectParams), _P]),
    "rt_moments": (_I, [ctypes.POINTER(MomentsParams), _P]),
    "rt_denoise_variance_scratch_bytes": (_SZ, [_I, _I]),
    "rt_denoise_variance": (_I, [ctypes.POINTER(DenoiseVarianceParams), _P]),
    "rt_upsample_scratch_bytes": (_SZ, [_I, _I]),
    "rt_upsample": (_I, [ctypes.POINTER(UpsampleParams), _P]),
    "rt_sample_pixels": (_I, [ctypes.POINTER(SamplePixelsParams), _P, _P]),
    "rt_sample_priority": (_I, [ctypes.POINTER(SamplePriorityParams), _P]),
    "rt_sample_plan_scratch_bytes": (_SZ, [_I, _I]),
    "rt_sample_plan": (_I, [ctypes.POINTER(SamplePlanParams), _P]),
    "rt_sample_resolve": (_I, [ctypes.POINTER(SampleResolveParams), _P]),
    "rt_foreign_mirror_wait": (_I, [_P]),
    "rt_foreign_last_tracer": (_I, [_P]),
    "rt_experimental_loaded": (_I, []),
    "rt_init_rng": (_I, [_P, _I, _I, _I, _I, _U32, _P]),
    "rt_shard_tiles": (ctypes.c_int64, [_I, _I, _I, _I]),
    "rt_unshard": (_I, [_P, _U64, _I, _I, _I, _P, ctypes.c_int64, _P]),
    "rt_shard_plan_capacity": (ctypes.c_int64, [_I, _I, _I]),
    "rt_shard_plan": (_I, [_I, _I, _I, _P, ctypes.c_int64, _P, _P]),
    "rt_entry_table_builds": (_U64, []),
    "rt_get_build_options": (None, [_P]),
    "rt_set_build_options": (_I, [_P]),
    "rt_lane_plan_capacity": (ctypes.c_int64, [ctypes.c_int64]),
    "rt_lane_plan": (ctypes.c_int64, [_P, ctypes.c_int64, ctypes.c_double, ctypes.c_double, _P, ctypes.c_int64, _P]),
    "rt_lone_plan": (ctypes.c_int64, [_P, ctypes.c_int64, ctypes.c_int64, _U32, _P]),
    "rt_lane_refine": (ctypes.c_int64, [_P, ctypes.c_int64, _P, ctypes.c_int64, _P, ctypes.c_double, _P, ctypes.c_int64,
                                        _P]),
    "rt_init_rng_tiles": (_I, [_P, _I, _I, _P, ctypes.c_int64, _U32, _P]),
    "rt_unshard_tiles": (_I, [_P, _U64, _I, _I, _I, _P, ctypes.c_int64, _P, _P]),
    "rt_comm_unique_id": (_I, [_P]),
    "rt_comm_init_rank": (_I, [ctypes.POINTER(_P), _I, _I, _P]),
    "rt_comm_init_all": (_I, [_P, _I, _P]),
    "rt_comm_destroy": (_I, [_P]),
    "rt_comm_rank": (_I, [_P]),
    "rt_comm_size": (_I, [_P]),
    "rt_comm_group_start": (_I, []),
    "rt_comm_group_end": (_I, []),
    "rt_gather_shards": (_I, [_P, _P, _SZ, _P, _SZ, _P, _I, _P]),
    "rt_tonemap_srgb8": (_I, [_P, _U64, _I, _I, _P, _P]),
    "rt_write_pfm": (_I, [ctypes.c_char_p, _P, _U64, _I, _I]),
    "rt_write_ppm": (_I, [ctypes.c_char_p, _P, _I, _I]),
    "rt_set_device": (_I, [_I]),
    "rt_device_count": (_I, []),
    "rt_malloc": (_I, [ctypes.POINTER(_P), _SZ]),
    "rt_malloc_pitch": (_I, [ctypes.POINTER(_P), ctypes.POINTER(_SZ), _SZ, _SZ]),
    "rt_free": (_I, [_P]),
    "rt_memcpy_h2d": (_I, [_P, _P, _SZ]),
    "rt_memcpy_d2h": (_I, [_P, _P, _SZ]),
    "rt_memcpy_d2d": (_I, [_P, _P, _SZ]),
    "rt_memset": (_I, [_P, _I, _SZ]),
    "rt_synchronize": (_I, []),
    "rt_last_error": (ctypes.c_char_p, []),
    "rt_cubemap_create": (_U64, [_FP, _I]),
    "rt_cubemap_destroy": (_I, [_U64]),
    "rt_scene_create": (_P, []),
    "rt_scene_destroy": (None, [_P]),
    "rt_scene_add_material": (_U32, [_P, ctypes.POINTER(GPUMaterial)]),
    "rt_scene_add_triangle": (None, [_P, _FP, _FP, _FP, _I]),
    "rt_scene_add_quad": (None, [_P, _FP, _FP, _FP, _FP, _I]),
    "rt_scene_add_sphere": (None, [_P, _FP, _F, _I]),
    "rt_scene_add_mesh_file": (_I, [_P, ctypes.c_char_p, _FP, _I]),
    "rt_scene_set_environment_file": (_I, [_P, ctypes.c_char_p]),
    "rt_scene_environment": (_I, [_P, ctypes.POINTER(_P), ctypes.POINTER(_I)]),
    "rt_scene_set_camera": (None, [_P, _FP, _F, _F]),
    "rt_scene_set_viewport": (None, [_P, _I, _I]),
    "rt_scene_upload": (_I, [_P, _P]),
    "rt_scene_gpu": (ctypes.POINTER(GPUScene), [_P]),
    "rt_scene_setup": (_I, [_P, _I, ctypes.c_char_p]),
    "rt_scene_setup_plane": (_I, [_P, _I, ctypes.c_char_p]),
    "rt_scene_build": (None, [_P]),
    "rt_scene_camera": (None, [_P, ctypes.POINTER(GPUCamera)]),
    "rt_scene_host_arrays": (_SZ, [_P, ctypes.POINTER(_P), ctypes.POINTER(_SZ), ctypes.POINTER(_P),
                                   ctypes.POINTER(_SZ), ctypes.POINTER(_P), ctypes.POINTER(_SZ), ctypes.POINTER(_P)]),
    "rt_scene_bvh_max_depth": (_I, [_P]),
    "rt_scene_materials": (_I, [_P, _P, ctypes.POINTER(_SZ)]),
    "rt_scene_spheres": (_I, [_P, _P, ctypes.POINTER(_SZ)]),
    "rt_bvh_build_device": (_I, [_P, _U32, _P, _U32, _P, _P, ctypes.POINTER(_U32), ctypes.POINTER(_I), _P]),
    "rt_scene_mirror_info": (_I, [_P, ctypes.POINTER(_SZ), ctypes.POINTER(_SZ), ctypes.POINTER(_SZ)]),
    "rt_scene_mirror_copy": (_I, [_P, _P, _P, _P]),
    "rt_scene_mirror_nodes": (_I, [_P, _P, ctypes.POINTER(_SZ)]),
    "rt_scene_mirror_face_leaf": (_I, [_P, _P, ctypes.POINTER(_SZ)]),
    "rt_scene_mirror_twins": (_I, [_P, _P, ctypes.POINTER(_SZ), _P, ctypes.POINTER(_SZ)]),
    "rt_mirror_build_check": (_I, [_P, _SZ, _P, _SZ, _P, _SZ, _P, _SZ, _P, ctypes.POINTER(ctypes.c_int)]),
    "rt_cluster_cull_host": (_I, [_P, _P, ctypes.c_float, _P]),
    "rt_twin_check_host": (_I, [_P, _P, _P]),
    "rt_twin_check_bounds_host": (_I, [_P, _P, _P, _P]),
    "rt_twin_visit_host": (None, [_P, _P, _P, ctypes.c_float, _P]),
    "rt_scene_mirror_leaf_twin": (_I, [_P, _U32, _P]),
    "rt_variant_host": (None, [_P, _P]),
    "rt_family_has_mode_host": (_I, [_I, _I]),
    "rt_xorwow_jump_matrix": (_I, [_I, ctypes.POINTER(ctypes.c_uint32)]),
    "rt_xorwow_init_host": (None, [_U32, _U64, _P]),
}

_lib = None


class RTError(RuntimeError):
    pass


def lib():
    """Load librt_hip.so (raises if it is missing: there is no fallback path)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RTError(f"{LIB_PATH} not built; run `python -c 'import __graft_entry__ as g; g.build()'`")
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


_exp_lib = None


def load_experimental():
    """Load librt_hip_exp.so: registers the exact alternatives kept for A/B measurement -- the
    wavefront tracer, refill, the lone-pixel kernel and the RT_TUNE A/B kernel variants -- with
    librt_hip.so, whose rt_render refuses them otherwise.  The benchmark's production path never
    needs it."""
    global _exp_lib
    lib()
    if _exp_lib is None:
        if not os.path.exists(EXP_LIB_PATH):
            raise RTError(f"{EXP_LIB_PATH} not built; run `python -c 'import __graft_entry__ as g; g.build()'`")
        _exp_lib = ctypes.CDLL(EXP_LIB_PATH)
    if lib().rt_experimental_loaded() != 1:
        raise RTError("librt_hip_exp.so loaded but its kernels are not registered with librt_hip.so: "
                      + lib().rt_last_error().decode(errors="replace"))
    return _exp_lib


def _check(code, what):
    if code:
        raise RTError(f"{what} failed ({code}): {lib().rt_last_error().decode(errors='replace')}")


def _f3(v):
    return (ctypes.c_float * 3)(*[float(x) for x in v])


def _stream_ptr(stream=None):
    s = stream if stream is not None else torch.cuda.current_stream()
    return ctypes.c_void_p(s.cuda_stream)


def _scene_ptr(scene):
    """The GPUScene* of a Scene, or of a GPUScene filled by the caller."""
    return ctypes.cast(scene.gpu if hasattr(scene, "gpu") else ctypes.pointer(scene), ctypes.c_void_p)


def _is_rays(t):
    """A float32 CUDA tensor [N, 8] of rt_ray rows."""
    return t.dtype == torch.float32 and t.is_cuda and t.is_contiguous() and t.dim() == 2 and t.shape[1] == 8


class Scene:
    """RayTracing::Scene mirror (RayTracing/Scene.h:87-129)."""

    def __init__(self):
        self.handle = lib().rt_scene_create()
        if not self.handle:
            raise RTError("rt_scene_create failed")

    def __del__(self):
        if getattr(self, "handle", None) and _lib is not None:
            _lib.rt_scene_destroy(self.handle)
            self.handle = None

    # --- building (Scene.cpp:46-139) -------------------------------------------------
    def add_material(self, albedo=(0, 0, 0), emissive=(0, 0, 0), specular=(0, 0, 0, 0), roughness=0.9,
                     specular_percent=0.0, ior=1.0):
        m = GPUMaterial()
        m.albedo[:] = [*map(float, albedo[:3]), 1.0]
        m.emissive[:] = [*map(float, emissive[:3]), 1.0]
        m.specular[:] = [*map(float, (list(specular) + [0.0])[:4])]
        m.roughness, m.specular_percent, m.IOR = roughness, specular_percent, ior
        return lib().rt_scene_add_material(self.handle, ctypes.byref(m))

    def add_triangle(self, a, b, c, material=0):
        lib().rt_scene_add_triangle(self.handle, _f3(a), _f3(b), _f3(c), material)

    def add_quad(self, a, b, c, d, material=0):
        lib().rt_scene_add_quad(self.handle, _f3(a), _f3(b), _f3(c), _f3(d), material)

    def add_sphere(self, position, radius, material=0):
        lib().rt_scene_add_sphere(self.handle, _f3(position), float(radius), material)

    def add_loaded_scene(self, mesh_path, transform, material=0):
        t = (ctypes.c_float * 16)(*[float(x) for x in transform])
        _check(lib().rt_scene_add_mesh_file(self.handle, mesh_path.encode(), t, material), "add_loaded_scene")

    def set_environment(self, path):
        _check(lib().rt_scene_set_environment_file(self.handle, path.encode()), "set_environment")

    def environment(self):
        """Host copy of the level-0 cube texels [6, size, size, 4] (None when no sky is set)."""
        p, n = ctypes.c_void_p(), ctypes.c_int()
        _check(lib().rt_scene_environment(self.handle, ctypes.byref(p), ctypes.byref(n)), "rt_scene_environment")
        if not p.value:
            return None
        k = n.value
        buf = ctypes.string_at(p.value, 6 * k * k * 16)
        return np.frombuffer(buf, dtype=np.float32).reshape(6, k, k, 4).copy()

    def setup(self, which="bunny", assets_dir=ASSETS_DIR):
        """CUDARayTracer::SetupCornellBox + SetupStanfordBunny (or the config-4/5 scenes)."""
        _check(lib().rt_scene_setup(self.handle, SCENES[which], assets_dir.encode()), f"setup({which})")

    def setup_plane(self, n=708, assets_dir=ASSETS_DIR):
        _check(lib().rt_scene_setup_plane(self.handle, int(n), assets_dir.encode()), f"setup_plane({n})")

    def set_camera(self, position=(0, 0, 0), angle_x=0.0, angle_y=180.0):
        lib().rt_scene_set_camera(self.handle, _f3(position), float(angle_x), float(angle_y))

    def set_viewport(self, width, height):
        lib().rt_scene_set_viewport(self.handle, int(width), int(height))

    def upload(self, rng_state_ptr):
        """Scene::Upload (Scene.cpp:182-234): BVH build if dirty, H2D copies, GPUScene fill."""
        _check(lib().rt_scene_upload(self.handle, ctypes.c_void_p(rng_state_ptr)), "upload")

    @property
    def gpu(self):
        return lib().rt_scene_gpu(self.handle)

    def build(self):
        """Host half of upload (camera + BVH) with no device work."""
        lib().rt_scene_build(self.handle)

    def camera(self):
        c = GPUCamera()
        lib().rt_scene_camera(self.handle, ctypes.byref(c))
        return c

    def max_depth(self):
        return lib().rt_scene_bvh_max_depth(self.handle)

    def mirror(self, trees=False):
        """The kernel's triangle mirror built on the host (mirror.h): leaf-ordered (N,12) float32
        records (v0, e1, e2, face id bits, pair/tree index, flag); with trees=True also the leaf
        trees: nodes (K,16) and their triangle records (M,12) (leaftree.h)."""
        import numpy as np
        n = [ctypes.c_size_t() for _ in range(3)]
        _check(lib().rt_scene_mirror_info(self.handle, *[ctypes.byref(x) for x in n]), "rt_scene_mirror_info")
        tris = np.zeros((n[0].value, 12), dtype=np.float32)
        tree = np.zeros((n[1].value, 16), dtype=np.float32)
        ltris = np.zeros((n[2].value, 12), dtype=np.float32)
        _check(lib().rt_scene_mirror_copy(self.handle, tris.ctypes.data, tree.ctypes.data, ltris.ctypes.data),
               "rt_scene_mirror_copy")
        return (tris, tree, ltris) if trees else tris

    def mirror_nodes(self):
        """The traversal's private node array (mirror.h nodes) as (N, 8) float32 (uint32 view for
        first / count)."""
        import numpy as np
        n = ctypes.c_size_t()
        _check(lib().rt_scene_mirror_nodes(self.handle, None, ctypes.byref(n)), "rt_scene_mirror_nodes")
        out = np.zeros((n.value, 8), dtype=np.float32)
        _check(lib().rt_scene_mirror_nodes(self.handle, out.ctypes.data, ctypes.byref(n)), "rt_scene_mirror_nodes")
        return out

    def mirror_face_leaf(self):
        """Scenes with big leaves: each face's leaf in the private node array (uint32; 0xffffffff none,
        0xfffffffe two leaves), the deferred leaves' guard table (rt_fast.h); empty otherwise."""
        import numpy as np
        n = ctypes.c_size_t()
        _check(lib().rt_scene_mirror_face_leaf(self.handle, None, ctypes.byref(n)), "rt_scene_mirror_face_leaf")
        out = np.zeros(n.value, dtype=np.uint32)
        if n.value:
            _check(lib().rt_scene_mirror_face_leaf(self.handle, out.ctypes.data, ctypes.byref(n)), "rt_scene_mirror_face_leaf")
        return out

    def mirror_twins(self):
        """The big leaves' twin records (mirror.h): quads (Q, 28) and units (U, 16) float32."""
        import numpy as np
        nq, nu = ctypes.c_size_t(), ctypes.c_size_t()
        _check(lib().rt_scene_mirror_twins(self.handle, None, ctypes.byref(nq), None, ctypes.byref(nu)), "rt_scene_mirror_twins")
        q = np.zeros((nq.value, 28), dtype=np.float32)
        u = np.zeros((nu.value, 16), dtype=np.float32)
        _check(lib().rt_scene_mirror_twins(self.handle, q.ctypes.data, ctypes.byref(nq), u.ctypes.data, ctypes.byref(nu)),
               "rt_scene_mirror_twins")
        return q, u

    def mirror_leaf_twin(self, first):
        """The twin record (mirror.h pairs) of the big leaf whose first leaf-ordered record is `first`: 12 float32
        (KD, KE, KDD, KDD1, lo.xyz, 0, hi.xyz, 0)."""
        import numpy as np
        rec = np.zeros(12, dtype=np.float32)
        _check(lib().rt_scene_mirror_leaf_twin(self.handle, int(first), rec.ctypes.data), "rt_scene_mirror_leaf_twin")
        return rec

    def materials(self):
        """Host copy of the GPUMaterial array as (M, 16) float32: albedo 0-3, emissive 4-7, specular 8-11,
        roughness, specular_percent, IOR, padding (what rt_hit.material indexes)."""
        n = ctypes.c_size_t()
        _check(lib().rt_scene_materials(self.handle, None, ctypes.byref(n)), "rt_scene_materials")
        out = np.zeros((n.value, 16), dtype=np.float32)
        if n.value:
            _check(lib().rt_scene_materials(self.handle, out.ctypes.data, ctypes.byref(n)), "rt_scene_materials")
        return out

    def spheres(self):
        """Host copy of the sphere array as (S, 8) float32: centre 0-2, radius, material (an int32), padding."""
        n = ctypes.c_size_t()
        _check(lib().rt_scene_spheres(self.handle, None, ctypes.byref(n)), "rt_scene_spheres")
        out = np.zeros((n.value, 8), dtype=np.float32)
        if n.value:
            _check(lib().rt_scene_spheres(self.handle, out.ctypes.data, ctypes.byref(n)), "rt_scene_spheres")
        return out

    def host_arrays(self):
        """numpy copies of the host arrays: nodes (N,8) f32/u32 view, face indices, vertices, faces."""
        import numpy as np
        ptrs = [ctypes.c_void_p() for _ in range(4)]
        counts = [ctypes.c_size_t() for _ in range(3)]
        lib().rt_scene_host_arrays(self.handle, ctypes.byref(ptrs[0]), ctypes.byref(counts[0]), ctypes.byref(ptrs[1]),
                                   ctypes.byref(counts[1]), ctypes.byref(ptrs[2]), ctypes.byref(counts[2]),
                                   ctypes.byref(ptrs[3]))

        def grab(p, nbytes):
            if not p.value or nbytes == 0:
                return np.zeros(0, dtype=np.uint8)
            return np.frombuffer(ctypes.string_at(p.value, nbytes), dtype=np.uint8).copy()

        nn, nf, nv = counts[0].value, counts[1].value, counts[2].value
        return {"nodes": grab(ptrs[0], nn * 32), "face_indices": grab(ptrs[1], nf * 4),
                "vertices": grab(ptrs[2], nv * 32), "faces": grab(ptrs[3], nf * 16)}


def mirror_build_check(nodes, face_indices, faces, vertices):
    """rt_mirror_build_check: the host mirror of raw reference arrays (numpy: nodes (N,8) 32-bit, face
    indices u32, faces (F,4) u32, vertices (V,8) f32) -> (words 10-11 of every record as (n, 2) uint32,
    whether twin records were built)."""
    import numpy as np
    nodes, fi = np.ascontiguousarray(nodes), np.ascontiguousarray(face_indices, dtype=np.uint32)
    faces, vertices = np.ascontiguousarray(faces), np.ascontiguousarray(vertices)
    meta = np.zeros((fi.size, 2), dtype=np.uint32)
    tw = ctypes.c_int(0)
    _check(lib().rt_mirror_build_check(nodes.ctypes.data, nodes.shape[0], fi.ctypes.data, fi.size, faces.ctypes.data,
                                       faces.shape[0], vertices.ctypes.data, vertices.shape[0], meta.ctypes.data,
                                       ctypes.byref(tw)), "rt_mirror_build_check")
    return meta, bool(tw.value)


def entry_table_builds():
    """Entry tables rt_render has built so far in this process (rt_entry_table_builds)."""
    return int(lib().rt_entry_table_builds())


def bvh_build_device(vertices, faces, stream=None):
    """BVH::Calculate on the GPU (rt_bvh_build_device) from device tensors of GPUVertex (N,8) f32
    and GPUFace (F,4) u32 rows; returns (nodes (2F-1, 8) f32 device tensor, face_indices (F,) int32
    device tensor, node_count, max_depth)."""
    import torch
    nf = faces.shape[0]
    nodes = torch.empty((max(1, 2 * nf - 1), 8), dtype=torch.float32, device=faces.device)
    fi = torch.empty((nf,), dtype=torch.int32, device=faces.device)
    count, depth = _U32(0), _I(0)
    _check(lib().rt_bvh_build_device(vertices.data_ptr(), vertices.shape[0], faces.data_ptr(), nf, nodes.data_ptr(),
                                     fi.data_ptr(), ctypes.byref(count), ctypes.byref(depth), _stream_ptr(stream)),
           "rt_bvh_build_device")
    return nodes, fi, count.value, depth.value


def alloc_surface(width, height, device=None):
    """A pitched float4 surface (RGBA fp32), rows padded to a 256-byte pitch like cudaMallocPitch."""
    row_floats = ((width * 16 + 255) // 256) * 256 // 4
    t = torch.zeros((height, row_floats), dtype=torch.float32, device=device or "cuda")
    return t


def surface_view(t, width):
    """[H, W, 4] view of a pitched surface tensor."""
    return t[:, : width * 4].reshape(t.shape[0], width, 4)


def alloc_rng(count, device=None):
    return torch.zeros((count * RNG_STATE_BYTES // 4,), dtype=torch.int32, device=device or "cuda")


def init_rng_states(rng, width, height, seed, shard_index=0, shard_count=1, stream=None):
    _check(lib().rt_init_rng(ctypes.c_void_p(rng.data_ptr()), width, height, shard_index, shard_count, seed,
                             _stream_ptr(stream)), "rt_init_rng")


def render(scene, surface, last, width, height, spp, bounces, frame_index=0, shard_index=0, shard_count=1,
           out_shard=None, stats=None, segment_counter=None, stream=None, tracer="fast", tile_list=None,
           wave_clock=None, tune=0, lane_slots=None, lane_cost=None, priority_waves=0, refill_lanes=0,
           waves_per_simd=0, lone_slots=None, validate=False):
    """rt_render: one frame (or one shard of it) on `stream` (default: torch's current stream).
    tile_list: device int32 tensor of tile ids (a row of a sharding.Plan) instead of the
    round-robin deal; wave_clock: device int64 tensor [entries*4] receiving per-wave clocks;
    tune: diagnostic A/B knobs (0 = production); lane_slots: device int32 lane map (rt_lane_plan,
    a multiple of 64 entries); lane_cost: device int32/uint32 [slots] receiving per-pixel work;
    lone_slots: device int32 slots for the lone-pixel kernel (rt_lone_plan; needs lane_slots);
    validate: RT_RENDER_VALIDATE (lone_slots and lane_slots checked disjoint first; synchronises)."""
    p = RenderParams()
    if lone_slots is not None and lone_slots.numel() > 0:
        assert lone_slots.dtype == torch.int32 and lone_slots.is_cuda and lone_slots.dim() == 1
        p.lone_slots, p.lone_count = lone_slots.data_ptr(), lone_slots.numel()
    if lane_slots is not None:
        assert lane_slots.dtype == torch.int32 and lane_slots.is_cuda and lane_slots.numel() % 64 == 0
        p.lane_slots, p.lane_slot_count = lane_slots.data_ptr(), lane_slots.numel()
        p.priority_waves = int(priority_waves)
    if lane_cost is not None:
        assert lane_cost.dtype == torch.int32 and lane_cost.is_cuda
        p.lane_cost = lane_cost.data_ptr()
    if tile_list is not None:
        assert tile_list.dtype == torch.int32 and tile_list.is_cuda and tile_list.dim() == 1
        p.tile_list, p.tile_count = tile_list.data_ptr(), tile_list.numel()
    if wave_clock is not None:
        n = tile_list.numel() if tile_list is not None else tiles_of(width, height, shard_index, shard_count)
        waves = lane_slots.numel() // 64 if lane_slots is not None else 4 * n
        assert wave_clock.dtype == torch.int64 and wave_clock.numel() >= waves
        p.wave_clock = wave_clock.data_ptr()
    p.tune = int(tune)
    p.refill_lanes = int(refill_lanes)
    p.waves_per_simd = int(waves_per_simd)
    p.surface = surface.data_ptr() if surface is not None else None
    p.surface_last_frame = last.data_ptr() if last is not None else None
    p.width, p.height = width, height
    p.pitch = surface.shape[1] * 4 if surface is not None else width * 16
    p.frame_index, p.spp, p.bounces = frame_index, spp, bounces
    p.shard_index, p.shard_count = shard_index, shard_count
    p.out_shard = out_shard.data_ptr() if out_shard is not None else None
    p.flags = TRACERS[tracer] | (RT_RENDER_VALIDATE if validate else 0)
    if segment_counter is not None:
        p.segment_counter = segment_counter.data_ptr()
    if stats is not None:
        p.flags |= RT_RENDER_STATS
        p.stats = stats.data_ptr()
    _check(lib().rt_render(ctypes.byref(p), _scene_ptr(scene), _stream_ptr(stream)), "rt_render")


def _trace(scene, rays, count, width, height, hits, stream, waves_per_simd):
    if hits is None:
        hits = torch.empty((count, 12), dtype=torch.float32, device=rays.device if rays is not None else "cuda")
    assert hits.dtype == torch.float32 and hits.is_cuda and hits.is_contiguous() and hits.dim() == 2
    assert hits.shape[1] == 12 and hits.shape[0] >= count
    p = TraceParams()
    p.rays = rays.data_ptr() if rays is not None else None
    p.count, p.width, p.height = count, width, height
    p.hits = hits.data_ptr()
    p.waves_per_simd = int(waves_per_simd)
    _check(lib().rt_trace_rays(ctypes.byref(p), _scene_ptr(scene), _stream_ptr(stream)), "rt_trace_rays")
    return hits


def trace_rays(scene, rays, hits=None, stream=None, waves_per_simd=0):
    """rt_trace_rays: the closest hit of every ray of a float32 CUDA tensor [N, 8] (rt_ray rows: origin,
    tmax, direction, a zero word) on `stream` (default: torch's current stream), as a float32 [N, 12]
    tensor of rt_hit rows (`hits`, or a new one; hit_fields gives typed views).  The scene must have
    been uploaded (Scene.upload; its RNG pointer may be 0 for a scene that is only queried)."""
    assert _is_rays(rays)
    return _trace(scene, rays, rays.shape[0], 0, 0, hits, stream, waves_per_simd)


def trace_camera(scene, width, height, hits=None, stream=None, waves_per_simd=0):
    """rt_trace_rays in camera mode: the rays through the pixel centres of the uploaded scene's camera
    (Scene.set_viewport before upload), row i = pixel (i % width, i // width); float32 [H*W, 12]."""
    return _trace(scene, None, int(width) * int(height), int(width), int(height), hits, stream, waves_per_simd)


def hit_fields(hits):
    """Typed views of a [N, 12] hit tensor (torch or numpy): t, kind / id / material (int32), normal [N, 3],
    position [N, 3], bx, by."""
    ints = hits.view(torch.int32) if isinstance(hits, torch.Tensor) else hits.view(np.int32)
    return {"t": hits[:, 0], "kind": ints[:, 1], "id": ints[:, 2], "material": ints[:, 3], "normal": hits[:, 4:7],
            "bx": hits[:, 7], "position": hits[:, 8:11], "by": hits[:, 11]}


def gbuffer(scene, width, height, stream=None, waves_per_simd=0):
    """First-hit images of an uploaded Scene's camera (rt_trace_rays in camera mode: the pixel centres, no
    jitter) as device tensors, rows bottom to top like the surface: depth [H, W] (t; inf on a miss),
    normal / position / albedo [H, W, 3] (0 on a miss; albedo is the hit material's), material, prim (-1 on
    a miss; sphere or face index) and kind [H, W] int32."""
    w, h = int(width), int(height)
    f = hit_fields(trace_camera(scene, w, h, stream=stream, waves_per_simd=waves_per_simd))
    hit = f["kind"] != HIT_MISS
    mats = torch.from_numpy(scene.materials()).to(hit.device)
    albedo = torch.zeros((w * h, 3), dtype=torch.float32, device=hit.device)
    if mats.shape[0]:
        albedo = torch.where(hit[:, None], mats[f["material"].long().clamp(0, mats.shape[0] - 1), :3], albedo)
    return {"depth": torch.where(hit, f["t"], torch.full_like(f["t"], float("inf"))).reshape(h, w),
            "normal": f["normal"].reshape(h, w, 3).clone(), "position": f["position"].reshape(h, w, 3).clone(),
            "albedo": albedo.reshape(h, w, 3), "material": f["material"].reshape(h, w).clone(),
            "prim": torch.where(hit, f["id"], torch.full_like(f["id"], -1)).reshape(h, w),
            "kind": f["kind"].reshape(h, w).clone()}


def occluded(scene, rays, out=None, stream=None, waves_per_simd=0):
    """rt_occluded: whether each ray of a float32 CUDA tensor [N, 8] (rt_ray rows, as trace_rays takes them) hits
    anything before its tmax, as a uint8 tensor [N] (`out`, or a new one): byte i is `kind != 0` of the record
    trace_rays gives for ray i, for every ray, at a fraction of the cost where the traversal may stop at the first
    occluder.  Stream-ordered on `stream` (default: torch's current stream)."""
    assert _is_rays(rays)
    n = rays.shape[0]
    if out is None:
        with _allocating_on(stream):
            out = torch.empty((n,), dtype=torch.uint8, device=rays.device)
    assert out.dtype == torch.uint8 and out.is_cuda and out.is_contiguous() and out.dim() == 1 and out.shape[0] >= n
    if n == 0:  # rt_occluded returns at once for count 0; an empty tensor has no address to pass
        return out
    p = OcclusionParams()
    p.rays, p.count, p.occluded = rays.data_ptr(), n, out.data_ptr()
    p.waves_per_simd = int(waves_per_simd)
    _check(lib().rt_occluded(ctypes.byref(p), _scene_ptr(scene), _stream_ptr(stream)), "rt_occluded")
    return out


NEAREST_MISS, NEAREST_SPHERE, NEAREST_FACE = 0, 1, 2  # rt_nearest.kind


def closest_points(scene, points, out=None, waves_per_simd=0, stream=None):
    """rt_closest_point: the nearest point of the scene's surface to every row of a float32 CUDA tensor [N, 4]
    (rt_point rows: position, search radius -- inf for none), as a float32 [N, 8] tensor of rt_nearest rows (`out`, or
    a new one; nearest_fields gives typed views): distance, kind, id, material, the point, the triangle's region.  A
    point with nothing within its radius gets a miss: its radius and zeros.  Exact and unsigned (rt_abi.h).
    Stream-ordered on `stream` (default: torch's current stream)."""
    assert points.dtype == torch.float32 and points.is_cuda and points.is_contiguous() and points.dim() == 2
    assert points.shape[1] == 4
    n = points.shape[0]
    if out is None:
        with _allocating_on(stream):
            out = torch.empty((n, 8), dtype=torch.float32, device=points.device)
    assert out.dtype == torch.float32 and out.is_cuda and out.is_contiguous() and out.dim() == 2
    assert out.shape[1] == 8 and out.shape[0] >= n
    if n == 0:  # rt_closest_point returns at once for count 0; an empty tensor has no address to pass
        return out
    p = ClosestParams()
    p.points, p.count, p.nearest = points.data_ptr(), n, out.data_ptr()
    p.waves_per_simd = int(waves_per_simd)
    _check(lib().rt_closest_point(ctypes.byref(p), _scene_ptr(scene), _stream_ptr(stream)), "rt_closest_point")
    return out


def nearest_fields(nearest):
    """Typed views of a [N, 8] record tensor (torch or numpy): distance, kind / id / material / region (int32),
    point [N, 3]."""
    ints = nearest.view(torch.int32) if isinstance(nearest, torch.Tensor) else nearest.view(np.int32)
    return {"distance": nearest[:, 0], "kind": ints[:, 1], "id": ints[:, 2], "material": ints[:, 3],
            "point": nearest[:, 4:7], "region": ints[:, 7]}


def closest_points_host(scene, points):
    """rt_closest_point_host: closest_points' records by brute force on the host (a built or uploaded Scene, a
    float32 numpy array [N, 4]) as a float32 numpy array [N, 8].  No BVH and no device: for checking."""
    pts = np.ascontiguousarray(points, dtype=np.float32)
    assert pts.ndim == 2 and pts.shape[1] == 4
    out = np.zeros((pts.shape[0], 8), dtype=np.float32)
    _check(lib().rt_closest_point_host(scene.handle, pts.ctypes.data, pts.shape[0], out.ctypes.data), "rt_closest_point_host")
    return out


def closest_bound_host(p, lo, hi):
    """closest.h box_bound on the host (rt_closest_bound_host): the kernel's lower bound on the computed squared
    distance from p to any face with its vertices in the box [lo, hi]; -1 = no bound."""
    return float(lib().rt_closest_bound_host(_f3(p), _f3(lo), _f3(hi)))


def _grid_axes(lo, hi, shape):
    """The cell centres of a (nz, ny, nx) grid over the box [lo, hi] as device tensors (z, y, x)."""
    axes = []
    for n, a, b in ((shape[0], lo[2], hi[2]), (shape[1], lo[1], hi[1]), (shape[2], lo[0], hi[0])):
        i = torch.arange(n, dtype=torch.float32, device="cuda")
        axes.append(float(a) + (i + 0.5) * ((float(b) - float(a)) / n))
    return axes


def distance_grid(scene, lo, hi, shape, radius=float("inf"), stream=None, waves_per_simd=0):
    """The unsigned distance from the centre of every cell of a regular grid to the scene's surface: `shape` =
    (nz, ny, nx) cells over the box [lo, hi] (x, y, z), as a float32 device tensor [nz, ny, nx].  A cell with nothing
    within `radius` holds `radius`.  Tensor code over closest_points."""
    nz, ny, nx = (int(s) for s in shape)
    with _allocating_on(stream):
        z, y, x = torch.meshgrid(*_grid_axes(lo, hi, (nz, ny, nx)), indexing="ij")
        pts = torch.stack([x, y, z, torch.full_like(x, float(radius))], dim=-1).reshape(-1, 4).contiguous()
    rec = closest_points(scene, pts, stream=stream, waves_per_simd=waves_per_simd)
    return rec[:, 0].reshape(nz, ny, nx).clone()


HITS_MAX = 16  # RT_HITS_MAX
RT_HITS_CULL_BACK, RT_HITS_CULL_FRONT, RT_HITS_COUNT_ALL = 1, 2, 4  # rt_hits_params.flags


def _trace_hits(scene, rays, count, width, height, max_hits, flags, hits, counts, stream, waves_per_simd):
    k = int(max_hits)
    device = rays.device if rays is not None else "cuda"
    with _allocating_on(stream):
        if hits is None:
            hits = torch.empty((count, k, 12), dtype=torch.float32, device=device)
        if counts is None:
            counts = torch.empty((count,), dtype=torch.int32, device=device)
    assert hits.dtype == torch.float32 and hits.is_cuda and hits.is_contiguous() and hits.dim() == 3
    assert hits.shape[1] == k and hits.shape[2] == 12 and hits.shape[0] >= count
    if counts is not False:
        assert counts.dtype == torch.int32 and counts.is_cuda and counts.is_contiguous() and counts.dim() == 1
        assert counts.shape[0] >= count
    if count == 0:  # rt_trace_hits returns at once for count 0; an empty tensor has no address to pass
        return hits, (None if counts is False else counts)
    p = HitsParams()
    p.rays = rays.data_ptr() if rays is not None else None
    p.count, p.width, p.height = count, width, height
    p.hits = hits.data_ptr()
    p.counts = None if counts is False else counts.data_ptr()
    p.max_hits, p.flags, p.waves_per_simd = k, int(flags), int(waves_per_simd)
    _check(lib().rt_trace_hits(ctypes.byref(p), _scene_ptr(scene), _stream_ptr(stream)), "rt_trace_hits")
    return hits, (None if counts is False else counts)


def trace_hits(scene, rays, max_hits, flags=0, hits=None, counts=None, stream=None, waves_per_simd=0):
    """rt_trace_hits: the first `max_hits` (1..16) hits of every ray of a float32 CUDA tensor [N, 8] (rt_ray rows), in
    order of distance, as (hits, counts): a float32 [N, K, 12] tensor of rt_hit rows -- row k of a ray its k-th hit, the
    rows past the last a miss record (t = tmax, zeros) -- and an int32 [N] tensor of list lengths.  flags:
    RT_HITS_CULL_BACK / RT_HITS_CULL_FRONT keep one winding's triangles (on a loaded mesh: one record per crossing),
    RT_HITS_COUNT_ALL makes counts the number of all hits below tmax (it may exceed K).  `hits` / `counts`: tensors to
    fill in place (counts=False: none kept, None is returned for it).  Exact, as trace_rays (rt_abi.h); stream-ordered
    on `stream` (default: torch's current stream)."""
    assert _is_rays(rays)
    return _trace_hits(scene, rays, rays.shape[0], 0, 0, max_hits, flags, hits, counts, stream, waves_per_simd)


def trace_hits_camera(scene, width, height, max_hits, flags=0, hits=None, counts=None, stream=None, waves_per_simd=0):
    """rt_trace_hits in camera mode: trace_camera's rays (the pixel centres of the uploaded scene's camera), ray i =
    pixel (i % width, i // width); (hits [H*W, K, 12], counts [H*W])."""
    return _trace_hits(scene, None, int(width) * int(height), int(width), int(height), max_hits, flags, hits, counts, stream,
                       waves_per_simd)


def hit_list_host(t, payload, max_hits, tmax, count_all=False):
    """rt_hit_list_host: the kernel's list code (csrc/hit_list.h) on the host -- the pairs (t[j], payload[j]) offered in
    order to an empty list of `max_hits` entries under `tmax`.  Returns (t float32 [n], payload uint32 [n], total)."""
    t = np.ascontiguousarray(t, dtype=np.float32).reshape(-1)
    payload = np.ascontiguousarray(payload, dtype=np.uint32).reshape(-1)
    assert t.shape == payload.shape
    out_t, out_p = np.zeros(HITS_MAX, dtype=np.float32), np.zeros(HITS_MAX, dtype=np.uint32)
    total = ctypes.c_int64(0)
    n = lib().rt_hit_list_host(int(max_hits), float(tmax), 1 if count_all else 0, t.shape[0], t.ctypes.data, payload.ctypes.data,
                               out_t.ctypes.data, out_p.ctypes.data, ctypes.byref(total))
    if n < 0:
        raise RTError("rt_hit_list_host failed: " + lib().rt_last_error().decode(errors="replace"))
    return out_t[:n].copy(), out_p[:n].copy(), int(total.value)


# contains(): three fixed unit directions in general position (no component 0, none parallel to a box face or diagonal)
CONTAINS_DIRECTIONS = ((0.36, 0.48, 0.8), (-0.6, 0.64, -0.48), (0.8, -0.36, 0.48))


def contains(scene, points, flags=RT_HITS_CULL_BACK, stream=None, waves_per_simd=0):
    """Whether each row of a float32 CUDA tensor [N, 3] lies inside a closed body of the scene, as a bool tensor [N]:
    the parity of the surface crossings along a ray to infinity, counted under one winding (rt_trace_hits with
    RT_HITS_COUNT_ALL | `flags`, so that a loaded mesh's twin faces count once), by majority over three fixed
    directions.  Meaningful for closed surfaces; spheres count as they are crossed (one distance each)."""
    assert points.dtype == torch.float32 and points.is_cuda and points.dim() == 2 and points.shape[1] == 3
    n = points.shape[0]
    with _allocating_on(stream):
        votes = torch.zeros((n,), dtype=torch.int32, device=points.device)
        rays = torch.zeros((n, 8), dtype=torch.float32, device=points.device)
        rays[:, 0:3] = points
        rays[:, 3] = RAY_TMAX
        hits = torch.empty((n, 1, 12), dtype=torch.float32, device=points.device)
    for d in CONTAINS_DIRECTIONS:
        with _allocating_on(stream):
            rays[:, 4:7] = torch.tensor(d, dtype=torch.float32, device=points.device)
        _, counts = trace_hits(scene, rays, 1, flags=RT_HITS_COUNT_ALL | int(flags), hits=hits, stream=stream,
                               waves_per_simd=waves_per_simd)
        with _allocating_on(stream):
            votes += counts & 1
    with _allocating_on(stream):
        return votes >= 2


def signed_distance_grid(scene, lo, hi, shape, radius=float("inf"), flags=RT_HITS_CULL_BACK, stream=None, waves_per_simd=0):
    """distance_grid with a sign: the same distances (bit for bit), negated at the cell centres `contains` finds inside."""
    nz, ny, nx = (int(s) for s in shape)
    dist = distance_grid(scene, lo, hi, shape, radius=radius, stream=stream, waves_per_simd=waves_per_simd)
    with _allocating_on(stream):
        z, y, x = torch.meshgrid(*_grid_axes(lo, hi, (nz, ny, nx)), indexing="ij")
        pts = torch.stack([x, y, z], dim=-1).reshape(-1, 3).contiguous()
    inside = contains(scene, pts, flags=flags, stream=stream).reshape(nz, ny, nx)
    with _allocating_on(stream):
        return torch.where(inside, -dist, dist)


def radiance(scene, rays, rng, bounces=REFERENCE_BOUNCES, samples=1, out=None, stream=None, waves_per_simd=0):
    """rt_radiance: the path-traced radiance along every ray of a float32 CUDA tensor [N, 8] (rt_ray rows, as
    trace_rays takes them; tmax is not read) as a float32 [N, 4] tensor (`out`, or a new one): rgb = the mean of
    `samples` evaluations of the reference's ray_color along the ray, w = 1.  `rng`: an int32 CUDA tensor of N states
    (ray_rng, alloc_rng), state i read for ray i and written back advanced.  Pass unit directions unless the rays
    reproduce the reference's camera (rt_abi.h).  Stream-ordered on `stream` (default: torch's current stream)."""
    assert _is_rays(rays)
    n = rays.shape[0]
    assert rng.dtype == torch.int32 and rng.is_cuda and rng.is_contiguous() and rng.numel() >= n * (RNG_STATE_BYTES // 4)
    if out is None:
        with _allocating_on(stream):
            out = torch.empty((n, 4), dtype=torch.float32, device=rays.device)
    assert out.dtype == torch.float32 and out.is_cuda and out.is_contiguous() and out.dim() == 2
    assert out.shape[1] == 4 and out.shape[0] >= n
    if n == 0:  # rt_radiance returns at once for count 0; an empty tensor has no address to pass
        return out
    p = RadianceParams()
    p.rays, p.count, p.rng, p.radiance = rays.data_ptr(), n, rng.data_ptr(), out.data_ptr()
    p.bounces, p.samples = int(bounces), int(samples)
    p.waves_per_simd = int(waves_per_simd)
    _check(lib().rt_radiance(ctypes.byref(p), _scene_ptr(scene), _stream_ptr(stream)), "rt_radiance")
    return out


def ray_rng(count, seed, device=None, stream=None):
    """`count` RNG states for radiance(): state i is curand_init(seed, i, 0) (alloc_rng + rt_init_rng of a count x 1
    frame), allocated and initialised on `stream` (default: torch's current stream)."""
    with _allocating_on(stream):
        rng = alloc_rng(int(count), device=device)
    if int(count) > 0:
        init_rng_states(rng, int(count), 1, seed, stream=stream)
    return rng


def panorama_rays(origin, width, height):
    """A float32 [H*W, 8] numpy table of rt_ray rows: the equirectangular rays of a width x height panorama from
    `origin`.  Row y*W + x, rows bottom to top like the surface: longitude phi = 2 pi (x + 0.5) / W - pi, latitude
    theta = pi (y + 0.5) / H - pi / 2, direction (cos theta sin phi, sin theta, cos theta cos phi) -- the centre
    column looks along +z, x grows to the right of it -- computed in float64 and rounded; tmax = RAY_TMAX.  (The
    renderer's camera looking along +z has +x on its LEFT: shown as an image this map is the mirror image of what that
    camera sees; flip the columns for a view from inside.)"""
    w, h = int(width), int(height)
    phi = 2.0 * np.pi * (np.arange(w, dtype=np.float64) + 0.5) / w - np.pi
    theta = np.pi * (np.arange(h, dtype=np.float64) + 0.5) / h - 0.5 * np.pi
    ct, st = np.cos(theta)[:, None], np.sin(theta)[:, None]
    out = np.zeros((h, w, 8), dtype=np.float32)
    out[..., 0:3] = np.asarray(origin, dtype=np.float32).reshape(3)
    out[..., 3] = RAY_TMAX
    out[..., 4], out[..., 5], out[..., 6] = ct * np.sin(phi)[None, :], st * np.ones((1, w)), ct * np.cos(phi)[None, :]
    return out.reshape(h * w, 8)


def panorama(scene, width, height, origin=None, samples=REFERENCE_SPP, bounces=REFERENCE_BOUNCES, seed=0xDEADBEEF,
             device=None, stream=None):
    """A width x height equirectangular panorama of an uploaded Scene seen from `origin` (default: its camera's
    position) as a new pitched surface (alloc_surface layout, rows bottom to top): radiance() along panorama_rays()
    with the states ray_rng(width * height, seed).  The rays are uploaded with a synchronous copy; the rest is
    stream-ordered on `stream` (default: torch's current stream), where everything here is allocated."""
    w, h = int(width), int(height)
    if origin is None:
        origin = tuple(scene.camera().origin)
    with _allocating_on(stream):
        rays = torch.from_numpy(panorama_rays(origin, w, h)).to(device or "cuda")
        rng = ray_rng(w * h, seed, device=rays.device, stream=stream)
        rgba = radiance(scene, rays, rng, bounces=bounces, samples=samples, stream=stream)
        surface = alloc_surface(w, h, device=rays.device)
        surface_view(surface, w).copy_(rgba.view(h, w, 4))
    return surface


def _is_pitched(t, w, h):
    """A pitched float4 surface tensor (alloc_surface layout) of at least w x h."""
    return (t.dtype == torch.float32 and t.is_cuda and t.dim() == 2 and t.stride(1) == 1 and t.shape[0] >= h
            and t.shape[1] >= w * 4 and (t.stride(0) * 4) % 16 == 0)


def sample_pixels(scene, width, height, samples, rng, accum, pixels=None, moments=None, bounces=REFERENCE_BOUNCES,
                  stream=None, waves_per_simd=0):
    """rt_sample_pixels: samples[i] more of the renderer's samples for pixel pixels[i] (= y * width + x; None: entry i
    is pixel i) of the uploaded Scene's camera, added to the undivided accumulator `accum` (a pitched surface: sum of
    rgb, sample count), to `moments` (float32 [H*W, 2], optional) and the pixel's state in `rng` (H*W states in the
    renderer's layout).  `samples`: int16 / uint16 CUDA tensor (read as uint16), one entry each; `pixels`: int32.
    Stream-ordered on `stream` (default: torch's current stream)."""
    w, h = int(width), int(height)
    assert samples.is_cuda and samples.is_contiguous() and samples.element_size() == 2 and not samples.is_floating_point()
    n = samples.numel()
    assert rng.dtype == torch.int32 and rng.is_cuda and rng.is_contiguous() and rng.numel() >= w * h * (RNG_STATE_BYTES // 4)
    assert _is_pitched(accum, w, h)
    p = SamplePixelsParams()
    if pixels is not None:
        assert pixels.dtype == torch.int32 and pixels.is_cuda and pixels.is_contiguous() and pixels.numel() >= n
        p.pixels = pixels.data_ptr() if n else None
    if moments is not None:
        assert moments.dtype == torch.float32 and moments.is_cuda and moments.is_contiguous() and moments.numel() >= 2 * w * h
        p.moments = moments.data_ptr()
    if n == 0:  # rt_sample_pixels returns at once for count 0; an empty tensor has no address to pass
        return accum
    p.samples, p.count, p.rng = samples.data_ptr(), n, rng.data_ptr()
    p.accum, p.accum_pitch = accum.data_ptr(), accum.stride(0) * 4
    p.width, p.height, p.bounces, p.waves_per_simd = w, h, int(bounces), int(waves_per_simd)
    _check(lib().rt_sample_pixels(ctypes.byref(p), _scene_ptr(scene), _stream_ptr(stream)), "rt_sample_pixels")
    return accum


def sample_priority(accum, moments, width, height, out=None, stream=None):
    """rt_sample_priority: float32 [H*W] priorities (`out`, or a new tensor) from an accumulator and its moments: the
    relative variance of the mean, +inf where fewer than two samples are known."""
    w, h = int(width), int(height)
    assert _is_pitched(accum, w, h)
    assert moments.dtype == torch.float32 and moments.is_cuda and moments.is_contiguous() and moments.numel() >= 2 * w * h
    if out is None:
        with _allocating_on(stream):
            out = torch.empty((w * h,), dtype=torch.float32, device=accum.device)
    assert out.dtype == torch.float32 and out.is_cuda and out.is_contiguous() and out.numel() >= w * h
    p = SamplePriorityParams()
    p.accum, p.accum_pitch, p.moments, p.priority = accum.data_ptr(), accum.stride(0) * 4, moments.data_ptr(), out.data_ptr()
    p.width, p.height = w, h
    _check(lib().rt_sample_priority(ctypes.byref(p), _stream_ptr(stream)), "rt_sample_priority")
    return out


def sample_plan_scratch_bytes(width, height):
    """rt_sample_plan_scratch_bytes (needs no GPU)."""
    return int(lib().rt_sample_plan_scratch_bytes(int(width), int(height)))


def sample_plan(priority, width, height, budget, min_samples=0, max_samples=64, scale=SAMPLE_SCALE_DEFAULT, pixels=None,
                samples=None, total=None, scratch=None, stream=None):
    """rt_sample_plan: the list of the next round from float32 [H*W] priorities and a total `budget` of samples.
    Returns (pixels int32 [H*W], samples int16 [H*W] holding uint16 counts, total int64 [1]): every pixel once, sorted
    by count descending, 8x8 sub-tile order inside a count.  Tensors not given are allocated on `stream`."""
    w, h = int(width), int(height)
    n = w * h
    assert priority.dtype == torch.float32 and priority.is_cuda and priority.is_contiguous() and priority.numel() >= n
    need = sample_plan_scratch_bytes(w, h)
    with _allocating_on(stream):
        if pixels is None:
            pixels = torch.empty((n,), dtype=torch.int32, device=priority.device)
        if samples is None:
            samples = torch.empty((n,), dtype=torch.int16, device=priority.device)
        if total is None:
            total = torch.empty((1,), dtype=torch.int64, device=priority.device)
        if scratch is None:
            scratch = torch.empty((need,), dtype=torch.uint8, device=priority.device)
    assert pixels.dtype == torch.int32 and pixels.is_cuda and pixels.is_contiguous() and pixels.numel() >= n
    assert samples.element_size() == 2 and not samples.is_floating_point() and samples.is_cuda and samples.is_contiguous()
    assert samples.numel() >= n and total.dtype == torch.int64 and total.is_cuda and total.numel() >= 1
    assert scratch.is_cuda and scratch.is_contiguous() and scratch.numel() * scratch.element_size() >= need
    p = SamplePlanParams()
    p.priority, p.width, p.height, p.budget = priority.data_ptr(), w, h, int(budget)
    p.min_samples, p.max_samples, p.scale = int(min_samples), int(max_samples), float(scale)
    p.pixels, p.samples, p.total = pixels.data_ptr(), samples.data_ptr(), total.data_ptr()
    p.scratch, p.scratch_bytes = scratch.data_ptr(), scratch.numel() * scratch.element_size()
    _check(lib().rt_sample_plan(ctypes.byref(p), _stream_ptr(stream)), "rt_sample_plan")
    return pixels, samples, total


def sample_resolve(accum, width, height, out=None, stream=None):
    """rt_sample_resolve: the mean image of an accumulator as a pitched surface (`out`, or a new one): rgb / count where
    count >= 1, else 0; alpha 1."""
    w, h = int(width), int(height)
    assert _is_pitched(accum, w, h)
    if out is None:
        with _allocating_on(stream):
            out = alloc_surface(w, h, device=accum.device)
    assert _is_pitched(out, w, h)
    p = SampleResolveParams()
    p.accum, p.accum_pitch, p.out, p.out_pitch = accum.data_ptr(), accum.stride(0) * 4, out.data_ptr(), out.stride(0) * 4
    p.width, p.height = w, h
    _check(lib().rt_sample_resolve(ctypes.byref(p), _stream_ptr(stream)), "rt_sample_resolve")
    return out


class AdaptiveSampler:
    """Adaptive sampling of an uploaded Scene's camera at width x height (the scene's viewport): it owns the states
    (rt_init_rng(seed), the renderer's own), the undivided accumulator, the luminance moments, the list of the current
    round and the planner's scratch.  warmup(spp) gives every pixel spp samples; step(budget_spp) spends
    budget_spp * width * height samples where the relative variance of the mean is largest.  Every pixel always holds
    exactly what the renderer's first counts()[y, x] samples of that pixel sum to (rt_abi.h).  Everything runs on
    `stream` (default: torch's current stream at each call) without synchronisation."""

    def __init__(self, scene, width, height, bounces=REFERENCE_BOUNCES, seed=0xDEADBEEF, device=None, stream=None):
        self.scene, self.width, self.height, self.bounces, self.seed = scene, int(width), int(height), int(bounces), seed
        self.stream = stream
        n = self.width * self.height
        with _allocating_on(stream):
            self.rng = alloc_rng(n, device=device)
            self.accum = alloc_surface(self.width, self.height, device=self.rng.device)
            self.moments = torch.zeros((n, 2), dtype=torch.float32, device=self.rng.device)
            self.priority = torch.empty((n,), dtype=torch.float32, device=self.rng.device)
            self.pixels = torch.empty((n,), dtype=torch.int32, device=self.rng.device)
            self.samples = torch.empty((n,), dtype=torch.int16, device=self.rng.device)
            self.total = torch.zeros((1,), dtype=torch.int64, device=self.rng.device)
            self.scratch = torch.empty((sample_plan_scratch_bytes(self.width, self.height),), dtype=torch.uint8,
                                       device=self.rng.device)
        self.reset()

    def reset(self):
        """Forget every sample: zero accumulator and moments, the states of sample 0."""
        with _allocating_on(self.stream):
            self.accum.zero_()
            self.moments.zero_()
        init_rng_states(self.rng, self.width, self.height, self.seed, stream=self.stream)

    def warmup(self, spp):
        """A uniform round: spp samples for every pixel (pixels=None)."""
        with _allocating_on(self.stream):
            self.samples.fill_(int(spp))
        sample_pixels(self.scene, self.width, self.height, self.samples, self.rng, self.accum, moments=self.moments,
                      bounces=self.bounces, stream=self.stream)

    def step(self, budget_spp, min_samples=0, max_samples=64, scale=SAMPLE_SCALE_DEFAULT):
        """One adaptive round of at most budget_spp * width * height samples: priority, plan, sample.  `total`
        (device int64 [1]) then holds the samples the round spent."""
        budget = int(round(float(budget_spp) * self.width * self.height))
        sample_priority(self.accum, self.moments, self.width, self.height, out=self.priority, stream=self.stream)
        sample_plan(self.priority, self.width, self.height, budget, min_samples=min_samples, max_samples=max_samples,
                    scale=scale, pixels=self.pixels, samples=self.samples, total=self.total, scratch=self.scratch,
                    stream=self.stream)
        sample_pixels(self.scene, self.width, self.height, self.samples, self.rng, self.accum, pixels=self.pixels,
                      moments=self.moments, bounces=self.bounces, stream=self.stream)

    def image(self, out=None):
        """The mean image as a pitched surface (rt_sample_resolve)."""
        return sample_resolve(self.accum, self.width, self.height, out=out, stream=self.stream)

    def counts(self):
        """Samples per pixel so far: float32 [H, W], a view of the accumulator's alpha."""
        return surface_view(self.accum, self.width)[..., 3]


def ao_directions(count=256):
    """A [count, 4] float32 table of unit vectors for ambient_occlusion (w = 0): the Fibonacci sphere points
    z = 1 - (2k + 1) / count, azimuth k * pi * (3 - sqrt(5)), computed in float64 and rounded."""
    k = np.arange(int(count), dtype=np.float64)
    z = 1.0 - (2.0 * k + 1.0) / float(count)
    r = np.sqrt(np.maximum(0.0, 1.0 - z * z))
    phi = k * (np.pi * (3.0 - np.sqrt(5.0)))
    out = np.zeros((int(count), 4), dtype=np.float32)
    out[:, 0], out[:, 1], out[:, 2] = r * np.cos(phi), r * np.sin(phi), z
    return out


_ao_default_tables = {}  # device -> ao_directions(256) on it


def _ao_default_directions(device):
    """ao_directions(256) on `device`, built and uploaded once per device (a synchronous copy from pageable host
    memory: complete when it returns, so the table is safe to read on any stream)."""
    key = torch.device(device)
    if key.type == "cuda" and key.index is None:
        key = torch.device("cuda", torch.cuda.current_device())
    t = _ao_default_tables.get(key)
    if t is None:
        t = _ao_default_tables[key] = torch.from_numpy(ao_directions(256)).to(key)
    return t


def ao_scratch_bytes(width, height, samples):
    """rt_ao_scratch_bytes: bytes of scratch rt_ao needs."""
    return int(lib().rt_ao_scratch_bytes(int(width), int(height), int(samples)))


def ambient_occlusion(scene, hits, width, height, radius, samples=8, bias=0.001, directions=None, out=None, scratch=None,
                      stream=None, waves_per_simd=0):
    """rt_ao: the ambient-occlusion image [H, W] float32 (1 = open, 0 = closed; 1 where the camera ray missed) of an
    uploaded Scene from the first-hit records `hits` (float32 [H*W, 12], what trace_camera returns): per pixel,
    `samples` cosine-weighted rays of length `radius` from the hit point, offset along its normal by `bias` times the
    hit distance.  `directions`: a float32 [K, 4] table of unit vectors; default ao_directions(256), uploaded once
    per device and kept.  Stream-ordered on `stream` (default: torch's current stream) when `directions` is a CUDA
    tensor or the default; a numpy table is uploaded by this call with a synchronous copy.  What is allocated here
    is allocated on that stream."""
    w, h = int(width), int(height)
    assert hits.dtype == torch.float32 and hits.is_cuda and hits.is_contiguous() and hits.dim() == 2
    assert hits.shape[1] == 12 and hits.shape[0] >= w * h
    need = ao_scratch_bytes(w, h, samples)
    with _allocating_on(stream):
        if directions is None:
            directions = _ao_default_directions(hits.device)
        if not isinstance(directions, torch.Tensor):
            directions = torch.from_numpy(np.ascontiguousarray(directions, dtype=np.float32)).to(hits.device)
        if out is None:
            out = torch.empty((h, w), dtype=torch.float32, device=hits.device)
        if scratch is None and need:
            scratch = torch.empty((need,), dtype=torch.uint8, device=hits.device)
    assert directions.dtype == torch.float32 and directions.is_cuda and directions.is_contiguous()
    assert directions.dim() == 2 and directions.shape[1] == 4
    assert out.dtype == torch.float32 and out.is_cuda and out.is_contiguous() and out.numel() >= w * h
    p = AoParams()
    p.hits, p.width, p.height = hits.data_ptr(), w, h
    p.directions, p.direction_count, p.samples = directions.data_ptr(), directions.shape[0], int(samples)
    p.radius, p.bias, p.ao = float(radius), float(bias), out.data_ptr()
    if scratch is not None:
        assert scratch.is_cuda and scratch.is_contiguous()
        p.scratch, p.scratch_bytes = scratch.data_ptr(), scratch.numel() * scratch.element_size()
    p.waves_per_simd = int(waves_per_simd)
    _check(lib().rt_ao(ctypes.byref(p), _scene_ptr(scene), _stream_ptr(stream)), "rt_ao")
    return out


def denoise_scratch_bytes(width, height):
    """rt_denoise_scratch_bytes: bytes of scratch rt_denoise needs for a width x height frame."""
    return int(lib().rt_denoise_scratch_bytes(int(width), int(height)))


def _allocating_on(stream):
    """Context in which torch allocates (and fills) on `stream`; None = torch's current stream, as it is."""
    return torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()


def _denoise(surface, hits, materials, width, height, out, scratch, iterations, normal_power_log2, sigma_plane, sigma_color,
             stream):
    w, h = int(width), int(height)
    assert _is_surface(surface, w, h) and _is_hits(hits, w, h)
    need = denoise_scratch_bytes(w, h)
    # what is allocated here is allocated on the stream the kernels run on: the zero fill of `out` is ordered before
    # them, and the caching allocator does not hand the scratch to another stream's work while they still run
    with _allocating_on(stream):
        if out is None:
            out = alloc_surface(w, h, device=surface.device)
        if scratch is None:
            scratch = torch.empty((need // 4,), dtype=torch.float32, device=surface.device)
    assert _is_surface(out, w, h)
    assert scratch.is_cuda and scratch.is_contiguous()
    p = DenoiseParams()
    p.surface, p.pitch = surface.data_ptr(), surface.stride(0) * 4
    p.width, p.height = w, h
    p.hits = hits.data_ptr()
    p.materials, p.material_count = _materials_of(materials)
    p.out, p.out_pitch = out.data_ptr(), out.stride(0) * 4
    p.scratch, p.scratch_bytes = scratch.data_ptr(), scratch.numel() * scratch.element_size()
    p.iterations, p.normal_power_log2 = int(iterations), int(normal_power_log2)
    p.sigma_plane, p.sigma_color = float(sigma_plane), float(sigma_color)
    _check(lib().rt_denoise(ctypes.byref(p), _stream_ptr(stream)), "rt_denoise")
    return out


def denoise_raw(surface, hits, materials, width, height, out=None, scratch=None, iterations=DENOISE_DEFAULT,
                normal_power_log2=DENOISE_DEFAULT, sigma_plane=DENOISE_DEFAULT, sigma_color=DENOISE_DEFAULT, stream=None):
    """rt_denoise on tensors only: `surface` a pitched float4 surface (alloc_surface), `hits` a float32 [H*W, 12]
    tensor of rt_hit rows (record y*W + x, what trace_camera returns), `materials` a float32 CUDA tensor [M, 16]
    of GPUMaterial rows (M may be 0).  Returns `out` (a new surface when None; `out is surface` is allowed).
    `scratch`: any contiguous CUDA tensor of at least denoise_scratch_bytes(width, height) bytes, contents
    irrelevant (allocated when None).  A filter parameter left at DENOISE_DEFAULT takes the library's default
    (DENOISE_DEFAULTS).  Stream-ordered on `stream` (default: torch's current stream); tensors allocated here are
    allocated on that stream, tensors passed in must be safe to use on it."""
    assert isinstance(materials, torch.Tensor)
    return _denoise(surface, hits, materials, width, height, out, scratch, iterations, normal_power_log2, sigma_plane,
                    sigma_color, stream)


def denoise(scene, surface, width, height, hits=None, out=None, scratch=None, iterations=DENOISE_DEFAULT,
            normal_power_log2=DENOISE_DEFAULT, sigma_plane=DENOISE_DEFAULT, sigma_color=DENOISE_DEFAULT, stream=None):
    """A viewable image from one low-sample frame of an uploaded Scene: rt_denoise guided by the camera's
    first-hit records (`hits`, or trace_camera(scene, width, height) when None) and the scene's materials.
    Returns `out` (a new surface when None).  Do not pass the tracer's last-frame surface as `out`: the
    progressive accumulation would then average filtered colours."""
    if hits is None:
        with _allocating_on(stream):
            hits = trace_camera(scene, width, height, stream=stream)
    return _denoise(surface, hits, scene, width, height, out, scratch, iterations, normal_power_log2, sigma_plane,
                    sigma_color, stream)


def _as_camera(camera):
    """A GPUCamera from a GPUCamera or 15 floats in its layout (origin, viewport size, aspect, horizontal,
    vertical, lower-left corner)."""
    if isinstance(camera, GPUCamera):
        return camera
    v = np.ascontiguousarray(camera, dtype=np.float32).reshape(-1)
    assert v.size == 15, "a camera is a GPUCamera or 15 floats"
    return GPUCamera.from_buffer_copy(v.tobytes())


def camera_floats(camera):
    """The 15 floats of a GPUCamera as a numpy float32 array."""
    return np.frombuffer(bytes(_as_camera(camera)), dtype=np.float32).copy()


def _is_surface(t, w, h):
    return (t.dtype == torch.float32 and t.is_cuda and t.dim() == 2 and t.stride(1) == 1 and t.shape[0] >= h
            and t.shape[1] >= 4 * w)


def _is_hits(t, w, h):
    return (t.dtype == torch.float32 and t.is_cuda and t.is_contiguous() and t.dim() == 2 and t.shape[1] == 12
            and t.shape[0] >= w * h)


def _is_history(t, w, h):
    return t.dtype == torch.float32 and t.is_cuda and t.is_contiguous() and t.numel() >= w * h


def reproject_raw(surface, hits, camera, width, height, prev=None, out=None, out_history=None,
                  max_history=REPROJECT_DEFAULT, sigma_plane=REPROJECT_DEFAULT, normal_min=REPROJECT_DEFAULT, stream=None):
    """rt_reproject on tensors only: `surface` a pitched float4 surface holding a frame rendered with frame_index 0,
    `hits` the float32 [H*W, 12] records of trace_camera for `camera` (a GPUCamera, as Scene.camera() returns it after
    the upload, or its 15 floats).  `prev` = (prev_surface, prev_hits, prev_history, prev_camera): what the previous
    call returned and was given; None on the first frame.  Returns (out, out_history): the accumulated surface and
    the float32 [H, W] number of frames it holds per pixel (new tensors when None; `out is surface` is allowed,
    `out is prev_surface` is not).  A filter parameter left at REPROJECT_DEFAULT takes the library's default
    (REPROJECT_DEFAULTS).  Stream-ordered on `stream` (default: torch's current stream); tensors allocated here are
    allocated on that stream, tensors passed in must be safe to use on it."""
    w, h = int(width), int(height)
    assert _is_surface(surface, w, h) and _is_hits(hits, w, h)
    with _allocating_on(stream):
        if out is None:
            out = alloc_surface(w, h, device=surface.device)
        if out_history is None:
            out_history = torch.zeros((h, w), dtype=torch.float32, device=surface.device)
    assert _is_surface(out, w, h) and _is_history(out_history, w, h)
    p = ReprojectParams()
    p.surface, p.pitch, p.hits = surface.data_ptr(), surface.stride(0) * 4, hits.data_ptr()
    p.out, p.out_pitch, p.out_history = out.data_ptr(), out.stride(0) * 4, out_history.data_ptr()
    p.camera = _as_camera(camera)
    if prev is not None:
        prev_surface, prev_hits, prev_history, prev_camera = prev
        assert _is_surface(prev_surface, w, h) and _is_hits(prev_hits, w, h) and _is_history(prev_history, w, h)
        p.prev_surface, p.prev_pitch = prev_surface.data_ptr(), prev_surface.stride(0) * 4
        p.prev_hits, p.prev_history = prev_hits.data_ptr(), prev_history.data_ptr()
        p.prev_camera = _as_camera(prev_camera)
    p.width, p.height = w, h
    p.max_history, p.sigma_plane, p.normal_min = int(max_history), float(sigma_plane), float(normal_min)
    _check(lib().rt_reproject(ctypes.byref(p), _stream_ptr(stream)), "rt_reproject")
    return out, out_history


class TemporalAccumulator:
    """Temporal accumulation of a moving camera's frames (rt_reproject): two accumulated surfaces, two histories
    and two hit buffers used in turn, plus the previous camera.  **filter_params are reproject_raw's max_history,
    sigma_plane and normal_min.  Static geometry only."""

    def __init__(self, width, height, **filter_params):
        assert not set(filter_params) - set(REPROJECT_DEFAULTS), sorted(set(filter_params) - set(REPROJECT_DEFAULTS))
        self.width, self.height = int(width), int(height)
        self.filter_params = dict(filter_params)
        self._slots = [None, None]  # (surface, hits, history), allocated at first use
        self.reset()

    def reset(self):
        """Forget the history: the next push starts a new accumulation."""
        self._latest = None  # index of the slot the last push wrote
        self._camera = None

    def push(self, scene, surface, hits=None, stream=None):
        """Accumulate `surface`, a frame of the uploaded `scene`'s current camera rendered with frame_index 0; `hits`:
        that camera's trace_camera records (traced here when None).  Returns the accumulated surface, which stays
        valid until the next-but-one push."""
        w, h = self.width, self.height
        camera = scene.camera()
        k = 0 if self._latest is None else 1 - self._latest
        with _allocating_on(stream):
            if self._slots[k] is None:
                self._slots[k] = (alloc_surface(w, h, device=surface.device),
                                  torch.empty((w * h, 12), dtype=torch.float32, device=surface.device),
                                  torch.zeros((h, w), dtype=torch.float32, device=surface.device))
            out, own_hits, history = self._slots[k]
            if hits is None:
                trace_camera(scene, w, h, hits=own_hits, stream=stream)
            else:
                assert _is_hits(hits, w, h)
                own_hits.copy_(hits[: w * h])
        prev = None
        if self._latest is not None:
            prev = (*self._slots[self._latest], self._camera)
        reproject_raw(surface, own_hits, camera, w, h, prev=prev, out=out, out_history=history, stream=stream,
                      **self.filter_params)
        self._latest, self._camera = k, camera
        return out

    @property
    def history(self):
        """[H, W] view of the latest history: the number of frames the latest accumulated surface holds per pixel
        (None before the first push)."""
        return None if self._latest is None else self._slots[self._latest][2]


def _materials_of(scene_or_materials):
    """(device pointer or None, count) of a Scene's, a GPUScene's or a float32 CUDA [M, 16] tensor's material table."""
    m = scene_or_materials
    if isinstance(m, torch.Tensor):
        assert m.dtype == torch.float32 and m.is_cuda and m.is_contiguous() and m.dim() == 2 and m.shape[1] == 16
        return (m.data_ptr() if m.shape[0] else None), m.shape[0]
    gpu = m.gpu.contents if hasattr(m, "gpu") else m
    return gpu.gpu_materials, gpu.material_count


def moments(scene_or_materials, surface, hits, width, height, out=None, stream=None):
    """rt_moments: the luminance moments (l, l*l, 0, alpha) of one frame, `surface`, divided by its first hits'
    albedo, as a pitched float4 surface -- what a second rt_reproject accumulates for rt_denoise_variance.
    `scene_or_materials`: an uploaded Scene (or GPUScene), or a float32 CUDA tensor [M, 16] of GPUMaterial rows.
    Returns `out` (a new surface when None; `out is surface` is refused).  Stream-ordered on `stream` (default:
    torch's current stream); a surface allocated here is allocated on that stream."""
    w, h = int(width), int(height)
    assert _is_surface(surface, w, h) and _is_hits(hits, w, h)
    with _allocating_on(stream):
        if out is None:
            out = alloc_surface(w, h, device=surface.device)
    assert _is_surface(out, w, h)
    p = MomentsParams()
    p.surface, p.pitch, p.width, p.height = surface.data_ptr(), surface.stride(0) * 4, w, h
    p.hits = hits.data_ptr()
    p.materials, p.material_count = _materials_of(scene_or_materials)
    p.out, p.out_pitch = out.data_ptr(), out.stride(0) * 4
    _check(lib().rt_moments(ctypes.byref(p), _stream_ptr(stream)), "rt_moments")
    return out


def denoise_variance_scratch_bytes(width, height):
    """rt_denoise_variance_scratch_bytes: bytes of scratch rt_denoise_variance needs for a width x height frame."""
    return int(lib().rt_denoise_variance_scratch_bytes(int(width), int(height)))


def _denoise_variance(surface, hits, materials, width, height, moments, history, out, out_variance, scratch, iterations,
                      normal_power_log2, sigma_plane, sigma_lum, min_history, stream):
    w, h = int(width), int(height)
    assert _is_surface(surface, w, h) and _is_hits(hits, w, h)
    assert moments is None or _is_surface(moments, w, h)
    assert history is None or _is_history(history, w, h)
    need = denoise_variance_scratch_bytes(w, h)
    # allocated on the stream the kernels run on, as in _denoise
    with _allocating_on(stream):
        if out is None:
            out = alloc_surface(w, h, device=surface.device)
        if out_variance is None:
            out_variance = torch.zeros((h, w), dtype=torch.float32, device=surface.device)
        if scratch is None:
            scratch = torch.empty((need // 4,), dtype=torch.float32, device=surface.device)
    assert _is_surface(out, w, h) and _is_history(out_variance, w, h)
    assert scratch.is_cuda and scratch.is_contiguous()
    p = DenoiseVarianceParams()
    p.surface, p.pitch, p.width, p.height = surface.data_ptr(), surface.stride(0) * 4, w, h
    p.hits = hits.data_ptr()
    p.materials, p.material_count = _materials_of(materials)
    if moments is not None:
        p.moments, p.moments_pitch = moments.data_ptr(), moments.stride(0) * 4
    if history is not None:
        p.history = history.data_ptr()
    p.out, p.out_pitch, p.out_variance = out.data_ptr(), out.stride(0) * 4, out_variance.data_ptr()
    p.scratch, p.scratch_bytes = scratch.data_ptr(), scratch.numel() * scratch.element_size()
    p.iterations, p.normal_power_log2 = int(iterations), int(normal_power_log2)
    p.sigma_plane, p.sigma_lum, p.min_history = float(sigma_plane), float(sigma_lum), float(min_history)
    _check(lib().rt_denoise_variance(ctypes.byref(p), _stream_ptr(stream)), "rt_denoise_variance")
    return out, out_variance


def denoise_variance_raw(surface, hits, materials, width, height, moments=None, history=None, out=None, out_variance=None,
                         scratch=None, iterations=DENOISE_DEFAULT, normal_power_log2=DENOISE_DEFAULT,
                         sigma_plane=DENOISE_DEFAULT, sigma_lum=DENOISE_DEFAULT, min_history=DENOISE_DEFAULT, stream=None):
    """rt_denoise_variance on tensors only: `surface` the accumulated image (a pitched float4 surface), `hits` the
    float32 [H*W, 12] records of trace_camera, `materials` a float32 CUDA tensor [M, 16] of GPUMaterial rows (M may
    be 0), `moments` the accumulated moments surface (moments() through reproject_raw) and `history` the colour's
    float32 [H, W] history, either or both None.  Returns (out, out_variance): the filtered surface (`out is surface`
    is allowed) and the float32 [H, W] filtered variance of the albedo-divided luminance (new tensors when None).
    `scratch`: any contiguous CUDA tensor of at least denoise_variance_scratch_bytes(width, height) bytes.  A filter
    parameter left at DENOISE_DEFAULT takes the library's default (DENOISE_VARIANCE_DEFAULTS).  Stream-ordered on
    `stream` (default: torch's current stream); tensors allocated here are allocated on that stream, tensors passed
    in must be safe to use on it."""
    assert isinstance(materials, torch.Tensor)
    return _denoise_variance(surface, hits, materials, width, height, moments, history, out, out_variance, scratch,
                             iterations, normal_power_log2, sigma_plane, sigma_lum, min_history, stream)


def denoise_variance(scene, surface, width, height, hits=None, moments=None, history=None, out=None, out_variance=None,
                     scratch=None, iterations=DENOISE_DEFAULT, normal_power_log2=DENOISE_DEFAULT,
                     sigma_plane=DENOISE_DEFAULT, sigma_lum=DENOISE_DEFAULT, min_history=DENOISE_DEFAULT, stream=None):
    """rt_denoise_variance for an uploaded Scene: guided by the camera's first-hit records (`hits`, or
    trace_camera(scene, width, height) when None) and the scene's materials; otherwise denoise_variance_raw.  Feed it
    the accumulated image with the history and moments that belong to it (VarianceAccumulator does all of it)."""
    if hits is None:
        with _allocating_on(stream):
            hits = trace_camera(scene, width, height, stream=stream)
    return _denoise_variance(surface, hits, scene, width, height, moments, history, out, out_variance, scratch,
                             iterations, normal_power_log2, sigma_plane, sigma_lum, min_history, stream)


def upsample_scratch_bytes(low_width, low_height):
    """rt_upsample_scratch_bytes: bytes of scratch rt_upsample needs for a low frame of low_width x low_height pixels."""
    return int(lib().rt_upsample_scratch_bytes(int(low_width), int(low_height)))


def _upsample(low_surface, low_hits, hits, materials, low_width, low_height, scale, out, scratch, normal_power_log2,
              sigma_plane, stream):
    lw, lh, s = int(low_width), int(low_height), int(scale)
    w, h = lw * s, lh * s
    assert _is_surface(low_surface, lw, lh) and _is_hits(low_hits, lw, lh) and _is_hits(hits, w, h)
    need = upsample_scratch_bytes(lw, lh)
    with _allocating_on(stream):  # as _denoise: what is allocated here is allocated on the stream the kernels run on
        if out is None:
            out = alloc_surface(w, h, device=low_surface.device)
        if scratch is None:
            scratch = torch.empty((need // 4,), dtype=torch.float32, device=low_surface.device)
    assert _is_surface(out, w, h)
    assert scratch.is_cuda and scratch.is_contiguous()
    p = UpsampleParams()
    p.low_surface, p.low_pitch = low_surface.data_ptr(), low_surface.stride(0) * 4
    p.low_hits, p.hits = low_hits.data_ptr(), hits.data_ptr()
    p.low_width, p.low_height, p.scale = lw, lh, s
    p.materials, p.material_count = _materials_of(materials)
    p.out, p.out_pitch = out.data_ptr(), out.stride(0) * 4
    p.scratch, p.scratch_bytes = scratch.data_ptr(), scratch.numel() * scratch.element_size()
    p.normal_power_log2, p.sigma_plane = int(normal_power_log2), float(sigma_plane)
    _check(lib().rt_upsample(ctypes.byref(p), _stream_ptr(stream)), "rt_upsample")
    return out


def upsample_raw(low_surface, low_hits, hits, materials, low_width, low_height, scale, out=None, scratch=None,
                 normal_power_log2=UPSAMPLE_DEFAULT, sigma_plane=UPSAMPLE_DEFAULT, stream=None):
    """rt_upsample on tensors only: `low_surface` a pitched float4 surface of low_width x low_height pixels, `low_hits`
    and `hits` float32 [N, 12] tensors of rt_hit rows of one camera at the low size and at the output size
    (scale * low_width x scale * low_height; scale 2, 3 or 4), `materials` a float32 CUDA tensor [M, 16] of
    GPUMaterial rows (M may be 0).  Returns `out`, a surface of the output size (a new one when None; it may overlap
    none of the inputs).  `scratch`: any contiguous CUDA tensor of at least upsample_scratch_bytes(low_width,
    low_height) bytes, contents irrelevant (allocated when None).  A filter parameter left at UPSAMPLE_DEFAULT takes
    the library's default (UPSAMPLE_DEFAULTS).  Stream-ordered on `stream` (default: torch's current stream); tensors
    allocated here are allocated on that stream, tensors passed in must be safe to use on it."""
    assert isinstance(materials, torch.Tensor)
    return _upsample(low_surface, low_hits, hits, materials, low_width, low_height, scale, out, scratch,
                     normal_power_log2, sigma_plane, stream)


def upsample(scene, low_surface, low_width, low_height, scale, low_hits=None, hits=None, out=None, scratch=None,
             normal_power_log2=UPSAMPLE_DEFAULT, sigma_plane=UPSAMPLE_DEFAULT, stream=None):
    """A frame of scale * low_width x scale * low_height pixels from a frame of an uploaded Scene rendered at low_width x
    low_height: rt_upsample guided by the camera's first-hit records at both sizes (`low_hits`, `hits`; each traced
    with trace_camera on the call's stream when None -- the uploaded camera serves both sizes, its aspect being the
    same) and the scene's materials.  Returns `out` (a new surface when None)."""
    lw, lh, s = int(low_width), int(low_height), int(scale)
    with _allocating_on(stream):
        if low_hits is None:
            low_hits = trace_camera(scene, lw, lh, stream=stream)
        if hits is None:
            hits = trace_camera(scene, lw * s, lh * s, stream=stream)
    return _upsample(low_surface, low_hits, hits, scene, lw, lh, s, out, scratch, normal_power_log2, sigma_plane, stream)


class VarianceAccumulator:
    """The per-frame chain of the variance-steered filter: rt_reproject on the colour (a TemporalAccumulator),
    rt_moments on the new frame, rt_reproject on the moments with a history of their own, rt_denoise_variance on
    the accumulated image.  **filter_params are denoise_variance_raw's iterations, normal_power_log2, sigma_plane,
    sigma_lum and min_history; `reproject_params` (a dict) are reproject_raw's max_history, sigma_plane and
    normal_min, used for both reprojections.  Static geometry only."""

    def __init__(self, width, height, reproject_params=None, **filter_params):
        unknown = set(filter_params) - set(DENOISE_VARIANCE_DEFAULTS)
        assert not unknown, sorted(unknown)
        self.width, self.height = int(width), int(height)
        self.filter_params = dict(filter_params)
        self._colour = TemporalAccumulator(width, height, **(reproject_params or {}))
        self._moment_slots = [None, None]  # (accumulated moments, their history)
        self._buffers = None               # (moments of the frame, filtered image, variance, scratch)
        self.reset()

    @property
    def reproject_params(self):
        return self._colour.filter_params

    def reset(self):
        """Forget the history: the next push starts a new accumulation."""
        self._colour.reset()
        self._pushed = False

    def push(self, scene, surface, hits=None, stream=None):
        """Accumulate `surface`, a frame of the uploaded `scene`'s current camera rendered with frame_index 0, and
        filter the accumulated image; `hits`: that camera's trace_camera records (traced here when None).  Returns
        the filtered surface, valid until the next push."""
        w, h = self.width, self.height
        before, prev_camera = self._colour._latest, self._colour._camera
        accumulated = self._colour.push(scene, surface, hits=hits, stream=stream)
        k = self._colour._latest
        _, own_hits, history = self._colour._slots[k]
        with _allocating_on(stream):
            if self._moment_slots[k] is None:
                self._moment_slots[k] = (alloc_surface(w, h, device=surface.device),
                                         torch.zeros((h, w), dtype=torch.float32, device=surface.device))
            if self._buffers is None:
                self._buffers = (alloc_surface(w, h, device=surface.device), alloc_surface(w, h, device=surface.device),
                                 torch.zeros((h, w), dtype=torch.float32, device=surface.device),
                                 torch.empty((denoise_variance_scratch_bytes(w, h) // 4,), dtype=torch.float32,
                                             device=surface.device))
        frame_moments, filtered, variance, scratch = self._buffers
        moments(scene, surface, own_hits, w, h, out=frame_moments, stream=stream)
        prev = None
        if before is not None:
            prev = (self._moment_slots[before][0], self._colour._slots[before][1], self._moment_slots[before][1], prev_camera)
        acc_moments, moments_history = self._moment_slots[k]
        reproject_raw(frame_moments, own_hits, self._colour._camera, w, h, prev=prev, out=acc_moments,
                      out_history=moments_history, stream=stream, **self._colour.filter_params)
        _denoise_variance(accumulated, own_hits, scene, w, h, acc_moments, history, filtered, variance, scratch,
                          stream=stream, **{**{k_: DENOISE_DEFAULT for k_ in DENOISE_VARIANCE_DEFAULTS}, **self.filter_params})
        self._pushed = True
        return filtered

    @property
    def accumulated(self):
        """The latest accumulated (unfiltered) surface (None before the first push)."""
        return None if not self._pushed else self._colour._slots[self._colour._latest][0]

    @property
    def history(self):
        """[H, W]: the number of frames the accumulated surface holds per pixel (None before the first push)."""
        return None if not self._pushed else self._colour.history

    @property
    def moments(self):
        """The latest accumulated moments surface (None before the first push)."""
        return None if not self._pushed else self._moment_slots[self._colour._latest][0]

    @property
    def variance(self):
        """[H, W]: the filtered variance of the albedo-divided luminance of the latest filtered image (None before
        the first push)."""
        return None if not self._pushed else self._buffers[2]


def foreign_mirror_wait(gpu_scene):
    """rt_foreign_mirror_wait: block until the background mirror build of a foreign GPUScene (a
    ctypes GPUScene filled by the caller) has finished; the next render installs it."""
    _check(lib().rt_foreign_mirror_wait(ctypes.byref(gpu_scene)), "rt_foreign_mirror_wait")


def foreign_last_tracer(gpu_scene):
    """rt_foreign_last_tracer: 1 production tracer, 0 reference layout (fingerprint mismatch),
    -1 no mirror yet (test diagnostics; synchronises the device)."""
    return int(lib().rt_foreign_last_tracer(ctypes.byref(gpu_scene)))


def cluster_cull_host(origin, nd, best, node):
    """The render kernel's leaf-tree cull predicate (rt_fast.h cluster_cull) on the host."""
    import numpy as np
    o = np.ascontiguousarray(origin, dtype=np.float32)
    d = np.ascontiguousarray(nd, dtype=np.float32)
    k = np.ascontiguousarray(node, dtype=np.float32)
    return bool(lib().rt_cluster_cull_host(o.ctypes.data, d.ctypes.data, float(best), k.ctypes.data))


def shard_tiles(width, height, shard_index, shard_count):
    return int(lib().rt_shard_tiles(width, height, shard_index, shard_count))


tiles_of = shard_tiles


def shard_plan(width, height, shard_count, tile_cost=None):
    """rt_shard_plan: (tile_lists int32 [shard_count, capacity] -1 padded, counts int64 [shard_count])
    on the host; tile_cost None = round-robin, else longest-processing-time-first."""
    cap = int(lib().rt_shard_plan_capacity(width, height, shard_count))
    lists = np.zeros((shard_count, cap), dtype=np.int32)
    counts = np.zeros((shard_count,), dtype=np.int64)
    cost_ptr = None
    if tile_cost is not None:
        cost = np.ascontiguousarray(tile_cost, dtype=np.float64)
        assert cost.size == sharding.tiles_total(width, height)
        cost_ptr = cost.ctypes.data
    _check(lib().rt_shard_plan(width, height, shard_count, cost_ptr, cap, lists.ctypes.data, counts.ctypes.data),
           "rt_shard_plan")
    return lists, counts


def build_options():
    """Current rt_build_options (a BuildOptions)."""
    o = BuildOptions()
    lib().rt_get_build_options(ctypes.byref(o))
    return o


def set_build_options(**changes):
    """rt_set_build_options with the given fields changed (no arguments: the defaults)."""
    if not changes:
        _check(lib().rt_set_build_options(None), "rt_set_build_options")
        return
    o = build_options()
    for k, v in changes.items():
        setattr(o, k, v)
    _check(lib().rt_set_build_options(ctypes.byref(o)), "rt_set_build_options")


def lane_plan(cost, parallel_units=48000.0, slack=1.0):
    """rt_lane_plan: (int32 numpy lane map, number of leading long waves) from per-slot work
    (numpy uint32/int32 [slots], a probe frame's lane_cost)."""
    cost = np.ascontiguousarray(np.asarray(cost).astype(np.uint32))
    cap = int(lib().rt_lane_plan_capacity(cost.size))
    out = np.empty(max(cap, 1), dtype=np.int32)
    nlong = ctypes.c_int64(0)
    n = int(lib().rt_lane_plan(cost.ctypes.data, cost.size, float(parallel_units), float(slack), out.ctypes.data, cap,
                               ctypes.byref(nlong)))
    if n < 0:
        raise RTError("rt_lane_plan failed: " + lib().rt_last_error().decode(errors="replace"))
    return out[:n].copy(), int(nlong.value)


def lane_refine(lane_map, cost, wave_ticks, theta=0.75):
    """rt_lane_refine: (int32 numpy lane map, waves made by splitting) -- the waves of `lane_map`
    whose measured clock (numpy int64 [waves], a timing frame's wave_clock) is within theta of the
    longest split in two, all waves ordered longest first."""
    m = np.ascontiguousarray(np.asarray(lane_map, dtype=np.int32).ravel())
    cost = np.ascontiguousarray(np.asarray(cost).astype(np.uint32))
    ticks = np.ascontiguousarray(np.asarray(wave_ticks, dtype=np.int64))
    assert m.size % 64 == 0 and ticks.size >= m.size // 64
    out = np.empty(2 * m.size, dtype=np.int32)
    nsplit = ctypes.c_int64(0)
    n = int(lib().rt_lane_refine(m.ctypes.data, m.size, cost.ctypes.data, cost.size, ticks.ctypes.data, float(theta),
                                 out.ctypes.data, out.size, ctypes.byref(nsplit)))
    if n < 0:
        raise RTError("rt_lane_refine failed: " + lib().rt_last_error().decode(errors="replace"))
    return out[:n].copy(), int(nsplit.value)


def lone_plan(cost, max_lone, min_cost=1):
    """rt_lone_plan: (int32 numpy lone slots, heaviest first; the cost array with those slots marked
    for rt_lane_plan) from per-slot work (a probe frame's lane_cost)."""
    cost = np.ascontiguousarray(np.asarray(cost).astype(np.uint32)).copy()
    out = np.empty(max(int(max_lone), 1), dtype=np.int32)
    n = int(lib().rt_lone_plan(cost.ctypes.data, cost.size, int(max_lone), int(min_cost), out.ctypes.data))
    if n < 0:
        raise RTError("rt_lone_plan failed: " + lib().rt_last_error().decode(errors="replace"))
    return out[:n].copy(), cost


def init_rng_tiles(rng, width, height, tile_list, seed, stream=None):
    """rt_init_rng_tiles: compact states for a device int32 tile list."""
    _check(lib().rt_init_rng_tiles(ctypes.c_void_p(rng.data_ptr()), width, height, ctypes.c_void_p(tile_list.data_ptr()),
                                   tile_list.numel(), seed, _stream_ptr(stream)), "rt_init_rng_tiles")


def unshard_tiles(surface, width, height, shards, tile_lists, stream=None):
    """rt_unshard_tiles: shards [N, capacity*256, 4] f32, tile_lists device int32 [N, capacity]."""
    n, cap = tile_lists.shape
    _check(lib().rt_unshard_tiles(ctypes.c_void_p(surface.data_ptr()), surface.shape[1] * 4, width, height, n,
                                  ctypes.c_void_p(shards.data_ptr()), cap, ctypes.c_void_p(tile_lists.data_ptr()),
                                  _stream_ptr(stream)), "rt_unshard_tiles")


class Comm:
    """rt_comm (RCCL) for the frame-end gather.  Rank 0 makes the id (``unique_id()``); the caller
    hands it to every rank; each rank constructs ``Comm(nranks, rank, id)`` on its device."""

    ID_BYTES = 128

    @staticmethod
    def unique_id():
        buf = (ctypes.c_uint8 * Comm.ID_BYTES)()
        _check(lib().rt_comm_unique_id(buf), "rt_comm_unique_id")
        return bytes(buf)

    def __init__(self, nranks, rank, uid):
        assert len(uid) == Comm.ID_BYTES
        self.handle = ctypes.c_void_p()
        buf = (ctypes.c_uint8 * Comm.ID_BYTES)(*uid)
        _check(lib().rt_comm_init_rank(ctypes.byref(self.handle), nranks, rank, buf), "rt_comm_init_rank")
        self.rank, self.nranks = rank, nranks

    def gather(self, shard, shard_bytes, gathered=None, stride=0, recv_bytes=None, root=0, stream=None):
        rb = None
        if recv_bytes is not None:
            rb = (ctypes.c_size_t * self.nranks)(*[int(b) for b in recv_bytes])
        _check(lib().rt_gather_shards(self.handle, ctypes.c_void_p(shard.data_ptr()), int(shard_bytes),
                                      ctypes.c_void_p(gathered.data_ptr() if gathered is not None else None),
                                      int(stride), rb, root, _stream_ptr(stream)), "rt_gather_shards")

    def close(self):
        if self.handle:
            _check(lib().rt_comm_destroy(self.handle), "rt_comm_destroy")
            self.handle = ctypes.c_void_p()


def unshard(surface, width, height, shard_count, shards, per_shard, stream=None):
    _check(lib().rt_unshard(ctypes.c_void_p(surface.data_ptr()), surface.shape[1] * 4, width, height, shard_count,
                            ctypes.c_void_p(shards.data_ptr()), per_shard, _stream_ptr(stream)), "rt_unshard")


def tonemap(surface, width, height, stream=None):
    """The reference viewer's display transform (main.cpp:78-94 into an sRGB back buffer):
    [H, W, 3] uint8 on the GPU, rows top to bottom."""
    out = torch.empty((height, width, 3), dtype=torch.uint8, device=surface.device)
    _check(lib().rt_tonemap_srgb8(ctypes.c_void_p(surface.data_ptr()), surface.shape[1] * 4, width, height,
                                  ctypes.c_void_p(out.data_ptr()), _stream_ptr(stream)), "rt_tonemap_srgb8")
    return out


def write_pfm(path, surface, width, height):
    """Linear RGB of a pitched float4 surface (torch, any device; or a numpy [H, row] array) as
    PFM, rows bottom to top -- the surface's own order."""
    host = surface.detach().to("cpu").contiguous().numpy() if isinstance(surface, torch.Tensor) else np.ascontiguousarray(surface, dtype=np.float32)
    _check(lib().rt_write_pfm(os.fsencode(path), host.ctypes.data, host.shape[1] * 4, width, height), "rt_write_pfm")


def write_ppm(path, rgb):
    """[H, W, 3] uint8 (tonemap's output, any device) as binary PPM."""
    host = rgb.detach().to("cpu").contiguous().numpy() if isinstance(rgb, torch.Tensor) else np.ascontiguousarray(rgb, dtype=np.uint8)
    _check(lib().rt_write_ppm(os.fsencode(path), host.ctypes.data, host.shape[1], host.shape[0]), "rt_write_ppm")


def raytracing_process(surface, last, width, height, frame_index, scene):
    """The reference entry point (main_raytracing.cu:202): spp 5, 6 bounces, null stream."""
    lib().raytracing_process(ctypes.c_void_p(surface.data_ptr()), ctypes.c_void_p(last.data_ptr()), width, height,
                             surface.shape[1] * 4, frame_index, ctypes.cast(scene.gpu, ctypes.c_void_p))


def init_rng(thread_block_count, thread_block_size, rng, seed):
    """The reference entry point (Random.cu:10)."""
    lib().init_rng(thread_block_count, thread_block_size, ctypes.c_void_p(rng.data_ptr()), seed)


class RayTracer:
    """CUDARayTracer mirror (RayTracing/RayTracing.{h,cpp}), headless.

    ``process()`` = one progressive frame: lazy RNG init (fixed seed instead of the
    reference's time-based one), camera update + upload, render, copy to the last-frame
    surface, frame_index++ (RayTracing.cpp:205-234).
    """

    def __init__(self, width, height, scene="bunny", spp=REFERENCE_SPP, bounces=REFERENCE_BOUNCES, seed=0xDEADBEEF):
        self.width, self.height, self.spp, self.bounces, self.seed = width, height, spp, bounces, seed
        self.scene = Scene()
        self.scene.setup(scene)
        self.surface = alloc_surface(width, height)
        self.last_frame = alloc_surface(width, height)
        self.rng = None
        self.frame_index = 0
        self._accumulator = None  # reprojected()'s TemporalAccumulator

    def on_resize(self, width, height):
        self.width, self.height = width, height
        self.surface = alloc_surface(width, height)
        self.last_frame = alloc_surface(width, height)
        self.rng = None
        self.frame_index = 0
        self._accumulator = None
        self._variance_accumulator = None

    def process(self, stats=None):
        if self.rng is None:
            self.rng = alloc_rng(self.width * self.height)
            init_rng_states(self.rng, self.width, self.height, self.seed)
        self.scene.set_viewport(self.width, self.height)
        self.scene.upload(self.rng.data_ptr())
        render(self.scene, self.surface, self.last_frame, self.width, self.height, self.spp, self.bounces,
               frame_index=self.frame_index, stats=stats)
        self.last_frame.copy_(self.surface)
        self.frame_index += 1
        return surface_view(self.surface, self.width)

    def gbuffer(self, stream=None, waves_per_simd=0):
        """First-hit images of the current camera and size (module-level gbuffer()).  Uploads the scene
        like process(); the frame index, the surfaces and the RNG states are left alone."""
        self.scene.set_viewport(self.width, self.height)
        self.scene.upload(self.rng.data_ptr() if self.rng is not None else 0)
        return gbuffer(self.scene, self.width, self.height, stream=stream, waves_per_simd=waves_per_simd)

    def denoised(self, **kw):
        """A denoised copy of the current frame as a new pitched surface (module-level denoise(); **kw are its
        filter parameters, hits, scratch, stream).  Uploads the scene like process(); `surface`, `last_frame`,
        the RNG states and the frame index are left alone."""
        assert "out" not in kw, "RayTracer.denoised returns a new surface"
        self.scene.set_viewport(self.width, self.height)
        self.scene.upload(self.rng.data_ptr() if self.rng is not None else 0)
        return denoise(self.scene, self.surface, self.width, self.height, **kw)

    def upsampled(self, scale=2, denoise=False, **kw):
        """The current frame as a new pitched surface of scale * width x scale * height pixels (module-level
        upsample(); **kw are its filter parameters, low_hits, hits, scratch, stream).  With denoise=True the frame
        goes through rt_denoise (its defaults) first.  Uploads the scene like process(); `surface`, `last_frame`, the
        RNG states and the frame index are left alone."""
        assert "out" not in kw, "RayTracer.upsampled returns a new surface"
        self.scene.set_viewport(self.width, self.height)
        self.scene.upload(self.rng.data_ptr() if self.rng is not None else 0)
        stream = kw.get("stream")
        with _allocating_on(stream):
            if kw.get("low_hits") is None:
                kw["low_hits"] = trace_camera(self.scene, self.width, self.height, stream=stream)
        low = self.surface
        if denoise:
            low = _denoise(low, kw["low_hits"], self.scene, self.width, self.height, None, None, DENOISE_DEFAULT,
                           DENOISE_DEFAULT, DENOISE_DEFAULT, DENOISE_DEFAULT, stream)
        return upsample(self.scene, low, self.width, self.height, scale, **kw)

    def ao(self, radius, **kw):
        """The ambient-occlusion image [H, W] of the current camera and size (module-level ambient_occlusion();
        **kw are its samples, bias, directions, hits, stream, ...).  Uploads the scene like process(); the frame
        index, the surfaces and the RNG states are left alone."""
        self.scene.set_viewport(self.width, self.height)
        self.scene.upload(self.rng.data_ptr() if self.rng is not None else 0)
        stream = kw.get("stream")
        hits = kw.pop("hits", None)
        if hits is None:
            with _allocating_on(stream):
                hits = trace_camera(self.scene, self.width, self.height, stream=stream)
        return ambient_occlusion(self.scene, hits, self.width, self.height, radius, **kw)

    def closest_points(self, points, **kw):
        """The nearest surface point of every row of a [N, 4] point tensor (module-level closest_points(); **kw are
        its out, waves_per_simd, stream).  Uploads the scene like process() and works before any frame is rendered;
        the frame index, the surfaces and the RNG states are left alone."""
        self.scene.set_viewport(self.width, self.height)
        self.scene.upload(self.rng.data_ptr() if self.rng is not None else 0)
        return closest_points(self.scene, points, **kw)

    def layers(self, max_hits, flags=0, stream=None, waves_per_simd=0):
        """The first `max_hits` surfaces behind every pixel (trace_hits_camera: the pixel centres, no jitter) as device
        tensors, rows bottom to top like the surface: depth [H, W, K] (t; inf past the last hit), prim (sphere or face
        index, -1 past the last hit) and kind [H, W, K] int32, and count [H, W] int32 (the list length, or with
        RT_HITS_COUNT_ALL in `flags` every hit below tmax).  Uploads the scene like process(); the frame index, the
        surfaces and the RNG states are left alone."""
        self.scene.set_viewport(self.width, self.height)
        self.scene.upload(self.rng.data_ptr() if self.rng is not None else 0)
        w, h, k = self.width, self.height, int(max_hits)
        hits, counts = trace_hits_camera(self.scene, w, h, k, flags=flags, stream=stream, waves_per_simd=waves_per_simd)
        with _allocating_on(stream):
            f = hit_fields(hits.reshape(w * h * k, 12))
            hit = f["kind"] != HIT_MISS
            return {"depth": torch.where(hit, f["t"], torch.full_like(f["t"], float("inf"))).reshape(h, w, k),
                    "prim": torch.where(hit, f["id"], torch.full_like(f["id"], -1)).reshape(h, w, k),
                    "kind": f["kind"].reshape(h, w, k).clone(), "count": counts.reshape(h, w)}

    def panorama(self, width, height, origin=None, samples=None, bounces=None, seed=None, stream=None):
        """A width x height equirectangular panorama of the scene seen from `origin` (default: the camera's position),
        as a new pitched surface (alloc_surface layout, rows bottom to top): radiance() along panorama_rays(), `samples`
        paths per pixel (default: spp), `bounces` (default: the tracer's), states ray_rng(width * height, seed) (default:
        the tracer's seed).  Uploads the scene like process(); the frame index, the surfaces and the tracer's RNG states
        are left alone."""
        w, h = int(width), int(height)
        self.scene.set_viewport(self.width, self.height)
        self.scene.upload(self.rng.data_ptr() if self.rng is not None else 0)
        return panorama(self.scene, w, h, origin=origin, samples=self.spp if samples is None else samples,
                        bounces=self.bounces if bounces is None else bounces, seed=self.seed if seed is None else seed,
                        device=self.surface.device, stream=stream)

    def adaptive(self, rounds, budget_spp, warmup=2, bounces=None, seed=None, stream=None, **kw):
        """An adaptively sampled image of the current camera and size: a new AdaptiveSampler, warmup(`warmup`), then
        `rounds` steps of budget_spp samples per pixel each (**kw are step()'s min_samples, max_samples, scale).
        Returns the sampler: image() is the picture, counts() the samples per pixel.  Uploads the scene like
        process(); the frame index, the surfaces and the tracer's RNG states are left alone."""
        self.scene.set_viewport(self.width, self.height)
        self.scene.upload(self.rng.data_ptr() if self.rng is not None else 0)
        sampler = AdaptiveSampler(self.scene, self.width, self.height, bounces=self.bounces if bounces is None else bounces,
                                  seed=self.seed if seed is None else seed, device=self.surface.device, stream=stream)
        sampler.warmup(warmup)
        for _ in range(int(rounds)):
            sampler.step(budget_spp, **kw)
        return sampler

    def reprojected(self, **kw):
        """The current frame accumulated with the frames of earlier calls, whatever cameras they had (a lazily
        created TemporalAccumulator; **kw are its filter parameters, and push's hits and stream).  Meant for frames
        rendered with frame_index == 0: set ``tracer.frame_index = 0`` after moving the camera, as the reference's
        Process() does on its dirty flag, then process(), then this.  Returns the accumulated surface, valid until
        the next-but-one call.  Uploads the scene like process(); `surface`, `last_frame`, the RNG states and the
        frame index are left alone.  on_resize drops the accumulator."""
        self.scene.set_viewport(self.width, self.height)
        self.scene.upload(self.rng.data_ptr() if self.rng is not None else 0)
        push_kw = {k: kw.pop(k) for k in ("hits", "stream") if k in kw}
        if self._accumulator is None:
            self._accumulator = TemporalAccumulator(self.width, self.height)
        assert not set(kw) - set(REPROJECT_DEFAULTS), sorted(set(kw) - set(REPROJECT_DEFAULTS))
        self._accumulator.filter_params.update(kw)
        return self._accumulator.push(self.scene, self.surface, **push_kw)

    def filtered(self, **kw):
        """The current frame accumulated with the frames of earlier calls and filtered by rt_denoise_variance (a
        lazily created VarianceAccumulator, kept apart from reprojected()'s accumulator; **kw are its filter
        parameters, `reproject_params`, and push's hits and stream).  Meant for frames rendered with frame_index == 0,
        like reprojected().  Returns the filtered surface, valid until the next call; the accumulator itself
        (accumulated image, history, variance) is `tracer.variance_accumulator`.  Uploads the scene like process();
        `surface`, `last_frame`, the RNG states and the frame index are left alone.  on_resize drops the accumulator."""
        self.scene.set_viewport(self.width, self.height)
        self.scene.upload(self.rng.data_ptr() if self.rng is not None else 0)
        push_kw = {k: kw.pop(k) for k in ("hits", "stream") if k in kw}
        reproject_params = kw.pop("reproject_params", None)
        acc = self.variance_accumulator
        if acc is None or (acc.width, acc.height) != (self.width, self.height):
            acc = self._variance_accumulator = VarianceAccumulator(self.width, self.height)
        assert not set(kw) - set(DENOISE_VARIANCE_DEFAULTS), sorted(set(kw) - set(DENOISE_VARIANCE_DEFAULTS))
        acc.filter_params.update(kw)
        acc.reproject_params.update(reproject_params or {})
        return acc.push(self.scene, self.surface, **push_kw)

    @property
    def variance_accumulator(self):
        """filtered()'s VarianceAccumulator (None before the first call and after on_resize)."""
        return getattr(self, "_variance_accumulator", None)

    def save(self, path):
        """The current frame: ``.pfm`` linear RGB, ``.ppm`` as the reference's viewer shows it
        (exposure 0.5, ACES film, sRGB; main.cpp:78-94, 438)."""
        if str(path).lower().endswith(".pfm"):
            write_pfm(path, self.surface, self.width, self.height)
        elif str(path).lower().endswith(".ppm"):
            write_ppm(path, tonemap(self.surface, self.width, self.height))
        else:
            raise ValueError("RayTracer.save: .pfm or .ppm")


from . import sharding  # noqa: E402  (multi-GPU tile bookkeeping; the data path is in librt_hip.so)
