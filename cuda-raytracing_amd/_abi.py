"""The C-ABI of librt_hip.so as ctypes (include/rt_abi.h): its structures, the constants that mirror it, the signature
of every symbol, and the one place the two libraries are loaded (`_lib`, `_exp_lib`)."""
import ctypes
import os

import torch  # noqa: F401  imported before the library so librt_hip.so binds to the HIP runtime torch already loaded

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
ROOT_DIR = os.path.dirname(PKG_DIR)
LIB_PATH = os.path.join(PKG_DIR, "librt_hip.so")
EXP_LIB_PATH = os.path.join(PKG_DIR, "librt_hip_exp.so")  # experimental render paths (A/B + their tests)
ASSETS_DIR = os.path.join(ROOT_DIR, "assets")

RT_RENDER_STATS, RT_RENDER_VALIDATE = 1, 16  # rt_render_params.flags, with one of:
TRACERS = {"fast": 0, "ref": 2, "flat": 4, "wavefront": 8}
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

HIT_MISS, HIT_SPHERE, HIT_TRIANGLE = 0, 1, 2  # rt_hit.kind
NEAREST_MISS, NEAREST_SPHERE, NEAREST_FACE = 0, 1, 2  # rt_nearest.kind
HITS_MAX = 16  # RT_HITS_MAX
RT_HITS_CULL_BACK, RT_HITS_CULL_FRONT, RT_HITS_COUNT_ALL = 1, 2, 4  # rt_hits_params.flags
RAY_TMAX = 1e30  # the renderer's own initial closest distance (main_raytracing.cu:85)
DENOISE_DEFAULT = -1  # RT_DENOISE_DEFAULT: in a filter parameter of rt_denoise, the measured default
# the defaults rt_denoise substitutes (csrc/denoise.hip; profiles/denoise_quality.txt)
DENOISE_DEFAULTS = {"iterations": 5, "normal_power_log2": 5, "sigma_plane": 0.03, "sigma_color": 8.0}
REPROJECT_DEFAULT = -1  # RT_REPROJECT_DEFAULT: in a filter parameter of rt_reproject, the measured default
# the defaults rt_reproject substitutes (csrc/reproject.hip; profiles/reproject_quality.txt)
REPROJECT_DEFAULTS = {"max_history": 32, "sigma_plane": 0.03, "normal_min": 0.9}
# the defaults rt_denoise_variance substitutes (csrc/denoise_variance.hip; profiles/variance_quality.txt)
DENOISE_VARIANCE_DEFAULTS = {"iterations": 5, "normal_power_log2": 5, "sigma_plane": 0.03, "sigma_lum": 4.0, "min_history": 4.0}
UPSAMPLE_DEFAULT = -1  # RT_UPSAMPLE_DEFAULT: in a filter parameter of rt_upsample, the measured default
# the defaults rt_upsample substitutes (csrc/upsample.hip; profiles/upsample_quality.txt)
UPSAMPLE_DEFAULTS = {"normal_power_log2": 0, "sigma_plane": 0.03}
# AdaptiveSampler.step's scale: priorities are relative variances of the mean, quantised to 0..65535 after the
# scaling.  The best point of profiles/adaptive_quality.txt's grid (tools/adaptive_quality.py) on both of its scenes:
# 2^28 saturates every pixel whose relative variance is above 2^-12, so a round is shared almost evenly among the
# pixels that have not converged, and the few below that get in proportion less.
SAMPLE_SCALE_DEFAULT = 268435456.0


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


for _struct, _size in ((GPUCamera, 60), (GPUScene, 136), (GPUMaterial, 64), (Ray, 32), (Hit, 48), (TraceParams, 40),
                       (OcclusionParams, 32), (AoParams, 72), (RadianceParams, 48), (Point, 16), (Nearest, 32),
                       (ClosestParams, 32), (DenoiseParams, 96), (ReprojectParams, 224), (MomentsParams, 64),
                       (DenoiseVarianceParams, 136), (UpsampleParams, 104), (SamplePixelsParams, 80),
                       (SamplePriorityParams, 40), (SamplePlanParams, 80), (SampleResolveParams, 40)):
    assert ctypes.sizeof(_struct) == _size, (_struct.__name__, ctypes.sizeof(_struct), _size)

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
    "rt_lane_refine": (ctypes.c_int64, [_P, ctypes.c_int64, _P, ctypes.c_int64, _P, ctypes.c_double, _P, ctypes.c_int64, _P]),
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

_lib = None      # librt_hip.so once lib() has loaded it; read elsewhere only by Scene.__del__
_exp_lib = None  # librt_hip_exp.so once load_experimental() has loaded it


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
        raise RTError("librt_hip_exp.so loaded but its kernels are not registered with librt_hip.so: " + _last_error())
    return _exp_lib


def _last_error():
    return lib().rt_last_error().decode(errors="replace")


def _check(code, what):
    if code:
        raise RTError(f"{what} failed ({code}): {_last_error()}")
