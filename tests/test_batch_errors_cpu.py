"""The host-side refusals of the four ray-batch entry points (rt_trace_rays, rt_occluded, rt_ao, rt_radiance) that need
no device, as one table: the exact rt_last_error text of each, and rows with two faults at once that pin which check
comes first.  A row whose message is None must return 0 (count 0: before the scene is looked at)."""
import ctypes

import pytest

import rt_testlib as T

D = 0x1000  # non-null, 16-byte aligned, never dereferenced on these paths
NAN, INF = float("nan"), float("inf")
DEFAULTS = {
    "rt_trace_rays": ("TraceParams", dict(rays=D, hits=D, count=64)),
    "rt_occluded": ("OcclusionParams", dict(rays=D, occluded=D, count=64)),
    "rt_ao": ("AoParams", dict(hits=D, directions=D, ao=D, width=8, height=4, direction_count=64, samples=4, radius=8.0,
                               bias=0.001)),
    "rt_radiance": ("RadianceParams", dict(rays=D, rng=D, radiance=D, count=64, bounces=6, samples=1)),
}
WAVES = "waves_per_simd must be 0 (default), 5, 6 or 7"
UPLOAD = ("this GPUScene was not uploaded by rt_scene_upload (a foreign scene has no private mirror to query; foreign "
          "scenes are not supported here)")
FLAGS, NEG, RAYS31 = "flags must be 0", "negative count", "more than 2^31 rays in one call"
NO_RAYS = "null rays (there is no camera mode)"
CAMERA = "camera mode needs width, height > 0"
RH16, R16 = "rays and hits must be 16-byte aligned", "rays must be 16-byte aligned"
HD16, AO4 = "hits and directions must be 16-byte aligned", "ao must be 4-byte aligned"
RR16, RNG8 = "rays and radiance must be 16-byte aligned", "rng must be 8-byte aligned"
WH, PIX30 = "width and height must be > 0", "more than 2^30 pixels"
DIRS, SAMPLES64 = "direction_count must be 1..65536", "samples must be 1..64"
RADIUS, BIAS = "radius must be > 0 and not NaN", "bias must be >= 0 and finite"
BOUNCES, SAMPLES24 = "bounces must be >= 0", "samples must be 1..2^24"
# (call, parameter overrides or None for null params, scene given, message after "call: " or None for success); in
# each block the single faults in the call's order of checks, then the rows with two
TABLE = [("rt_trace_rays", kw, s, m) for kw, s, m in [
    (None, True, "null params"), ({}, False, "null scene"), (dict(hits=None), True, "null hits"),
    (dict(flags=1), True, FLAGS), (dict(waves_per_simd=4), True, WAVES), (dict(waves_per_simd=8), True, WAVES),
    (dict(rays=None, width=0, height=4), True, CAMERA), (dict(rays=None, width=4, height=-1), True, CAMERA),
    (dict(count=-1), True, NEG), (dict(count=2 ** 31 + 1), True, RAYS31),
    (dict(rays=None, width=65536, height=65536), True, RAYS31), (dict(rays=D + 4), True, RH16),
    (dict(hits=D + 8), True, RH16), (dict(count=0), True, None), (dict(count=2 ** 31), True, UPLOAD), ({}, True, UPLOAD),
    (None, False, "null params"), (dict(hits=None), False, "null scene"), (dict(hits=None, flags=1), True, "null hits"),
    (dict(flags=1, waves_per_simd=4), True, FLAGS), (dict(waves_per_simd=8, count=-1), True, WAVES),
    (dict(waves_per_simd=4, rays=None, width=0), True, WAVES), (dict(count=-1, rays=D + 4), True, NEG),
    (dict(count=2 ** 31 + 1, hits=D + 4), True, RAYS31), (dict(count=0, rays=D + 4), True, RH16),
]] + [("rt_occluded", kw, s, m) for kw, s, m in [
    (None, True, "null params"), ({}, False, "null scene"), (dict(occluded=None), True, "null occluded"),
    (dict(rays=None), True, NO_RAYS), (dict(flags=1), True, FLAGS), (dict(waves_per_simd=4), True, WAVES),
    (dict(waves_per_simd=8), True, WAVES), (dict(count=-1), True, NEG), (dict(count=2 ** 31 + 1), True, RAYS31),
    (dict(rays=D + 4), True, R16), (dict(count=0), True, None), (dict(count=0, occluded=D + 1), True, None),
    ({}, True, UPLOAD),
    (dict(occluded=None), False, "null scene"), (dict(occluded=None, rays=None), True, "null occluded"),
    (dict(rays=None, flags=1), True, NO_RAYS), (dict(occluded=None, waves_per_simd=4), True, "null occluded"),
    (dict(flags=1, waves_per_simd=4), True, FLAGS), (dict(waves_per_simd=8, count=-1), True, WAVES),
    (dict(count=-1, rays=D + 4), True, NEG), (dict(count=2 ** 31 + 1, rays=D + 4), True, RAYS31),
    (dict(count=0, rays=D + 4), True, R16),
]] + [("rt_ao", kw, s, m) for kw, s, m in [
    (None, True, "null params"), ({}, False, "null scene"), (dict(hits=None), True, "null hits"),
    (dict(directions=None), True, "null directions"), (dict(ao=None), True, "null ao"), (dict(flags=1), True, FLAGS),
    (dict(waves_per_simd=4), True, WAVES), (dict(waves_per_simd=8), True, WAVES), (dict(width=0), True, WH),
    (dict(height=-1), True, WH), (dict(width=65536, height=32768), True, PIX30), (dict(direction_count=0), True, DIRS),
    (dict(direction_count=65537), True, DIRS), (dict(samples=0), True, SAMPLES64), (dict(samples=65), True, SAMPLES64),
    (dict(radius=0.0), True, RADIUS), (dict(radius=-1.0), True, RADIUS), (dict(radius=NAN), True, RADIUS),
    (dict(bias=-1.0), True, BIAS), (dict(bias=INF), True, BIAS), (dict(bias=NAN), True, BIAS),
    (dict(hits=D + 4), True, HD16), (dict(directions=D + 8), True, HD16), (dict(ao=D + 2), True, AO4),
    ({}, True, UPLOAD), (dict(width=32768, height=32768), True, UPLOAD),
    (dict(hits=None, ao=None), True, "null hits"), (dict(ao=None, waves_per_simd=4), True, "null ao"),
    (dict(flags=1, waves_per_simd=4), True, FLAGS), (dict(waves_per_simd=8, width=0), True, WAVES),
    (dict(width=0, samples=0), True, WH), (dict(width=65536, height=32768, direction_count=0), True, PIX30),
    (dict(samples=0, direction_count=0), True, DIRS), (dict(radius=NAN, bias=-1.0), True, RADIUS),
    (dict(bias=INF, hits=D + 4), True, BIAS), (dict(hits=D + 4, ao=D + 2), True, HD16),
]] + [("rt_radiance", kw, s, m) for kw, s, m in [
    (None, True, "null params"), ({}, False, "null scene"), (dict(rays=None), True, NO_RAYS),
    (dict(rng=None), True, "null rng"), (dict(radiance=None), True, "null radiance"), (dict(flags=1), True, FLAGS),
    (dict(waves_per_simd=4), True, WAVES), (dict(waves_per_simd=8), True, WAVES), (dict(count=-1), True, NEG),
    (dict(count=2 ** 31 + 1), True, RAYS31), (dict(bounces=-1), True, BOUNCES), (dict(samples=0), True, SAMPLES24),
    (dict(samples=2 ** 24 + 1), True, SAMPLES24), (dict(rays=D + 8), True, RR16), (dict(radiance=D + 4), True, RR16),
    (dict(rng=D + 4), True, RNG8), (dict(count=0), True, None), ({}, True, UPLOAD), (dict(bounces=0), True, UPLOAD),
    (dict(rays=None, rng=None), True, NO_RAYS), (dict(radiance=None, waves_per_simd=8), True, "null radiance"),
    (dict(flags=1, waves_per_simd=4), True, FLAGS), (dict(waves_per_simd=4, count=-1), True, WAVES),
    (dict(count=-1, rays=D + 8), True, NEG), (dict(count=2 ** 31 + 1, bounces=-1), True, RAYS31),
    (dict(bounces=-1, samples=0), True, BOUNCES), (dict(samples=0, radiance=D + 4), True, SAMPLES24),
    (dict(radiance=D + 4, rng=D + 4), True, RR16), (dict(count=0, rng=D + 4), True, RNG8),
]]


@pytest.mark.parametrize("call, overrides, with_scene, message", TABLE,
                         ids=lambda v: None if isinstance(v, (dict, bool)) else v)
def test_refusal(call, overrides, with_scene, message):
    rt = T.load_rt()
    L = rt.lib()
    p = None
    if overrides is not None:
        cls, defaults = DEFAULTS[call]
        p = getattr(rt, cls)()
        for k, v in {**defaults, **overrides}.items():
            setattr(p, k, v)
    scene = ctypes.byref(rt.GPUScene()) if with_scene else None
    code = getattr(L, call)(ctypes.byref(p) if p is not None else None, scene, None)
    if message is None:
        assert code == 0
    else:
        assert code != 0 and L.rt_last_error() == (call + ": " + message).encode(), (overrides, code, L.rt_last_error())
