"""The host-side refusals of rt_render that need no device, and those of the calls that set a frame up and put it
together (rt_init_rng, rt_init_rng_tiles, rt_unshard, rt_unshard_tiles, rt_shard_tiles), as one table: the exact
rt_last_error text of each, and rows with two faults at once that pin which check comes first.  A row whose message
is an int must return that value (a shard without tiles is no error: rt_render returns 0 before it looks further).

Every row but those carries a fault that is refused before rt_render first asks the runtime about a pointer (its
buffer-size checks), so the table says nothing about, and leaves nothing in, the runtime's own error state; the
refusals behind that point are tests/test_gpu_render_errors.py's."""
import ctypes

import pytest

import rt_testlib as T

D = 0x1000  # non-null, 16-byte aligned, never dereferenced on these paths
STATS = 1   # RT_RENDER_STATS
# an 8 x 8 frame (one tile) on a surface of 128-byte rows; the scene's three pointers rt_render asks for
RENDER = dict(surface=D, width=8, height=8, pitch=128, spp=1, bounces=1, shard_index=0, shard_count=1,
              rng_state=D, gpu_bvh_nodes=D, gpu_materials=D)
# the other calls' arguments in the order of rt_abi.h (the stream, last, is null)
ARGS = {
    "rt_init_rng": dict(states=D, width=8, height=8, shard_index=0, shard_count=1, seed=7),
    "rt_init_rng_tiles": dict(states=D, width=8, height=8, tile_list=D, tile_count=1, seed=7),
    "rt_unshard": dict(surface=D, pitch=128, width=8, height=8, shard_count=1, shards=D, per_shard=1),
    "rt_unshard_tiles": dict(surface=D, pitch=128, width=8, height=8, shard_count=1, shards=D, per_shard=1, tile_lists=D),
    "rt_shard_tiles": dict(width=8, height=8, shard_index=0, shard_count=1),
}
FRAME, SHARD = "bad frame size / spp / bounces", "bad shard"
SURFACE = "need a surface with pitch >= 16*width, or out_shard"
SHARDED = "sharded render needs out_shard"
UPLOAD = "scene not uploaded (rng_state / bvh / materials missing)"
NO_STATS, CUBE = "stats flag without buffer", "unknown environment cube map handle"
TILES = "tile_list needs 0 < tile_count < 2^28"
LANES = "lane_slots needs a positive multiple of 64 entries (< 2^30)"
SLOTS = "more than 2^32 pixel slots in one launch"
REFILL = "refill_lanes must be in [0, 64]"
WAVES = "waves_per_simd must be 0 (default), 1-4 (LDS-capped residency), 5, 6 or 7"
TUNE = "RT_TUNE occupancy override 1 (compiler's choice) is not built"
BAD = "bad arguments"
NO_TILES = dict(shard_index=1, shard_count=2, out_shard=D)  # the frame's one tile is shard 0's
MANY = dict(tile_list=D, tile_count=2 ** 28)                # 2^36 pixel slots
# (call, overrides, message after "call: " or the value returned); rt_render's overrides name fields of rt_render_params
# or of the GPUScene, or null one of the two with params=None / scene=None.  In each block the single faults in the
# call's order of checks, then the rows with two
TABLE = [("rt_render", kw, m) for kw, m in [
    (dict(params=None), "null argument"), (dict(scene=None), "null argument"),
    (dict(width=0), FRAME), (dict(height=-1), FRAME), (dict(spp=0), FRAME), (dict(bounces=-1), FRAME),
    (dict(shard_count=0), SHARD), (dict(shard_index=-1), SHARD), (dict(shard_index=1), SHARD),
    (dict(surface=None), SURFACE), (dict(pitch=127), SURFACE), (dict(shard_count=2), SHARDED),
    (dict(rng_state=None), UPLOAD), (dict(gpu_bvh_nodes=None), UPLOAD), (dict(gpu_materials=None), UPLOAD),
    (dict(flags=STATS), NO_STATS), (dict(environment_cubemap_tex=0xDEAD0), CUBE),
    (dict(tile_list=D, tile_count=0), TILES), (dict(tile_list=D, tile_count=2 ** 28 + 1), TILES),
    (NO_TILES, 0),
    (dict(lane_slots=D, lane_slot_count=100), LANES), (dict(lane_slots=D, lane_slot_count=0), LANES),
    (dict(lane_slots=D, lane_slot_count=2 ** 30 + 64), LANES), (MANY, SLOTS),
    (dict(refill_lanes=65), REFILL), (dict(refill_lanes=-1), REFILL),
    (dict(waves_per_simd=8), WAVES), (dict(waves_per_simd=-1), WAVES), (dict(tune=1 << 9), TUNE),
    (dict(params=None, scene=None), "null argument"), (dict(width=0, shard_count=0), FRAME),
    (dict(shard_count=0, surface=None), SHARD), (dict(surface=None, shard_count=2), SURFACE),
    (dict(shard_count=2, rng_state=None), SHARDED), (dict(gpu_materials=None, flags=STATS), UPLOAD),
    (dict(flags=STATS, environment_cubemap_tex=0xDEAD0), NO_STATS),
    (dict(environment_cubemap_tex=0xDEAD0, tile_list=D, tile_count=0), CUBE),
    (dict(tile_list=D, tile_count=0, lane_slots=D, lane_slot_count=100), TILES),
    (dict(NO_TILES, lane_slots=D, lane_slot_count=100), 0), (dict(NO_TILES, tune=1 << 9), 0),
    (dict(MANY, lane_slots=D, lane_slot_count=100), LANES), (dict(MANY, refill_lanes=65), SLOTS),
    (dict(lane_slots=D, lane_slot_count=100, refill_lanes=65), LANES),
    (dict(refill_lanes=65, waves_per_simd=8), REFILL), (dict(waves_per_simd=8, tune=1 << 9), WAVES),
]] + [("rt_init_rng", kw, BAD) for kw in [
    dict(states=None), dict(width=0), dict(height=0), dict(shard_count=0), dict(shard_index=-1), dict(shard_index=1),
    dict(shard_index=2, shard_count=2),
]] + [("rt_init_rng_tiles", kw, BAD) for kw in [
    dict(states=None), dict(tile_list=None), dict(width=0), dict(height=0), dict(tile_count=0), dict(tile_count=-1),
    dict(tile_count=2 ** 28 + 1),
]] + [("rt_unshard", kw, BAD) for kw in [
    dict(surface=None), dict(shards=None), dict(shard_count=0), dict(per_shard=0), dict(width=0), dict(height=0),
]] + [("rt_unshard_tiles", kw, BAD) for kw in [
    dict(surface=None), dict(shards=None), dict(tile_lists=None), dict(shard_count=0), dict(per_shard=0), dict(width=0),
    dict(height=0),
]] + [("rt_shard_tiles", kw, m) for kw, m in [
    (dict(width=0), 0), (dict(height=0), 0), (dict(shard_count=0), 0), (dict(shard_index=-1), 0), (dict(shard_index=1), 0),
    (dict(shard_index=2, shard_count=2), 0), ({}, 1), (dict(width=33, height=17, shard_count=4), 2),
]]


def call(rt, name, overrides):
    L = rt.lib()
    if name != "rt_render":
        return getattr(L, name)(*{**ARGS[name], **overrides}.values(), *([] if name == "rt_shard_tiles" else [None]))
    p, scene = rt.RenderParams(), rt.GPUScene()
    for k, v in {**RENDER, **overrides}.items():
        if k not in ("params", "scene"):
            setattr(scene if hasattr(scene, k) else p, k, v)
    return L.rt_render(ctypes.byref(p) if overrides.get("params", 1) else None,
                       ctypes.byref(scene) if overrides.get("scene", 1) else None, None)


@pytest.mark.parametrize("name, overrides, message", TABLE, ids=lambda v: None if isinstance(v, dict) else str(v))
def test_refusal(name, overrides, message):
    rt = T.load_rt()
    code = call(rt, name, overrides)
    if isinstance(message, int):
        assert code == message
    else:
        error = rt.lib().rt_last_error()
        assert code == 1 and error == (name + ": " + message).encode(), (overrides, code, error)
