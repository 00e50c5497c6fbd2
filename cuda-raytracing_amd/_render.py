"""Rendering a frame: rt_render, the RNG states, the shard / lane / lone plans and the multi-GPU gather around it,
the display transform and image files, and the reference's two entry points."""
import ctypes
import os

import numpy as np
import torch

from . import sharding  # multi-GPU tile bookkeeping; the data path is in librt_hip.so
from ._abi import RT_RENDER_STATS, RT_RENDER_VALIDATE, TRACERS, RenderParams, RTError, _check, _last_error, lib
from ._args import _is_tensor, _launch, _stream_ptr


def init_rng_states(rng, width, height, seed, shard_index=0, shard_count=1, stream=None):
    _check(lib().rt_init_rng(ctypes.c_void_p(rng.data_ptr()), width, height, shard_index, shard_count, seed,
                             _stream_ptr(stream)), "rt_init_rng")


def shard_tiles(width, height, shard_index, shard_count):
    return int(lib().rt_shard_tiles(width, height, shard_index, shard_count))


tiles_of = shard_tiles


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
        assert _is_tensor(lone_slots, torch.int32, 1, contiguous=False)
        p.lone_slots, p.lone_count = lone_slots.data_ptr(), lone_slots.numel()
    if lane_slots is not None:
        assert _is_tensor(lane_slots, torch.int32, contiguous=False) and lane_slots.numel() % 64 == 0
        p.lane_slots, p.lane_slot_count = lane_slots.data_ptr(), lane_slots.numel()
        p.priority_waves = int(priority_waves)
    if lane_cost is not None:
        assert _is_tensor(lane_cost, torch.int32, contiguous=False)
        p.lane_cost = lane_cost.data_ptr()
    if tile_list is not None:
        assert _is_tensor(tile_list, torch.int32, 1, contiguous=False)
        p.tile_list, p.tile_count = tile_list.data_ptr(), tile_list.numel()
    if wave_clock is not None:
        n = tile_list.numel() if tile_list is not None else tiles_of(width, height, shard_index, shard_count)
        waves = lane_slots.numel() // 64 if lane_slots is not None else 4 * n
        assert wave_clock.dtype == torch.int64 and wave_clock.numel() >= waves
        p.wave_clock = wave_clock.data_ptr()
    p.tune, p.refill_lanes, p.waves_per_simd = int(tune), int(refill_lanes), int(waves_per_simd)
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
    _launch("rt_render", p, stream, scene)


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
        raise RTError("rt_lane_plan failed: " + _last_error())
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
        raise RTError("rt_lane_refine failed: " + _last_error())
    return out[:n].copy(), int(nsplit.value)


def lone_plan(cost, max_lone, min_cost=1):
    """rt_lone_plan: (int32 numpy lone slots, heaviest first; the cost array with those slots marked
    for rt_lane_plan) from per-slot work (a probe frame's lane_cost)."""
    cost = np.ascontiguousarray(np.asarray(cost).astype(np.uint32)).copy()
    out = np.empty(max(int(max_lone), 1), dtype=np.int32)
    n = int(lib().rt_lone_plan(cost.ctypes.data, cost.size, int(max_lone), int(min_cost), out.ctypes.data))
    if n < 0:
        raise RTError("rt_lone_plan failed: " + _last_error())
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
    host = (surface.detach().to("cpu").contiguous().numpy() if isinstance(surface, torch.Tensor)
            else np.ascontiguousarray(surface, dtype=np.float32))
    _check(lib().rt_write_pfm(os.fsencode(path), host.ctypes.data, host.shape[1] * 4, width, height), "rt_write_pfm")


def write_ppm(path, rgb):
    """[H, W, 3] uint8 (tonemap's output, any device) as binary PPM."""
    host = (rgb.detach().to("cpu").contiguous().numpy() if isinstance(rgb, torch.Tensor)
            else np.ascontiguousarray(rgb, dtype=np.uint8))
    _check(lib().rt_write_ppm(os.fsencode(path), host.ctypes.data, host.shape[1], host.shape[0]), "rt_write_ppm")


def raytracing_process(surface, last, width, height, frame_index, scene):
    """The reference entry point (main_raytracing.cu:202): spp 5, 6 bounces, null stream."""
    lib().raytracing_process(ctypes.c_void_p(surface.data_ptr()), ctypes.c_void_p(last.data_ptr()), width, height,
                             surface.shape[1] * 4, frame_index, ctypes.cast(scene.gpu, ctypes.c_void_p))


def init_rng(thread_block_count, thread_block_size, rng, seed):
    """The reference entry point (Random.cu:10)."""
    lib().init_rng(thread_block_count, thread_block_size, ctypes.c_void_p(rng.data_ptr()), seed)
