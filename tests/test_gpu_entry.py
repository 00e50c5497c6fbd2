"""Camera rays started from their sub-tile's entry record (csrc/entry_frontier.h, rt_build_options.entry_frontier)
render the frame the root-started kernel renders, and the oracle's: bunny, 2 spp, 6 bounces, frames 0 and 1
chained, surface and final RNG states bit for bit, with the option on and off -- at 5, 6 and 7 waves per SIMD in
plain order, through a permuted lane map and through the tile lists of a 2-rank shard plan (the lanes of a wave
then belong to different sub-tiles), at a viewport with partial sub-tiles, and after a viewport change on one
scene object (the table's key)."""
import contextlib

import numpy as np
import pytest
import torch

import rt_testlib as T

pytestmark = pytest.mark.gpu
W, H, SPP, BOUNCES, FRAMES = 256, 144, 2, 6, 2
_ORACLE = {}


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    torch.cuda.set_device(0)
    return T.load_rt()


@contextlib.contextmanager
def entry(rt, on):
    rt.set_build_options(entry_frontier=1 if on else 0)
    try:
        yield
    finally:
        rt.set_build_options()


def oracle_frames(w, h):
    """(frame 1 of two chained frames, final RNG states), rendered once per viewport and left unchanged."""
    if (w, h) not in _ORACLE:
        o = T.OracleScene("bunny")
        rng = T.oracle_rng_frame(T.SEED, w, h)
        img = None
        for f in range(FRAMES):
            img = o.render(w, h, SPP, BOUNCES, frame_index=f, rng=rng, last=img)
        _ORACLE[(w, h)] = (img, rng.copy())
    return _ORACLE[(w, h)]


def bunny(rt, w, h):
    s = rt.Scene()
    s.setup("bunny")
    s.set_viewport(w, h)
    return s


def frames(rt, s, w, h, wps=0, lane_slots=None, tile_list=None):
    """Two chained full-layout frames of scene `s`: (surface, RNG states as [w * h, 6] uint32)."""
    rng = rt.alloc_rng(w * h)
    rt.init_rng_states(rng, w, h, T.SEED)
    s.upload(rng.data_ptr())
    bufs = [rt.alloc_surface(w, h), rt.alloc_surface(w, h)]
    for f in range(FRAMES):
        rt.render(s, bufs[f & 1], bufs[(f + 1) & 1], w, h, SPP, BOUNCES, f, waves_per_simd=wps, lane_slots=lane_slots,
                  tile_list=tile_list)
    torch.cuda.synchronize()
    return (rt.surface_view(bufs[(FRAMES - 1) & 1], w).cpu().numpy().copy(),
            rng.view(-1, 12)[:, :6].cpu().numpy().view(np.uint32).copy())


def same(got, want, what):
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), f"{what}: surfaces differ"
    assert np.array_equal(got[1], want[1]), f"{what}: final RNG states differ"


def on_off_oracle(rt, w, h, what, **kw):
    want = oracle_frames(w, h)
    before = rt.entry_table_builds()
    with entry(rt, True):
        on = frames(rt, bunny(rt, w, h), w, h, **kw)
    assert rt.entry_table_builds() == before + 1, "one table for the two frames of one camera"
    with entry(rt, False):
        off = frames(rt, bunny(rt, w, h), w, h, **kw)
    assert rt.entry_table_builds() == before + 1, "no table with the option off"
    same(on, off, f"{what}: entry records on vs off")
    same(on, want, f"{what}: entry records on vs the oracle")


@pytest.mark.parametrize("wps", [5, 6, 7])
def test_plain_order(rt, wps):
    on_off_oracle(rt, W, H, f"{wps} waves", wps=wps)


def test_permuted_lane_map(rt):
    """Every slot once, in random order, with idle lanes in between: a wave's lanes come from all over the frame."""
    tiles = rt.sharding.tiles_total(W, H)
    gen = np.random.default_rng(5)
    m = np.full(tiles * 256 + 64 * 37, -1, dtype=np.int32)
    m[gen.choice(m.size, tiles * 256, replace=False)] = gen.permutation(tiles * 256).astype(np.int32)
    on_off_oracle(rt, W, H, "lane map", lane_slots=torch.from_numpy(m).cuda(),
                  tile_list=torch.arange(tiles, dtype=torch.int32, device="cuda"))


def test_partial_sub_tiles(rt):
    on_off_oracle(rt, 250, 141, "250x141")


def sharded(rt, n):
    """The frames through the tile lists of an n-rank plan (compact shards), unsharded."""
    lists, counts = rt.shard_plan(W, H, n)
    cap = lists.shape[1]
    s = bunny(rt, W, H)
    shards = torch.zeros((2, n, cap * 256, 4), dtype=torch.float32, device="cuda")
    for r in range(n):
        mine = torch.from_numpy(lists[r, : counts[r]]).cuda()
        rng = rt.alloc_rng(cap * 256)
        rt.init_rng_tiles(rng, W, H, mine, T.SEED)
        s.upload(rng.data_ptr())
        for f in range(FRAMES):
            rt.render(s, None, shards[(f + 1) & 1, r], W, H, SPP, BOUNCES, f, r, n, out_shard=shards[f & 1, r], tile_list=mine)
        torch.cuda.synchronize()
    out = rt.alloc_surface(W, H)
    rt.unshard_tiles(out, W, H, shards[(FRAMES - 1) & 1], torch.from_numpy(lists).cuda())
    torch.cuda.synchronize()
    return rt.surface_view(out, W).cpu().numpy().copy()


def test_shard_plan_tile_lists(rt):
    want = oracle_frames(W, H)[0]
    before = rt.entry_table_builds()
    with entry(rt, True):
        on = sharded(rt, 2)
    built = rt.entry_table_builds() - before
    assert built >= 1, "the sharded frames (out_shard, rank of n) did not get a table"
    with entry(rt, False):
        off = sharded(rt, 2)
    assert rt.entry_table_builds() == before + built, "no table with the option off"
    assert np.array_equal(on.view(np.uint32), off.view(np.uint32))
    assert np.array_equal(on.view(np.uint32), want.view(np.uint32))


def test_viewport_change_rebuilds(rt):
    """One scene object rendered at 256x144, then at 250x141: the second equals a fresh scene's frames."""
    want = oracle_frames(250, 141)
    with entry(rt, True):
        s = bunny(rt, W, H)
        before = rt.entry_table_builds()
        first = frames(rt, s, W, H)
        assert rt.entry_table_builds() == before + 1
        s.set_viewport(250, 141)
        second = frames(rt, s, 250, 141)
        assert rt.entry_table_builds() == before + 2, "the viewport is part of the table's key"
    same(first, oracle_frames(W, H), "256x144")
    same(second, want, "250x141 after 256x144")
