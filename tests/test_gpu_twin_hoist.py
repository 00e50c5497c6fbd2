"""The big-leaf rounds with the twin test's bounds hoisted (rt_fast.h quad_test on the leaf's twin record and the
visit's bounds, unit_test on the leaf's constants): two chained frames of the bunny at 64x36 and 256x144 and of the
4-bunny scene at 256x144 (its 21- and 903-triangle leaves), at 5, 6 and 7 waves per SIMD, surface and final RNG
states bit for bit the CPU oracle's, through the lean kernel (tune 0) and through the general one (RT_TUNE bits
16-19 = 3, the XCD run length set explicitly to its default), in plain tile order and through a permuted lane map.
Every oracle frame is rendered once and shared."""
import numpy as np
import pytest
import torch

import rt_testlib as T

pytestmark = pytest.mark.gpu
BOUNCES, FRAMES = 6, 2
CASES = {"bunny-64x36": ("bunny", 64, 36, 4), "bunny-256x144": ("bunny", 256, 144, 2), "bunny4-256x144": ("bunny4", 256, 144, 1)}
GENERAL = 3 << 16
_ORACLE = {}


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    torch.cuda.set_device(0)
    return T.load_rt()


def oracle_frames(case):
    """(the second of two chained frames, final RNG states) of the CPU oracle."""
    if case not in _ORACLE:
        which, w, h, spp = CASES[case]
        o = T.OracleScene(which)
        rng = T.oracle_rng_frame(T.SEED, w, h)
        img = None
        for f in range(FRAMES):
            img = o.render(w, h, spp, BOUNCES, frame_index=f, rng=rng, last=img)
        _ORACLE[case] = (img, rng.copy())
    return _ORACLE[case]


def frames(rt, case, wps=0, tune=0, lane_slots=None, tile_list=None):
    which, w, h, spp = CASES[case]
    s = rt.Scene()
    s.setup(which)
    s.set_viewport(w, h)
    rng = rt.alloc_rng(w * h)
    rt.init_rng_states(rng, w, h, T.SEED)
    s.upload(rng.data_ptr())
    quads, units = s.mirror_twins()
    assert len(quads) > 0 and len(units) > 0, "no twin records: the big-leaf rounds under test would not run"
    bufs = [rt.alloc_surface(w, h), rt.alloc_surface(w, h)]
    for f in range(FRAMES):
        rt.render(s, bufs[f & 1], bufs[(f + 1) & 1], w, h, spp, BOUNCES, f, waves_per_simd=wps, tune=tune,
                  lane_slots=lane_slots, tile_list=tile_list)
    torch.cuda.synchronize()
    return (rt.surface_view(bufs[(FRAMES - 1) & 1], w).cpu().numpy().copy(),
            rng.view(-1, 12)[:, :6].cpu().numpy().view(np.uint32).copy())


def same(got, want, what):
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), f"{what}: surfaces differ"
    assert np.array_equal(got[1], want[1]), f"{what}: final RNG states differ"


@pytest.mark.parametrize("wps", [5, 6, 7])
@pytest.mark.parametrize("case", list(CASES))
def test_plain_order(rt, case, wps):
    want = oracle_frames(case)
    lean = frames(rt, case, wps)
    general = frames(rt, case, wps, tune=GENERAL)
    same(lean, want, f"{case} at {wps} waves, lean kernel vs the oracle")
    same(general, lean, f"{case} at {wps} waves, general kernel vs lean")


@pytest.mark.parametrize("wps", [5, 6, 7])
@pytest.mark.parametrize("case", list(CASES))
def test_permuted_lane_map(rt, case, wps):
    """Every slot once, in random order, with idle lanes in between: a wave's lanes come from all over the frame, so
    the lanes waiting at one big leaf hold rays with unrelated origins."""
    _, w, h, _ = CASES[case]
    tiles = rt.sharding.tiles_total(w, h)
    gen = np.random.default_rng(5)
    m = np.full(tiles * 256 + 64 * 37, -1, dtype=np.int32)
    m[gen.choice(m.size, tiles * 256, replace=False)] = gen.permutation(tiles * 256).astype(np.int32)
    kw = dict(lane_slots=torch.from_numpy(m).cuda(), tile_list=torch.arange(tiles, dtype=torch.int32, device="cuda"))
    want = oracle_frames(case)
    lean = frames(rt, case, wps, **kw)
    general = frames(rt, case, wps, tune=GENERAL, **kw)
    same(lean, want, f"{case} at {wps} waves, lane map, lean kernel vs the oracle")
    same(general, lean, f"{case} at {wps} waves, lane map, general kernel vs lean")
