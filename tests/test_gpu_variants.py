"""The kernel variants that no other GPU test launches, each against the RT_TUNE 0 production frame.

Of the 19 (family, MODE) pairs rt_variant.h choose_variant can return (tests/test_variant_cpu.py), the suite already
renders prod 17 and lean 17 | 128 (test_gpu_lean.py), prod 21, timing 29, screen 53 (test_gpu_multi.py: the deferred
tree leaves, the big-leaf screens), timing 25 | 128 (the lane_cost probes of test_gpu_multi.py), stats 2
(test_gpu_parity.py), refill 81 and 85 (test_gpu_multi.py).  The ten below are the rest.  Each is one 64x64
frame, 2 spp, 3 bounces, with the plugin loaded; surface and final RNG states must equal, bit for bit, the frame
the same scene renders at RT_TUNE 0 with default build options -- every variant is exact.  The bunny for the modes
without leaf trees, the 4-bunny scene for those with; the screen modes without leaf trees (49, 57) need a scene
with screenable leaves, which the bunny has none of, so they render the 4-bunny scene built without leaf trees.
Each case first asks the chooser (rt_variant_host) which variant its frame gets, with has_tree and screens read
from the scene's mirror, so a case cannot pass on another kernel than the one it names.
"""
import numpy as np
import pytest
import torch

import rt_testlib as T
from test_variant_cpu import FAMILIES, choose

pytestmark = pytest.mark.gpu
W = H = 64
SPP, BOUNCES = 2, 3
NO_TREES = dict(leaf_tree_min=1 << 30)
# id: scene, build options, stats frame, lane_cost frame, RT_TUNE, the (family, MODE) it must reach
CASES = {
    "timing25": ("bunny", {}, False, True, 3 << 16, ("timing", 25)),  # a knob the kernel reads (the XCD run's default)
    "timing9": ("bunny", {}, True, False, 256 | 4096, ("timing", 9)),
    "stats6": ("bunny4", {}, True, False, 128, ("stats", 6)),
    "ab1": ("bunny", {}, False, False, 4096, ("ab", 1)),
    "ab5": ("bunny4", {}, False, False, 4096, ("ab", 5)),
    "ab2_scalar": ("bunny", {}, False, False, 2 << 4, ("ab2", 2)),
    "ab2_pairs": ("bunny", {}, False, False, 3 << 4, ("ab2", 0)),
    "screen49": ("bunny4", dict(leaf_screens=1, **NO_TREES), False, False, 0, ("screen", 49)),
    "screen57": ("bunny4", dict(leaf_screens=1, **NO_TREES), False, True, 0, ("screen", 57)),
    "screen61": ("bunny4", dict(leaf_screens=1), False, True, 0, ("screen", 61)),
}


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    torch.cuda.set_device(0)
    rt = T.load_rt()
    rt.load_experimental()
    return rt


def frame(rt, which, stats=False, lane_cost=False, tune=0):
    """(surface, final RNG states, has_tree, screens) of one frame of scene `which` under the current build options."""
    s = rt.Scene()
    s.setup(which)
    s.set_viewport(W, H)
    rng = rt.alloc_rng(W * H)
    rt.init_rng_states(rng, W, H, T.SEED)
    s.upload(rng.data_ptr())
    a, b = rt.alloc_surface(W, H), rt.alloc_surface(W, H)
    kw = {}
    if stats:
        kw["stats"] = torch.zeros(rt.STAT_COUNT, dtype=torch.int64, device="cuda")
    if lane_cost:
        kw["lane_cost"] = torch.zeros(rt.sharding.tiles_total(W, H) * 256, dtype=torch.int32, device="cuda")
    rt.render(s, a, b, W, H, SPP, BOUNCES, tune=tune, **kw)
    torch.cuda.synchronize()
    tris, tree, _ = s.mirror(trees=True)
    nodes = s.host_arrays()["nodes"].view(np.uint32).reshape(-1, 8)
    kinds = tris.view(np.uint32).reshape(-1, 12)[nodes[nodes[:, 7] > 8][:, 6], 11]  # mirror.h pf of the big leaves
    return (rt.surface_view(a, W).cpu().numpy().copy(), rng.view(-1, 12)[:, :6].cpu().numpy().view(np.uint32).copy(),
            len(tree) > 0, bool((kinds == 3).any()))


@pytest.fixture(scope="module")
def references(rt):
    """The RT_TUNE 0 frame of each scene, rendered once and left unchanged."""
    return {which: frame(rt, which) for which in ("bunny", "bunny4")}


@pytest.mark.parametrize("case", sorted(CASES))
def test_variant_equals_production(rt, references, case):
    which, options, stats, lane_cost, tune, variant = CASES[case]
    if options:
        rt.set_build_options(**options)
    try:
        surface, rng, has_tree, screens = frame(rt, which, stats, lane_cost, tune)
    finally:
        rt.set_build_options()
    v = choose(rt, tune=tune, stats=stats, lane_cost=lane_cost, has_tree=has_tree, screens=screens, arrays_complete=1,
               depth=20)
    assert (FAMILIES[v["family"]], v["mode"]) == variant, f"{case}: the frame ran {FAMILIES[v['family']]} {v['mode']}"
    want = references[which]
    nan_g, nan_w = np.isnan(surface), np.isnan(want[0])  # (a NaN's payload bits are the ISA's choice)
    assert np.array_equal(nan_g, nan_w), f"{case}: NaN positions differ"
    mism = int((surface.view(np.uint32)[~nan_g] != want[0].view(np.uint32)[~nan_w]).sum())
    assert mism == 0, f"{case}: {mism} surface words differ from the RT_TUNE 0 frame"
    assert np.array_equal(rng, want[1]), f"{case}: final RNG states differ"
