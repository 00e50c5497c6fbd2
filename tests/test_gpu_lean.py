"""The fixed-policy ("lean") production kernel (rt_fast_lean.hip, MODE 17 | 128): a frame that sets no RT_TUNE
knob the kernel reads, on a scene without leaf trees whose mirror holds every array, renders through it
(rt_variant.h choose_variant).  Every case is a 64x36 frame, 4 spp, 6 bounces, at 5, 6 and 7 waves per SIMD,
surface and final RNG states compared bit for bit.

The reference is the CPU oracle (rt_testlib) wherever it can build the scene: the bunny, the 4-bunny
leaf-tree scene.  The oracle has no entry point for caller-built geometry, so the hand-built scenes (flat
boxes, a camera component below the filter's range, a vertex beyond it) are compared with the product's
reference-layout tracer instead (tracer="ref": BVHRayHit with IEEE divisions throughout, itself pinned to
the oracle by test_gpu_parity.py), rendered once per scene and shared by the three occupancies.
"""
import numpy as np
import pytest
import torch

import rt_testlib as T

pytestmark = pytest.mark.gpu
W, H, SPP, BOUNCES = 64, 36, 4, 6
WAVES = [5, 6, 7]
_ORACLE = {}  # oracle frames rendered once (the 4-bunny one only if its tests run)


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    torch.cuda.set_device(0)
    return T.load_rt()


def render(rt, make, wps=0, tune=0, tracer="fast"):
    """(surface [H, W, 4] float32, final RNG states [H * W, 6] uint32) of one frame of the scene `make` returns."""
    s = make(rt)
    s.set_viewport(W, H)
    rng = rt.alloc_rng(W * H)
    rt.init_rng_states(rng, W, H, T.SEED)
    s.upload(rng.data_ptr())
    a, b = rt.alloc_surface(W, H), rt.alloc_surface(W, H)
    rt.render(s, a, b, W, H, SPP, BOUNCES, waves_per_simd=wps, tune=tune, tracer=tracer)
    torch.cuda.synchronize()
    return (rt.surface_view(a, W).cpu().numpy().copy(),
            rng.view(-1, 12)[:, :6].cpu().numpy().view(np.uint32).copy())


def same(got, want, what):
    nan_g, nan_w = np.isnan(got[0]), np.isnan(want[0])  # (a NaN's payload bits are the ISA's choice)
    assert np.array_equal(nan_g, nan_w), f"{what}: NaN positions differ"
    mism = int((got[0].view(np.uint32)[~nan_g] != want[0].view(np.uint32)[~nan_w]).sum())
    assert mism == 0, f"{what}: {mism} surface words differ"
    assert np.array_equal(got[1], want[1]), f"{what}: final RNG states differ"


def oracle_frame(which):
    o = T.OracleScene(which)
    rng = T.oracle_rng_frame(T.SEED, W, H)
    img = o.render(W, H, SPP, BOUNCES, rng=rng)
    return img, rng


def bunny(rt):
    s = rt.Scene()
    s.setup("bunny")
    return s


def bunny4(rt):
    s = rt.Scene()
    s.setup("bunny4")
    return s


def quad_box(rt, camera=(0.0, 0.0, 0.0), far_vertex=False):
    """A closed room of axis-aligned quads around the camera, lit by its ceiling, with one sphere inside.  Every
    wall is flat along one axis, so the leaf boxes over it have equal bounds there and a ray's slab interval on
    that axis is a point (tmin == tmax on a hit): the filter cannot decide `tmax >= tmin` and the IEEE slab
    runs.  The two end walls are one quad laid down ten times: the median split cannot separate coincident
    triangles, so each half is a big leaf (10 > 8 triangles, equal distances decided by leaf order) and the
    mirror holds pair, quad and unit records -- what the lean kernel needs to be chosen."""
    s = rt.Scene()
    white = s.add_material(albedo=(0.7, 0.7, 0.7))
    red = s.add_material(albedo=(0.7, 0.2, 0.2), specular=(0.9, 0.9, 0.9), specular_percent=0.3, roughness=0.2)
    light = s.add_material(albedo=(0.0, 0.0, 0.0), emissive=(6.0, 6.0, 6.0))
    lo, hi = (-8.0, -6.0, -4.0), (8.0, 6.0, 20.0)  # the camera at the origin looks along +z
    n = 6  # each wall as an n x n grid of quads: several leaves per wall, some of them big

    def wall(axis, at, mat):
        u, v = [k for k in range(3) if k != axis]
        for i in range(n):
            for j in range(n):
                def p(a, b):
                    q = [0.0, 0.0, 0.0]
                    q[axis] = at
                    q[u] = lo[u] + (hi[u] - lo[u]) * a / n
                    q[v] = lo[v] + (hi[v] - lo[v]) * b / n
                    return tuple(q)
                s.add_quad(p(i, j), p(i + 1, j), p(i + 1, j + 1), p(i, j + 1), mat)

    wall(0, lo[0], red)
    wall(0, hi[0], white)
    wall(1, lo[1], white)
    wall(1, hi[1], light)
    for z in (lo[2], hi[2]):
        for _ in range(10):
            s.add_quad((lo[0], lo[1], z), (hi[0], lo[1], z), (hi[0], hi[1], z), (lo[0], hi[1], z), white)
    s.add_sphere((2.0, -3.0, 12.0), 2.5, red)
    if far_vertex:
        # one vertex beyond the mirror's filtered range (2^62): the scene is not `fast`, every lane is exact
        s.add_triangle((3.0, 5.0, 15.0), (4.0, 5.0, 15.0), (3.5, float(2.0 ** 63), 15.0), white)
    s.set_camera(camera, 0.0, 180.0)
    return s


@pytest.fixture(scope="module")
def references(rt):
    """One reference per scene, shared by the occupancies and left unchanged."""
    ref = {"bunny": oracle_frame("bunny")}
    # the lean kernel is chosen only when the mirror has every array: the box must have big leaves with twin records
    box = quad_box(rt)
    box.set_viewport(W, H)
    box.build()
    quads, units = box.mirror_twins()
    assert len(quads) > 0 and len(units) > 0, "the box scene has no big-leaf records: the general kernel would render it"
    ref["box"] = render(rt, quad_box, tracer="ref")
    ref["box_tiny_origin"] = render(rt, lambda r: quad_box(r, camera=(1e-20, 0.0, 0.0)), tracer="ref")
    ref["box_far_vertex"] = render(rt, lambda r: quad_box(r, far_vertex=True), tracer="ref")
    return ref


@pytest.mark.parametrize("wps", WAVES)
def test_bunny_vs_oracle(rt, references, wps):
    same(render(rt, bunny, wps), references["bunny"], f"bunny at {wps} waves")


@pytest.mark.parametrize("wps", WAVES)
def test_flat_boxes(rt, references, wps):
    """tmin == tmax on every wall hit: the exact slab decides."""
    same(render(rt, quad_box, wps), references["box"], f"quad box at {wps} waves")


@pytest.mark.parametrize("wps", WAVES)
def test_tiny_camera_component(rt, references, wps):
    """One camera-origin component at 1e-20, below the filter's 2^-60: primary rays are not fast, the secondary
    rays (origins on the walls) are, so fast and exact lanes mix in one wave."""
    got = render(rt, lambda r: quad_box(r, camera=(1e-20, 0.0, 0.0)), wps)
    same(got, references["box_tiny_origin"], f"tiny origin at {wps} waves")


@pytest.mark.parametrize("wps", WAVES)
def test_vertex_outside_filtered_range(rt, references, wps):
    """A vertex beyond 2^62: the mirror's `fast` flag is 0 and every lane takes the IEEE slab."""
    got = render(rt, lambda r: quad_box(r, far_vertex=True), wps)
    same(got, references["box_far_vertex"], f"far vertex at {wps} waves")


@pytest.mark.parametrize("wps", WAVES)
def test_leaf_trees(rt, wps):
    """The smallest leaf-tree scene of test_gpu_trees.py (4 bunnies, threshold 200).  Leaf-tree scenes have no
    lean variant (its build measured slower): a knob-free frame of one must still take the general MODE 21."""
    rt.set_build_options(leaf_tree_min=200)
    try:
        s = {}

        def make(r):
            s["scene"] = bunny4(r)
            return s["scene"]

        got = render(rt, make, wps)
        _, tree, _ = s["scene"].mirror(trees=True)
    finally:
        rt.set_build_options()
    assert len(tree) > 0, "the lowered threshold did not produce leaf trees"
    if "bunny4" not in _ORACLE:
        _ORACLE["bunny4"] = oracle_frame("bunny4")
    same(got, _ORACLE["bunny4"], f"bunny4 with leaf trees at {wps} waves")


@pytest.mark.parametrize("wps", WAVES)
def test_lean_equals_general(rt, references, wps):
    """tune 0 (the lean kernel) and the XCD run length set explicitly to its default (RT_TUNE bits 16-19 = 3:
    the same frame through the general kernel) are identical, and the oracle's."""
    lean = render(rt, bunny, wps, tune=0)
    general = render(rt, bunny, wps, tune=3 << 16)
    same(lean, general, f"lean vs general at {wps} waves")
    same(general, references["bunny"], f"general at {wps} waves")
