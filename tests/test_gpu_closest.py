"""Closest-point queries on the GPU (rt_closest_point, csrc/rt_closest.hip) against tests/closest_ref.py and, on the
product scenes, against the host brute force (rt_closest_point_host, pinned to closest_ref by
tests/test_closest_cpu.py).  Every comparison is bytewise on whole 32-byte records: the arithmetic is specified, so no
tolerance applies."""
import numpy as np
import pytest
import torch

import adversarial_cases as AC
import closest_cases as CC
import closest_ref as CR
import rt_testlib as T

pytestmark = pytest.mark.gpu

F32 = np.float32


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F32)).cuda()


@pytest.fixture(scope="module")
def hand():
    h = CC.hand()
    h["scene"].upload(0)
    return h["scene"], h["arrays"], h["points"], CR.closest(h["arrays"], h["points"])


def test_hand_built_scene(hand):
    rt = T.load_rt()
    scene, _, points, want = hand
    got = rt.closest_points(scene, dev(points))
    assert got.shape == (len(points), 8) and got.dtype == torch.float32
    CC.same_records(got.cpu().numpy(), want, "hand-built scene")


@pytest.mark.parametrize("name", CC.ADVERSARIAL)
def test_adversarial_scene(name):
    rt = T.load_rt()
    c = CC.adversarial(name)
    with AC.build_options(rt, c["tree"]):
        c["scene"].upload(0)
        _, tree, _ = c["scene"].mirror(trees=True)
    assert (tree.shape[0] > 0) == c["tree"]  # scene B walks its leaf tree
    want = CR.closest(c["arrays"], c["points"], rows=256)
    for waves in (0, 5, 6, 7):
        got = rt.closest_points(c["scene"], dev(c["points"]), waves_per_simd=waves)
        CC.same_records(got.cpu().numpy(), want, f"adversarial scene {name}, waves {waves}")


@pytest.fixture(scope="module", params=["bunny", "bunny4"])
def product(request):
    rt = T.load_rt()
    c = CC.product(request.param)
    c["scene"].upload(0)
    want = rt.closest_points_host(c["scene"], c["points"])
    kind = CR.fields(want)["kind"]
    assert (kind == 0).sum() >= 64 and (kind == 1).sum() >= 1 and (kind == 2).sum() >= 1024
    return request.param, c["scene"], dev(c["points"]), want


@pytest.mark.parametrize("waves", [0, 5, 6, 7])
def test_product_scene(product, waves):
    rt = T.load_rt()
    which, scene, points, want = product
    if which == "bunny4":  # its 12,318-triangle leaf is walked through its leaf tree
        _, tree, _ = scene.mirror(trees=True)
        assert tree.shape[0] > 0
    got = rt.closest_points(scene, points, waves_per_simd=waves)
    CC.same_records(got.cpu().numpy(), want, f"{which}, waves {waves}")


@pytest.mark.parametrize("spheres", [True, False], ids=["as built", "no sphere"])
@pytest.mark.parametrize("name", list(CC.DECKS))
def test_deep_stacks(name, spheres):
    """BVHs 29, 39 and 62 levels deep: the stack-40 and stack-64 builds.  Without the deck's sphere the apex's walk
    pushes one entry per level; as built, deck29's stays inside the stack's LDS entries, so only the sphere-less case
    runs the stack-40 build's overflow entries (tests/test_closest_cpu.py test_decks_need_their_deep_stacks)."""
    rt = T.load_rt()
    c = CC.deck(name, spheres)
    c["scene"].upload(0)
    assert c["scene"].max_depth() == CC.DECKS[name]
    want = rt.closest_points_host(c["scene"], c["points"])
    got = rt.closest_points(c["scene"], dev(c["points"]))
    CC.same_records(got.cpu().numpy(), want, f"{name}, spheres {spheres}")


@pytest.mark.parametrize("count", [1, 63, 64, 65])
def test_partial_waves(hand, count):
    rt = T.load_rt()
    scene, _, points, want = hand
    out = torch.full((count + 64, 8), 0, dtype=torch.float32, device="cuda")
    out.view(torch.uint8).fill_(0xA5)
    before = out.cpu().numpy().copy()
    got = rt.closest_points(scene, dev(points[:count]), out=out)
    assert got.data_ptr() == out.data_ptr()  # out= is returned in place
    res = out.cpu().numpy()
    CC.same_records(res[:count], want[:count], f"{count} points")
    assert res[count:].tobytes() == before[count:].tobytes()  # records at and past `count` untouched


def test_empty_batch(hand):
    rt = T.load_rt()
    scene = hand[0]
    got = rt.closest_points(scene, torch.empty((0, 4), dtype=torch.float32, device="cuda"))
    assert got.shape == (0, 8)
    p = rt.ClosestParams()  # and the call itself: count 0 with live pointers
    buf = torch.zeros((4, 8), dtype=torch.float32, device="cuda")
    p.points, p.count, p.nearest = buf.data_ptr(), 0, buf.data_ptr()
    import ctypes
    assert rt.lib().rt_closest_point(ctypes.byref(p), rt._scene_ptr(scene), None) == 0


def test_repeatable_on_a_stream(hand):
    rt = T.load_rt()
    scene, _, points, want = hand
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        p = dev(points)
        a = rt.closest_points(scene, p, stream=s)
        b = rt.closest_points(scene, p, stream=s)
    s.synchronize()
    CC.same_records(a.cpu().numpy(), want, "first call on a stream")
    CC.same_records(b.cpu().numpy(), want, "second call on a stream")


def test_buffer_checks(hand):
    """The refusals that need a device: a short buffer and an overlap."""
    rt = T.load_rt()
    scene, _, points, _ = hand
    p = dev(points[:64])
    with pytest.raises(rt.RTError, match="rt_closest_point: points too small"):
        q = rt.ClosestParams()  # 2^31 points are allowed; these buffers do not hold them
        import ctypes
        out = torch.zeros((64, 8), dtype=torch.float32, device="cuda")
        q.points, q.count, q.nearest = p.data_ptr(), 2 ** 31, out.data_ptr()
        rt._check(rt.lib().rt_closest_point(ctypes.byref(q), rt._scene_ptr(scene), None), "rt_closest_point")
    both = torch.zeros((64, 8), dtype=torch.float32, device="cuda")
    with pytest.raises(rt.RTError, match="rt_closest_point: nearest overlaps points"):
        rt.closest_points(scene, both.view(-1)[:256].view(64, 4), out=both)


def test_raytracer_closest_points():
    rt = T.load_rt()
    tr = rt.RayTracer(32, 18, scene="bunny", spp=1, bounces=2)
    c = CC.product("bunny")
    pts = c["points"][:256]
    want = rt.closest_points_host(c["scene"], pts)
    CC.same_records(tr.closest_points(dev(pts)).cpu().numpy(), want, "a fresh tracer")  # before any frame
    assert tr.frame_index == 0 and tr.rng is None
    tr.process()
    surface, last, rng, frame = tr.surface.clone(), tr.last_frame.clone(), tr.rng.clone(), tr.frame_index
    CC.same_records(tr.closest_points(dev(pts)).cpu().numpy(), want, "after a frame")
    assert torch.equal(tr.surface.view(torch.uint8), surface.view(torch.uint8))
    assert torch.equal(tr.last_frame.view(torch.uint8), last.view(torch.uint8))
    assert torch.equal(tr.rng.view(torch.uint8), rng.view(torch.uint8)) and tr.frame_index == frame


def test_distance_grid(hand):
    rt = T.load_rt()
    scene, arrays, _, _ = hand
    lo, hi, n = (-4.0, -4.0, -4.0), (8.0, 8.0, 8.0), 8
    grid = rt.distance_grid(scene, lo, hi, (n, n, n))
    assert grid.shape == (n, n, n) and grid.dtype == torch.float32
    c = F32(-4.0) + (np.arange(n, dtype=F32) + F32(0.5)) * F32(1.5)  # the cell centres
    z, y, x = np.meshgrid(c, c, c, indexing="ij")
    pts = np.stack([x, y, z, np.full_like(x, np.inf)], axis=-1).reshape(-1, 4)
    want = CR.closest(arrays, pts, rows=512)[:, 0].reshape(n, n, n)
    assert grid.cpu().numpy().tobytes() == want.tobytes()
    # a radius: cells with nothing in reach hold it
    near = rt.distance_grid(scene, lo, hi, (n, n, n), radius=1.0).cpu().numpy()
    assert ((near == 1.0) | (near == want)).all() and (near == 1.0).any() and (near[want < 1.0] == want[want < 1.0]).all()
