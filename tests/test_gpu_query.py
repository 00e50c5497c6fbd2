"""Ray queries on the GPU (rt_trace_rays, csrc/rt_query.hip) against tests/query_ref.py.  Every comparison
is bytewise on whole 48-byte records: the arithmetic is specified, so no tolerance applies."""
import numpy as np
import pytest
import torch

import query_ref as Q
import rt_testlib as T

pytestmark = pytest.mark.gpu

W, H = 64, 36
F32 = np.float32


def same_records(got, want, what):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got
    g, w = np.ascontiguousarray(got, F32).view(np.uint32).reshape(-1, 12), np.ascontiguousarray(want, F32).view(np.uint32).reshape(-1, 12)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.nonzero((g != w).any(axis=1))[0]
    if bad.size:
        i = int(bad[0])
        pytest.fail(f"{what}: {bad.size} of {g.shape[0]} records differ; first {i}:\n got  {g[i].view(F32)} {g[i, 1:4]}\n"
                    f" want {w[i].view(F32)} {w[i, 1:4]}")


def uploaded(which, w, h):
    """A product scene uploaded for queries only: no RNG states."""
    rt = T.load_rt()
    s = rt.Scene()
    s.setup(which)
    s.set_viewport(w, h)
    s.upload(0)
    return s


def unit_vectors(n, seed):
    v = np.random.default_rng(seed).normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32)


@pytest.fixture(scope="module")
def bunny():
    """The bunny scene on the device, its reference arrays, and the reference's records for the 64x36 pixel-centre
    rays (computed once; tests 1, 2 and 8 share them)."""
    osc = T.OracleScene("bunny")
    arrays = Q.Arrays(osc.arrays())
    rays = Q.camera_rays(osc.camera(W, H), W, H)
    hits, counters, leaf_size = Q.trace(arrays, rays)
    assert (leaf_size > 8).any()  # the wave-cooperative big-leaf rounds are exercised
    return {"scene": uploaded("bunny", W, H), "arrays": arrays, "rays": rays, "hits": hits, "oracle": osc}


@pytest.mark.parametrize("waves", [0, 5, 6, 7])
def test_camera_mode_bunny(bunny, waves):
    rt = T.load_rt()
    got = rt.trace_camera(bunny["scene"], W, H, waves_per_simd=waves)
    assert got.shape == (W * H, 12) and got.dtype == torch.float32
    same_records(got, bunny["hits"], "camera mode 64x36")
    # the same rays passed explicitly
    same_records(rt.trace_rays(bunny["scene"], torch.from_numpy(bunny["rays"]).cuda()), bunny["hits"], "explicit pixel-centre rays")


def test_incoherent_rays_bunny(bunny):
    rt = T.load_rt()
    n = 1041  # not a multiple of 64
    ref = bunny["hits"]
    hit = np.nonzero(ref.view(np.uint32)[:, 1] != 0)[0][:n]
    assert hit.size == n
    rays = np.zeros((n, 8), dtype=F32)
    rays[:, 0:3] = ref[hit, 8:11] + ref[hit, 4:7] * F32(0.01)
    rays[:, 3] = F32(1e30)
    rays[:, 4:7] = unit_vectors(n, 20240607)
    free, _, _ = Q.trace(bunny["arrays"], rays)
    rays[::3, 3] = free[::3, 0] * F32(0.5)  # every third ray: half its unbounded distance
    want = free.copy()
    want[::3], _, _ = Q.trace(bunny["arrays"], rays[::3])
    assert (want.view(np.uint32)[::3, 1] == 0).all() and (want[::3, 0] == rays[::3, 3]).all()
    kinds = set(want.view(np.uint32)[:, 1].tolist())
    assert {0, 2} <= kinds
    same_records(rt.trace_rays(bunny["scene"], torch.from_numpy(rays).cuda()), want, "incoherent rays")


# --- the hand-built scene: two quads, three spheres (one encloses the origin) -----------------------------------
SPHERES = [((1.0, 1.0, 3.0), 0.5, 3), ((0.0, 3.0, 0.0), 1.0, 1), ((0.0, 0.0, 0.0), 1.0, 0)]


@pytest.fixture(scope="module")
def handmade():
    rt = T.load_rt()
    s = rt.Scene()
    s.add_material(albedo=(0.5, 0.5, 0.5))
    s.add_material(albedo=(0.9, 0.1, 0.1), emissive=(1, 2, 3))
    s.add_material(albedo=(0.1, 0.9, 0.1))
    s.add_material(albedo=(0.1, 0.1, 0.9), emissive=(0.5, 0.25, 0.125))
    s.add_quad((-2, -2, 5), (2, -2, 5), (2, 2, 5), (-2, 2, 5), 1)
    s.add_quad((4, -2, -2), (4, 2, -2), (4, 2, 2), (4, -2, 2), 2)
    for c, r, m in SPHERES:
        s.add_sphere(c, r, m)
    s.set_viewport(16, 16)
    s.upload(0)
    a = dict(s.host_arrays())
    sph = np.zeros((len(SPHERES), 8), dtype=np.uint32)
    for i, (c, r, m) in enumerate(SPHERES):
        sph[i, 0:4] = np.array([*c, r], dtype=F32).view(np.uint32)
        sph[i, 4] = m
    a["spheres"], a["materials"] = sph, s.materials()
    return s, Q.Arrays(a)


def handmade_rays():
    big = 1e30
    cases = [
        # one direction component exactly 0
        ((0.3, 0.2, 1.5), big, (0.1, 0.0, 1.0)),
        ((1.5, 0.3, 0.4), big, (1.0, 0.25, 0.0)),
        # two components exactly 0 (axis-parallel)
        ((0.5, -0.5, 1.5), big, (0.0, 0.0, 1.0)),
        ((1.5, 0.3, 0.4), big, (1.0, 0.0, 0.0)),
        ((1.5, 0.3, 0.4), big, (0.0, -1.0, 0.0)),
        # starting on a quad, towards and away from the rest of the scene
        ((0.5, -1.0, 5.0), big, (0.0, 0.0, -1.0)),
        ((-1.0, 0.5, 5.0), big, (0.1, 0.2, 1.0)),
        ((4.0, 0.5, 0.5), big, (-1.0, -0.125, -0.125)),
        # the sphere at t = 1, the quad behind it at t = 3.5: unbounded, tmax between them, tmax before both
        ((1.0, 1.0, 1.5), big, (0.0, 0.0, 1.0)),
        ((1.0, 1.0, 1.5), 2.0, (0.0, 0.0, 1.0)),
        ((1.0, 1.0, 1.5), 0.5, (0.0, 0.0, 1.0)),
        # past the sphere to the quad, tmax before the quad
        ((1.7, 1.0, 1.5), 3.0, (0.0, 0.0, 1.0)),
        # misses
        ((0.0, 20.0, 0.0), big, (0.0, 1.0, 0.0)),
        ((10.0, 10.0, 10.0), big, (1.0, 1.0, 1.0)),
        ((-3.0, -3.0, 1.0), big, (-1.0, 0.2, 0.1)),
        # a direction of length 3 and directions of length 1
        ((-1.0, -2.5, 1.0), big, (1.0, 2.0, 2.0)),
        ((-2.0, -1.5, 1.0), big, (0.6, 0.0, 0.8)),
        ((1.5, -1.0, 0.0), big, (1.0, 0.0, 0.0)),
        # from inside the sphere that encloses the origin
        ((0.0, 0.0, 0.0), big, (0.2, 0.1, 1.0)),
        ((0.0, 0.0, 0.0), 0.5, (0.2, 0.1, 1.0)),
    ]
    rays = np.zeros((len(cases) + 60, 8), dtype=F32)
    for i, (o, tmax, d) in enumerate(cases):
        rays[i, 0:3], rays[i, 3], rays[i, 4:7] = o, tmax, d
    g = np.random.default_rng(7)
    k = len(cases)
    rays[k:, 0:3] = g.uniform(-3, 3, size=(60, 3)).astype(F32)
    rays[k:, 3] = F32(big)
    rays[k:, 4:7] = unit_vectors(60, 8) * g.uniform(0.5, 3, size=(60, 1)).astype(F32)
    return rays, len(cases)


@pytest.fixture(scope="module")
def handmade_ref(handmade):
    rays, named = handmade_rays()
    hits, counters, _ = Q.trace(handmade[1], rays)
    return rays, hits, named


def test_hand_built_scene(handmade, handmade_ref):
    rt = T.load_rt()
    rays, want, named = handmade_ref
    kind, t = want.view(np.uint32)[:, 1], want[:, 0]
    # the cases are what their comments say (so the comparison below means something)
    assert kind[8] == 1 and t[8] == 1.0 and kind[9] == 1 and kind[10] == 0 and t[10] == 0.5
    assert kind[11] == 0 and t[11] == 3.0
    assert (kind[12:15] == 0).all() and (t[12:15] == F32(1e30)).all()
    assert kind[0] == 2 and kind[2] == 2 and kind[3] == 2 and kind[15] == 2 and t[15] == 6.0 and kind[16] == 2
    assert kind[7] == 1 and want.view(np.uint32)[7, 2] == 2
    assert kind[18] == 1 and want.view(np.uint32)[18, 2] == 2 and kind[19] == 0
    assert {0, 1, 2} <= set(kind[named:].tolist())
    same_records(rt.trace_rays(handmade[0], torch.from_numpy(rays).cuda()), want, "hand-built scene")


@pytest.mark.parametrize("count", [1, 63, 64, 65])
def test_partial_waves(handmade, handmade_ref, count):
    rt = T.load_rt()
    rays, want, _ = handmade_ref
    sentinel = float(np.array([0x7FC0BEEF], dtype=np.uint32).view(F32)[0])
    hits = torch.full((count + 64, 12), sentinel, dtype=torch.float32, device="cuda")
    before = hits.cpu().numpy().copy()
    dev = torch.from_numpy(rays[:count].copy()).cuda()
    out = rt.trace_rays(handmade[0], dev, hits=hits)
    assert out.data_ptr() == hits.data_ptr()
    got = hits.cpu().numpy()
    same_records(got[:count], want[:count], f"{count} rays")
    assert got[count:].tobytes() == before[count:].tobytes()  # rows at and past `count` keep the sentinel


@pytest.fixture(scope="module")
def bunny4():
    w, h = 32, 18
    osc = T.OracleScene("bunny4")
    want, _, leaf_size = Q.trace(osc.arrays(), Q.camera_rays(osc.camera(w, h), w, h))
    assert leaf_size.max() >= 1024  # a leaf large enough for a leaf tree is hit (rt_build_options.leaf_tree_min)
    scene = uploaded("bunny4", w, h)
    _, tree, _ = scene.mirror(trees=True)
    assert tree.shape[0] > 0
    return scene, want, w, h


@pytest.mark.parametrize("waves", [0, 6, 7])
def test_leaf_tree_scene(bunny4, waves):
    """bunny4: its 12,318-triangle leaf has a leaf tree, so this is the MODE 21 kernel (each occupancy build)."""
    rt = T.load_rt()
    scene, want, w, h = bunny4
    same_records(rt.trace_camera(scene, w, h, waves_per_simd=waves), want, f"bunny4 camera mode 32x18, waves {waves}")


def test_consistent_with_the_renderer(bunny):
    """The renderer's own frame-0 sample rays, traced as a query: where they hit, the one-bounce frame holds the hit
    material's emission."""
    rt = T.load_rt()
    scene = rt.Scene()
    scene.setup("bunny")
    scene.set_viewport(W, H)
    rng = rt.alloc_rng(W * H)
    rt.init_rng_states(rng, W, H, T.SEED)
    scene.upload(rng.data_ptr())
    surf, last = rt.alloc_surface(W, H), rt.alloc_surface(W, H)
    rt.render(scene, surf, last, W, H, 1, 1)
    cam = np.frombuffer(bytes(scene.camera()), dtype=F32)  # GPUCamera: 15 floats
    rays = Q.camera_rays(cam, W, H, jitter=Q.frame_jitter(T.SEED, W, H))
    f = rt.hit_fields(rt.trace_rays(scene, torch.from_numpy(rays).cuda()).cpu().numpy())
    rgb = rt.surface_view(surf, W).cpu().numpy().reshape(-1, 4)[:, 0:3]
    hit = f["kind"] != 0
    assert hit.sum() > 0
    emissive = scene.materials()[:, 4:7]
    assert np.ascontiguousarray(rgb[hit]).tobytes() == np.ascontiguousarray(emissive[f["material"][hit]]).tobytes()


def test_repeatable_on_a_stream(bunny):
    rt = T.load_rt()
    dev = torch.from_numpy(bunny["rays"]).cuda()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        a = rt.trace_rays(bunny["scene"], dev, stream=s)
        b = rt.trace_rays(bunny["scene"], dev, stream=s)
    s.synchronize()
    assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    same_records(a, bunny["hits"], "non-default stream")


def test_gbuffer(bunny):
    rt = T.load_rt()
    tracer = rt.RayTracer(W, H, "bunny", spp=1, bounces=1, seed=T.SEED)
    tracer.process()
    torch.cuda.synchronize()
    state = lambda: (tracer.frame_index, tracer.surface.cpu().numpy().tobytes(), tracer.last_frame.cpu().numpy().tobytes(),
                     tracer.rng.cpu().numpy().tobytes())
    before = state()
    g = tracer.gbuffer()
    torch.cuda.synchronize()
    assert state() == before and before[0] == 1
    shapes = {"depth": ((H, W), torch.float32), "normal": ((H, W, 3), torch.float32), "position": ((H, W, 3), torch.float32),
              "albedo": ((H, W, 3), torch.float32), "material": ((H, W), torch.int32), "prim": ((H, W), torch.int32),
              "kind": ((H, W), torch.int32)}
    assert set(g) == set(shapes)
    for k, (shape, dtype) in shapes.items():
        assert tuple(g[k].shape) == shape and g[k].dtype == dtype and g[k].is_cuda, k
    ref = bunny["hits"]
    ints = ref.view(np.int32)
    hit = ints[:, 1] != 0
    host = {k: v.cpu().numpy() for k, v in g.items()}
    assert host["depth"].tobytes() == np.where(hit, ref[:, 0], F32(np.inf)).astype(F32).reshape(H, W).tobytes()
    assert host["normal"].tobytes() == np.ascontiguousarray(ref[:, 4:7]).tobytes()
    assert host["position"].tobytes() == np.ascontiguousarray(ref[:, 8:11]).tobytes()
    assert host["kind"].tobytes() == np.ascontiguousarray(ints[:, 1]).tobytes()
    assert host["material"].tobytes() == np.ascontiguousarray(ints[:, 3]).tobytes()
    assert host["prim"].tobytes() == np.where(hit, ints[:, 2], -1).astype(np.int32).tobytes()
    albedo = np.where(hit[:, None], tracer.scene.materials()[ints[:, 3], 0:3], F32(0)).astype(F32)
    assert host["albedo"].tobytes() == albedo.tobytes()
    # and before any frame was rendered: no RNG states exist, none are made
    fresh = rt.RayTracer(W, H, "bunny", spp=1, bounces=1, seed=T.SEED)
    g2 = fresh.gbuffer()
    assert fresh.rng is None and fresh.frame_index == 0
    assert g2["depth"].cpu().numpy().tobytes() == host["depth"].tobytes()
