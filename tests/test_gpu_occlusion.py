"""Occlusion queries and AO on the GPU (rt_occluded, rt_ao, csrc/rt_occlude.hip) against tests/occlusion_ref.py.
rt_occluded's contract is bytewise: byte i is `kind != 0` of rt_trace_rays' record for ray i, for every ray.  rt_ao's
arithmetic is specified, so its image compares bytewise too.  tests/test_occlusion_cpu.py shows that the cases are
not trivial."""
import numpy as np
import pytest
import torch

import adversarial_cases as AC
import occlusion_cases as OC
import occlusion_ref as O
import query_ref as Q
import rt_testlib as T

pytestmark = pytest.mark.gpu

F32 = np.float32
W, H = OC.W, OC.H


def same_bytes(got, want, what):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got
    want = np.asarray(want, dtype=np.uint8)
    assert got.dtype == np.uint8 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    if bad.size:
        i = int(bad[0])
        pytest.fail(f"{what}: {bad.size} of {want.size} bytes differ; first at ray {i}: got {got[i]}, want {want[i]}")


def occluded_want(hits):
    return (OC.kinds(hits) != 0).astype(np.uint8)


def uploaded(which, w, h):
    """A product scene uploaded for queries only: no RNG states."""
    rt = T.load_rt()
    s = rt.Scene()
    s.setup(which)
    s.set_viewport(w, h)
    s.upload(0)
    return s


@pytest.fixture(scope="module")
def bunny():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    torch.cuda.set_device(0)
    return dict(OC.bunny(), scene=uploaded("bunny", W, H))


@pytest.mark.parametrize("waves", [0, 5, 6, 7])
def test_camera_rays_bunny(bunny, waves):
    rt = T.load_rt()
    want = occluded_want(bunny["hits"])
    assert {0, 1} <= set(want.tolist())
    got = rt.occluded(bunny["scene"], torch.from_numpy(bunny["rays"]).cuda(), waves_per_simd=waves)
    assert got.shape == (W * H,) and got.dtype == torch.uint8 and got.is_cuda
    same_bytes(got, want, f"bunny 64x36 pixel-centre rays, waves {waves}")


def test_incoherent_rays_bunny(bunny):
    rt = T.load_rt()
    rays, want, free = OC.incoherent()
    k, kf = OC.kinds(want), OC.kinds(free)
    assert (kf == 0).sum() >= 64 and (kf != 0).sum() >= 64 and (k[::3] == 0).sum() >= 64
    dev = torch.from_numpy(rays).cuda()
    got = rt.occluded(bunny["scene"], dev)
    same_bytes(got, occluded_want(want), "incoherent rays")
    # and against rt_trace_rays on the device: the contract in its own terms
    records = rt.hit_fields(rt.trace_rays(bunny["scene"], dev))
    assert torch.equal(got, (records["kind"] != 0).to(torch.uint8))


def test_tmax_at_and_just_above_the_hit(bunny):
    rt = T.load_rt()
    at, above, want_at, want_above = OC.tmax_edges()
    assert want_above.sum() >= 64 and (want_at == 0).sum() >= 64
    same_bytes(rt.occluded(bunny["scene"], torch.from_numpy(at).cuda()), want_at, "tmax = t")
    # compared to the reference only: not every one of these is occluded (occlusion_cases.tmax_edges)
    same_bytes(rt.occluded(bunny["scene"], torch.from_numpy(above).cuda()), want_above, "tmax = nextafter(t, inf)")


@pytest.fixture(scope="module")
def bunny4():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    torch.cuda.set_device(0)
    scene = uploaded("bunny4", OC.AW, OC.AH)
    _, tree, _ = scene.mirror(trees=True)
    assert tree.shape[0] > 0  # a leaf tree: the MODE 21 kernel
    return dict(OC.bunny4(), scene=scene)


@pytest.mark.parametrize("waves", [0, 6, 7])
def test_leaf_tree_scene(bunny4, waves):
    rt = T.load_rt()
    want = occluded_want(bunny4["hits"])
    assert {0, 1} <= set(want.tolist())
    got = rt.occluded(bunny4["scene"], torch.from_numpy(bunny4["rays"]).cuda(), waves_per_simd=waves)
    same_bytes(got, want, f"bunny4 32x18 pixel-centre rays, waves {waves}")


# --- the hand-built scene of tests/test_gpu_query.py: spheres, tmax between and before hits, a ray inside a sphere ---
@pytest.fixture(scope="module")
def handmade():
    import test_gpu_query as TQ
    rt = T.load_rt()
    s = rt.Scene()
    s.add_material(albedo=(0.5, 0.5, 0.5))
    s.add_material(albedo=(0.9, 0.1, 0.1), emissive=(1, 2, 3))
    s.add_material(albedo=(0.1, 0.9, 0.1))
    s.add_material(albedo=(0.1, 0.1, 0.9), emissive=(0.5, 0.25, 0.125))
    s.add_quad((-2, -2, 5), (2, -2, 5), (2, 2, 5), (-2, 2, 5), 1)
    s.add_quad((4, -2, -2), (4, 2, -2), (4, 2, 2), (4, -2, 2), 2)
    for c, r, m in TQ.SPHERES:
        s.add_sphere(c, r, m)
    s.set_viewport(16, 16)
    s.upload(0)
    a = dict(s.host_arrays())
    sph = np.zeros((len(TQ.SPHERES), 8), dtype=np.uint32)
    for i, (c, r, m) in enumerate(TQ.SPHERES):
        sph[i, 0:4] = np.array([*c, r], dtype=F32).view(np.uint32)
        sph[i, 4] = m
    a["spheres"], a["materials"] = sph, s.materials()
    rays, named = TQ.handmade_rays()
    assert len(rays) == 80
    want, _, _ = Q.trace(Q.Arrays(a), rays)
    return s, rays, want


def test_hand_built_scene(handmade):
    rt = T.load_rt()
    scene, rays, want = handmade
    k = OC.kinds(want)
    assert k[8] == 1 and k[9] == 1 and k[10] == 0 and k[11] == 0 and k[18] == 1 and k[19] == 0  # the tmax cases
    assert {0, 1, 2} <= set(k.tolist())
    same_bytes(rt.occluded(scene, torch.from_numpy(rays).cuda()), occluded_want(want), "hand-built scene")


@pytest.mark.parametrize("count", [1, 63, 64, 65])
def test_partial_waves(handmade, count):
    rt = T.load_rt()
    scene, rays, want = handmade
    out = torch.full((count + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    got = rt.occluded(scene, torch.from_numpy(rays[:count].copy()).cuda(), out=out)
    assert got.data_ptr() == out.data_ptr()
    host = out.cpu().numpy()
    same_bytes(host[:count], occluded_want(want[:count]), f"{count} rays")
    assert (host[count:] == 0xA5).all()  # bytes at and past `count` are untouched


# --- the adversarial scenes: every ray, the non-finite, zero-direction and gate families included (the fallback) -----
@pytest.fixture(scope="module", params=["A", "B"] + ["C:" + v for v in AC.GATES if not AC.GATES[v][1]])
def adversarial(request):
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    torch.cuda.set_device(0)
    rt = T.load_rt()
    name = request.param
    with AC.build_options(rt, name == "B"):
        case = AC.build_case(rt, name)
        case.scene.upload(0)
        _, tree, _ = case.scene.mirror(trees=True)
    assert (len(tree) > 0) == (name == "B")  # B: the leaf-tree kernel; A and C: the lean kernel
    if name.startswith("C:"):
        assert not AC.expected_fast(case.scene.host_arrays()["nodes"])  # outside the filtered range
    return name, case, AC.ray_set(case)


def test_adversarial_rays(adversarial):
    rt = T.load_rt()
    name, case, rs = adversarial
    want = occluded_want(rs.want)
    assert {0, 1} <= set(want.tolist())
    assert {5, 6} <= set(rs.family.tolist())  # ray gates and non-finite rays are in the set
    same_bytes(rt.occluded(case.scene, torch.from_numpy(rs.rays).cuda()), want, f"adversarial scene {name}")


def test_repeatable_on_a_stream(bunny):
    rt = T.load_rt()
    dev = torch.from_numpy(bunny["rays"]).cuda()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        a = rt.occluded(bunny["scene"], dev, stream=s)
        b = rt.occluded(bunny["scene"], dev, stream=s)
    s.synchronize()
    assert torch.equal(a, b)
    same_bytes(a, occluded_want(bunny["hits"]), "non-default stream")


# --- AO ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["bunny", "bunny4"])
def test_ao(which, request):
    rt = T.load_rt()
    c = OC.ao_case(which)
    scene = request.getfixturevalue(which)["scene"] if which == "bunny4" else uploaded("bunny", OC.AW, OC.AH)
    n = OC.AW * OC.AH
    counts = np.bincount(c["occ"], minlength=OC.AO_SAMPLES + 1)
    assert (counts >= 10).all(), counts
    kw = dict(samples=OC.AO_SAMPLES, bias=OC.AO_BIAS, directions=OC.ao_directions())
    # over the reference's own camera records
    got = rt.ambient_occlusion(scene, torch.from_numpy(c["hits"]).cuda(), OC.AW, OC.AH, OC.AO_RADIUS, **kw)
    assert got.shape == (OC.AH, OC.AW) and got.dtype == torch.float32 and got.is_cuda
    host = got.cpu().numpy().reshape(-1)
    assert host.tobytes() == c["ao"].tobytes(), f"{which}: {(host != c['ao']).sum()} of {n} AO values differ"
    miss = OC.kinds(c["hits"]) == 0
    assert miss.any() and (host[miss].view(np.uint32) == 0x3F800000).all()  # missed pixels are exactly 1.0f
    # and over the GPU's own records
    records = rt.trace_camera(scene, OC.AW, OC.AH)
    assert records.cpu().numpy().tobytes() == c["hits"].tobytes()
    again = rt.ambient_occlusion(scene, records, OC.AW, OC.AH, OC.AO_RADIUS, **kw)
    assert again.cpu().numpy().tobytes() == c["ao"].tobytes()


def test_raytracer_ao_leaves_the_frame_alone():
    rt = T.load_rt()
    c = OC.ao_case("bunny")
    tracer = rt.RayTracer(OC.AW, OC.AH, "bunny", spp=1, bounces=1, seed=T.SEED)
    tracer.process()
    torch.cuda.synchronize()
    state = lambda: (tracer.frame_index, tracer.surface.cpu().numpy().tobytes(), tracer.last_frame.cpu().numpy().tobytes(),
                     tracer.rng.cpu().numpy().tobytes())
    before = state()
    got = tracer.ao(OC.AO_RADIUS, samples=OC.AO_SAMPLES, bias=OC.AO_BIAS, directions=OC.ao_directions())
    torch.cuda.synchronize()
    assert state() == before and before[0] == 1
    assert got.cpu().numpy().reshape(-1).tobytes() == c["ao"].tobytes()
    # and before any frame was rendered: no RNG states exist, none are made
    fresh = rt.RayTracer(OC.AW, OC.AH, "bunny", spp=1, bounces=1, seed=T.SEED)
    g2 = fresh.ao(OC.AO_RADIUS, samples=OC.AO_SAMPLES, bias=OC.AO_BIAS, directions=OC.ao_directions())
    assert fresh.rng is None and fresh.frame_index == 0
    assert g2.cpu().numpy().tobytes() == got.cpu().numpy().tobytes()


def test_empty_batch(bunny):
    rt = T.load_rt()
    got = rt.occluded(bunny["scene"], torch.zeros((0, 8), dtype=torch.float32, device="cuda"))
    assert got.shape == (0,) and got.dtype == torch.uint8 and got.is_cuda


def test_default_direction_table_is_kept(bunny):
    """directions=None: ao_directions(256), uploaded once per device, and the image that table gives when passed."""
    rt = T.load_rt()
    records = rt.trace_camera(bunny["scene"], W, H)
    a = rt.ambient_occlusion(bunny["scene"], records, W, H, OC.AO_RADIUS, samples=2)
    table = rt._ao_default_directions(records.device)
    assert table.is_cuda and table.cpu().numpy().tobytes() == rt.ao_directions(256).tobytes()
    b = rt.ambient_occlusion(bunny["scene"], records, W, H, OC.AO_RADIUS, samples=2)
    assert rt._ao_default_directions(records.device) is table
    c = rt.ambient_occlusion(bunny["scene"], records, W, H, OC.AO_RADIUS, samples=2, directions=rt.ao_directions(256))
    assert torch.equal(a, b) and torch.equal(a, c) and 0.0 < float(a.mean()) < 1.0
