"""rt_radiance on the GPU (csrc/rt_radiance.hip), bit for bit.

1. Against the CPU oracle's per-offset sample table (radiance_ref, whose soundness tests/test_radiance_cpu.py shows): a
   ray that is the jittered camera ray of draws (2i, 2i + 1) of a pixel's state, handed the state advanced by 2i + 2,
   gets table row i and leaves the state advanced by 2i + draws_i -- every pixel, i < 4, no ray left out.
2. Against the renderer (oracle-pinned elsewhere, not under test here): the same rays of sample 0 give rt_render's
   spp = 1 surface and final states.
3. Arbitrary rays: panoramas of a purely emissive box give the emissive colour of rt_trace_rays' first hit.
4. samples, bounces = 0.  5. Ragged counts, occupancies, a stream, canaries, rays that are not traced.  6. Refusals.
"""
import ctypes

import numpy as np
import pytest
import torch

import radiance_cases as RC
import radiance_ref as R
import rt_testlib as T
import scene_cases as C

pytestmark = pytest.mark.gpu

F32, U32 = np.float32, np.uint32
ENTRIES = 4
USER_CASES = ["room_closed", "room_tilted", "room_inside_sphere", "spheres70", "deck62", "deck29_plain"]
PRODUCT = {"bunny": (64, 36, 6), "bunny4": (64, 36, 6)}  # width, height, bounces


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    torch.cuda.set_device(0)
    return T.load_rt()


# --- one description of every scene used here: the uploaded product scene and the oracle's view of it ---------------
_SETUPS = {}


def setup(rt, name):
    """{"scene", "oracle", "w", "h", "bounces", "camera", "states": the frame's initial states uint32 [w * h, 6]}."""
    got = _SETUPS.get(name)
    if got is None:
        if name in PRODUCT:
            w, h, bounces = PRODUCT[name]
            s = rt.Scene()
            s.setup(name)
            s.set_viewport(w, h)
            o = T.OracleScene(name)
        else:
            case = RC.CASE if name == RC.CASE["name"] else C.BY_NAME[name]
            w, h, bounces = case["width"], case["height"], case["bounces"]
            s = C.apply_product(rt, case)
            o, code = C.apply_oracle(case)
            assert code == 0
        s.upload(0)  # queried only: rt_radiance takes its states from the caller
        got = _SETUPS[name] = {"scene": s, "oracle": o, "w": w, "h": h, "bounces": bounces, "camera": o.camera(w, h),
                               "states": T.oracle_rng_frame(T.SEED, w, h)}
    return got


def sample_rays(su, i):
    """(rays of table entry i for every pixel, the states to hand rt_radiance with them)."""
    base = R.xorwow_advance(su["states"], 2 * i)
    u = R.uniforms(base, 2)
    return R.jittered_camera_rays(su["camera"], su["w"], su["h"], u[:, 0], u[:, 1]), R.xorwow_advance(base, 2)


def run(rt, scene, rays, states6, **kw):
    """rt.radiance on host arrays -> (float32 [N, 4], final states uint32 [N, 12])."""
    d_rays = torch.from_numpy(np.ascontiguousarray(rays, dtype=F32)).cuda()
    d_rng = torch.from_numpy(R.pack_states(states6).copy()).cuda()
    out = rt.radiance(scene, d_rays, d_rng, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy(), d_rng.cpu().numpy().view(U32).reshape(-1, R.STATE_WORDS)


def same_words(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    g, w = got.view(U32), want.view(U32)
    nan = np.isnan(got) & np.isnan(want) if got.dtype == F32 else np.zeros(got.shape, bool)
    differing = (g != w) & ~nan
    if differing.any():
        k = tuple(int(v[0]) for v in np.nonzero(differing))
        pytest.fail(f"{what}: {int(differing.any(axis=-1).sum())} of {got.shape[0]} rows differ; first at {k}: got {got[k]!r} "
                    f"({g[k]:#010x}), want {want[k]!r} ({w[k]:#010x})")


def same_states(got12, want6, what):
    same_words(got12[:, :6], np.asarray(want6, dtype=U32), what + ": states")
    assert not got12[:, 6:].any(), what + ": the unused words of the states were written"


# --- 1. the oracle, single samples ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", USER_CASES + list(PRODUCT))
def test_single_samples_against_the_oracle_table(rt, name):
    su = setup(rt, name)
    P = su["w"] * su["h"]
    tables = R.frame_tables(name, su["oracle"], su["w"], su["h"], su["bounces"], su["states"], ENTRIES if name in PRODUCT else 14)
    rays, states = zip(*[sample_rays(su, i) for i in range(ENTRIES)])
    got, rng = run(rt, su["scene"], np.concatenate(rays), np.concatenate(states), bounces=su["bounces"], samples=1)
    want = np.ones((ENTRIES * P, 4), dtype=F32)
    want_rng = np.zeros((ENTRIES * P, 6), dtype=U32)
    for i in range(ENTRIES):
        want[i * P:(i + 1) * P, 0:3] = tables[:, i, 0:3]
        want_rng[i * P:(i + 1) * P] = R.xorwow_advance(su["states"], 2 * i + tables[:, i, 3].astype(np.int64))
    assert (tables[:, :ENTRIES, 3] > 2).any() and (tables[:, :ENTRIES, 0:3] != 0).any(), "a table of misses in the dark proves nothing"
    same_words(got, want, f"{name}: radiance of {ENTRIES} x {P} camera samples")
    same_states(rng, want_rng, name)


# --- 2. the renderer -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["room_open_sky", "bunny"])
def test_sample_zero_is_the_renderers_frame(rt, name):
    su = setup(rt, name)
    w, h = su["w"], su["h"]
    s = su["scene"]
    frame_rng = rt.alloc_rng(w * h)
    rt.init_rng_states(frame_rng, w, h, T.SEED)
    before = frame_rng.cpu().numpy().view(U32).reshape(-1, R.STATE_WORDS)[:, :6].copy()
    assert np.array_equal(before, su["states"])
    s.upload(frame_rng.data_ptr())
    try:
        surface = rt.alloc_surface(w, h)
        rt.render(s, surface, None, w, h, 1, su["bounces"], frame_index=0)
        torch.cuda.synchronize()
        want = rt.surface_view(surface, w).cpu().numpy().reshape(w * h, 4)
        want_rng = frame_rng.cpu().numpy().view(U32).reshape(-1, R.STATE_WORDS)[:, :6]
    finally:
        s.upload(0)
    rays, states = sample_rays(su, 0)
    got, rng = run(rt, s, rays, states, bounces=su["bounces"], samples=1)
    assert (want[:, 0:3] != 0).any() and (want_rng != R.xorwow_advance(su["states"], 2)).any()
    same_words(got, want, f"{name}: rt_render spp 1 against rt_radiance")
    same_states(rng, want_rng, name)


# --- 3. arbitrary rays: the first hit's emission ---------------------------------------------------------------------
@pytest.mark.parametrize("where", list(RC.ORIGINS))
def test_panorama_of_the_emissive_box(rt, where):
    su = setup(rt, RC.CASE["name"])
    s = su["scene"]
    pw, ph = RC.PANORAMA
    rays = rt.panorama_rays(RC.ORIGINS[where], pw, ph)
    states = np.stack([T.oracle_rng_state(T.SEED, 5)] * (pw * ph))
    states[:, 0] += np.arange(pw * ph, dtype=U32)  # distinct states (any words do: only their advance is checked)
    hits = rt.hit_fields(rt.trace_rays(s, torch.from_numpy(rays).cuda()).cpu().numpy())
    hit = hits["kind"] != rt.HIT_MISS
    assert int(hit.sum()) >= 64 and int((~hit).sum()) >= 64, (where, int(hit.sum()))
    assert (hits["kind"] == rt.HIT_SPHERE).any() or where == "outside"
    emissive = s.materials()[:, 4:7]
    want = np.zeros((pw * ph, 4), dtype=F32)
    want[:, 3] = 1.0
    want[hit, 0:3] = emissive[hits["material"][hit]]
    assert len(set(map(tuple, want[hit, 0:3]))) >= 3, "several materials in view"
    got, rng = run(rt, s, rays, states, bounces=1, samples=1)
    same_words(got, want, f"emissive box from {where}")
    same_states(rng, R.xorwow_advance(states, np.where(hit, 4, 0)), f"emissive box from {where}")


# --- 4. samples, bounces = 0 -----------------------------------------------------------------------------------------
def test_samples_are_chained_single_samples(rt):
    su = setup(rt, "room_tilted")
    rays, states = sample_rays(su, 0)
    colours, st = [], states
    for _ in range(3):
        c, r12 = run(rt, su["scene"], rays, st, bounces=su["bounces"], samples=1)
        colours.append(c[:, 0:3])
        st = r12[:, :6].copy()
    want = np.ones((rays.shape[0], 4), dtype=F32)
    want[:, 0:3] = (((colours[0] + colours[1]).astype(F32) + colours[2]).astype(F32) / F32(3.0)).astype(F32)
    assert any((colours[0] != c).any() for c in colours[1:]), "the three samples of a ray differ somewhere"
    got, rng = run(rt, su["scene"], rays, states, bounces=su["bounces"], samples=3)
    same_words(got, want, "samples = 3 against three chained calls")
    same_states(rng, st, "samples = 3")


def test_zero_bounces(rt):
    su = setup(rt, "room_tilted")
    rays, states = sample_rays(su, 0)
    got, rng = run(rt, su["scene"], rays, states, bounces=0, samples=2)
    want = np.zeros((rays.shape[0], 4), dtype=F32)
    want[:, 3] = 1.0
    same_words(got, want, "bounces = 0")
    same_states(rng, states, "bounces = 0")


# --- 5. shapes and occupancy -----------------------------------------------------------------------------------------
_FULL = {}


def full_batch(rt, name):
    """(rays, states, radiance, final states) of sample 0 of every pixel at the default occupancy, once per scene."""
    if name not in _FULL:
        su = setup(rt, name)
        rays, states = sample_rays(su, 0)
        _FULL[name] = (rays, states, *run(rt, su["scene"], rays, states, bounces=su["bounces"], samples=1))
    return _FULL[name]


@pytest.mark.parametrize("count", [1, 63, 64, 65, 0])
def test_counts_and_canaries(rt, count):
    su = setup(rt, "room_closed")
    rays, states, want, want_rng = full_batch(rt, "room_closed")
    extra = 7
    d_rays = torch.from_numpy(rays[:count + extra].copy()).cuda()[:count]
    packed = R.pack_states(states[:count + extra]).view(U32).reshape(-1, R.STATE_WORDS).copy()
    packed[count:] = 0xC0FFEE11
    d_rng = torch.from_numpy(packed.reshape(-1).view(np.int32)).cuda()
    out = torch.full((count + extra, 4), -7.5, dtype=torch.float32, device="cuda")
    ret = rt.radiance(su["scene"], d_rays, d_rng, bounces=su["bounces"], samples=1, out=out)
    torch.cuda.synchronize()
    assert ret is out
    got, rng = out.cpu().numpy(), d_rng.cpu().numpy().view(U32).reshape(-1, R.STATE_WORDS)
    same_words(got[:count], want[:count], f"count {count}")
    same_words(rng[:count], want_rng[:count], f"count {count}: states")
    assert (got[count:] == F32(-7.5)).all() and (rng[count:] == 0xC0FFEE11).all(), "rows past count were written"
    if count == 0:
        empty = rt.radiance(su["scene"], d_rays, d_rng)
        assert empty.shape == (0, 4)


@pytest.mark.parametrize("wps", [5, 6, 7])
@pytest.mark.parametrize("name", ["room_closed", "bunny4"])
def test_waves_per_simd(rt, name, wps):
    su = setup(rt, name)
    rays, states, want, want_rng = full_batch(rt, name)
    got, rng = run(rt, su["scene"], rays, states, bounces=su["bounces"], samples=1, waves_per_simd=wps)
    same_words(got, want, f"{name} at {wps} waves per SIMD against the default")
    same_words(rng, want_rng, f"{name} at {wps} waves per SIMD: states")


def test_on_a_stream(rt):
    su = setup(rt, "room_closed")
    rays, states, want, want_rng = full_batch(rt, "room_closed")
    d_rays = torch.from_numpy(rays).cuda()
    d_rng = torch.from_numpy(R.pack_states(states).copy()).cuda()
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    out = rt.radiance(su["scene"], d_rays, d_rng, bounces=su["bounces"], samples=1, stream=stream)
    stream.synchronize()
    same_words(out.cpu().numpy(), want, "on a non-default stream")
    same_words(d_rng.cpu().numpy().view(U32).reshape(-1, R.STATE_WORDS), want_rng, "on a non-default stream: states")


def test_rays_that_are_not_traced(rt):
    """Zero, infinite and NaN directions give (0, 0, 0, 1) and leave their states alone; a NaN origin is traced as
    rt_trace_rays traces it -- every test against it fails, so the path is one miss: the sky along the direction, no
    draw.  The other rays of the batch are not disturbed."""
    su = setup(rt, "room_tilted")
    assert C.BY_NAME["room_tilted"]["sky"]
    rays, states, _, _ = full_batch(rt, "room_tilted")
    n = 130
    rays, states = rays[:n].copy(), states[:n].copy()
    clean, clean_rng = run(rt, su["scene"], rays, states, bounces=su["bounces"], samples=2)
    away = np.array([0.6, 0.8, 0.0], dtype=F32)  # from (100, 0, 0) it leaves the room behind: a certain miss
    rays[129, 0:3], rays[129, 4:7] = (100.0, 0.0, 0.0), away
    dead = {3: (0.0, 0.0, 0.0), 64: (np.inf, 0.0, 0.0), 65: (0.0, -np.inf, 1.0), 100: (np.nan, 0.0, 1.0), 127: (1.0, 1.0, np.nan)}
    for k, d in dead.items():
        rays[k, 4:7] = d
    nan_origin = {17: (np.nan, np.nan, np.nan), 128: (np.nan, 0.5, 1.0)}
    for k, o in nan_origin.items():
        rays[k, 0:3], rays[k, 4:7] = o, away
    got, rng = run(rt, su["scene"], rays, states, bounces=su["bounces"], samples=2)
    want, want_rng = clean.copy(), clean_rng[:, :6].copy()
    for k in dead:
        want[k], want_rng[k] = (0.0, 0.0, 0.0, 1.0), states[k]
    assert (got[129, 0:3] > 0).any() and (rng[129, :6] == states[129]).all(), "the reference ray misses into the sky"
    for k in list(nan_origin) + [129]:
        want[k], want_rng[k] = got[129], states[k]
    same_words(got, want, "a batch with rays that are not traced")
    same_states(rng, want_rng, "a batch with rays that are not traced")


# --- 6. refusals -------------------------------------------------------------------------------------------------------
def buffers(n):
    rays = torch.zeros((n, 8), dtype=torch.float32, device="cuda")
    rays[:, 6] = 1.0
    rng = torch.full((n * R.STATE_WORDS,), 0x1234567, dtype=torch.int32, device="cuda")
    out = torch.full((n, 4), 3.25, dtype=torch.float32, device="cuda")
    return rays, rng, out


def test_foreign_scene_is_refused(rt):
    su = setup(rt, "room_closed")
    g = su["scene"].gpu.contents
    f = rt.GPUScene()
    ctypes.pointer(f)[0] = g
    other_nodes = torch.zeros((64,), dtype=torch.float32, device="cuda")  # another address: no mirror is registered for it
    f.gpu_bvh_nodes = other_nodes.data_ptr()
    rays, rng, out = buffers(64)
    with pytest.raises(rt.RTError, match="rt_radiance: this GPUScene was not uploaded by rt_scene_upload"):
        rt.radiance(f, rays, rng, out=out)
    torch.cuda.synchronize()
    assert bool((out == 3.25).all()) and bool((rng == 0x1234567).all())


@pytest.mark.parametrize("case", C.REFUSED, ids=[c["name"] for c in C.REFUSED])
def test_too_deep_bvh_is_refused(rt, case):
    s = C.apply_product(rt, case)
    s.upload(0)
    rays, rng, out = buffers(64)
    text = f"rt_radiance: the scene's BVH is {case['expect']['depth']} levels deep; the traversal stack holds depth <= 62"
    with pytest.raises(rt.RTError, match=text):
        rt.radiance(s, rays, rng, out=out)
    torch.cuda.synchronize()
    assert bool((out == 3.25).all()) and bool((rng == 0x1234567).all())


def test_short_and_overlapping_buffers_are_refused(rt):
    su = setup(rt, "room_closed")
    s = su["scene"]
    L = rt.lib()
    rays, rng, out = buffers(64)

    def refused(word, **kw):
        p = rt.RadianceParams()
        p.rays, p.count, p.rng, p.radiance = rays.data_ptr(), 64, rng.data_ptr(), out.data_ptr()
        p.bounces, p.samples = 1, 1
        for k, v in kw.items():
            setattr(p, k, v)
        code = L.rt_radiance(ctypes.byref(p), ctypes.cast(s.gpu, ctypes.c_void_p), None)
        msg = L.rt_last_error()
        assert code != 0 and msg.startswith(b"rt_radiance: ") and word in msg, (kw, code, msg)

    # (torch's tensors are carved out of larger allocations, so only a count beyond any allocation is certainly short)
    refused(b"rays too small", count=2 ** 31)
    big = torch.zeros((64 * 12 + 64 * 4,), dtype=torch.float32, device="cuda")
    refused(b"radiance overlaps rays", rays=big.data_ptr(), radiance=big.data_ptr() + 64 * 32 - 16)
    refused(b"radiance overlaps rng", rng=big.data_ptr(), radiance=big.data_ptr() + 64 * 48 - 16)
    torch.cuda.synchronize()
    assert bool((out == 3.25).all()) and bool((rng == 0x1234567).all())


def test_raytracer_panorama_leaves_the_frame_alone(rt):
    w, h = 64, 36
    tr = rt.RayTracer(w, h, scene="bunny", spp=2, bounces=3, seed=T.SEED)
    tr.process()
    torch.cuda.synchronize()
    frame, states, index = tr.surface.clone(), tr.rng.clone(), tr.frame_index
    pano = tr.panorama(48, 24)
    torch.cuda.synchronize()
    assert pano.shape == rt.alloc_surface(48, 24).shape
    view = rt.surface_view(pano, 48).cpu().numpy()
    assert np.isfinite(view).all() and (view[:, :, 3] == 1).all() and (view[:, :, 0:3] > 0).any()
    assert torch.equal(tr.surface, frame) and torch.equal(tr.rng, states) and tr.frame_index == index
    # the same rays and states through the module-level calls
    rays = torch.from_numpy(rt.panorama_rays(tuple(tr.scene.camera().origin), 48, 24)).cuda()
    again = rt.radiance(tr.scene, rays, rt.ray_rng(48 * 24, T.SEED), bounces=3, samples=2)
    torch.cuda.synchronize()
    assert np.array_equal(again.cpu().numpy().reshape(24, 48, 4), view)
    # ray_rng: state i is curand_init(seed, i, 0)
    st = rt.ray_rng(70, T.SEED).cpu().numpy().view(U32).reshape(-1, R.STATE_WORDS)
    assert np.array_equal(st[:, :6], np.stack([T.oracle_rng_state(T.SEED, i) for i in range(70)]))
