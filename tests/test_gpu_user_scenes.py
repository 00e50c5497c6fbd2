"""Caller-built scenes (tests/scene_cases.py) on the GPU against the live CPU oracle: every frame, the progressive
second frame and the final RNG states, bit for bit (tolerance 0: equal bytes, equal NaN positions), through the
default kernel, the general kernel, the two reference-layout tracers and the wavefront tracer.

What makes each case worth rendering (which materials are seen, how deep the DFS stack gets, which kernel the
chooser picks) is asserted on the oracle alone by tests/test_user_scenes_cpu.py; the depth cases' stack use is
checked there against the stack each kernel is launched with, before anything here runs.  The oracle's frames are
rendered once per case (scene_cases.oracle_frames) and shared.

The scenes no kernel may see -- a BVH deeper than rt_variant.h's kMaxBvhDepth, a scene without triangles -- are
refused; those tests need the device only for the buffers they prove untouched.
"""
import numpy as np
import pytest
import torch

import denoise_ref as D
import occlusion_ref as O
import rt_testlib as T
import scene_cases as C
from test_user_scenes_cpu import default_variant

pytestmark = pytest.mark.gpu
ids = lambda cases: [c["name"] for c in cases]
WAVES_CASES = [C.BY_NAME["room_closed"], C.BY_NAME["deck62"]]
CHAIN_CASES = [C.BY_NAME[n] for n in ("room_closed", "room_tilted", "room_inside_sphere")]
CAMERA_CASES = [c for c in C.CASES if c["camera"] not in (C.DEFAULT_CAMERA, C.DECK_CAMERA) or c["name"] == "box_front"]


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    torch.cuda.set_device(0)
    rt = T.load_rt()
    rt.load_experimental()  # the wavefront tracer lives in librt_hip_exp.so
    return rt


def uploaded(rt, case):
    s = C.apply_product(rt, case)
    w, h = case["width"], case["height"]
    rng = rt.alloc_rng(w * h)
    rt.init_rng_states(rng, w, h, T.SEED)
    s.upload(rng.data_ptr())
    return s, rng


def frames_of(rt, case, tracer="fast", tune=0, wps=0):
    """([FRAMES surfaces [h, w, 4]], final RNG states [h * w, 6] uint32): frame 0 and the progressive frames after it."""
    s, rng = uploaded(rt, case)
    w, h = case["width"], case["height"]
    a, b = rt.alloc_surface(w, h), rt.alloc_surface(w, h)
    outs = []
    for f in range(C.FRAMES):
        cur, prev = (a, b) if f % 2 == 0 else (b, a)
        rt.render(s, cur, prev, w, h, case["spp"], case["bounces"], frame_index=f, tracer=tracer, tune=tune, waves_per_simd=wps)
        outs.append(rt.surface_view(cur, w).cpu().numpy().copy())
    torch.cuda.synchronize()
    return outs, rng.view(-1, 12)[:, :6].cpu().numpy().view(np.uint32).copy()


def same(got, case, what):
    """`got` (frames_of) equals the oracle's frames and states; a failure names the first differing pixel."""
    want = C.oracle_frames(case)
    frames, rng = got
    for f, (g, o) in enumerate(zip(frames, want["frames"])):
        nan_g, nan_o = np.isnan(g), np.isnan(o)  # (a NaN's payload bits are the ISA's choice)
        bad = (nan_g != nan_o) | (~nan_g & ~nan_o & (g.view(np.uint32) != o.view(np.uint32)))
        if bad.any():
            y, x, c = [int(v[0]) for v in np.nonzero(bad)]
            raise AssertionError(f"{case['name']} {what}, frame {f}: {int(bad.sum())} of {bad.size} words differ; first at pixel "
                                 f"({x}, {y}) channel {c}: got {g[y, x, c]!r} ({g.view(np.uint32)[y, x, c]:#010x}), oracle "
                                 f"{o[y, x, c]!r} ({o.view(np.uint32)[y, x, c]:#010x})")
    bad = (rng != want["rng"]).any(axis=1)
    assert not bad.any(), f"{case['name']} {what}: final RNG states of {int(bad.sum())} pixels differ, first pixel {int(np.flatnonzero(bad)[0])}"


@pytest.mark.parametrize("case", C.CASES, ids=ids(C.CASES))
def test_default_frame(rt, case):
    s = C.apply_product(rt, case)
    s.build()
    v = default_variant(rt, s)
    assert v["mode"] == (17 | 128 if case["expect"]["lean"] else 17), "tests/test_user_scenes_cpu.py pins the same"
    same(frames_of(rt, case), case, "default kernel")


@pytest.mark.parametrize("case", C.CASES, ids=ids(C.CASES))
def test_general_kernel(rt, case):
    """The XCD run length set explicitly to its default (RT_TUNE bits 16-19 = 3): the same frame through MODE 17 general."""
    same(frames_of(rt, case, tune=3 << 16), case, "general kernel")


@pytest.mark.parametrize("tracer", ["ref", "flat", "wavefront"])
@pytest.mark.parametrize("case", C.CASES, ids=ids(C.CASES))
def test_other_tracers(rt, case, tracer):
    same(frames_of(rt, case, tracer=tracer), case, f"tracer={tracer}")


@pytest.mark.parametrize("wps", [5, 6, 7])
@pytest.mark.parametrize("case", WAVES_CASES, ids=ids(WAVES_CASES))
def test_waves_per_simd(rt, case, wps):
    same(frames_of(rt, case, wps=wps), case, f"{wps} waves per SIMD")


@pytest.mark.parametrize("case", CAMERA_CASES, ids=ids(CAMERA_CASES))
def test_camera_poses_with_entry_records(rt, case):
    """The poses again with the entry_frontier build option on, where the chooser then starts camera rays from entry
    records (test_default_frame is the option off, the shipped default)."""
    s = C.apply_product(rt, case)
    s.build()
    assert rt.build_options().entry_frontier == 0, "shipped off"
    v = default_variant(rt, s, want_entry=1)
    assert v["use_entry"] == 1, "every pose scene is shallow, lean and inside the filtered range"
    built = rt.entry_table_builds()
    rt.set_build_options(entry_frontier=1)
    try:
        got = frames_of(rt, case)
    finally:
        rt.set_build_options()
    assert rt.entry_table_builds() > built, "the option did not reach the frame"
    same(got, case, "entry records on")


# --- trace_camera -> ambient_occlusion -> denoise on a ragged frame ------------------------------------------------------
AO_SAMPLES, AO_RADIUS, AO_BIAS = 2, 3.0, 0.001


@pytest.mark.parametrize("case", CHAIN_CASES, ids=ids(CHAIN_CASES))
def test_query_ao_denoise_chain(rt, case):
    import query_ref as Q
    w, h = case["width"], case["height"]
    assert (w * h) % 64, "a last wave that is not whole"
    o = C.oracle_frames(case)
    want_hits, _, _ = Q.trace(o["arrays"], Q.camera_rays(o["camera"], w, h))
    s, _ = uploaded(rt, case)
    records = rt.trace_camera(s, w, h)
    assert records.cpu().numpy().tobytes() == want_hits.tobytes(), "first-hit records"
    table = rt.ao_directions(256)
    want_ao, occ, _ = O.ao(o["arrays"], want_hits, w, h, table, AO_SAMPLES, AO_RADIUS, AO_BIAS)
    assert 0 < int(occ.sum()) < occ.size * AO_SAMPLES, "some samples occluded, some open"
    ao = rt.ambient_occlusion(s, records, w, h, AO_RADIUS, samples=AO_SAMPLES, bias=AO_BIAS, directions=table)
    got_ao = ao.cpu().numpy().reshape(-1)
    assert got_ao.tobytes() == want_ao.tobytes(), f"{int((got_ao != want_ao).sum())} of {w * h} AO values differ"
    # the oracle's frame 0 through the filter, guided by the GPU's records
    surface = rt.alloc_surface(w, h)
    rt.surface_view(surface, w).copy_(torch.from_numpy(o["frames"][0]).cuda())
    out = rt.denoise(s, surface, w, h, hits=records)
    torch.cuda.synchronize()
    got = rt.surface_view(out, w).cpu().numpy()
    want = D.denoise(o["frames"][0], want_hits, s.materials())
    nan_g, nan_w = np.isnan(got), np.isnan(want)
    assert np.array_equal(nan_g, nan_w) and np.array_equal(got.view(np.uint32)[~nan_g], want.view(np.uint32)[~nan_w]), "denoised frame"


# --- the inputs that must not reach a kernel ---------------------------------------------------------------------------
def patterned(rt, w, h):
    surface = rt.alloc_surface(w, h)
    surface.copy_(torch.arange(surface.numel(), dtype=torch.float32, device="cuda").reshape(surface.shape) * 0.5 + 3.0)
    return surface, surface.clone()


@pytest.mark.parametrize("case", C.REFUSED, ids=ids(C.REFUSED))
def test_too_deep_bvh_is_refused_everywhere(rt, case):
    """Depth 63 and 80: the render, query, occlusion and AO entry points name the limit and launch nothing."""
    w, h = case["width"], case["height"]
    s, rng = uploaded(rt, case)  # the upload itself is host work and copies
    assert s.max_depth() == case["expect"]["depth"]
    rng_before = rng.clone()
    surface, before = patterned(rt, w, h)
    last = rt.alloc_surface(w, h)
    text = f"is {case['expect']['depth']} levels deep; the traversal stack holds depth <= 62"
    for tracer in ("fast", "ref", "flat", "wavefront"):
        with pytest.raises(rt.RTError, match="rt_render: the scene's BVH " + text):
            rt.render(s, surface, last, w, h, 1, 1, tracer=tracer)
    with pytest.raises(rt.RTError, match="rt_render: the scene's BVH " + text):
        rt.render(s, surface, last, w, h, 1, 1, tune=3 << 16)
    hits = torch.full((w * h, 12), 5.0, dtype=torch.float32, device="cuda")
    rays = torch.zeros((64, 8), dtype=torch.float32, device="cuda")
    rays[:, 3], rays[:, 6] = 1e30, -1.0
    occ = torch.full((64,), 9, dtype=torch.uint8, device="cuda")
    ao = torch.full((h, w), 4.0, dtype=torch.float32, device="cuda")
    with pytest.raises(rt.RTError, match="rt_trace_rays: the scene's BVH " + text):
        rt.trace_camera(s, w, h, hits=hits)
    with pytest.raises(rt.RTError, match="rt_trace_rays: the scene's BVH " + text):
        rt.trace_rays(s, rays, hits=hits)
    with pytest.raises(rt.RTError, match="rt_occluded: the scene's BVH " + text):
        rt.occluded(s, rays, out=occ)
    with pytest.raises(rt.RTError, match="rt_ao: the scene's BVH " + text):
        rt.ambient_occlusion(s, hits, w, h, 1.0, samples=1, out=ao)
    torch.cuda.synchronize()
    assert torch.equal(surface, before) and torch.equal(rng, rng_before)
    assert bool((hits == 5.0).all()) and bool((occ == 9).all()) and bool((ao == 4.0).all())


def test_scene_without_triangles_is_refused(rt):
    """BVH::Calculate's lone root of a triangle-less scene reads as an inner node whose children are itself and one
    past the array: no tracer terminates on it.  rt_scene_upload refuses it before any device state
    exists, so rt_render finds a scene that was never uploaded."""
    w, h = 37, 19
    s = rt.Scene()
    s.add_sphere((0.0, 0.0, 5.0), 1.0, s.add_material(albedo=(0.5, 0.5, 0.5)))
    s.set_viewport(w, h)
    rng = rt.alloc_rng(w * h)
    with pytest.raises(rt.RTError, match="rt_scene_upload: the scene has no triangles to traverse"):
        s.upload(rng.data_ptr())
    gpu = s.gpu.contents
    assert not gpu.gpu_bvh_nodes and not gpu.rng_state and not gpu.gpu_spheres
    surface, before = patterned(rt, w, h)
    for tracer in ("fast", "ref", "flat", "wavefront"):
        with pytest.raises(rt.RTError, match="rt_render: scene not uploaded"):
            rt.render(s, surface, rt.alloc_surface(w, h), w, h, 1, 1, tracer=tracer)
    with pytest.raises(rt.RTError):
        rt.trace_camera(s, w, h)
    torch.cuda.synchronize()
    assert torch.equal(surface, before)
