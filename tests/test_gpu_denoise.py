"""rt_denoise on the GPU (csrc/denoise.hip) against tests/denoise_ref.py.  Every comparison is bytewise, on the
inputs as downloaded from the device: the filter's arithmetic is specified, so no tolerance applies."""
import numpy as np
import pytest
import torch

import denoise_cases as C
import denoise_ref as D
import rt_testlib as T

pytestmark = pytest.mark.gpu

W, H = 64, 36
F32 = np.float32
SENTINEL = float(np.array([0x7FC0BEEF], dtype=np.uint32).view(F32)[0])


def same_image(got, want, what):
    g = np.ascontiguousarray(got, F32).view(np.uint32)
    w = np.ascontiguousarray(want, F32).view(np.uint32)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.argwhere((g != w).any(axis=-1))
    if bad.size:
        y, x = (int(v) for v in bad[0])
        pytest.fail(f"{what}: {len(bad)} of {g.shape[0] * g.shape[1]} pixels differ; first (x {x}, y {y}):\n"
                    f" got  {g[y, x].view(F32)} {g[y, x]}\n want {w[y, x].view(F32)} {w[y, x]}")


def to_surface(rt, image, extra_floats=0, fill=0.0):
    """[H, W, 4] numpy -> a pitched device surface (alloc_surface's pitch plus `extra_floats`, padding = fill)."""
    h, w = image.shape[0:2]
    row = rt.alloc_surface(w, h).shape[1] + extra_floats
    t = torch.full((h, row), fill, dtype=torch.float32, device="cuda")
    t[:, : w * 4] = torch.from_numpy(np.ascontiguousarray(image).reshape(h, w * 4)).cuda()
    return t


def image_of(rt, surface, w):
    return rt.surface_view(surface, w).cpu().numpy()


@pytest.fixture(scope="module")
def rendered():
    """One 5-spp frame of the bunny scene at 64x36 and its camera's hit records, on the device and downloaded."""
    rt = T.load_rt()
    scene = rt.Scene()
    scene.setup("bunny")
    scene.set_viewport(W, H)
    rng = rt.alloc_rng(W * H)
    rt.init_rng_states(rng, W, H, T.SEED)
    scene.upload(rng.data_ptr())
    surf, last = rt.alloc_surface(W, H), rt.alloc_surface(W, H)
    rt.render(scene, surf, last, W, H, 5, 6)
    hits = rt.trace_camera(scene, W, H)
    torch.cuda.synchronize()
    host = {"surface": image_of(rt, surf, W).copy(), "hits": hits.cpu().numpy().copy(), "materials": scene.materials()}
    kinds = host["hits"].view(np.uint32)[:, 1]
    assert (kinds != 0).sum() > W * H // 2 and (kinds == 0).sum() > 0
    return {"scene": scene, "surface": surf, "hits": hits, "rng": rng, "host": host, "ref": {}}


def reference(r, **kw):
    key = tuple(sorted(kw.items()))
    if key not in r["ref"]:
        r["ref"][key] = D.denoise(r["host"]["surface"], r["host"]["hits"], r["host"]["materials"], **kw)
    return r["ref"][key]


@pytest.mark.parametrize("kw", [{}, {"iterations": 1}, {"iterations": 3}, {"iterations": 5}, {"iterations": 6},
                                {"sigma_color": 0.0}, {"normal_power_log2": 0}, {"iterations": 6, "sigma_color": 0.0},
                                {"iterations": 2, "normal_power_log2": 8, "sigma_plane": 0.004, "sigma_color": 0.5}],
                         ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()) or "defaults")
def test_rendered_input(rendered, kw):
    rt = T.load_rt()
    before = rendered["surface"].clone()
    out = rt.denoise(rendered["scene"], rendered["surface"], W, H, hits=rendered["hits"], **kw)
    torch.cuda.synchronize()
    assert out.data_ptr() != rendered["surface"].data_ptr() and torch.equal(before, rendered["surface"])
    want = reference(rendered, **kw)
    same_image(image_of(rt, out, W), want, f"bunny 64x36 {kw}")
    if not kw:
        # the filter did something, and hits=None traces the same records
        assert (want != rendered["host"]["surface"]).any(axis=-1).mean() > 0.5
        same_image(image_of(rt, rt.denoise(rendered["scene"], rendered["surface"], W, H), W), want, "hits=None")


@pytest.mark.parametrize("size", [(37, 19), (1, 1), (5, 3), (16, 16), (130, 9)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("iterations", [1, 6, D.DEFAULTS["iterations"]])
def test_synthetic_input(size, iterations):
    rt = T.load_rt()
    w, h = size
    image, hits, materials = C.synthetic(w, h, seed=w * 131 + h)
    if w >= 16 and h >= 16:
        f = image[..., 0:3]
        assert np.isnan(f).any() and np.isposinf(f).any() and (f == F32(1e30)).any()
        u = hits.view(np.uint32)
        assert (u[:, 3] >= materials.shape[0]).any() and ((hits[:, 0] == 0) & (u[:, 1] != 0)).any()
        assert 0.15 < (u[:, 1] == 0).mean() < 0.45
    surf = to_surface(rt, image, extra_floats=12, fill=SENTINEL)      # a pitch wider than width * 16 ...
    out = torch.full((h, surf.shape[1] - 4), SENTINEL, dtype=torch.float32, device="cuda")  # ... another for the output
    assert surf.stride(0) * 4 > w * 16 and out.stride(0) != surf.stride(0)
    pad_before, in_pad_before = out.cpu().numpy()[:, w * 4:].copy(), surf.cpu().numpy()[:, w * 4:].copy()
    assert np.isnan(pad_before).all()
    got = rt.denoise_raw(surf, torch.from_numpy(hits).cuda(), torch.from_numpy(materials).cuda(), w, h, out=out,
                         iterations=iterations)
    torch.cuda.synchronize()
    assert got is out
    want = D.denoise(image, hits, materials, iterations=iterations)
    same_image(image_of(rt, out, w), want, f"synthetic {w}x{h}, {iterations} passes")
    pad = out.cpu().numpy()[:, w * 4:]
    assert pad.size > 0 and pad.tobytes() == pad_before.tobytes()  # the padding of the output rows is not written
    assert surf.cpu().numpy()[:, w * 4:].tobytes() == in_pad_before.tobytes()
    same_image(image_of(rt, surf, w), image, "the input surface")


def test_no_materials():
    """material_count 0: every index is beyond the table, every albedo 1."""
    rt = T.load_rt()
    w, h = 37, 19
    image, hits, materials = C.synthetic(w, h, seed=3)
    out = rt.denoise_raw(to_surface(rt, image), torch.from_numpy(hits).cuda(), torch.zeros((0, 16), device="cuda"), w, h)
    same_image(image_of(rt, out, w), D.denoise(image, hits, materials[:0]), "no materials")


def test_in_place(rendered):
    rt = T.load_rt()
    for kw in ({}, {"iterations": 1}):
        surf = rendered["surface"].clone()
        out = rt.denoise(rendered["scene"], surf, W, H, hits=rendered["hits"], out=surf, **kw)
        torch.cuda.synchronize()
        assert out is surf
        same_image(image_of(rt, surf, W), reference(rendered, **kw), f"out == surface {kw}")


def test_side_stream_and_dirty_scratch(rendered):
    rt = T.load_rt()
    want = reference(rendered)
    nbytes = rt.denoise_scratch_bytes(W, H)
    for fill in (float("nan"), 1e30):
        scratch = torch.full((nbytes // 4 + 64,), fill, dtype=torch.float32, device="cuda")
        out = torch.full_like(rendered["surface"], float("nan"))
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            a = rt.denoise(rendered["scene"], rendered["surface"], W, H, hits=rendered["hits"], out=out, scratch=scratch, stream=s)
            b = rt.denoise(rendered["scene"], rendered["surface"], W, H, hits=rendered["hits"], scratch=scratch, stream=s)
        s.synchronize()
        same_image(image_of(rt, a, W), want, "side stream, dirty scratch")
        same_image(image_of(rt, b, W), want, "side stream, scratch reused")
        tail = scratch[nbytes // 4:].cpu().numpy()
        assert tail.tobytes() == np.full(64, fill, dtype=F32).tobytes()  # nothing written past the stated size
    with pytest.raises(rt.RTError, match="scratch too small"):
        rt.denoise(rendered["scene"], rendered["surface"], W, H, hits=rendered["hits"],
                   scratch=torch.empty((nbytes // 4 - 1,), dtype=torch.float32, device="cuda"))


def test_side_stream_allocates_its_own_temporaries(rendered):
    """A side stream that is not torch's current one, nothing passed in: hits, scratch and out are made on that stream
    (the zero fill of a new `out` must not land on another stream behind the filter's writes)."""
    rt = T.load_rt()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    assert torch.cuda.current_stream() != s
    outs = [rt.denoise(rendered["scene"], rendered["surface"], W, H, stream=s) for _ in range(3)]
    tracer = rt.RayTracer(W, H, "bunny", seed=T.SEED)
    tracer.process()
    torch.cuda.synchronize()
    outs.append(tracer.denoised(stream=s))
    assert torch.cuda.current_stream() != s
    s.synchronize()
    for i, out in enumerate(outs):
        same_image(image_of(rt, out, W), reference(rendered), f"side stream, own temporaries, call {i}")


def test_raytracer_denoised(rendered):
    rt = T.load_rt()
    a = rt.RayTracer(W, H, "bunny", seed=T.SEED)
    b = rt.RayTracer(W, H, "bunny", seed=T.SEED)
    a.process()
    b.process()
    torch.cuda.synchronize()
    state = lambda tr: (tr.frame_index, tr.surface.cpu().numpy().tobytes(), tr.last_frame.cpu().numpy().tobytes(),
                        tr.rng.cpu().numpy().tobytes())
    before = state(a)
    out = a.denoised()
    torch.cuda.synchronize()
    assert state(a) == before and before[0] == 1
    assert out.data_ptr() not in (a.surface.data_ptr(), a.last_frame.data_ptr()) and out.shape == a.surface.shape
    # the tracer's first frame is the fixture's frame (same seed, spp and bounces): so is its denoised image
    same_image(image_of(rt, a.surface, W), rendered["host"]["surface"], "RayTracer frame 0")
    same_image(image_of(rt, out, W), reference(rendered), "RayTracer.denoised()")
    same_image(image_of(rt, a.denoised(iterations=2, sigma_color=0.0), W), reference(rendered, iterations=2, sigma_color=0.0),
               "RayTracer.denoised(iterations=2, sigma_color=0)")
    a.process()
    b.process()
    torch.cuda.synchronize()
    assert state(a) == state(b) and a.frame_index == 2
