"""rt_upsample on the GPU (csrc/upsample.hip) against tests/upsample_ref.py.  Every comparison is bytewise, on the
inputs as downloaded from the device: the upsampler's arithmetic is specified, so no tolerance applies."""
import numpy as np
import pytest
import torch

import denoise_ref as D
import rt_testlib as T
import upsample_cases as UC
import upsample_ref as U

pytestmark = pytest.mark.gpu

W, H = 64, 36  # the tracer's size in the RayTracer tests; the rendered tests' outputs are 64x36 or 66x36
F32 = np.float32
SENTINEL = float(np.array([0x7FC0BEEF], dtype=np.uint32).view(F32)[0])
RENDERED = {2: (32, 18), 3: (22, 12), 4: (16, 9)}  # scale -> low size


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
    """The bunny scene; per scale a 5-spp frame at the low size and the camera's records at both sizes, all from one
    upload with the low size as the viewport (the output size has the same aspect, so the same camera)."""
    rt = T.load_rt()
    scene = rt.Scene()
    scene.setup("bunny")
    per_scale = {}
    for s, (lw, lh) in RENDERED.items():
        scene.set_viewport(lw, lh)
        rng = rt.alloc_rng(lw * lh)
        rt.init_rng_states(rng, lw, lh, T.SEED)
        scene.upload(rng.data_ptr())
        surf, last = rt.alloc_surface(lw, lh), rt.alloc_surface(lw, lh)
        rt.render(scene, surf, last, lw, lh, 5, 6)
        low_hits = rt.trace_camera(scene, lw, lh)
        hits = rt.trace_camera(scene, lw * s, lh * s)
        torch.cuda.synchronize()
        host = {"low": image_of(rt, surf, lw).copy(), "low_hits": low_hits.cpu().numpy().copy(),
                "hits": hits.cpu().numpy().copy(), "materials": scene.materials()}
        kinds = host["hits"].view(np.uint32)[:, 1]
        assert (kinds != 0).sum() > lw * lh * s * s // 2 and (kinds == 0).sum() > 0
        per_scale[s] = {"surface": surf, "low_hits": low_hits, "hits": hits, "rng": rng, "host": host, "ref": {}}
    return {"scene": scene, "scales": per_scale}


def reference(r, **kw):
    key = tuple(sorted(kw.items()))
    if key not in r["ref"]:
        h = r["host"]
        scale = int(round((h["hits"].shape[0] / h["low_hits"].shape[0]) ** 0.5))
        r["ref"][key] = U.upsample(h["low"], h["low_hits"], h["hits"], h["materials"], scale, **kw)
    return r["ref"][key]


@pytest.mark.parametrize("scale", [2, 3, 4])
def test_rendered_input(rendered, scale):
    rt = T.load_rt()
    lw, lh = RENDERED[scale]
    r = rendered["scales"][scale]
    # the scene's uploaded camera is the last scale's; upload this one's again, as a caller of these sizes would have
    rendered["scene"].set_viewport(lw, lh)
    rendered["scene"].upload(r["rng"].data_ptr())
    before = r["surface"].clone()
    out = rt.upsample(rendered["scene"], r["surface"], lw, lh, scale, low_hits=r["low_hits"], hits=r["hits"])
    torch.cuda.synchronize()
    assert torch.equal(before, r["surface"]) and out.shape[0] == lh * scale
    want, stage = reference(r)
    same_image(image_of(rt, out, lw * scale), want, f"bunny {lw}x{lh} x{scale}")
    assert (stage == 1).mean() > 0.5, np.bincount(stage.reshape(-1))
    same_image(image_of(rt, rt.upsample(rendered["scene"], r["surface"], lw, lh, scale), lw * scale), want, "no records passed")
    same_image(image_of(rt, rt.upsample(rendered["scene"], r["surface"], lw, lh, scale, low_hits=r["low_hits"]), lw * scale),
               want, "hits=None")
    same_image(image_of(rt, rt.upsample(rendered["scene"], r["surface"], lw, lh, scale, hits=r["hits"]), lw * scale),
               want, "low_hits=None")


@pytest.mark.parametrize("low_size, scale", [((1, 1), 2), ((5, 3), 2), ((37, 19), 2), ((22, 3), 3), ((17, 2), 4), ((19, 17), 3)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else "x%d" % v)
def test_synthetic_input(low_size, scale):
    rt = T.load_rt()
    lw, lh = low_size
    w, h = lw * scale, lh * scale
    low, low_hits, hits, materials = UC.synthetic(lw, lh, scale, seed=lw * 131 + lh)
    want, stage = U.upsample(low, low_hits, hits, materials, scale)
    if lw * lh >= 15:
        share = np.bincount(stage.reshape(-1), minlength=4)[1:4] / stage.size
        assert (share >= 0.01).all(), share  # every stage decides pixels
    surf = to_surface(rt, low, extra_floats=12, fill=SENTINEL)        # a pitch wider than the rows ...
    out = torch.full((h, rt.alloc_surface(w, h).shape[1] + 20), SENTINEL, dtype=torch.float32, device="cuda")  # ... another
    assert surf.stride(0) * 4 > lw * 16 and out.stride(0) * 4 > w * 16 and out.stride(0) != surf.stride(0)
    pad_before, in_pad_before = out.cpu().numpy()[:, w * 4:].copy(), surf.cpu().numpy()[:, lw * 4:].copy()
    assert np.isnan(pad_before).all()
    d_low_hits, d_hits, d_materials = (torch.from_numpy(a).cuda() for a in (low_hits, hits, materials))
    got = rt.upsample_raw(surf, d_low_hits, d_hits, d_materials, lw, lh, scale, out=out)
    torch.cuda.synchronize()
    assert got is out
    same_image(image_of(rt, out, w), want, f"synthetic {lw}x{lh} x{scale}")
    pad = out.cpu().numpy()[:, w * 4:]
    assert pad.size > 0 and pad.tobytes() == pad_before.tobytes()  # the padding of the output rows is not written
    assert surf.cpu().numpy()[:, lw * 4:].tobytes() == in_pad_before.tobytes()
    same_image(image_of(rt, surf, lw), low, "the low surface")
    assert d_low_hits.cpu().numpy().tobytes() == low_hits.tobytes() and d_hits.cpu().numpy().tobytes() == hits.tobytes()
    assert d_materials.cpu().numpy().tobytes() == materials.tobytes()


@pytest.mark.parametrize("kw", [{"normal_power_log2": 0}, {"normal_power_log2": 8}, {"sigma_plane": 0.004}],
                         ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_parameters(kw):
    rt = T.load_rt()
    lw, lh, scale = 37, 19, 2
    low, low_hits, hits, materials = UC.synthetic(lw, lh, scale, seed=7)
    want, stage = U.upsample(low, low_hits, hits, materials, scale, **kw)
    if "sigma_plane" in kw:
        # a tighter plane tolerance leaves fewer usable taps: more pixels go on to stage 2 and 3
        _, stage_default = U.upsample(low, low_hits, hits, materials, scale)
        assert (stage > 1).sum() > (stage_default > 1).sum()
    out = rt.upsample_raw(to_surface(rt, low), torch.from_numpy(low_hits).cuda(), torch.from_numpy(hits).cuda(),
                          torch.from_numpy(materials).cuda(), lw, lh, scale, **kw)
    same_image(image_of(rt, out, lw * scale), want, f"synthetic {kw}")


def test_no_materials():
    """material_count 0: every index is beyond the table, every albedo 1."""
    rt = T.load_rt()
    lw, lh, scale = 22, 3, 3
    low, low_hits, hits, materials = UC.synthetic(lw, lh, scale, seed=3)
    out = rt.upsample_raw(to_surface(rt, low), torch.from_numpy(low_hits).cuda(), torch.from_numpy(hits).cuda(),
                          torch.zeros((0, 16), device="cuda"), lw, lh, scale)
    same_image(image_of(rt, out, lw * scale), U.upsample(low, low_hits, hits, materials[:0], scale)[0], "no materials")


def test_side_stream_and_dirty_scratch(rendered):
    rt = T.load_rt()
    scale = 2
    lw, lh = RENDERED[scale]
    r = rendered["scales"][scale]
    want, _ = reference(r)
    args = (rendered["scene"], r["surface"], lw, lh, scale)
    records = dict(low_hits=r["low_hits"], hits=r["hits"])
    nbytes = rt.upsample_scratch_bytes(lw, lh)
    for fill in (float("nan"), 1e30):
        scratch = torch.full((nbytes // 4 + 64,), fill, dtype=torch.float32, device="cuda")
        out = torch.full((lh * scale, rt.alloc_surface(lw * scale, lh * scale).shape[1]), float("nan"), device="cuda")
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            a = rt.upsample(*args, out=out, scratch=scratch, stream=s, **records)
            b = rt.upsample(*args, scratch=scratch, stream=s, **records)
        s.synchronize()
        same_image(image_of(rt, a, lw * scale), want, "side stream, dirty scratch")
        same_image(image_of(rt, b, lw * scale), want, "side stream, scratch reused")
        tail = scratch[nbytes // 4:].cpu().numpy()
        assert tail.tobytes() == np.full(64, fill, dtype=F32).tobytes()  # nothing written past the stated size
    with pytest.raises(rt.RTError, match="scratch too small"):
        rt.upsample(*args, scratch=torch.empty((nbytes // 4 - 1,), dtype=torch.float32, device="cuda"), **records)


def test_side_stream_allocates_its_own_temporaries(rendered):
    """A side stream that is not torch's current one, nothing passed in: both sets of records, scratch and out are made
    on that stream."""
    rt = T.load_rt()
    scale = 2
    lw, lh = RENDERED[scale]
    r = rendered["scales"][scale]
    rendered["scene"].set_viewport(lw, lh)
    rendered["scene"].upload(r["rng"].data_ptr())
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    assert torch.cuda.current_stream() != s
    outs = [rt.upsample(rendered["scene"], r["surface"], lw, lh, scale, stream=s) for _ in range(3)]
    assert torch.cuda.current_stream() != s
    s.synchronize()
    for i, out in enumerate(outs):
        same_image(image_of(rt, out, lw * scale), reference(r)[0], f"side stream, own temporaries, call {i}")


def test_raytracer_upsampled():
    rt = T.load_rt()
    a = rt.RayTracer(W, H, "bunny", seed=T.SEED)
    b = rt.RayTracer(W, H, "bunny", seed=T.SEED)
    a.process()
    b.process()
    torch.cuda.synchronize()
    state = lambda tr: (tr.frame_index, tr.surface.cpu().numpy().tobytes(), tr.last_frame.cpu().numpy().tobytes(),
                        tr.rng.cpu().numpy().tobytes())
    before = state(a)
    scale = 2
    out = a.upsampled()
    filtered = a.upsampled(scale=scale, denoise=True)
    low_hits, hits = rt.trace_camera(a.scene, W, H), rt.trace_camera(a.scene, W * scale, H * scale)
    torch.cuda.synchronize()
    assert state(a) == before and before[0] == 1
    assert out.data_ptr() not in (a.surface.data_ptr(), a.last_frame.data_ptr())
    assert out.shape[0] == H * scale and out.shape[1] >= W * scale * 4
    frame, materials = image_of(rt, a.surface, W), a.scene.materials()
    low_hits, hits = low_hits.cpu().numpy(), hits.cpu().numpy()
    same_image(image_of(rt, out, W * scale), U.upsample(frame, low_hits, hits, materials, scale)[0], "RayTracer.upsampled()")
    same_image(image_of(rt, filtered, W * scale), U.upsample(D.denoise(frame, low_hits, materials), low_hits, hits, materials, scale)[0],
               "RayTracer.upsampled(denoise=True)")
    same_image(image_of(rt, a.upsampled(scale=3, sigma_plane=0.01), W * 3),
               U.upsample(frame, low_hits, rt.trace_camera(a.scene, W * 3, H * 3).cpu().numpy(), materials, 3, sigma_plane=0.01)[0],
               "RayTracer.upsampled(scale=3, sigma_plane=0.01)")
    a.process()
    b.process()
    torch.cuda.synchronize()
    assert state(a) == state(b) and a.frame_index == 2
