"""rt_moments and rt_denoise_variance on the GPU (csrc/denoise_variance.hip) against tests/variance_ref.py, and the
chain of the four calls (VarianceAccumulator) against the chain of the restatements.  Every comparison but the quality
test's is bytewise, on the inputs as downloaded from the device: the arithmetic is specified, so no tolerance applies."""
import numpy as np
import pytest
import torch

import denoise_cases as DC
import denoise_ref as D
import reproject_cases as RC
import reproject_ref as R
import rt_testlib as T
import variance_cases as C
import variance_ref as V
from test_gpu_denoise import SENTINEL, image_of, same_image, to_surface

pytestmark = pytest.mark.gpu

W, H = 64, 36
F32 = np.float32
COUNT = 8  # frames of the dolly: tests/test_gpu_reproject.py's sanity configuration (RC.dolly, T.SEED, 5 spp / 6 bounces)
SIZES = [(1, 1), (5, 3), (16, 16), (37, 19), (130, 9)]


def same_plane(got, want, what):
    h, w = want.shape
    same_image(np.asarray(got, F32).reshape(h, w, 1), np.asarray(want, F32).reshape(h, w, 1), what)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("iterations", [1, 3, 6])
@pytest.mark.parametrize("given", [False, True], ids=["null", "moments+history"])
def test_synthetic_input(size, iterations, given):
    rt = T.load_rt()
    w, h = size
    case = C.synthetic(w, h, seed=w * 131 + h)
    # three surfaces, three pitches, all wider than width * 16, the padding a NaN sentinel
    surf = to_surface(rt, case["surface"], extra_floats=12, fill=SENTINEL)
    mom = to_surface(rt, case["moments"], extra_floats=4, fill=SENTINEL)
    out = torch.full((h, surf.shape[1] - 4), SENTINEL, dtype=torch.float32, device="cuda")
    assert len({surf.stride(0), mom.stride(0), out.stride(0)}) == 3 and min(surf.stride(0), mom.stride(0), out.stride(0)) > w * 4
    ov = torch.full((h * w + 5,), SENTINEL, dtype=torch.float32, device="cuda")
    hist = torch.from_numpy(case["history"]).cuda()
    hits, mats = torch.from_numpy(case["hits"]).cuda(), torch.from_numpy(case["materials"]).cuda()
    nbytes = rt.denoise_variance_scratch_bytes(w, h)
    scratch = torch.full((nbytes // 4 + 64,), float("nan"), dtype=torch.float32, device="cuda")
    pads = [t.cpu().numpy()[:, w * 4:].copy() for t in (surf, mom, out)]
    assert all(np.isnan(p).all() and p.size for p in pads)
    kw = {"moments": mom, "history": hist} if given else {}
    got, got_v = rt.denoise_variance_raw(surf, hits, mats, w, h, out=out, out_variance=ov, scratch=scratch,
                                         iterations=iterations, **kw)
    torch.cuda.synchronize()
    assert got is out and got_v is ov
    det = {}
    want, want_v = V.denoise_variance(case["surface"], case["hits"], case["materials"], iterations=iterations, details=det,
                                      **({"moments": case["moments"], "history": case["history"]} if given else {}))
    if given and w * h >= 15:
        assert det["temporal"].any() and det["spatial"].any()
    same_image(image_of(rt, out, w), want, f"synthetic {w}x{h}, {iterations} passes, given {given}")
    host_v = ov.cpu().numpy()
    same_plane(host_v[: w * h], want_v, f"synthetic {w}x{h}, {iterations} passes, given {given} (variance)")
    assert host_v[w * h:].tobytes() == np.full(5, SENTINEL, F32).tobytes()  # nothing written past width * height
    tail = scratch[nbytes // 4:].cpu().numpy()
    assert np.isnan(tail).all() and tail.size == 64                           # nor past the stated scratch size
    # padding of the output and of the inputs unchanged, inputs unchanged
    for t, pad in zip((surf, mom, out), pads):
        assert t.cpu().numpy()[:, w * 4:].tobytes() == pad.tobytes()
    same_image(image_of(rt, surf, w), case["surface"], "the input surface")
    same_image(image_of(rt, mom, w), case["moments"], "the moments")
    assert hits.cpu().numpy().tobytes() == case["hits"].tobytes() and hist.cpu().numpy().tobytes() == case["history"].tobytes()


def test_parameters_and_partial_inputs():
    """Explicit parameters, moments without history (history 1 everywhere: temporal only with min_history 1), history
    without moments (spatial everywhere), no materials, out_variance left to the call."""
    rt = T.load_rt()
    w, h = 37, 19
    case = C.synthetic(w, h, seed=3)
    surf, mom = to_surface(rt, case["surface"]), to_surface(rt, case["moments"])
    hits, mats = torch.from_numpy(case["hits"]).cuda(), torch.from_numpy(case["materials"]).cuda()
    hist = torch.from_numpy(case["history"]).cuda()
    for kw, dev, host, materials in [
            ({"sigma_lum": 0.5, "min_history": 2.0, "normal_power_log2": 0, "sigma_plane": 0.1, "iterations": 2},
             {"moments": mom, "history": hist}, {"moments": case["moments"], "history": case["history"]}, True),
            ({"min_history": 1.0}, {"moments": mom}, {"moments": case["moments"]}, True),
            ({}, {"moments": mom}, {"moments": case["moments"]}, True),
            ({}, {"history": hist}, {"history": case["history"]}, True),
            ({"iterations": 3}, {"moments": mom, "history": hist}, {"moments": case["moments"], "history": case["history"]}, False)]:
        m_dev = mats if materials else torch.zeros((0, 16), device="cuda")
        m_host = case["materials"] if materials else case["materials"][:0]
        out, var = rt.denoise_variance_raw(surf, hits, m_dev, w, h, **dev, **kw)
        torch.cuda.synchronize()
        want, want_v = V.denoise_variance(case["surface"], case["hits"], m_host, **host, **kw)
        same_image(image_of(rt, out, w), want, f"37x19 {kw} {sorted(dev)}")
        same_plane(var.cpu().numpy(), want_v, f"37x19 {kw} {sorted(dev)} (variance)")
        assert var.shape == (h, w)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_moments(size):
    """rt_moments against the restatement, and rt_reproject on its output against reproject_ref on the restated moments
    (the records, cameras and histories are reproject_cases'; their material indices run into a table of two, so one
    material of three is beyond it)."""
    rt = T.load_rt()
    w, h = size
    case = RC.synthetic(w, h, seed=w * 131 + h)
    table = DC.material_table([(0.73, 0.41, 0.2), (0.0, 1.5, 0.01)])
    mats = torch.from_numpy(table).cuda()
    surf = to_surface(rt, case["surface"], extra_floats=12, fill=SENTINEL)
    out = torch.full((h, surf.shape[1] - 4), SENTINEL, dtype=torch.float32, device="cuda")
    pad_before = out.cpu().numpy()[:, w * 4:].copy()
    hits, prev_hits = torch.from_numpy(case["hits"]).cuda(), torch.from_numpy(case["prev_hits"]).cuda()
    got = rt.moments(mats, surf, hits, w, h, out=out)
    torch.cuda.synchronize()
    assert got is out
    want = V.moments(case["surface"], case["hits"], table)
    same_image(image_of(rt, out, w), want, f"moments {w}x{h}")
    assert out.cpu().numpy()[:, w * 4:].tobytes() == pad_before.tobytes()
    same_image(image_of(rt, surf, w), case["surface"], "the input surface")
    if w >= 16 and h >= 16:
        assert (~np.isfinite(want[..., 0:2])).any() and np.isfinite(want[..., 0:2]).all(axis=-1).mean() > 0.9
    with pytest.raises(rt.RTError, match="out must not overlap surface"):
        rt.moments(mats, surf, hits, w, h, out=surf)
    # the moments of the previous frame as the previous accumulated moments: the second rt_reproject of the chain
    prev_want = V.moments(case["prev_surface"], case["prev_hits"], table)
    prev = rt.moments(mats, to_surface(rt, case["prev_surface"]), prev_hits, w, h)
    same_image(image_of(rt, prev, w), prev_want, f"moments of the previous frame {w}x{h}")
    prev_hist = torch.from_numpy(case["prev_history"]).cuda()
    acc, acc_h = rt.reproject_raw(out, hits, case["camera"], w, h, prev=(prev, prev_hits, prev_hist, case["prev_camera"]),
                                  max_history=case["max_history"])
    torch.cuda.synchronize()
    want_acc, want_h = R.reproject(want, case["hits"], case["camera"],
                                   (prev_want, case["prev_hits"], case["prev_history"], case["prev_camera"]),
                                   max_history=case["max_history"])
    same_image(image_of(rt, acc, w), want_acc, f"reprojected moments {w}x{h}")
    same_plane(acc_h.cpu().numpy(), want_h, f"reprojected moments {w}x{h} (history)")


def test_out_is_surface():
    rt = T.load_rt()
    w, h = 37, 19
    case = C.synthetic(w, h, seed=w * 131 + h)
    hits, mats = torch.from_numpy(case["hits"]).cuda(), torch.from_numpy(case["materials"]).cuda()
    mom, hist = to_surface(rt, case["moments"]), torch.from_numpy(case["history"]).cuda()
    for it in (1, 5):
        surf = to_surface(rt, case["surface"])
        apart, apart_v = rt.denoise_variance_raw(surf, hits, mats, w, h, moments=mom, history=hist, iterations=it)
        same, same_v = rt.denoise_variance_raw(surf, hits, mats, w, h, moments=mom, history=hist, iterations=it, out=surf)
        torch.cuda.synchronize()
        assert same is surf and apart.data_ptr() != surf.data_ptr()
        assert image_of(rt, same, w).tobytes() == image_of(rt, apart, w).tobytes()
        assert same_v.cpu().numpy().tobytes() == apart_v.cpu().numpy().tobytes()
        want, _ = V.denoise_variance(case["surface"], case["hits"], case["materials"], moments=case["moments"],
                                     history=case["history"], iterations=it)
        same_image(image_of(rt, same, w), want, f"out == surface, {it} passes")
    surf = to_surface(rt, case["surface"])
    with pytest.raises(rt.RTError, match="out must not overlap moments"):
        rt.denoise_variance_raw(surf, hits, mats, w, h, moments=mom, history=hist, out=mom)
    with pytest.raises(rt.RTError, match="scratch too small"):
        rt.denoise_variance_raw(surf, hits, mats, w, h,
                                scratch=torch.empty((rt.denoise_variance_scratch_bytes(w, h) // 4 - 1,), device="cuda"))


# --- the chain on rendered frames ----------------------------------------------------------------------------------
def host_frame(rt, scene, surf, hits):
    return {"image": image_of(rt, surf, W).copy(), "records": hits.cpu().numpy().copy(), "cam15": rt.camera_floats(scene.camera())}


@pytest.fixture(scope="module")
def chain():
    """COUNT frames of the bunny at 64x36 along the dolly, 5 spp each with frame_index 0, pushed through a
    VarianceAccumulator; every frame's inputs and results downloaded.  Then a 64-frame target at the last camera with
    another seed, and the last accumulated image through rt_denoise."""
    rt = T.load_rt()
    scene = rt.Scene()
    scene.setup("bunny")
    scene.set_viewport(W, H)
    rng = rt.alloc_rng(W * H)
    rt.init_rng_states(rng, W, H, T.SEED)
    acc = rt.VarianceAccumulator(W, H)
    assert acc.history is None and acc.accumulated is None and acc.variance is None
    surf, unused = rt.alloc_surface(W, H), rt.alloc_surface(W, H)
    frames = []
    for k in range(COUNT):
        scene.set_camera(*RC.dolly(k, COUNT - 1))
        scene.upload(rng.data_ptr())
        rt.render(scene, surf, unused, W, H, 5, 6)
        hits = rt.trace_camera(scene, W, H) if k % 2 else None  # records given and traced by push in turn
        out = acc.push(scene, surf, hits=hits)
        torch.cuda.synchronize()
        f = host_frame(rt, scene, surf, rt.trace_camera(scene, W, H))
        f.update(filtered=image_of(rt, out, W).copy(), accumulated=image_of(rt, acc.accumulated, W).copy(),
                 history=acc.history.cpu().numpy().copy(), variance=acc.variance.cpu().numpy().copy(),
                 moments=image_of(rt, acc.moments, W).copy())
        frames.append(f)
    denoised = image_of(rt, rt.denoise(scene, acc.accumulated, W, H), W).copy()
    target_rng = rt.alloc_rng(W * H)
    rt.init_rng_states(target_rng, W, H, 12345)
    scene.upload(target_rng.data_ptr())
    bufs = [rt.alloc_surface(W, H), rt.alloc_surface(W, H)]
    for i in range(64):
        rt.render(scene, bufs[i & 1], bufs[(i + 1) & 1], W, H, 5, 6, i)
    torch.cuda.synchronize()
    scene.upload(rng.data_ptr())
    return {"scene": scene, "rng": rng, "acc": acc, "frames": frames, "materials": scene.materials(), "denoised": denoised,
            "target": image_of(rt, bufs[63 & 1], W).copy()}


def test_chain_equals_the_restated_chain(chain):
    """At every frame: rt_reproject (colour), rt_moments, rt_reproject (moments, own history), rt_denoise_variance."""
    mats = chain["materials"]
    prev_c = prev_m = None
    spatial_share = []
    for k, f in enumerate(chain["frames"]):
        acc_c, hist_c = R.reproject(f["image"], f["records"], f["cam15"], prev_c)
        m = V.moments(f["image"], f["records"], mats)
        acc_m, hist_m = R.reproject(m, f["records"], f["cam15"], prev_m)
        det = {}
        want, want_v = V.denoise_variance(acc_c, f["records"], mats, moments=acc_m, history=hist_c, details=det)
        same_image(f["accumulated"], acc_c, f"frame {k}: accumulated")
        same_plane(f["history"], hist_c, f"frame {k}: history")
        same_image(f["moments"], acc_m, f"frame {k}: accumulated moments")
        same_image(f["filtered"], want, f"frame {k}: filtered")
        same_plane(f["variance"], want_v, f"frame {k}: variance")
        spatial_share.append(float(det["spatial"].sum()) / max(1, int((det["spatial"] | det["temporal"]).sum())))
        prev_c = (acc_c, f["records"], hist_c, f["cam15"])
        prev_m = (acc_m, f["records"], hist_m, f["cam15"])
    print("share of filtered pixels on the spatial estimate, per frame: " + " ".join(f"{s:.3f}" for s in spatial_share))
    # both estimates were at work along the way: every pixel spatial on the first frames, most temporal on the last
    assert spatial_share[0] == 1.0 and spatial_share[-1] < 0.5
    last = chain["frames"][-1]
    assert (last["filtered"] != last["accumulated"]).any(axis=-1).mean() > 0.5 and (last["variance"] > 0).mean() > 0.5


def test_accumulator_reset_and_side_stream(chain):
    """A side stream that is not torch's current one, no outputs passed in: they are made (and zero-filled) on that
    stream.  After reset() the first push is the first frame's again."""
    rt = T.load_rt()
    scene, f0 = chain["scene"], chain["frames"][0]
    mats = torch.from_numpy(chain["materials"]).cuda()
    surf, hits = to_surface(rt, f0["image"]), torch.from_numpy(f0["records"]).cuda()
    scene.set_camera(*RC.dolly(0, COUNT - 1))
    scene.upload(chain["rng"].data_ptr())
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    assert torch.cuda.current_stream() != s
    res = [rt.denoise_variance_raw(surf, hits, mats, W, H, stream=s) for _ in range(3)]
    res.append(rt.denoise_variance(scene, surf, W, H, stream=s))  # traces its own records on the stream, too
    mom = rt.moments(scene, surf, hits, W, H, stream=s)
    acc = rt.VarianceAccumulator(W, H, reproject_params={"max_history": 16}, sigma_lum=2.0)
    pushed = acc.push(scene, surf, stream=s)
    assert torch.cuda.current_stream() != s
    s.synchronize()
    want, want_v = V.denoise_variance(f0["image"], f0["records"], chain["materials"])
    for i, (out, var) in enumerate(res):
        same_image(image_of(rt, out, W), want, f"side stream, call {i}")
        same_plane(var.cpu().numpy(), want_v, f"side stream, call {i} (variance)")
    m = V.moments(f0["image"], f0["records"], chain["materials"])
    same_image(image_of(rt, mom, W), m, "side stream, moments")
    # the first push: NULL-prev reprojections (history 1 or 0), then the filter with sigma_lum 2
    acc_c, hist_c = R.reproject(f0["image"], f0["records"], f0["cam15"], None)
    acc_m, _ = R.reproject(m, f0["records"], f0["cam15"], None)
    first, first_v = V.denoise_variance(acc_c, f0["records"], chain["materials"], moments=acc_m, history=hist_c, sigma_lum=2.0)
    same_image(image_of(rt, pushed, W), first, "side stream, push")
    same_plane(acc.variance.cpu().numpy(), first_v, "side stream, push (variance)")
    assert acc.reproject_params == {"max_history": 16}
    acc.push(scene, surf)
    acc.reset()
    assert acc.history is None and acc.accumulated is None and acc.variance is None
    again = acc.push(scene, surf, hits=hits)
    torch.cuda.synchronize()
    same_image(image_of(rt, again, W), first, "after reset")


def test_raytracer_filtered(chain):
    rt = T.load_rt()
    tr = rt.RayTracer(W, H, "bunny", seed=T.SEED)
    tr.scene.set_camera(*RC.dolly(0, COUNT - 1))
    tr.process()
    torch.cuda.synchronize()
    state = lambda: (tr.frame_index, tr.surface.cpu().numpy().tobytes(), tr.last_frame.cpu().numpy().tobytes(),
                     tr.rng.cpu().numpy().tobytes())
    assert tr.variance_accumulator is None
    before = state()
    out = tr.filtered()
    torch.cuda.synchronize()
    assert state() == before and before[0] == 1
    assert out.data_ptr() not in (tr.surface.data_ptr(), tr.last_frame.data_ptr())
    # the tracer's first frame is the chain's (same seed, camera, spp and bounces), and so is its filtered image
    same_image(image_of(rt, tr.surface, W), chain["frames"][0]["image"], "RayTracer frame 0")
    same_image(image_of(rt, out, W), chain["frames"][0]["filtered"], "first filtered()")
    tr.scene.set_camera(*RC.dolly(1, COUNT - 1))
    tr.frame_index = 0
    tr.process()
    torch.cuda.synchronize()
    before = state()
    out1 = tr.filtered()
    torch.cuda.synchronize()
    assert state() == before and before[0] == 1
    same_image(image_of(rt, out1, W), chain["frames"][1]["filtered"], "second filtered()")
    same_plane(tr.variance_accumulator.variance.cpu().numpy(), chain["frames"][1]["variance"], "second filtered() (variance)")
    assert tr._accumulator is None  # reprojected()'s accumulator is another one and was not touched
    tr.on_resize(W, H)
    assert tr.variance_accumulator is None


def test_filtered_beats_the_accumulated_image(chain):
    """8 frames along the dolly, 5 spp each, accumulated and filtered by VarianceAccumulator.push, against a converged
    render at the last camera with another seed (display error over hit pixels): the filtered image is closer to it
    than the accumulated image is.  That inequality is the only bound.  How the filtered image compares with the
    accumulated image through rt_denoise (defaults) is printed here and recorded, with the figures at a user's frame
    size, in profiles/variance_quality.txt; it is not asserted.

    Measured (profiles/variance_quality.txt, last lines): accumulated 0.1489, then rt_denoise 0.1212, then
    rt_denoise_variance 0.1087 = 0.730 of the accumulated image's and 0.897 of rt_denoise's; with two other seeds of
    the frames 0.761 / 0.877 and 0.748 / 0.883.

    The mask drops only hit pixels whose last-frame, accumulated or target colour is not finite and must keep 99 % of
    the hit pixels.  For the existing pipeline alone (render, rt_reproject, the target) at this size and seed the mask
    drops 0 of the 1483 hit pixels, and as many with the filter's chain."""
    f = chain["frames"][-1]
    single, accumulated, filtered, target = f["image"], f["accumulated"], f["filtered"], chain["target"]
    hit = (f["records"].view(np.uint32)[:, 1] != 0).reshape(H, W)
    finite = lambda im: np.isfinite(im[..., 0:3]).all(axis=-1)
    mask = hit & finite(single) & finite(accumulated) & finite(target)
    print(f"{int(hit.sum())} hit pixels, {int(hit.sum() - mask.sum())} dropped because the last frame, the accumulated image or the "
          "target is not finite there")
    assert mask.sum() >= 0.99 * hit.sum() and hit.sum() > W * H // 2
    assert finite(filtered)[mask].all()
    e_single, e_acc = D.display_error(single, target, mask), D.display_error(accumulated, target, mask)
    e_den, e_fil = D.display_error(chain["denoised"], target, mask), D.display_error(filtered, target, mask)
    print(f"display error over {int(mask.sum())} hit pixels: last frame {e_single:.4f}, accumulated {e_acc:.4f}, accumulated + rt_denoise "
          f"{e_den:.4f}, accumulated + rt_denoise_variance {e_fil:.4f} (ratio to accumulated {e_fil / e_acc:.3f}, to accumulated + "
          f"rt_denoise {e_fil / e_den:.3f}); mean history {f['history'][hit].mean():.2f}")
    assert e_fil < e_acc
