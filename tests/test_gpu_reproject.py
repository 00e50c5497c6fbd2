"""rt_reproject on the GPU (csrc/reproject.hip) against tests/reproject_ref.py.  Every comparison is bytewise, on
the inputs as downloaded from the device: the arithmetic is specified, so no tolerance applies."""
import numpy as np
import pytest
import torch

import denoise_ref as D
import query_ref as Q
import reproject_cases as C
import reproject_ref as R
import rt_testlib as T
from test_gpu_denoise import SENTINEL, image_of, same_image, to_surface

pytestmark = pytest.mark.gpu

W, H = 64, 36
F32 = np.float32
# the set-up camera, then a small translation plus about 2 degrees of rotation, then as much again
POSES = [((0.0, 0.0, 0.0), 0.0, 180.0), ((0.4, 0.2, 0.3), 1.0, 182.0), ((0.8, 0.3, 0.7), 1.5, 184.0)]


def same_history(got, want, what):
    same_image(np.asarray(got, F32).reshape(H, W, 1), np.asarray(want, F32).reshape(H, W, 1), what + " (history)")


def frame_at(rt, scene, rng, pose):
    """One 5-spp frame (frame_index 0) of `scene` at `pose` with its camera and records, on the device and downloaded."""
    scene.set_camera(*pose)
    scene.upload(rng.data_ptr())
    surf = rt.alloc_surface(W, H)
    rt.render(scene, surf, rt.alloc_surface(W, H), W, H, 5, 6)
    hits = rt.trace_camera(scene, W, H)
    cam = scene.camera()
    torch.cuda.synchronize()
    return {"surface": surf, "hits": hits, "camera": cam, "image": image_of(rt, surf, W).copy(),
            "records": hits.cpu().numpy().copy(), "cam15": rt.camera_floats(cam)}


@pytest.fixture(scope="module")
def frames():
    """Three 5-spp frames of the bunny scene at 64x36 along POSES, a previous history of mixed values, and the
    reference's result for frame 1 reprojected onto frame 0."""
    rt = T.load_rt()
    scene = rt.Scene()
    scene.setup("bunny")
    scene.set_viewport(W, H)
    rng = rt.alloc_rng(W * H)
    rt.init_rng_states(rng, W, H, T.SEED)
    f = [frame_at(rt, scene, rng, pose) for pose in POSES]
    g = np.random.default_rng(11)
    hist = np.floor(g.uniform(0, 9, size=(H, W))).astype(F32)  # 0 (never taken) to 8
    hist[g.random((H, W)) < 0.1] += F32(0.25)
    want = R.reproject(f[1]["image"], f[1]["records"], f[1]["cam15"], (f[0]["image"], f[0]["records"], hist, f[0]["cam15"]))
    return {"scene": scene, "rng": rng, "frames": f, "history": hist, "history_dev": torch.from_numpy(hist).cuda(), "want": want}


def test_bunny_two_cameras(frames):
    rt = T.load_rt()
    f0, f1 = frames["frames"][0:2]
    want, want_h = frames["want"]
    # the test is about something: most hit pixels take history, some reset, some sky takes history
    hit = (f1["records"].view(np.uint32)[:, 1] != 0).reshape(H, W)
    assert hit.sum() > W * H // 2 and (~hit).sum() > 0
    assert (want_h[hit] > 1).sum() > hit.sum() // 2 and (want_h[hit] <= 1).sum() > 0 and (want_h[~hit] > 1).sum() > 0
    assert (f0["cam15"] != f1["cam15"]).any()
    before = [t.clone() for t in (f1["surface"], f1["hits"], f0["surface"], f0["hits"], frames["history_dev"])]
    out, oh = rt.reproject_raw(f1["surface"], f1["hits"], f1["camera"], W, H,
                               prev=(f0["surface"], f0["hits"], frames["history_dev"], f0["camera"]))
    torch.cuda.synchronize()
    same_image(image_of(rt, out, W), want, "bunny 64x36, two cameras")
    same_history(oh.cpu().numpy(), want_h, "bunny 64x36, two cameras")
    assert oh.shape == (H, W) and out.data_ptr() != f1["surface"].data_ptr()
    for a, b in zip(before, (f1["surface"], f1["hits"], f0["surface"], f0["hits"], frames["history_dev"])):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    # the 15 floats work as well as the ctypes struct, and explicit parameters as well as the defaults
    kw = {"max_history": 3, "sigma_plane": 0.004, "normal_min": 0.99}
    out2, oh2 = rt.reproject_raw(f1["surface"], f1["hits"], f1["cam15"], W, H,
                                 prev=(f0["surface"], f0["hits"], frames["history_dev"], f0["cam15"]), **kw)
    want2, want2_h = R.reproject(f1["image"], f1["records"], f1["cam15"], (f0["image"], f0["records"], frames["history"], f0["cam15"]), **kw)
    same_image(image_of(rt, out2, W), want2, f"bunny 64x36, {kw}")
    same_history(oh2.cpu().numpy(), want2_h, f"bunny 64x36, {kw}")
    assert (want2_h != want_h).any()


def test_moved_camera_records_are_the_cpu_traversal_s(frames):
    """The records the comparison rests on, for the moved camera too: tests/query_ref.py on the CPU."""
    arrays = Q.Arrays(T.OracleScene("bunny").arrays())
    for f in frames["frames"][0:2]:
        want, _, _ = Q.trace(arrays, Q.camera_rays(f["cam15"], W, H))
        assert f["records"].tobytes() == want.tobytes()


@pytest.mark.parametrize("size", [(1, 1), (5, 3), (16, 16), (37, 19), (130, 9)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_synthetic_input(size):
    rt = T.load_rt()
    w, h = size
    case = C.synthetic(w, h, seed=w * 131 + h)
    # three surfaces, three pitches, all wider than width * 16, the padding a NaN sentinel
    surf = to_surface(rt, case["surface"], extra_floats=12, fill=SENTINEL)
    prev = to_surface(rt, case["prev_surface"], extra_floats=4, fill=SENTINEL)
    out = torch.full((h, surf.shape[1] - 4), SENTINEL, dtype=torch.float32, device="cuda")
    assert len({surf.stride(0), prev.stride(0), out.stride(0)}) == 3 and min(surf.stride(0), prev.stride(0), out.stride(0)) > w * 4
    oh = torch.full((h * w + 5,), SENTINEL, dtype=torch.float32, device="cuda")
    hits, prev_hits = torch.from_numpy(case["hits"]).cuda(), torch.from_numpy(case["prev_hits"]).cuda()
    prev_hist = torch.from_numpy(case["prev_history"]).cuda()
    pads = [t.cpu().numpy()[:, w * 4:].copy() for t in (surf, prev, out)]
    assert all(np.isnan(p).all() and p.size for p in pads)
    got, got_h = rt.reproject_raw(surf, hits, case["camera"], w, h, prev=(prev, prev_hits, prev_hist, case["prev_camera"]),
                                  out=out, out_history=oh, max_history=case["max_history"])
    torch.cuda.synchronize()
    assert got is out and got_h is oh
    want, want_h = R.reproject(case["surface"], case["hits"], case["camera"],
                               (case["prev_surface"], case["prev_hits"], case["prev_history"], case["prev_camera"]),
                               max_history=case["max_history"])
    if w >= 16 and h >= 16:
        kind = case["hits"].view(np.uint32)[:, 1].reshape(h, w)
        assert (want_h > 1).any() and (want_h == 1).any() and (want_h == 0).any() and ((kind == 0) & (want_h > 1)).any()
    same_image(image_of(rt, out, w), want, f"synthetic {w}x{h}")
    host_h = oh.cpu().numpy()
    same_image(host_h[: w * h].reshape(h, w, 1), want_h.reshape(h, w, 1), f"synthetic {w}x{h} (history)")
    assert host_h[w * h:].tobytes() == np.full(5, SENTINEL, F32).tobytes()  # nothing written past width * height
    # padding of the output and of the inputs unchanged, inputs unchanged
    for t, pad in zip((surf, prev, out), pads):
        assert t.cpu().numpy()[:, w * 4:].tobytes() == pad.tobytes()
    same_image(image_of(rt, surf, w), case["surface"], "the input surface")
    same_image(image_of(rt, prev, w), case["prev_surface"], "the previous surface")
    assert hits.cpu().numpy().tobytes() == case["hits"].tobytes() and prev_hits.cpu().numpy().tobytes() == case["prev_hits"].tobytes()
    assert prev_hist.cpu().numpy().tobytes() == case["prev_history"].tobytes()


def test_null_prev(frames):
    rt = T.load_rt()
    f1 = frames["frames"][1]
    image = f1["image"].copy()
    image[3, 5, 0:3] = (np.nan, 1.0, 2.0)
    image[7, 9, 1] = np.inf
    out, oh = rt.reproject_raw(to_surface(rt, image), f1["hits"], f1["camera"], W, H)
    torch.cuda.synchronize()
    want, want_h = R.reproject(image, f1["records"], f1["cam15"], None)
    assert want.tobytes() == image.tobytes() and (want_h == 0).sum() >= 2
    same_image(image_of(rt, out, W), want, "NULL prev")
    same_history(oh.cpu().numpy(), want_h, "NULL prev")


def test_out_is_surface(frames):
    rt = T.load_rt()
    f0, f1 = frames["frames"][0:2]
    surf = f1["surface"].clone()
    out, oh = rt.reproject_raw(surf, f1["hits"], f1["camera"], W, H, out=surf,
                               prev=(f0["surface"], f0["hits"], frames["history_dev"], f0["camera"]))
    torch.cuda.synchronize()
    assert out is surf
    same_image(image_of(rt, surf, W), frames["want"][0], "out is surface")
    same_history(oh.cpu().numpy(), frames["want"][1], "out is surface")
    with pytest.raises(rt.RTError, match="out must not overlap prev_surface"):
        rt.reproject_raw(f1["surface"], f1["hits"], f1["camera"], W, H, out=surf, prev=(surf, f0["hits"], frames["history_dev"], f0["camera"]))
    with pytest.raises(rt.RTError, match="out_history must not overlap prev_history"):
        rt.reproject_raw(f1["surface"], f1["hits"], f1["camera"], W, H, out_history=frames["history_dev"],
                         prev=(f0["surface"], f0["hits"], frames["history_dev"], f0["camera"]))


def test_hits_is_prev_hits_with_identical_cameras(frames):
    """A camera that stands still: the same records and camera on both sides, the frame accumulated in place."""
    rt = T.load_rt()
    f0, f1 = frames["frames"][0:2]
    out, oh = rt.reproject_raw(f1["surface"], f0["hits"], f0["camera"], W, H,
                               prev=(f0["surface"], f0["hits"], frames["history_dev"], f0["camera"]))
    torch.cuda.synchronize()
    want, want_h = R.reproject(f1["image"], f0["records"], f0["cam15"], (f0["image"], f0["records"], frames["history"], f0["cam15"]))
    same_image(image_of(rt, out, W), want, "hits is prev_hits")
    same_history(oh.cpu().numpy(), want_h, "hits is prev_hits")
    taken = frames["history"] >= 1
    assert (want_h[taken] > 1).mean() > 0.95


def test_side_stream_allocates_its_own_outputs(frames):
    """A side stream that is not torch's current one, no outputs passed in: they are made (and zero-filled) on that
    stream, so the fill cannot land behind the kernel's writes."""
    rt = T.load_rt()
    f0, f1 = frames["frames"][0:2]
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    assert torch.cuda.current_stream() != s
    res = [rt.reproject_raw(f1["surface"], f1["hits"], f1["camera"], W, H, stream=s,
                            prev=(f0["surface"], f0["hits"], frames["history_dev"], f0["camera"])) for _ in range(3)]
    acc = rt.TemporalAccumulator(W, H)
    scene = frames["scene"]
    scene.set_camera(*POSES[1])
    scene.upload(frames["rng"].data_ptr())
    torch.cuda.synchronize()
    pushed = acc.push(scene, f1["surface"], stream=s)  # traces its own records on the stream, too
    assert torch.cuda.current_stream() != s
    s.synchronize()
    for i, (out, oh) in enumerate(res):
        same_image(image_of(rt, out, W), frames["want"][0], f"side stream, call {i}")
        same_history(oh.cpu().numpy(), frames["want"][1], f"side stream, call {i}")
    first, first_h = R.reproject(f1["image"], f1["records"], f1["cam15"], None)
    same_image(image_of(rt, pushed, W), first, "side stream, push")
    same_history(acc.history.cpu().numpy(), first_h, "side stream, push")


def test_accumulator_chain(frames):
    rt = T.load_rt()
    scene, f = frames["scene"], frames["frames"]
    acc = rt.TemporalAccumulator(W, H, max_history=2)
    assert acc.history is None

    def run(order, give_hits):
        prev, outs = None, []
        for k in order:
            scene.set_camera(*POSES[k])
            scene.upload(frames["rng"].data_ptr())
            out = acc.push(scene, f[k]["surface"], hits=f[k]["hits"] if give_hits else None)
            torch.cuda.synchronize()
            want, want_h = R.reproject(f[k]["image"], f[k]["records"], f[k]["cam15"], prev, max_history=2)
            same_image(image_of(rt, out, W), want, f"chain {order}, camera {k}")
            same_history(acc.history.cpu().numpy(), want_h, f"chain {order}, camera {k}")
            assert acc.history.shape == (H, W)
            prev = (want, f[k]["records"], want_h, f[k]["cam15"])
            outs.append(out)
        return outs, prev[2]

    outs, last_h = run([0, 1, 2], give_hits=False)
    assert (last_h == 2).mean() > 0.5 and (last_h == 1).any()  # capped by max_history; some pixels reset on the way
    assert outs[0].data_ptr() == outs[2].data_ptr() != outs[1].data_ptr()  # valid until the next-but-one push
    acc.reset()
    assert acc.history is None
    run([2, 1], give_hits=True)  # a new chain: its first frame comes back as it went in


def test_raytracer_reprojected(frames):
    rt = T.load_rt()
    tr = rt.RayTracer(W, H, "bunny", seed=T.SEED)
    tr.process()
    torch.cuda.synchronize()
    state = lambda: (tr.frame_index, tr.surface.cpu().numpy().tobytes(), tr.last_frame.cpu().numpy().tobytes(),
                     tr.rng.cpu().numpy().tobytes())
    before = state()
    out = tr.reprojected()
    torch.cuda.synchronize()
    assert state() == before and before[0] == 1
    assert out.data_ptr() not in (tr.surface.data_ptr(), tr.last_frame.data_ptr())
    image0 = image_of(rt, tr.surface, W).copy()
    records0 = rt.trace_camera(tr.scene, W, H).cpu().numpy()
    cam0 = rt.camera_floats(tr.scene.camera())
    same_image(image0, frames["frames"][0]["image"], "RayTracer frame 0")  # same seed, spp and bounces as the fixture
    want0, want0_h = R.reproject(image0, records0, cam0, None)
    same_image(image_of(rt, out, W), want0, "first reprojected() = NULL-prev mode")
    same_history(tr._accumulator.history.cpu().numpy(), want0_h, "first reprojected()")
    # move the camera; like the reference's Process() on its dirty flag, start the progressive frame over
    tr.scene.set_camera(*POSES[1])
    tr.frame_index = 0
    tr.process()
    torch.cuda.synchronize()
    before = state()
    out1 = tr.reprojected(max_history=16)
    torch.cuda.synchronize()
    assert state() == before and before[0] == 1 and out1.data_ptr() != out.data_ptr()
    image1 = image_of(rt, tr.surface, W).copy()
    records1 = rt.trace_camera(tr.scene, W, H).cpu().numpy()
    cam1 = rt.camera_floats(tr.scene.camera())
    assert (cam1 != cam0).any() and records1.tobytes() == frames["frames"][1]["records"].tobytes()
    want1, want1_h = R.reproject(image1, records1, cam1, (want0, records0, want0_h, cam0), max_history=16)
    same_image(image_of(rt, out1, W), want1, "second reprojected()")
    same_history(tr._accumulator.history.cpu().numpy(), want1_h, "second reprojected()")
    assert (want1_h == 2).mean() > 0.5
    tr.on_resize(W, H)
    assert tr._accumulator is None


def test_accumulation_beats_the_single_frame(frames):
    """The whole point: 8 frames along a small dolly, 5 spp each, accumulated by push, are closer to a converged
    render at the last camera than the last frame alone (display error over hit pixels; the ratio is printed, and
    recorded at a user's frame size in profiles/reproject_quality.txt)."""
    rt = T.load_rt()
    scene, rng = frames["scene"], frames["rng"]
    count = 8
    acc = rt.TemporalAccumulator(W, H)
    surf, scratch = rt.alloc_surface(W, H), rt.alloc_surface(W, H)
    for k in range(count):
        scene.set_camera(*C.dolly(k, count - 1))
        scene.upload(rng.data_ptr())
        rt.render(scene, surf, scratch, W, H, 5, 6)
        out = acc.push(scene, surf)
    hits = rt.trace_camera(scene, W, H)
    torch.cuda.synchronize()
    single, accumulated = image_of(rt, surf, W).copy(), image_of(rt, out, W).copy()
    hist = acc.history.cpu().numpy()
    target_rng = rt.alloc_rng(W * H)
    rt.init_rng_states(target_rng, W, H, 12345)
    scene.upload(target_rng.data_ptr())
    bufs = [rt.alloc_surface(W, H), rt.alloc_surface(W, H)]
    for i in range(64):
        rt.render(scene, bufs[i & 1], bufs[(i + 1) & 1], W, H, 5, 6, i)
    torch.cuda.synchronize()
    scene.upload(rng.data_ptr())
    target = image_of(rt, bufs[63 & 1], W)
    hit = (hits.cpu().numpy().view(np.uint32)[:, 1] != 0).reshape(H, W)
    finite = lambda im: np.isfinite(im[..., 0:3]).all(axis=-1)
    mask = hit & finite(single) & finite(accumulated) & finite(target)  # a non-finite pixel has no error to measure
    assert mask.sum() > W * H // 2
    before, after = D.display_error(single, target, mask), D.display_error(accumulated, target, mask)
    print(f"display error over {int(mask.sum())} hit pixels: last frame {before:.4f}, {count} frames accumulated {after:.4f}, "
          f"ratio {after / before:.3f}; mean history over hit pixels {hist[hit].mean():.2f}")
    assert after < before
