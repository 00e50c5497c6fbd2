"""Render progressive frames of a benchmark config on cuda:0 and save the last one:
.pfm (linear) and .ppm (the reference viewer's tonemap).

    python tools/render_image.py [--config cfg2] [--frames 4] [--out gpurun_out/cfg2]
    python tools/render_image.py --aov PREFIX
    python tools/render_image.py --denoise
    python tools/render_image.py --ao RADIUS
    python tools/render_image.py --temporal K [--variance]
    python tools/render_image.py --panorama W
    python tools/render_image.py --adaptive ROUNDS
    python tools/render_image.py --upsample S [--denoise]
    python tools/render_image.py --hits K

--aov PREFIX also writes the first-hit images of the same camera (rt.gbuffer: pixel centres, no jitter) as
PREFIX_normal.pfm (normal * 0.5 + 0.5), PREFIX_depth.pfm (hit distance, inf on a miss) and PREFIX_albedo.pfm.
--denoise also writes OUT_denoised.pfm / .ppm next to the beauty frame: rt.denoise of the last frame, guided by the
same camera's first-hit records, into a surface of its own (the progressive history is not touched).
--ao RADIUS also writes OUT_ao.pfm (linear) / .ppm (8-bit, linear grey): rt.ambient_occlusion of the same camera's
first-hit records, 8 samples per pixel of length RADIUS (1 = open, 0 = closed, 1 where the camera ray missed).
--temporal K also writes OUT_temporal.pfm / .ppm: K frames of the config's spp, each rendered with frame_index 0 along a
small camera dolly that ends at the config's camera, accumulated by rt.TemporalAccumulator (rt_reproject).  With
--variance the frames go through rt.VarianceAccumulator instead (the same accumulation, then rt_denoise_variance), which
adds OUT_filtered.pfm / .ppm and OUT_variance.pfm (linear grey: the filtered variance of the albedo-divided luminance).
--panorama W also writes OUT_panorama.pfm / .ppm: the W x W/2 equirectangular panorama of the scene from the camera's
position at the config's spp and bounces (rt.panorama: rt_radiance along rt.panorama_rays).
--adaptive ROUNDS also writes OUT_adaptive.pfm / .ppm and OUT_samples.pfm: rt.AdaptiveSampler at the config's camera --
a warm-up of 2 samples a pixel, then ROUNDS rounds that each spend at most the config's spp per pixel where the relative
variance of the mean is largest -- and its samples per pixel as a linear grey image.
--upsample S (2, 3 or 4) renders everything above at 1/S of the config's size in each direction (a size that S does not
divide is refused) and also writes OUT_upsampled.pfm / .ppm at the config's size: rt.upsample of the last frame, guided
by the camera's first-hit records at both sizes.  With --denoise the low frame goes through rt.denoise first.
--hits K (1..16) also writes OUT_hitcount.pfm: per pixel, the number of surfaces the camera ray crosses (rt.trace_hits_camera
with RT_HITS_COUNT_ALL | RT_HITS_CULL_BACK, so that a loaded mesh's twin faces count once; K is the list kept beside the
count) as a linear grey image -- an x-ray of the scene.
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as G  # noqa: E402
import bench  # noqa: E402


def ao_outputs(ao):
    """An AO image [H, W] in record order (row 0 = the bottom of the frame, as the surface) as what the two writers
    take: (float32 [H, W * 4] grey RGBA, bottom to top, for write_pfm; uint8 [H, W, 3] linear grey, TOP to bottom,
    for write_ppm -- the beauty frame's rows are flipped by tonemap, these here)."""
    h, w = ao.shape
    grey = ao[:, :, None].expand(h, w, 3)
    rgba = torch.cat([grey, torch.ones((h, w, 1), dtype=torch.float32, device=ao.device)], dim=2)
    return rgba.reshape(h, w * 4), (grey.flip(0) * 255.0 + 0.5).to(torch.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg2")
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "gpurun_out", "frame"))
    ap.add_argument("--aov", default=None, metavar="PREFIX")
    ap.add_argument("--denoise", action="store_true")
    ap.add_argument("--ao", type=float, default=None, metavar="RADIUS")
    ap.add_argument("--temporal", type=int, default=None, metavar="K")
    ap.add_argument("--variance", action="store_true", help="with --temporal: also filter (rt_denoise_variance)")
    ap.add_argument("--panorama", type=int, default=None, metavar="W")
    ap.add_argument("--adaptive", type=int, default=None, metavar="ROUNDS")
    ap.add_argument("--upsample", type=int, default=None, metavar="S", choices=(2, 3, 4))
    ap.add_argument("--hits", type=int, default=None, metavar="K", choices=range(1, 17))
    args = ap.parse_args()
    assert not args.variance or args.temporal is not None, "--variance needs --temporal K"
    rt = G.load_package()
    scene_name, W, H, SPP, BOUNCES, _ = bench.CONFIGS[args.config]
    if args.upsample is not None:
        if W % args.upsample or H % args.upsample:
            sys.exit(f"--upsample {args.upsample} does not divide {W}x{H}")
        W, H = W // args.upsample, H // args.upsample
    torch.cuda.set_device(0)
    scene = rt.Scene()
    scene.setup(scene_name)
    scene.set_viewport(W, H)
    rng = rt.alloc_rng(W * H)
    rt.init_rng_states(rng, W, H, bench.SEED)
    scene.upload(rng.data_ptr())
    bufs = [rt.alloc_surface(W, H), rt.alloc_surface(W, H)]
    for i in range(args.frames):
        rt.render(scene, bufs[i & 1], bufs[(i + 1) & 1], W, H, SPP, BOUNCES, i)
    final = bufs[(args.frames - 1) & 1]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    rt.write_pfm(args.out + ".pfm", final, W, H)
    rt.write_ppm(args.out + ".ppm", rt.tonemap(final, W, H))
    print(f"wrote {args.out}.pfm / .ppm ({W}x{H}, {args.frames} frames x {SPP} spp)")
    clean = None
    if args.denoise:
        clean = rt.denoise(scene, final, W, H)
        rt.write_pfm(args.out + "_denoised.pfm", clean, W, H)
        rt.write_ppm(args.out + "_denoised.ppm", rt.tonemap(clean, W, H))
        print(f"wrote {args.out}_denoised.pfm / .ppm")
    if args.upsample is not None:
        big = rt.upsample(scene, clean if clean is not None else final, W, H, args.upsample)
        bw, bh = W * args.upsample, H * args.upsample
        rt.write_pfm(args.out + "_upsampled.pfm", big, bw, bh)
        rt.write_ppm(args.out + "_upsampled.ppm", rt.tonemap(big, bw, bh))
        print(f"wrote {args.out}_upsampled.pfm / .ppm ({bw}x{bh} from {W}x{H}" + (", denoised first)" if clean is not None else ")"))
    if args.ao is not None:
        ao = rt.ambient_occlusion(scene, rt.trace_camera(scene, W, H), W, H, args.ao)
        pfm, ppm = ao_outputs(ao)
        rt.write_pfm(args.out + "_ao.pfm", pfm, W, H)
        rt.write_ppm(args.out + "_ao.ppm", ppm)
        print(f"wrote {args.out}_ao.pfm / .ppm (radius {args.ao:g}, 8 samples)")
    if args.temporal is not None:
        assert args.temporal >= 1
        acc = rt.VarianceAccumulator(W, H) if args.variance else rt.TemporalAccumulator(W, H)
        frame, unused = rt.alloc_surface(W, H), rt.alloc_surface(W, H)
        for k in range(args.temporal):
            b = args.temporal - 1 - k  # steps before the config's camera (position 0, angles 0 / 180)
            scene.set_camera((-0.05 * b, -0.02 * b, -0.04 * b), 0.1 * b, 180.0 - 0.25 * b)
            scene.upload(rng.data_ptr())
            rt.render(scene, frame, unused, W, H, SPP, BOUNCES, 0)
            moving = acc.push(scene, frame)
        if args.variance:
            filtered, moving = moving, acc.accumulated
            rt.write_pfm(args.out + "_filtered.pfm", filtered, W, H)
            rt.write_ppm(args.out + "_filtered.ppm", rt.tonemap(filtered, W, H))
            rt.write_pfm(args.out + "_variance.pfm", ao_outputs(acc.variance)[0], W, H)
            print(f"wrote {args.out}_filtered.pfm / .ppm and {args.out}_variance.pfm (mean variance {float(acc.variance.mean()):.3g})")
        rt.write_pfm(args.out + "_temporal.pfm", moving, W, H)
        rt.write_ppm(args.out + "_temporal.ppm", rt.tonemap(moving, W, H))
        print(f"wrote {args.out}_temporal.pfm / .ppm ({args.temporal} frames x {SPP} spp along a dolly; "
              f"mean history {float(acc.history.mean()):.1f} frames)")
    if args.panorama is not None:
        pw, ph = args.panorama, args.panorama // 2
        assert pw >= 2
        pano = rt.panorama(scene, pw, ph, samples=SPP, bounces=BOUNCES, seed=bench.SEED)
        rt.write_pfm(args.out + "_panorama.pfm", pano, pw, ph)
        rt.write_ppm(args.out + "_panorama.ppm", rt.tonemap(pano, pw, ph))
        print(f"wrote {args.out}_panorama.pfm / .ppm ({pw}x{ph} equirectangular from the camera's position, {SPP} spp)")
    if args.adaptive is not None:
        assert args.adaptive >= 0
        sampler = rt.AdaptiveSampler(scene, W, H, bounces=BOUNCES, seed=bench.SEED)
        sampler.warmup(2)
        for _ in range(args.adaptive):
            sampler.step(SPP)
        image, counts = sampler.image(), sampler.counts()
        rt.write_pfm(args.out + "_adaptive.pfm", image, W, H)
        rt.write_ppm(args.out + "_adaptive.ppm", rt.tonemap(image, W, H))
        rt.write_pfm(args.out + "_samples.pfm", ao_outputs(counts.contiguous())[0], W, H)
        print(f"wrote {args.out}_adaptive.pfm / .ppm and {args.out}_samples.pfm ({args.adaptive} rounds of at most {SPP} spp after 2: "
              f"{float(counts.mean()):.2f} samples a pixel, {int(counts.min())} to {int(counts.max())})")
    if args.hits is not None:
        _, crossings = rt.trace_hits_camera(scene, W, H, args.hits, flags=rt.RT_HITS_COUNT_ALL | rt.RT_HITS_CULL_BACK)
        rt.write_pfm(args.out + "_hitcount.pfm", ao_outputs(crossings.reshape(H, W).float())[0], W, H)
        print(f"wrote {args.out}_hitcount.pfm (crossings per pixel: mean {float(crossings.float().mean()):.2f}, most {int(crossings.max())})")
    if args.aov:
        g = rt.gbuffer(scene, W, H)
        images = {"normal": g["normal"] * 0.5 + 0.5,
                  "depth": g["depth"][:, :, None].expand(H, W, 3), "albedo": g["albedo"]}
        os.makedirs(os.path.dirname(os.path.abspath(args.aov)), exist_ok=True)
        for name, rgb in images.items():
            rgba = torch.cat([rgb, torch.ones((H, W, 1), dtype=torch.float32, device=rgb.device)], dim=2)
            rt.write_pfm(f"{args.aov}_{name}.pfm", rgba.reshape(H, W * 4), W, H)
        print(f"wrote {args.aov}_normal.pfm / _depth.pfm / _albedo.pfm")


if __name__ == "__main__":
    main()
