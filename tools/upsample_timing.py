"""Upsampler timing (rt_upsample, csrc/upsample.hip) at the sizes a user renders, HIP events:

  for each output size (default 1920x1080 and 3840x2160) and each scale 2, 3, 4 the bunny scene is rendered at the low
  size with config 2's spp and bounces and the camera's hit records are traced at both sizes; then, interleaved,
    * rt_upsample, the whole call (prepare at the low size + gather at the output size);
    * a device-to-device copy, which gives the rate at which this device streams; the floor of a call is the bytes it
      must move at that rate: 64 B read and 16 B written per output pixel, 64 B read per low pixel;
    * one rt_denoise at the output size (what filtering a full-size frame costs instead);
    * the pipeline rt_render low + rt_trace_rays at both sizes + rt_denoise low + rt_upsample, against
    * rt_render at the output size.

    python tools/upsample_timing.py [--sizes 1920x1080,3840x2160] [--samples 12] [--batch 5] [--warmup 3] [--out FILE]

Below this tool's table profiles/upsample_timing.txt keeps the run that chose the gather's shape: rows marked * there are
the two kernels alone and the gather with its taps read straight from global memory, by a build that still held both
shapes.

A timed sample is `--batch` back-to-back calls between two events (one for the rows that render), reported per call;
rows are sampled round-robin (one sample of each per round) so that drift hits them alike; medians, with the extremes.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as G  # noqa: E402
import bench  # noqa: E402

SCALES = (2, 3, 4)
SCENE, _, _, SPP, BOUNCES, _ = bench.CONFIGS["cfg2"]
SINGLE = ("full", "low+up")      # rows that render: one call per sample


def time_rows(jobs, samples, batch, warmup):
    times = {k: [] for k in jobs}
    for fn in jobs.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    for _ in range(samples):
        for k, fn in jobs.items():
            n = 1 if k[0] in SINGLE else batch
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) / n)
    return times


def one_size(rt, W, H, args):
    n = W * H
    scene = rt.Scene()
    scene.setup(SCENE)
    scene.set_viewport(W, H)
    rng = rt.alloc_rng(n)
    rt.init_rng_states(rng, W, H, bench.SEED)
    scene.upload(rng.data_ptr())
    full = [rt.alloc_surface(W, H), rt.alloc_surface(W, H)]
    hits = rt.trace_camera(scene, W, H)
    out = rt.alloc_surface(W, H)
    filtered = rt.alloc_surface(W, H)
    dscratch = torch.empty((rt.denoise_scratch_bytes(W, H) // 4,), dtype=torch.float32, device="cuda")
    src, dst = torch.rand((n * 10,), device="cuda"), torch.empty((n * 10,), device="cuda")  # 40 B read + 40 B written per pixel
    frame_no = [0]

    def render_full():
        f = frame_no[0]
        rt.render(scene, full[f & 1], full[(f + 1) & 1], W, H, SPP, BOUNCES, f)
        frame_no[0] = f + 1

    jobs = {("full",): render_full, ("copy",): lambda: dst.copy_(src),
            ("denoise",): lambda: rt.denoise(scene, out, W, H, hits=hits, out=filtered, scratch=dscratch)}
    low_sizes, keep = {}, []
    for s in SCALES:
        assert W % s == 0 and H % s == 0, (W, H, s)
        lw, lh = W // s, H // s
        low_sizes[s] = (lw, lh)
        # a scene of its own for the low size, as a user of the pipeline has: rt_render keeps one table of the camera
        # rays' entry records per scene and rebuilds it when the frame size changes
        scene_full, scene = scene, rt.Scene()
        scene.setup(SCENE)
        scene.set_viewport(lw, lh)  # the same aspect: the camera is the output size's
        low_rng = rt.alloc_rng(lw * lh)
        rt.init_rng_states(low_rng, lw, lh, bench.SEED)
        scene.upload(low_rng.data_ptr())
        keep.append((scene, low_rng))
        low = [rt.alloc_surface(lw, lh), rt.alloc_surface(lw, lh)]
        rt.render(scene, low[0], low[1], lw, lh, SPP, BOUNCES, 0)
        low_hits = rt.trace_camera(scene, lw, lh)
        low_filtered = rt.alloc_surface(lw, lh)
        scratch = torch.empty((rt.upsample_scratch_bytes(lw, lh) // 4,), dtype=torch.float32, device="cuda")
        low_dscratch = torch.empty((rt.denoise_scratch_bytes(lw, lh) // 4,), dtype=torch.float32, device="cuda")
        hits_again = torch.empty_like(hits)

        def up(scene=scene, s=s, lw=lw, lh=lh, low=low, low_hits=low_hits, scratch=scratch):
            rt.upsample(scene, low[0], lw, lh, s, low_hits=low_hits, hits=hits, out=out, scratch=scratch)

        def pipeline(scene=scene, s=s, lw=lw, lh=lh, low=low, low_hits=low_hits, scratch=scratch, low_filtered=low_filtered,
                     low_dscratch=low_dscratch, hits_again=hits_again):
            rt.render(scene, low[0], low[1], lw, lh, SPP, BOUNCES, 0)
            rt.trace_camera(scene, lw, lh, hits=low_hits)
            rt.trace_camera(scene, W, H, hits=hits_again)
            rt.denoise(scene, low[0], lw, lh, hits=low_hits, out=low_filtered, scratch=low_dscratch)
            rt.upsample(scene, low_filtered, lw, lh, s, low_hits=low_hits, hits=hits_again, out=out, scratch=scratch)

        jobs[("upsample", s)] = up
        jobs[("low+up", s)] = pipeline
        scene = scene_full
    t = time_rows(jobs, args.samples, args.batch, args.warmup)
    med = {k: float(np.median(v)) for k, v in t.items()}
    row = lambda label, k: f"  {label:<58} median {med[k]:>8.4f} ms (min {min(t[k]):.4f}, max {max(t[k]):.4f})"
    rate = n * 80 / med[("copy",)] / 1e9  # TB/s, bytes read + bytes written
    lines = [f"output {W}x{H} = {n} pixels, scene {SCENE}, {SPP} spp x {BOUNCES} bounces",
             row("rt_render at the output size", ("full",)),
             row("rt_denoise at the output size (defaults)", ("denoise",)),
             row(f"device-to-device copy, 40 B/pixel read + as much written = {rate:.2f} TB/s", ("copy",))]
    for s in SCALES:
        lw, lh = low_sizes[s]
        floor = (n * 80 + lw * lh * 64) / rate / 1e9
        u = med[("upsample", s)]
        lines += [f" scale {s}: low {lw}x{lh}",
                  row("rt_upsample (prepare + gather from the LDS tile)", ("upsample", s)),
                  f"  {'floor: 80 B/output pixel + 64 B/low pixel at the copy rate':<58}        {floor:>8.4f} ms; rt_upsample = {u / floor:.2f} x"]
        p = med[("low+up", s)]
        lines += [row("render low + records at both sizes + denoise low + upsample", ("low+up", s)),
                  f"  {'':<58} = {p / med[('full',)]:.3f} of rt_render at the output size"]
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--samples", type=int, default=12, help="timed samples per row")
    ap.add_argument("--batch", type=int, default=5, help="calls per timed sample of the rows that do not render")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    args = ap.parse_args()
    assert args.samples >= 5 and args.batch >= 1
    assert torch.cuda.is_available(), "upsample_timing needs a GPU"
    rt = G.load_package()
    torch.cuda.set_device(0)
    lines = [f"rt_upsample timing, {torch.cuda.get_device_name(0)}; HIP events around {args.batch} back-to-back calls per sample "
             f"(one per sample for the rows that render), {args.warmup} warm-up calls, {args.samples} samples per row, rows interleaved",
             "command: python tools/upsample_timing.py " + " ".join(sys.argv[1:]), ""]
    for size in args.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        lines += one_size(rt, w, h, args) + [""]
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
