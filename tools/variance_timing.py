"""Timing of the variance-steered filter's calls (rt_moments, the second rt_reproject, rt_denoise_variance;
csrc/denoise_variance.hip) against one rt_denoise call and one surface copy in the same process, HIP events:

  at each size (default 1920x1080 and 3840x2160) one 5-spp frame of the bunny scene is rendered and its camera's hit
  records traced; then, interleaved,
    * rt_moments on the frame;
    * rt_reproject on the moments (the previous moments, records and camera being the same frame's: a camera that
      stands still), the second reprojection a frame of the chain pays;
    * rt_denoise_variance with 1..6 passes and a history of 32 everywhere (every lane on the temporal estimate), and
      rt_denoise with 1..6 passes: the time of a whole call, and from the differences the time of each pass;
    * rt_denoise_variance with 1 pass and no moments (every lane on the 7x7 spatial estimate, a first frame), and
      with the history 32 but for vertical bands 3 pixels wide every 200 pixels (1.5 % of the lanes, as after a
      warm-up along the dolly of profiles/variance_quality.txt): against the 1-pass call above, the prepare step's
      spatial estimate;
    * a device-to-device copy of one surface (16 B per pixel read and as much written).

    python tools/variance_timing.py [--sizes 1920x1080,3840x2160] [--samples 20] [--batch 5] [--warmup 3] [--out FILE]

A timed sample is `--batch` back-to-back calls between two events, reported per call; rows are sampled round-robin (one
sample of each per round) so that drift hits them alike; medians, with the extremes.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as G  # noqa: E402


def time_rows(jobs, samples, batch, warmup):
    times = {k: [] for k in jobs}
    for fn in jobs.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    for _ in range(samples):
        for k, fn in jobs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(batch):
                fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) / batch)
    return times


def one_size(rt, W, H, args):
    n = W * H
    scene = rt.Scene()
    scene.setup("bunny")
    scene.set_viewport(W, H)
    rng = rt.alloc_rng(n)
    rt.init_rng_states(rng, W, H, 0xDEADBEEF)
    scene.upload(rng.data_ptr())
    frame, unused = rt.alloc_surface(W, H), rt.alloc_surface(W, H)
    rt.render(scene, frame, unused, W, H, 5, 6, 0)
    hits = rt.trace_camera(scene, W, H)
    cam = scene.camera()
    hit = int((rt.hit_fields(hits)["kind"] != rt.HIT_MISS).sum())
    moments = rt.moments(scene, frame, hits, W, H)
    prev_moments, acc_moments = moments.clone(), rt.alloc_surface(W, H)
    full = torch.full((H, W), 32.0, device="cuda")
    banded = full.clone()
    for x in range(100, W, 200):
        banded[:, x:x + 3] = 1.0
    share = float((banded < 4).double().mean())
    hist_out = torch.zeros((H, W), device="cuda")
    out, var = rt.alloc_surface(W, H), torch.zeros((H, W), device="cuda")
    scratch = torch.empty((rt.denoise_variance_scratch_bytes(W, H) // 4,), device="cuda")
    dscratch = torch.empty((rt.denoise_scratch_bytes(W, H) // 4,), device="cuda")
    dst = torch.empty_like(frame)

    def variance(k, moments_=moments, history=full):
        rt.denoise_variance(scene, frame, W, H, hits=hits, moments=moments_, history=history, out=out, out_variance=var,
                            scratch=scratch, iterations=k)

    jobs = {("v", k): (lambda k=k: variance(k)) for k in range(1, 7)}
    jobs.update({("d", k): (lambda k=k: rt.denoise(scene, frame, W, H, hits=hits, out=out, scratch=dscratch, iterations=k))
                 for k in range(1, 7)})
    jobs["spatial"] = lambda: variance(1, None, None)
    jobs["banded"] = lambda: variance(1, moments, banded)
    jobs["moments"] = lambda: rt.moments(scene, frame, hits, W, H, out=acc_moments)
    jobs["reproject"] = lambda: rt.reproject_raw(moments, hits, cam, W, H, prev=(prev_moments, hits, full, cam), out=acc_moments,
                                                 out_history=hist_out)
    jobs["copy"] = lambda: dst.copy_(frame)
    t = time_rows(jobs, args.samples, args.batch, args.warmup)
    med = {k: float(np.median(v)) for k, v in t.items()}
    row = lambda k: f"median {med[k]:.4f} ms (min {min(t[k]):.4f}, max {max(t[k]):.4f})"
    rate = 2 * frame.numel() * 4 / med["copy"] / 1e9  # TB/s, bytes read + bytes written (the pitch's padding included)
    vcalls, dcalls = [med[("v", k)] for k in range(1, 7)], [med[("d", k)] for k in range(1, 7)]
    vpass = [vcalls[0]] + [vcalls[i] - vcalls[i - 1] for i in range(1, 6)]
    dpass = [dcalls[0]] + [dcalls[i] - dcalls[i - 1] for i in range(1, 6)]
    lines = [f"{W}x{H} = {n} pixels ({hit} hit), bunny scene, one frame at 5 spp x 6 bounces",
             f"  copy of one surface (16 B/pixel read + as much written): {row('copy')} = {rate:.2f} TB/s",
             f"  rt_moments (16 + 48 B/pixel read, 16 written):            {row('moments')} = {med['moments'] / med['copy']:.2f} copies",
             f"  rt_reproject on the moments (camera standing still):      {row('reproject')} = {med['reproject'] / med['copy']:.2f} copies",
             "  k passes = prepare + k passes, the last one remodulating (pass index s has step 1 << s; steps 1 and 2 from LDS tiles):",
             f"  {'':<44}" + "".join(f"{'k=' + str(k):>9}" for k in range(1, 7)),
             f"  {'rt_denoise_variance, history everywhere, ms':<44}" + "".join(f"{c:>9.3f}" for c in vcalls),
             f"  {'  min':<44}" + "".join(f"{min(t[('v', k)]):>9.3f}" for k in range(1, 7)),
             f"  {'  max':<44}" + "".join(f"{max(t[('v', k)]):>9.3f}" for k in range(1, 7)),
             f"  {'rt_denoise, ms':<44}" + "".join(f"{c:>9.3f}" for c in dcalls),
             f"  {'  min':<44}" + "".join(f"{min(t[('d', k)]):>9.3f}" for k in range(1, 7)),
             f"  {'  max':<44}" + "".join(f"{max(t[('d', k)]):>9.3f}" for k in range(1, 7)),
             f"  {'':<44}" + "".join(f"{'step ' + str(1 << s):>9}" for s in range(6)),
             f"  {'rt_denoise_variance per pass: call(k)-call(k-1)':<44}" + "".join(f"{p:>9.3f}" for p in vpass) + "   (step 1 includes prepare)",
             f"  {'rt_denoise per pass':<44}" + "".join(f"{p:>9.3f}" for p in dpass),
             f"  {'ratio':<44}" + "".join(f"{a / b:>9.2f}" for a, b in zip(vpass, dpass)),
             f"  default call (5 passes): rt_denoise_variance {vcalls[4]:.3f} ms, rt_denoise {dcalls[4]:.3f} ms: {vcalls[4] / dcalls[4]:.2f} x",
             "  the prepare step's spatial estimate, 1-pass calls:",
             f"    history everywhere (no lane spatial):           {row(('v', 1))}",
             f"    bands, {100 * share:.2f} % of the lanes spatial:            {row('banded')}   (+{med['banded'] - med[('v', 1)]:.4f} ms)",
             f"    no moments (every lane spatial, a first frame): {row('spatial')}   (+{med['spatial'] - med[('v', 1)]:.4f} ms)",
             f"  a frame of the chain on top of rt_reproject + rt_denoise: rt_moments + second rt_reproject + the difference of the default calls = "
             f"{med['moments'] + med['reproject'] + vcalls[4] - dcalls[4]:.3f} ms"]
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--samples", type=int, default=20, help="timed samples per row")
    ap.add_argument("--batch", type=int, default=5, help="calls per timed sample")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    args = ap.parse_args()
    assert args.samples >= 5 and args.batch >= 1
    assert torch.cuda.is_available(), "variance_timing needs a GPU"
    rt = G.load_package()
    torch.cuda.set_device(0)
    lines = [f"rt_moments / rt_reproject / rt_denoise_variance timing, {torch.cuda.get_device_name(0)}; HIP events around {args.batch} back-to-back "
             f"calls per sample, {args.warmup} warm-up calls, {args.samples} samples per row, rows interleaved", ""]
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
