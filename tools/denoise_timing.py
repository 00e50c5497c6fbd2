"""Denoiser timing (rt_denoise, csrc/denoise.hip) on benchmark configs' scenes and frame sizes, HIP events:

  for each config (default: cfg2 and cfg4 at 1920x1080, cfg3 at 3840x2160) one frame is rendered with the
  config's own spp and bounces and its camera's hit records are traced; then, interleaved,
    * rt_denoise with 1..6 passes: the time of a whole call, and from the differences the time of each pass;
    * a device-to-device copy of 48 B per pixel (the three buffers a pass reads), which gives the rate at which
      this device streams; the floor of one pass is the 64 B per pixel it must move (48 read, 16 written) at
      that rate;
    * the config's own rt.render frame.
  The table ends with the ratio of one default denoise to one rendered frame.

    python tools/denoise_timing.py [--configs cfg2,cfg4,cfg3] [--samples 20] [--batch 5] [--warmup 3] [--out FILE]

A timed sample is `--batch` back-to-back calls between two events, reported per call; rows are sampled
round-robin (one sample of each per round) so that drift hits them alike; medians, with the extremes.
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

def time_rows(jobs, samples, batch, warmup):
    times = {k: [] for k in jobs}
    for fn in jobs.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    for _ in range(samples):
        for k, (fn) in jobs.items():
            n = 1 if k == "frame" else batch
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) / n)
    return times


def one_config(rt, name, args):
    scene_name, W, H, SPP, BOUNCES, _ = bench.CONFIGS[name]
    n = W * H
    scene = rt.Scene()
    scene.setup(scene_name)
    scene.set_viewport(W, H)
    rng = rt.alloc_rng(n)
    rt.init_rng_states(rng, W, H, bench.SEED)
    scene.upload(rng.data_ptr())
    bufs = [rt.alloc_surface(W, H), rt.alloc_surface(W, H)]
    rt.render(scene, bufs[0], bufs[1], W, H, SPP, BOUNCES, 0)
    noisy = bufs[0].clone()
    hits = rt.trace_camera(scene, W, H)
    out = rt.alloc_surface(W, H)
    scratch = torch.empty((rt.denoise_scratch_bytes(W, H) // 4,), dtype=torch.float32, device="cuda")
    src, dst = torch.rand((n * 12,), device="cuda"), torch.empty((n * 12,), device="cuda")

    def denoise(iterations):
        rt.denoise(scene, noisy, W, H, hits=hits, out=out, scratch=scratch, iterations=iterations)

    frame_no = [1]

    def frame():
        f = frame_no[0]
        rt.render(scene, bufs[f & 1], bufs[(f + 1) & 1], W, H, SPP, BOUNCES, f)
        frame_no[0] = f + 1

    jobs = {it: (lambda it=it: denoise(it)) for it in range(1, 7)}
    jobs["copy"] = lambda: dst.copy_(src)
    jobs["frame"] = frame
    t = time_rows(jobs, args.samples, args.batch, args.warmup)
    med = {k: float(np.median(v)) for k, v in t.items()}
    hit = int((rt.hit_fields(hits)["kind"] != rt.HIT_MISS).sum())
    rate = 2 * n * 48 / med["copy"] / 1e9  # TB/s, bytes read + bytes written
    floor = n * 64 / rate / 1e9             # ms: one pass's 48 B read + 16 B written per pixel at that rate
    calls = [med[it] for it in range(1, 7)]
    passes = [calls[0]] + [calls[i] - calls[i - 1] for i in range(1, 6)]
    lines = [f"{name}: scene {scene_name}, {W}x{H} = {n} pixels ({hit} hit), frame {SPP} spp x {BOUNCES} bounces",
             f"  rendered frame (rt.render, default occupancy): median {med['frame']:.3f} ms (min {min(t['frame']):.3f}, max {max(t['frame']):.3f})",
             f"  device-to-device copy of 48 B/pixel ({n * 48 / 1e6:.1f} MB read + as much written): median {med['copy']:.4f} ms = {rate:.2f} TB/s;",
             f"  floor of one pass = the 64 B/pixel it moves (48 read, 16 written) at that rate: {floor:.4f} ms",
             "  rt_denoise with k passes = prepare + k passes, the last one remodulating (pass index s has step 1 << s):",
             f"  {'':<28}" + "".join(f"{'k=' + str(k):>9}" for k in range(1, 7)),
             f"  {'ms per call, median':<28}" + "".join(f"{c:>9.3f}" for c in calls),
             f"  {'min':<28}" + "".join(f"{min(t[k]):>9.3f}" for k in range(1, 7)),
             f"  {'max':<28}" + "".join(f"{max(t[k]):>9.3f}" for k in range(1, 7)),
             f"  {'':<28}" + "".join(f"{'step ' + str(1 << s):>9}" for s in range(6)),
             f"  {'ms per pass: call(k)-call(k-1)':<28}" + "".join(f"{p:>9.3f}" for p in passes) + "   (step 1 includes prepare)",
             f"  {'x the floor of one pass':<28}" + "".join(f"{p / floor:>9.1f}" for p in passes)]
    d = med[5]
    lines.append(f"  default denoise (5 passes): {d:.3f} ms = {d / med['frame']:.3f} of one rendered frame; "
                 f"{d / (5 * floor):.1f} x the floor of its 5 passes")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="cfg2,cfg4,cfg3")
    ap.add_argument("--samples", type=int, default=20, help="timed samples per row")
    ap.add_argument("--batch", type=int, default=5, help="denoise calls / copies per timed sample")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    args = ap.parse_args()
    assert args.samples >= 5 and args.batch >= 1
    assert torch.cuda.is_available(), "denoise_timing needs a GPU"
    rt = G.load_package()
    torch.cuda.set_device(0)
    lines = [f"rt_denoise timing, {torch.cuda.get_device_name(0)}; HIP events around {args.batch} back-to-back calls per sample "
             f"(one frame per sample for the render), {args.warmup} warm-up calls, {args.samples} samples per row, rows interleaved", ""]
    for name in args.configs.split(","):
        lines += one_config(rt, name, args) + [""]
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
