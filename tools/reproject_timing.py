"""Timing of rt_reproject (csrc/reproject.hip) with HIP events, on the bunny scene at 1920x1080 and 3840x2160:

  two frames one step of the quality tool's dolly apart are rendered and traced; then, interleaved,
    * rt_reproject of the second onto the first (the steady state of a moving camera),
    * rt_reproject with an unmoved camera (every projection lands on its own pixel: the most coherent gather),
    * rt_reproject without a previous frame (NULL prev: the pixel's own loads and stores only),
    * a device-to-device copy of a surface of the same size (16 B read and 16 B written per pixel), which gives the
      rate at which this device streams,
    * one rt_denoise call with its defaults.
  rt_reproject must move at least 152 B per pixel: its own colour and record in (16 + 48), colour and history out
  (16 + 4), and every previous pixel's colour, record and history in once (16 + 48 + 4); the taps ask for four times
  the last part, 272 B, most of which neighbouring lanes share.  The table gives the time, those 152 B per pixel as a
  rate, and that rate as a fraction of the copy's.

    python tools/reproject_timing.py [--sizes 1920x1080,3840x2160] [--samples 20] [--batch 50] [--warmup 3] [--out FILE]

A timed sample is `--batch` back-to-back calls between two events, reported per call; rows are sampled round-robin
(one sample of each per round) so that drift hits them alike; medians, with the extremes.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as G  # noqa: E402
import reproject_cases as C  # noqa: E402

MIN_BYTES = 152  # per pixel, see above


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


def one_size(rt, w, h, args):
    n = w * h
    scene = rt.Scene()
    scene.setup("bunny")
    scene.set_viewport(w, h)
    rng = rt.alloc_rng(n)
    rt.init_rng_states(rng, w, h, 0xDEADBEEF)
    frames = []
    for k in (0, 1):
        scene.set_camera(*C.dolly(k, 1))
        scene.upload(rng.data_ptr())
        surf = rt.alloc_surface(w, h)
        rt.render(scene, surf, rt.alloc_surface(w, h), w, h, 5, 6, 0)
        frames.append((surf, rt.trace_camera(scene, w, h), scene.camera()))
    (s0, h0, c0), (s1, h1, c1) = frames
    hist0 = torch.full((h, w), 4.0, device="cuda")
    out, hist = rt.alloc_surface(w, h), torch.zeros((h, w), device="cuda")
    copy_dst = rt.alloc_surface(w, h)
    denoised = rt.alloc_surface(w, h)
    scratch = torch.empty((rt.denoise_scratch_bytes(w, h) // 4,), dtype=torch.float32, device="cuda")
    jobs = {"moved": lambda: rt.reproject_raw(s1, h1, c1, w, h, prev=(s0, h0, hist0, c0), out=out, out_history=hist),
            "unmoved": lambda: rt.reproject_raw(s1, h0, c0, w, h, prev=(s0, h0, hist0, c0), out=out, out_history=hist),
            "null prev": lambda: rt.reproject_raw(s1, h1, c1, w, h, out=out, out_history=hist),
            "copy": lambda: copy_dst.copy_(s1),
            "denoise": lambda: rt.denoise(scene, s1, w, h, hits=h1, out=denoised, scratch=scratch)}
    t = time_rows(jobs, args.samples, args.batch, args.warmup)
    med = {k: float(np.median(v)) for k, v in t.items()}
    rt.reproject_raw(s1, h1, c1, w, h, prev=(s0, h0, hist0, c0), out=out, out_history=hist)
    torch.cuda.synchronize()
    took = float((hist > 1).double().mean())
    copy_bytes = 2 * s1.numel() * 4  # the padded rows, read and written
    copy_rate = copy_bytes / med["copy"] / 1e9  # TB/s
    lines = [f"{w}x{h} = {n} pixels, bunny scene, the two cameras 0.07 units and 0.27 degrees apart; {100 * took:.1f} % of the pixels take history",
             f"  {'':<44}{'median ms':>10}{'min':>9}{'max':>9}{'TB/s':>8}{'of the copy':>13}"]

    def row(name, key, nbytes):
        rate = nbytes / med[key] / 1e9
        lines.append(f"  {name:<44}{med[key]:>10.4f}{min(t[key]):>9.4f}{max(t[key]):>9.4f}{rate:>8.2f}{rate / copy_rate:>13.2f}")

    row("device copy of one surface (32 B/pixel)", "copy", copy_bytes)
    row(f"rt_reproject, moved camera ({MIN_BYTES} B/pixel)", "moved", n * MIN_BYTES)
    row(f"rt_reproject, unmoved camera ({MIN_BYTES} B/pixel)", "unmoved", n * MIN_BYTES)
    row("rt_reproject, NULL prev (36 B/pixel)", "null prev", n * 36)
    lines.append(f"  {'rt_denoise, defaults (5 passes)':<44}{med['denoise']:>10.4f}{min(t['denoise']):>9.4f}{max(t['denoise']):>9.4f}")
    lines.append(f"  rt_reproject (moved) = {med['moved'] / med['copy']:.2f} x the copy of one surface, {med['moved'] / med['denoise']:.3f} of one rt_denoise; "
                 f"the floor of its {MIN_BYTES} B/pixel at the copy's rate is {n * MIN_BYTES / copy_rate / 1e9:.4f} ms")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--samples", type=int, default=20, help="timed samples per row")
    ap.add_argument("--batch", type=int, default=50, help="calls per timed sample")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    args = ap.parse_args()
    assert args.samples >= 5 and args.batch >= 1
    assert torch.cuda.is_available(), "reproject_timing needs a GPU"
    rt = G.load_package()
    torch.cuda.set_device(0)
    lines = [f"rt_reproject timing, {torch.cuda.get_device_name(0)}; HIP events around {args.batch} back-to-back calls per sample, "
             f"{args.warmup} warm-up calls, {args.samples} samples per row, rows interleaved",
             "the kernel is the fastest of three shapes measured (profiles/reproject_variants.txt): 64 x 4-pixel blocks, all tap loads issued before the",
             "tests; tried and dropped: a tap's normal and position loaded only after its cheap tests (24 % slower), 32 x 8-pixel blocks (1 % slower)", ""]
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
