"""Ray-query throughput on a benchmark config's scene and frame size (default config 2; rt_trace_rays,
csrc/rt_query.hip), HIP events:

  (a) camera mode at the config's frame size, 1920x1080 for config 2 (coherent primary rays);
  (b) as many incoherent rays: origins at (a)'s hit positions + normal * 0.01 (missed pixels reuse the
      hit origins cyclically), fixed-seed unit directions;
  each at waves_per_simd 5, 6 and 7, and beside them a plain rt.render frame of the same size with spp = 1,
  bounces = 1 -- the same primary rays plus the RNG traffic, the sky lookups and the surface writes.

    python tools/query_timing.py [--config cfg2] [--calls 20] [--batch 10] [--warmup 3] [--out profiles/query_timing.txt]

A timed sample is `--batch` back-to-back calls between two events (a single call is well under a
millisecond, too short a window by itself), reported per call; the rows are sampled round-robin (one sample
of each per round) so that drift hits them alike; the table gives the median and the extremes of the samples.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg2")
    ap.add_argument("--calls", type=int, default=20, help="timed samples per row")
    ap.add_argument("--batch", type=int, default=10, help="calls per timed sample")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    args = ap.parse_args()
    assert args.calls >= 20 and args.batch >= 1, "at least 20 timed samples"
    assert torch.cuda.is_available(), "query_timing needs a GPU"
    rt = G.load_package()
    scene_name, W, H, _, _, _ = bench.CONFIGS[args.config]
    torch.cuda.set_device(0)
    scene = rt.Scene()
    scene.setup(scene_name)
    scene.set_viewport(W, H)
    rng = rt.alloc_rng(W * H)
    rt.init_rng_states(rng, W, H, bench.SEED)
    scene.upload(rng.data_ptr())
    n = W * H

    # (b)'s rays from (a)'s hits
    hits = torch.empty((n, 12), dtype=torch.float32, device="cuda")
    f = rt.hit_fields(rt.trace_camera(scene, W, H, hits=hits))
    hit = torch.nonzero(f["kind"] != rt.HIT_MISS)[:, 0]
    assert hit.numel() > 0
    src = hit[torch.arange(n, device="cuda") % hit.numel()]
    g = np.random.default_rng(20240607).normal(size=(n, 3))
    dirs = torch.from_numpy((g / np.linalg.norm(g, axis=1, keepdims=True)).astype(np.float32)).cuda()
    rays = torch.zeros((n, 8), dtype=torch.float32, device="cuda")
    rays[:, 0:3] = f["position"][src] + f["normal"][src] * 0.01
    rays[:, 3] = rt.RAY_TMAX
    rays[:, 4:7] = dirs
    surf, last = rt.alloc_surface(W, H), rt.alloc_surface(W, H)

    jobs = {}
    for w in (5, 6, 7):
        jobs[f"(a) camera mode, {w} waves/SIMD"] = lambda w=w: rt.trace_camera(scene, W, H, hits=hits, waves_per_simd=w)
        jobs[f"(b) incoherent rays, {w} waves/SIMD"] = lambda w=w: rt.trace_rays(scene, rays, hits=hits, waves_per_simd=w)
    for w in (5, 6, 7):
        jobs[f"rt.render spp=1 bounces=1, {w} waves/SIMD"] = lambda w=w: rt.render(scene, surf, last, W, H, 1, 1, waves_per_simd=w)
    times = {k: [] for k in jobs}
    for k, fn in jobs.items():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    for _ in range(args.calls):
        for k, fn in jobs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.batch):
                fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) / args.batch)

    kinds = torch.bincount(f["kind"].long(), minlength=3).tolist()
    lines = [f"ray queries on {args.config}'s scene ({scene_name}), {W}x{H} = {n} rays per call, {torch.cuda.get_device_name(0)}",
             f"HIP events around {args.batch} back-to-back calls per sample (ms per call), {args.warmup} warm-up calls, "
             f"{args.calls} samples per row, rows interleaved",
             f"(a)'s records: {kinds[0]} misses, {kinds[1]} sphere hits, {kinds[2]} triangle hits", "",
             f"{'what':<44}{'median ms':>10}{'min ms':>9}{'max ms':>9}{'Mrays/s (median)':>18}"]
    for k, t in times.items():
        med = float(np.median(t))
        lines.append(f"{k:<44}{med:>10.3f}{min(t):>9.3f}{max(t):>9.3f}{n / med / 1e3:>18.1f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
