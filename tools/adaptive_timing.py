"""Adaptive sampling's calls on the GPU (csrc/rt_adaptive.hip, csrc/sample_plan.hip), HIP events, at 1920x1080:

  (a) rt_sample_pixels with a uniform count of 8 (pixels = NULL: row order; and the same list in the planner's
      8x8 sub-tile order) against rt_render at 8 spp (a plain call: no lane map, the default occupancy) and against
      rt_radiance with samples = 8 along every pixel's first camera ray -- config 2's scene, W x H x 8 paths each;
  (b) a planned round (rt_sample_priority + rt_sample_plan after a 4-sample warm-up, budget 8 W H, at most 64 a pixel):
      the planner's list, sorted by count, against the same counts in plain row-major order;
  (c) rt_sample_priority, rt_sample_plan and rt_sample_resolve, each against a device-to-device copy of a surface;
  (d) the uniform 8-sample list in sub-tile order at 5 / 6 / 7 waves per SIMD: config 2's scene (MODE 17 lean) and
      config 4's (MODE 21).

Before anything is timed the tool asserts that the uniform round is rt_render's 8 spp frame bit for bit (accum.rgb / 8
and the final states).  Every row states its own total of samples: compare rows per sample.

    python tools/adaptive_timing.py [--configs cfg2,cfg4] [--calls 20] [--warmup 3] [--out FILE]

A timed sample is one call between two events; the RNG states are restored (untimed) before every sample, so every
sample of a row is the same work; the rows of a scene are sampled round-robin, so drift hits them alike.
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

F32, U32 = np.float32, np.uint32
BOUNCES, SPP, WARM_SPP, MAX_SAMPLES = 6, 8, 4, 64


def subtile_order(w, h):
    """Pixel indices y * w + x in rt_sample_plan's 8x8 sub-tile order."""
    out = []
    for ty in range(0, h, 8):
        rows = np.arange(ty, min(ty + 8, h))
        for tx in range(0, w, 8):
            cols = np.arange(tx, min(tx + 8, w))
            out.append((rows[:, None] * w + cols[None, :]).reshape(-1))
    return np.concatenate(out).astype(np.int32)


def first_rays(rt, scene, W, H, initial):
    """rt_ray rows of every pixel's first camera sample and the states past its jitter (tools/radiance_timing.py)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import radiance_timing as RT
    cam = np.frombuffer(bytes(scene.camera()), dtype=F32).copy()
    rays, states = RT.sample_zero(cam, W, H, initial.cpu().numpy().view(U32).reshape(W * H, 12))
    return torch.from_numpy(rays).cuda(), torch.from_numpy(states.view(np.int32).reshape(-1)).cuda()


def measure(rt, config, calls, warmup, lines, full):
    scene_name, W, H, _, _, _ = bench.CONFIGS[config]
    n = W * H
    scene = rt.Scene()
    scene.setup(scene_name)
    scene.set_viewport(W, H)
    rng = rt.alloc_rng(n)
    rt.init_rng_states(rng, W, H, bench.SEED)
    scene.upload(rng.data_ptr())
    initial = rng.clone()
    surface, accum, image = rt.alloc_surface(W, H), rt.alloc_surface(W, H), rt.alloc_surface(W, H)
    moments = torch.zeros((n, 2), dtype=torch.float32, device="cuda")
    uniform = torch.full((n,), SPP, dtype=torch.int16, device="cuda")
    tiles = torch.from_numpy(subtile_order(W, H)).cuda()

    def pixels(px, counts, w=0):
        rt.sample_pixels(scene, W, H, counts, rng, accum, pixels=px, moments=moments, bounces=BOUNCES, waves_per_simd=w)

    # identical work, identical answers
    rt.render(scene, surface, None, W, H, SPP, BOUNCES, frame_index=0)
    torch.cuda.synchronize()
    want_rng = rng.clone()
    for px in (None, tiles):
        rng.copy_(initial)
        accum.zero_()
        pixels(px, uniform)
        torch.cuda.synchronize()
        mean = rt.surface_view(accum, W)[..., 0:3] / SPP
        assert torch.equal(mean.view(torch.int32), rt.surface_view(surface, W)[..., 0:3].contiguous().view(torch.int32)), "accum / 8 != rt_render"
        assert torch.equal(rng, want_rng), "final states != rt_render's"

    jobs = {}  # name -> (samples, restore states?, call)
    if full:
        jobs[f"rt_render spp {SPP} (plain call)"] = (n * SPP, True, lambda: rt.render(scene, surface, None, W, H, SPP, BOUNCES, frame_index=0))
        rays, ray_start = first_rays(rt, scene, W, H, initial)
        ray_rng, ray_out = ray_start.clone(), torch.empty((n, 4), dtype=torch.float32, device="cuda")

        def radiance():
            ray_rng.copy_(ray_start)  # inside the timed window: a 100 MB copy, some 0.05 ms of the row's tens
            rt.radiance(scene, rays, ray_rng, bounces=BOUNCES, samples=SPP, out=ray_out)
        jobs[f"rt_radiance samples {SPP}, row order"] = (n * SPP, False, radiance)
        jobs[f"rt_sample_pixels uniform {SPP}, pixels NULL (row order)"] = (n * SPP, True, lambda: pixels(None, uniform))
    for w in (5, 6, 7):
        jobs[f"rt_sample_pixels uniform {SPP}, sub-tile order, {w} waves"] = (n * SPP, True, lambda w=w: pixels(tiles, uniform, w))
    if full:
        # (b) a planned round after a warm-up
        rng.copy_(initial)
        accum.zero_()
        moments.zero_()
        pixels(None, torch.full((n,), WARM_SPP, dtype=torch.int16, device="cuda"))
        warm_rng = rng.clone()
        prio = rt.sample_priority(accum, moments, W, H)
        scratch = torch.empty((rt.sample_plan_scratch_bytes(W, H),), dtype=torch.uint8, device="cuda")
        plan_px, plan_n, total = rt.sample_plan(prio, W, H, SPP * n, max_samples=MAX_SAMPLES, scratch=scratch)
        torch.cuda.synchronize()
        planned = int(total.cpu()[0])
        row_px = torch.arange(n, dtype=torch.int32, device="cuda")
        again_px, again_n = torch.empty_like(plan_px), torch.empty_like(plan_n)
        row_n = torch.empty_like(plan_n)
        row_n[plan_px.long()] = plan_n
        hist = np.bincount(plan_n.cpu().numpy().view(np.uint16).astype(np.int64), minlength=MAX_SAMPLES + 1)
        lines.append(f"{config}: planned round after {WARM_SPP} spp: {planned} samples of a budget of {SPP * n}; pixels with 0 / 1-7 / 8-63 / "
                     f"{MAX_SAMPLES} samples: {hist[0]} / {hist[1:8].sum()} / {hist[8:MAX_SAMPLES].sum()} / {hist[MAX_SAMPLES]}")
        jobs["rt_sample_pixels planned round, sorted list"] = (planned, "warm", lambda: pixels(plan_px, plan_n))
        jobs["rt_sample_pixels same counts, row-major list"] = (planned, "warm", lambda: pixels(row_px, row_n))
        # (c) the pixel kernels
        jobs["surface copy (device to device)"] = (0, False, lambda: image.copy_(surface))
        jobs["rt_sample_priority"] = (0, False, lambda: rt.sample_priority(accum, moments, W, H, out=prio))
        jobs["rt_sample_plan"] = (0, False, lambda: rt.sample_plan(prio, W, H, SPP * n, max_samples=MAX_SAMPLES, pixels=again_px,
                                                                   samples=again_n, total=total, scratch=scratch))
        jobs["rt_sample_resolve"] = (0, False, lambda: rt.sample_resolve(accum, W, H, out=image))

    def restore(how):
        if how == "warm":
            rng.copy_(warm_rng)
        elif how:
            rng.copy_(initial)

    for _, how, fn in jobs.values():
        for _ in range(warmup):
            restore(how)
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in jobs}
    for _ in range(calls):
        for k, (_, how, fn) in jobs.items():
            restore(how)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
    lines.append(f"{config}'s scene ({scene_name}), {W}x{H}, {BOUNCES} bounces: a uniform round of {SPP} == rt_render at {SPP} spp bit for bit "
                 f"(accum.rgb / {SPP} and final states; pixels NULL and sub-tile order): yes")
    lines.append(f"{'what':<62}{'samples':>10}{'median ms':>10}{'min ms':>9}{'max ms':>9}{'spread':>8}{'Msamples/s':>11}")
    for k, t in times.items():
        med = float(np.median(t))
        rate = f"{jobs[k][0] / med / 1e3:.1f}" if jobs[k][0] else ""
        lines.append(f"{k:<62}{jobs[k][0]:>10}{med:>10.3f}{min(t):>9.3f}{max(t):>9.3f}{100 * (max(t) - min(t)) / med:>7.1f}%{rate:>11}")
    lines.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="cfg2,cfg4")
    ap.add_argument("--calls", type=int, default=20, help="timed samples per row")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    args = ap.parse_args()
    assert args.calls >= 20, "at least 20 timed samples"
    assert torch.cuda.is_available(), "adaptive_timing needs a GPU"
    rt = G.load_package()
    torch.cuda.set_device(0)
    lines = [f"adaptive sampling's calls, {torch.cuda.get_device_name(0)}",
             f"HIP events around one call per sample (ms), states restored before every sample, {args.warmup} warm-up calls, "
             f"{args.calls} samples per row, a scene's rows interleaved; spread = (max - min) / median", ""]
    for config in args.configs.split(","):
        measure(rt, config, args.calls, args.warmup, lines, full=config == "cfg2")
    text = "\n".join(lines)
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
