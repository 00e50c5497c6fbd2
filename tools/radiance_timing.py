"""rt_radiance against the renderer on identical work (csrc/rt_radiance.hip against the production render kernel), HIP
events, on config 2's scene and on config 4's in one run:

  the yardstick: rt_render at spp = 1, 6 bounces, 1920x1080, frame_index 0 -- W x H paths;
  the same paths through rt_radiance: the jittered camera rays of sample 0 with the states advanced past the two jitter
  draws, in row order (wave = 64 pixels of a row) and in 8x8-tile order (wave = the renderer's sub-tile), at 5 / 6 / 7
  waves per SIMD.  Before anything is timed the tool asserts that both orders give rt_render's surface and final
  states bit for bit;
  an incoherent batch: panorama_rays from the camera's position, 2048x1024, 1 sample, at 5 / 6 / 7 waves per SIMD.

    python tools/radiance_timing.py [--configs cfg2,cfg4] [--calls 20] [--warmup 3] [--out FILE]
    rocprofv3 --pmc COUNTERS... -d DIR -- python tools/radiance_timing.py --once --configs cfg4    (a run of its own)

A timed sample is one call between two events; the RNG states are restored (untimed) before every sample, so every
sample of a row is the same work; the rows of a scene are sampled round-robin, so drift hits them alike.  The table
gives the median and the extremes, and each row's spread.
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
BOUNCES = 6
PANORAMA = (2048, 1024)


def xorwow_step(s):
    """curand's step on uint32 [N, 6] states (d, v0..v4) in place; returns the draws."""
    v = s[:, 1:]
    t = v[:, 0] ^ (v[:, 0] >> U32(2))
    new4 = (v[:, 4] ^ (v[:, 4] << U32(4))) ^ (t ^ (t << U32(1)))
    v[:, 0:4] = v[:, 1:5].copy()
    v[:, 4] = new4
    s[:, 0] += U32(362437)
    return v[:, 4] + s[:, 0]


def sample_zero(cam15, w, h, states12):
    """(rt_ray rows of every pixel's first camera sample, the states advanced past its two jitter draws), from the
    frame's initial states (uint32 [w * h, 12]): the renderer's sample start (rt_fast_body.h) in numpy fp32."""
    s = states12[:, :6].copy()
    ru = xorwow_step(s).astype(F32) * F32(2.0 ** -32) + F32(2.0 ** -33)
    rv = xorwow_step(s).astype(F32) * F32(2.0 ** -32) + F32(2.0 ** -33)
    cam = np.asarray(cam15, dtype=F32)
    co, ch, cv, cl = cam[0:3], cam[6:9], cam[9:12], cam[12:15]
    i = np.arange(w * h)
    ux = (((i % w).astype(F32) + ru) / F32(w)).astype(F32)
    uy = (((i // w).astype(F32) + rv) / F32(h)).astype(F32)
    rays = np.zeros((w * h, 8), dtype=F32)
    for k in range(3):
        rays[:, k] = co[k]
        rays[:, 4 + k] = (((cl[k] + (ch[k] * ux).astype(F32)).astype(F32) + (cv[k] * uy).astype(F32)).astype(F32) - co[k]).astype(F32)
    rays[:, 3] = F32(1e30)
    out = states12.copy()
    out[:, :6] = s
    return rays, out


def tile_order(w, h):
    """Pixel indices y * w + x in 8x8-tile order: entry 64 t + 8 ly + lx is pixel (8 tx + lx, 8 ty + ly) of tile t."""
    assert w % 8 == 0 and h % 8 == 0
    ty, tx, ly, lx = np.meshgrid(np.arange(h // 8), np.arange(w // 8), np.arange(8), np.arange(8), indexing="ij")
    return ((ty * 8 + ly) * w + tx * 8 + lx).reshape(-1)


def measure(rt, config, calls, warmup, lines):
    scene_name, W, H, _, _, _ = bench.CONFIGS[config]
    n = W * H
    scene = rt.Scene()
    scene.setup(scene_name)
    scene.set_viewport(W, H)
    frame_rng = rt.alloc_rng(n)
    rt.init_rng_states(frame_rng, W, H, bench.SEED)
    scene.upload(frame_rng.data_ptr())
    initial = frame_rng.clone()
    cam = np.frombuffer(bytes(scene.camera()), dtype=F32).copy()
    rays_np, states_np = sample_zero(cam, W, H, initial.cpu().numpy().view(U32).reshape(n, 12))
    perm = tile_order(W, H)
    rays = {"row order": torch.from_numpy(rays_np).cuda(), "8x8-tile order": torch.from_numpy(rays_np[perm]).cuda()}
    start = {"row order": torch.from_numpy(states_np.view(np.int32).reshape(-1)).cuda(),
             "8x8-tile order": torch.from_numpy(states_np[perm].view(np.int32).reshape(-1)).cuda()}
    pw, ph = PANORAMA
    rays["panorama 2048x1024"] = torch.from_numpy(rt.panorama_rays(tuple(cam[0:3]), pw, ph)).cuda()
    start["panorama 2048x1024"] = rt.ray_rng(pw * ph, bench.SEED)
    work = {k: v.clone() for k, v in start.items()}
    surface = rt.alloc_surface(W, H)
    assert surface.shape[1] == W * 4, "a dense surface"
    out = {k: torch.empty((r.shape[0], 4), dtype=torch.float32, device="cuda") for k, r in rays.items()}

    def render():
        rt.render(scene, surface, None, W, H, 1, BOUNCES, frame_index=0)

    def radiance(order, w):
        rt.radiance(scene, rays[order], work[order], bounces=BOUNCES, samples=1, out=out[order], waves_per_simd=w)

    # identical work, identical answers: the surface and the final states, both orders
    render()
    radiance("row order", 0)
    radiance("8x8-tile order", 0)
    torch.cuda.synchronize()
    want, want_rng = surface.view(n, 4), frame_rng.view(n, 12)
    inv = torch.from_numpy(perm).cuda()
    assert torch.equal(out["row order"].view(torch.int32), want.view(torch.int32)), "row order: radiance != rt_render"
    assert torch.equal(work["row order"].view(n, 12), want_rng), "row order: final states != rt_render's"
    assert torch.equal(out["8x8-tile order"].view(torch.int32), want[inv].view(torch.int32)), "tile order: radiance != rt_render"
    assert torch.equal(work["8x8-tile order"].view(n, 12), want_rng[inv]), "tile order: final states != rt_render's"

    if calls == 0:  # --once: a counter run needs no more than the launches above, and one at the renderer's 5 waves
        work["8x8-tile order"].copy_(start["8x8-tile order"])
        radiance("8x8-tile order", 5)
        torch.cuda.synchronize()
        lines.append(f"{config}: one rt_render and rt_radiance launches (row order, 8x8-tile order; the latter again at 5 waves), bit-equal")
        return
    jobs = {"rt_render spp 1 (the yardstick)": (n, None, render)}
    for order in rays:
        for w in (5, 6, 7):
            jobs[f"rt_radiance {order}, {w} waves"] = (rays[order].shape[0], order, lambda order=order, w=w: radiance(order, w))

    def restore(order):
        if order is None:
            frame_rng.copy_(initial)
        else:
            work[order].copy_(start[order])

    for _, order, fn in jobs.values():
        for _ in range(warmup):
            restore(order)
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in jobs}
    for _ in range(calls):
        for k, (_, order, fn) in jobs.items():
            restore(order)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1))

    med = {k: float(np.median(t)) for k, t in times.items()}
    base = med["rt_render spp 1 (the yardstick)"]
    lines.append(f"{config}'s scene ({scene_name}), {W}x{H}, {BOUNCES} bounces, 1 sample: rt_radiance == rt_render bit for bit "
                 f"(surface and final states, row order and 8x8-tile order): yes")
    lines.append(f"{'what':<46}{'median ms':>10}{'min ms':>9}{'max ms':>9}{'spread':>8}{'Mpaths/s':>10}{'/ render':>9}")
    for k, t in times.items():
        ratio = f"{med[k] / base:.3f}" if "panorama" not in k else ""
        lines.append(f"{k:<46}{med[k]:>10.3f}{min(t):>9.3f}{max(t):>9.3f}{100 * (max(t) - min(t)) / med[k]:>7.1f}%"
                     f"{jobs[k][0] / med[k] / 1e3:>10.1f}{ratio:>9}")
    lines.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="cfg2,cfg4")
    ap.add_argument("--calls", type=int, default=20, help="timed samples per row")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    ap.add_argument("--once", action="store_true", help="launch each kernel once and time nothing: the program of a counter run")
    args = ap.parse_args()
    if args.once:
        args.calls = 0
    assert args.once or args.calls >= 20, "at least 20 timed samples"
    assert torch.cuda.is_available(), "radiance_timing needs a GPU"
    rt = G.load_package()
    torch.cuda.set_device(0)
    lines = [f"rt_radiance against rt_render on the same paths, {torch.cuda.get_device_name(0)}",
             f"HIP events around one call per sample (ms), states restored before every sample, {args.warmup} warm-up calls, "
             f"{args.calls} samples per row, a scene's rows interleaved; spread = (max - min) / median",
             "compulsory traffic per path: rt_radiance 32 B ray + 2 x 48 B state + 16 B output = 144 B; rt_render 2 x 48 B state + "
             "16 B surface (+ 16 B history when given) = 112-128 B", ""]
    for config in args.configs.split(","):
        measure(rt, config, args.calls, args.warmup, lines)
    text = "\n".join(lines)
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
