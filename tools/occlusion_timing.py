"""Occlusion-query throughput against the closest-hit query on the same ray buffers (rt_occluded against
rt_trace_rays, csrc/rt_occlude.hip against csrc/rt_query.hip), on a benchmark config's scene and frame size, HIP
events, at 5, 6 and 7 waves per SIMD:

  (a) the camera's pixel-centre rays, tmax 1e30;
  (b) tools/query_timing.py's incoherent rays: origins at (a)'s hit positions + normal * 0.01, fixed-seed directions;
  (c) (b)'s rays with tmax = half of each ray's closest distance: nothing is occluded, no early exit -- the cost floor;
  (d) one AO sample per hit pixel as rt_ao forms it (sample 0, radius 8, bias 0.001, ao_directions(256));
  and rt_ao itself at 8 samples per pixel.

    python tools/occlusion_timing.py [--config cfg2] [--calls 20] [--batch 5] [--warmup 3] [--out FILE] [--lib PATH]

A timed sample is `--batch` back-to-back calls between two events, reported per call; all rows are sampled
round-robin (one sample of each per round, rt_trace_rays and rt_occluded of a batch next to each other), so drift
hits them alike; the table gives the median and the extremes of the samples, and per batch the spread of the rows.
Every batch is also checked: rt_occluded's bytes equal kind != 0 of rt_trace_rays' records.  --lib loads another
build of the library (an A/B variant) instead of the package's.
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

AO_RADIUS, AO_BIAS = 8.0, 0.001


def camera_rays(rt, scene, w, h):
    cam = torch.from_numpy(np.frombuffer(bytes(scene.camera()), dtype=np.float32).copy()).cuda()
    co, ch, cv, cl = cam[0:3], cam[6:9], cam[9:12], cam[12:15]
    i = torch.arange(w * h, device="cuda")
    ux = (((i % w).float() + 0.5) / float(w))[:, None]
    uy = (((i // w).float() + 0.5) / float(h))[:, None]
    rays = torch.zeros((w * h, 8), dtype=torch.float32, device="cuda")
    rays[:, 0:3] = co
    rays[:, 3] = rt.RAY_TMAX
    rays[:, 4:7] = ((cl + ch * ux) + cv * uy) - co
    return rays


def ao_sample_rays(rt, f, valid, table):
    """Sample 0 of every valid pixel, in rt_ao's arithmetic (rt_abi.h)."""
    j = (((valid * 0x9E3779B1) & 0xFFFFFFFF) >> 8) % table.shape[0]
    n, pos, t = f["normal"][valid], f["position"][valid], f["t"][valid]
    d0 = n + table[j, 0:3]
    dd = (d0[:, 0] * d0[:, 0] + d0[:, 1] * d0[:, 1]) + d0[:, 2] * d0[:, 2]
    d = torch.where((dd > 1e-6)[:, None], d0 * (1.0 / torch.sqrt(dd))[:, None], n)
    rays = torch.zeros((valid.numel(), 8), dtype=torch.float32, device="cuda")
    rays[:, 0:3] = pos + n * (AO_BIAS * t)[:, None]
    rays[:, 3] = AO_RADIUS
    rays[:, 4:7] = d
    return rays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg2")
    ap.add_argument("--calls", type=int, default=20, help="timed samples per row")
    ap.add_argument("--batch", type=int, default=5, help="calls per timed sample")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    ap.add_argument("--lib", default=None, help="a variant build of librt_hip.so to load instead")
    args = ap.parse_args()
    assert args.calls >= 20 and args.batch >= 1, "at least 20 timed samples"
    assert torch.cuda.is_available(), "occlusion_timing needs a GPU"
    rt = G.load_package()
    if args.lib:
        rt._abi.LIB_PATH = os.path.abspath(args.lib)  # lib() reads it at its first call, in the module that loads the library
    scene_name, W, H, _, _, _ = bench.CONFIGS[args.config]
    torch.cuda.set_device(0)
    scene = rt.Scene()
    scene.setup(scene_name)
    scene.set_viewport(W, H)
    scene.upload(0)
    n = W * H

    batches = {}
    batches["(a) camera rays"] = camera_rays(rt, scene, W, H)
    hits = torch.empty((n, 12), dtype=torch.float32, device="cuda")
    records = rt.trace_rays(scene, batches["(a) camera rays"])  # the first-hit records: (b)-(d)'s origins, rt_ao's input
    f = rt.hit_fields(records)
    valid = torch.nonzero(f["kind"] != rt.HIT_MISS)[:, 0]
    assert valid.numel() > 0
    src = valid[torch.arange(n, device="cuda") % valid.numel()]
    g = np.random.default_rng(20240607).normal(size=(n, 3))
    rays = torch.zeros((n, 8), dtype=torch.float32, device="cuda")
    rays[:, 0:3] = f["position"][src] + f["normal"][src] * 0.01
    rays[:, 3] = rt.RAY_TMAX
    rays[:, 4:7] = torch.from_numpy((g / np.linalg.norm(g, axis=1, keepdims=True)).astype(np.float32)).cuda()
    batches["(b) incoherent rays"] = rays
    half = rays.clone()
    half[:, 3] = rt.trace_rays(scene, rays)[:, 0] * 0.5
    batches["(c) incoherent, tmax = t/2"] = half
    table = torch.from_numpy(rt.ao_directions(256)).cuda()
    batches["(d) one AO sample per hit pixel"] = ao_sample_rays(rt, f, valid, table)

    out_bytes = torch.empty((n,), dtype=torch.uint8, device="cuda")
    ao_img = torch.empty((H, W), dtype=torch.float32, device="cuda")
    share = {}
    for name, r in batches.items():  # the contract, at full size
        occ = rt.occluded(scene, r)
        kind = rt.hit_fields(rt.trace_rays(scene, r))["kind"]
        assert torch.equal(occ, (kind != 0).to(torch.uint8)), name
        share[name] = float(occ.float().mean())

    jobs = {}
    for name, r in batches.items():
        for w in (5, 6, 7):
            jobs[f"{name}: rt_trace_rays, {w} waves"] = (r.shape[0], lambda r=r, w=w: rt.trace_rays(scene, r, hits=hits, waves_per_simd=w))
            jobs[f"{name}: rt_occluded,   {w} waves"] = (r.shape[0], lambda r=r, w=w: rt.occluded(scene, r, out=out_bytes, waves_per_simd=w))
    for w in (5, 6, 7):
        jobs[f"rt_ao 8 samples, radius {AO_RADIUS:g}, {w} waves"] = (
            n, lambda w=w: rt.ambient_occlusion(scene, records, W, H, AO_RADIUS, samples=8, bias=AO_BIAS, directions=table,
                                                out=ao_img, waves_per_simd=w))
    times = {k: [] for k in jobs}
    for k, (_, fn) in jobs.items():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    for _ in range(args.calls):
        for k, (_, fn) in jobs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.batch):
                fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) / args.batch)

    lines = [f"occlusion queries on {args.config}'s scene ({scene_name}), {W}x{H}, {torch.cuda.get_device_name(0)}"
             + (f", library {os.path.basename(args.lib)}" if args.lib else ""),
             f"HIP events around {args.batch} back-to-back calls per sample (ms per call), {args.warmup} warm-up calls, "
             f"{args.calls} samples per row, rows interleaved",
             "occluded share: " + "; ".join(f"{k} {100 * v:.1f} % of {batches[k].shape[0]}" for k, v in share.items()),
             "rt_occluded == (kind != 0) of rt_trace_rays on every batch: yes", "",
             f"{'what':<58}{'median ms':>10}{'min ms':>9}{'max ms':>9}{'Mrays/s':>10}{'occl/trace':>11}"]
    med = {k: float(np.median(t)) for k, t in times.items()}
    for k, t in times.items():
        count = valid.numel() * 8 if k.startswith("rt_ao") else jobs[k][0]  # rt_ao traces the hit pixels only
        ratio = ""
        if "rt_occluded" in k:
            ratio = f"{med[k] / med[k.replace('rt_occluded,  ', 'rt_trace_rays,')]:.3f}"
        lines.append(f"{k:<58}{med[k]:>10.3f}{min(t):>9.3f}{max(t):>9.3f}{count / med[k] / 1e3:>10.1f}{ratio:>11}")
    spread = max((max(t) - min(t)) / med[k] for k, t in times.items())
    lines.append("")
    lines.append(f"largest (max - min) / median over one row's samples: {100 * spread:.1f} %")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
