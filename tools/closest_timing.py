"""Closest-point query throughput (rt_closest_point, csrc/rt_closest.hip) on a benchmark config's scene, HIP events, at
5, 6 and 7 waves per SIMD, with rt_trace_rays on as many camera rays beside it as a yardstick.  2^20 points of three
kinds, each at radius inf and at 1 % of the root box's diagonal:

  (u) uniform in the scene's root box;
  (s) on the surface: the hit positions of rt_trace_rays' camera mode at the config's frame size;
  (f) far outside: 2 to 8 box diagonals from the box's centre.

    python tools/closest_timing.py [--config cfg2] [--calls 20] [--batch 2] [--warmup 3] [--points 1048576] [--out FILE]

A timed sample is `--batch` back-to-back calls between two events, reported per call; all rows are sampled round-robin
(one sample of each per round), so drift hits them alike; the table gives the median and the extremes of the samples.
Every batch is also checked: a 4096-point subsample of its records equals rt_closest_point_host's, bytewise.
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

CHECKED = 4096


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg2")
    ap.add_argument("--calls", type=int, default=20, help="timed samples per row")
    ap.add_argument("--batch", type=int, default=2, help="calls per timed sample")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--points", type=int, default=1 << 20)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    args = ap.parse_args()
    assert args.calls >= 20 and args.batch >= 1, "at least 20 timed samples"
    assert torch.cuda.is_available(), "closest_timing needs a GPU"
    rt = G.load_package()
    scene_name, W, H, _, _, _ = bench.CONFIGS[args.config]
    torch.cuda.set_device(0)
    scene = rt.Scene()
    scene.setup(scene_name)
    scene.set_viewport(W, H)
    scene.upload(0)
    n = args.points
    nodes = scene.host_arrays()["nodes"].view(np.float32).reshape(-1, 8)
    lo, hi = nodes[0, 0:3].astype(np.float64), nodes[0, 3:6].astype(np.float64)
    diag = float(np.linalg.norm(hi - lo))
    g = np.random.default_rng(20251021)

    records = rt.trace_camera(scene, W, H)
    f = rt.hit_fields(records)
    valid = torch.nonzero(f["kind"] != rt.HIT_MISS)[:, 0]
    assert valid.numel() > 0
    d = g.normal(size=(n, 3))
    kinds = {
        "(u) uniform in the box": torch.from_numpy(g.uniform(lo, hi, size=(n, 3)).astype(np.float32)).cuda(),
        "(s) on the surface": f["position"][valid[torch.arange(n, device="cuda") % valid.numel()]].contiguous(),
        "(f) far outside": torch.from_numpy(((lo + hi) * 0.5 + d / np.linalg.norm(d, axis=1, keepdims=True)
                                             * diag * g.uniform(2.0, 8.0, size=(n, 1))).astype(np.float32)).cuda(),
    }
    batches = {}
    for name, pos in kinds.items():
        for label, radius in (("radius inf", float("inf")), ("radius 1 % of the diagonal", 0.01 * diag)):
            p = torch.empty((n, 4), dtype=torch.float32, device="cuda")
            p[:, 0:3] = pos
            p[:, 3] = radius
            batches[f"{name}, {label}"] = p
    out = torch.empty((n, 8), dtype=torch.float32, device="cuda")
    share = {}
    sub = torch.from_numpy(g.choice(n, size=min(CHECKED, n), replace=False)).cuda()
    for name, p in batches.items():  # the contract, on a subsample of every batch and at every occupancy
        want = rt.closest_points_host(scene, p[sub].cpu().numpy())
        for w in (5, 6, 7):
            got = rt.closest_points(scene, p, out=out, waves_per_simd=w)[sub].cpu().numpy()
            assert got.tobytes() == want.tobytes(), (name, w)
        share[name] = float((rt.nearest_fields(out)["kind"] != 0).float().mean())

    rays = torch.zeros((n, 8), dtype=torch.float32, device="cuda")
    cam = torch.from_numpy(np.frombuffer(bytes(scene.camera()), dtype=np.float32).copy()).cuda()
    i = torch.arange(n, device="cuda") % (W * H)
    ux, uy = (((i % W).float() + 0.5) / float(W))[:, None], (((i // W).float() + 0.5) / float(H))[:, None]
    rays[:, 0:3] = cam[0:3]
    rays[:, 3] = rt.RAY_TMAX
    rays[:, 4:7] = ((cam[12:15] + cam[6:9] * ux) + cam[9:12] * uy) - cam[0:3]
    hits = torch.empty((n, 12), dtype=torch.float32, device="cuda")

    jobs = {}
    for name, p in batches.items():
        for w in (5, 6, 7):
            jobs[f"{name}: {w} waves"] = lambda p=p, w=w: rt.closest_points(scene, p, out=out, waves_per_simd=w)
    for w in (5, 6, 7):
        jobs[f"rt_trace_rays, camera rays: {w} waves"] = lambda w=w: rt.trace_rays(scene, rays, hits=hits, waves_per_simd=w)
    times = {k: [] for k in jobs}
    for fn in jobs.values():
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

    lines = [f"closest-point queries on {args.config}'s scene ({scene_name}), {n} points, {torch.cuda.get_device_name(0)}",
             f"HIP events around {args.batch} back-to-back calls per sample (ms per call), {args.warmup} warm-up calls, "
             f"{args.calls} samples per row, rows interleaved",
             "answered share: " + "; ".join(f"{k} {100 * v:.1f} %" for k, v in share.items()),
             f"rt_closest_point == rt_closest_point_host on {sub.numel()} points of every batch, at 5 / 6 / 7 waves: yes", "",
             f"{'what':<62}{'median ms':>10}{'min ms':>9}{'max ms':>9}{'Mpoints/s':>11}"]
    for k, t in times.items():
        m = float(np.median(t))
        lines.append(f"{k:<62}{m:>10.3f}{min(t):>9.3f}{max(t):>9.3f}{n / m / 1e3:>11.1f}")
    spread = max((max(t) - min(t)) / float(np.median(t)) for t in times.values())
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
