"""Ordered-hits throughput (rt_trace_hits, csrc/rt_hits.hip) on a benchmark config's scene, HIP events, for K = 1 / 4 /
8 / 16 and for RT_HITS_COUNT_ALL | RT_HITS_CULL_BACK (K = 4), each at 5, 6 and 7 waves per SIMD, with rt_trace_rays on
the same rays beside it in the same process as the yardstick.  Two ray sets:

  (c) the 1920x1080 pixel-centre camera rays;
  (i) 2^20 incoherent rays: from first hits of those, pushed off the surface, uniform random unit directions.

    python tools/hits_timing.py [--config cfg2] [--calls 20] [--batch 2] [--warmup 3] [--out FILE]

A timed sample is `--batch` back-to-back calls between two events, reported per call; all rows are sampled round-robin
(one sample of each per round), so drift hits them alike; the table gives the median and the extremes of the samples and
the ratio of each median to rt_trace_rays' on the same rays.  The ratio is reported, not gated.  Every ray set is also
checked: row 0 of the K = 1 list equals rt_trace_rays' record bytewise, at every occupancy.
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

W, H = 1920, 1080
INCOHERENT = 1 << 20
CASES = [("K = 1", 1, 0), ("K = 4", 4, 0), ("K = 8", 8, 0), ("K = 16", 16, 0), ("K = 4, COUNT_ALL | CULL_BACK", 4, 5)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg2")
    ap.add_argument("--calls", type=int, default=20, help="timed samples per row")
    ap.add_argument("--batch", type=int, default=2, help="calls per timed sample")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    args = ap.parse_args()
    assert args.calls >= 20 and args.batch >= 1, "at least 20 timed samples"
    assert torch.cuda.is_available(), "hits_timing needs a GPU"
    rt = G.load_package()
    scene_name = bench.CONFIGS[args.config][0]
    torch.cuda.set_device(0)
    scene = rt.Scene()
    scene.setup(scene_name)
    scene.set_viewport(W, H)
    scene.upload(0)

    # the camera rays in the kernels' operation order (rt_batch.h query_ray), in numpy: IEEE float32 division, no
    # contraction (a tensor divided by a scalar is multiplied by its reciprocal, which is an ulp off for some pixels)
    F32 = np.float32
    cam = np.frombuffer(bytes(scene.camera()), dtype=F32)
    i = np.arange(W * H)
    ux, uy = (((i % W).astype(F32) + F32(0.5)) / F32(W))[:, None], (((i // W).astype(F32) + F32(0.5)) / F32(H))[:, None]
    rays = np.zeros((W * H, 8), dtype=F32)
    rays[:, 0:3] = cam[0:3]
    rays[:, 3] = rt.RAY_TMAX
    rays[:, 4:7] = ((cam[12:15] + cam[6:9] * ux) + cam[9:12] * uy) - cam[0:3]
    camera = torch.from_numpy(rays).cuda()
    first = rt.trace_rays(scene, camera)
    assert first.cpu().numpy().tobytes() == rt.trace_camera(scene, W, H).cpu().numpy().tobytes()
    f = rt.hit_fields(first)
    valid = torch.nonzero(f["kind"] != rt.HIT_MISS)[:, 0]
    assert valid.numel() > 0
    pick = valid[torch.arange(INCOHERENT, device="cuda") % valid.numel()]
    g = np.random.default_rng(20261021)
    d = g.normal(size=(INCOHERENT, 3))
    incoherent = torch.zeros((INCOHERENT, 8), dtype=torch.float32, device="cuda")
    incoherent[:, 0:3] = f["position"][pick] + f["normal"][pick] * 0.01
    incoherent[:, 3] = rt.RAY_TMAX
    incoherent[:, 4:7] = torch.from_numpy((d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)).cuda()
    sets = {"(c) camera rays": camera, "(i) incoherent rays": incoherent}

    nmax = max(r.shape[0] for r in sets.values())
    hits = torch.empty((nmax * 16 * 12,), dtype=torch.float32, device="cuda")
    counts = torch.empty((nmax,), dtype=torch.int32, device="cuda")
    one = torch.empty((nmax, 12), dtype=torch.float32, device="cuda")
    buf = lambda n, k: hits[:n * k * 12].view(n, k, 12)
    mean_counts = {}
    for name, rays in sets.items():  # the K = 1 contract on every set and at every occupancy; the lists' lengths
        n = rays.shape[0]
        want = rt.trace_rays(scene, rays, hits=one)[:n].cpu().numpy().tobytes()
        for w in (5, 6, 7):
            got, _ = rt.trace_hits(scene, rays, 1, hits=buf(n, 1), counts=counts, waves_per_simd=w)
            assert got.cpu().numpy().tobytes() == want, (name, w)
        _, c = rt.trace_hits(scene, rays, 16, flags=rt.RT_HITS_COUNT_ALL, hits=buf(n, 16), counts=counts)
        mean_counts[name] = (float(c[:n].float().mean()), int(c[:n].max()))

    jobs, base = {}, {}
    for name, rays in sets.items():
        n = rays.shape[0]
        key = f"{name}: rt_trace_rays (default occupancy)"
        jobs[key] = lambda rays=rays: rt.trace_rays(scene, rays, hits=one)
        for label, k, flags in CASES:
            for w in (5, 6, 7):
                row = f"{name}: {label}: {w} waves"
                base[row] = key
                jobs[row] = lambda rays=rays, n=n, k=k, flags=flags, w=w: rt.trace_hits(
                    scene, rays, k, flags=flags, hits=buf(n, k), counts=counts, waves_per_simd=w)
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

    med = {k: float(np.median(t)) for k, t in times.items()}
    lines = [f"ordered hits on {args.config}'s scene ({scene_name}), {W}x{H} camera rays and {INCOHERENT} incoherent rays, "
             f"{torch.cuda.get_device_name(0)}",
             f"HIP events around {args.batch} back-to-back calls per sample (ms per call), {args.warmup} warm-up calls, "
             f"{args.calls} samples per row, rows interleaved",
             "hits below tmax per ray (COUNT_ALL): " + "; ".join(f"{k} mean {v[0]:.2f}, most {v[1]}" for k, v in mean_counts.items()),
             "row 0 of K = 1 == rt_trace_rays' record on every ray of both sets, at 5 / 6 / 7 waves: yes", "",
             f"{'what':<62}{'median ms':>10}{'min ms':>9}{'max ms':>9}{'Mrays/s':>10}{'x trace_rays':>14}"]
    for k, t in times.items():
        n = sets[k.split(":")[0]].shape[0]
        ratio = f"{med[k] / med[base[k]]:>14.2f}" if k in base else f"{'1.00':>14}"
        lines.append(f"{k:<62}{med[k]:>10.3f}{min(t):>9.3f}{max(t):>9.3f}{n / med[k] / 1e3:>10.1f}{ratio}")
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
