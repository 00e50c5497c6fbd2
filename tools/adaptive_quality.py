"""Quality of adaptive sampling (AdaptiveSampler: rt_sample_priority + rt_sample_plan + rt_sample_pixels) against uniform
sampling at equal budgets, measured on the GPU.

  scenes   config 2's scene (bunny) and tests/scene_cases.py room_open_sky, both at --size (default 480x270), 6 bounces
  target   a uniform round of 2048 samples a pixel with another seed
  error    RMS difference of the viewer's transform srgb(aces(0.5 c)) over the pixels whose colour is finite in both
           images, three channels (tools/reproject_quality.py's display error), averaged over --seeds seeds
  budget   --spp samples a pixel in total: uniform = warmup(spp); adaptive = warmup(w), then two steps of (spp - w) / 2
           each, over a grid of scale, max_samples and w.  A plan never spends more than its budget and rarely all of
           it (rt_abi.h: what the rounding and the cap leave over is not redistributed), so each row states the
           samples it really took.

    python tools/adaptive_quality.py [--size 480x270] [--spp 8] [--seeds 3] [--out profiles/adaptive_quality.txt]
"""
import argparse
import itertools
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as G  # noqa: E402
import scene_cases as C  # noqa: E402

GRID = {"scale": (2.0 ** 10, 2.0 ** 16, 2.0 ** 19, 2.0 ** 22, 2.0 ** 25, 2.0 ** 28), "max_samples": (16, 64), "warmup": (2, 4)}
BOUNCES, TARGET_SPP, TARGET_SEED, SEED = 6, 2048, 12345, 0xDEADBEEF


def display(rt, surface, w):
    x = rt.surface_view(surface, w)[..., 0:3].double() * 0.5
    x = ((x * (2.51 * x + 0.03)) / (x * (2.43 * x + 0.59) + 0.14)).clamp(0.0, 1.0)
    return torch.where(x <= 0.0031308, 12.92 * x, 1.055 * x.pow(1.0 / 2.4) - 0.055)


def scenes(rt, w, h):
    s = rt.Scene()
    s.setup("bunny")
    s.set_viewport(w, h)
    s.upload(0)
    yield "config 2's scene (bunny)", s
    case = dict(C.BY_NAME["room_open_sky"], width=w, height=h)
    s = C.apply_product(rt, case)
    s.upload(0)
    yield "room_open_sky", s


def measure(rt, name, scene, w, h, spp, seeds, lines):
    target = rt.AdaptiveSampler(scene, w, h, bounces=BOUNCES, seed=TARGET_SEED)
    target.warmup(TARGET_SPP)
    want = display(rt, target.image(), w)
    finite_want = torch.isfinite(want).all(dim=-1)

    def error(sampler):
        got = display(rt, sampler.image(), w)
        mask = finite_want & torch.isfinite(got).all(dim=-1)
        d = (got - want)[mask]
        return float((d * d).mean().sqrt()), float(sampler.counts().sum()) / (w * h), float(sampler.counts().max())

    def mean(rows):
        return tuple(float(np.mean(c)) for c in zip(*rows))

    uniform = {}
    for u in sorted({spp, spp // 2, spp - 1}):
        rows = []
        for k in range(seeds):
            s = rt.AdaptiveSampler(scene, w, h, bounces=BOUNCES, seed=SEED + k)
            s.warmup(u)
            rows.append(error(s))
        uniform[u] = mean(rows)
    points = []
    for scale, max_samples, warm in itertools.product(*GRID.values()):
        rows = []
        for k in range(seeds):
            s = rt.AdaptiveSampler(scene, w, h, bounces=BOUNCES, seed=SEED + k)
            s.warmup(warm)
            for _ in range(2):
                s.step((spp - warm) / 2.0, max_samples=max_samples, scale=scale)
            rows.append(error(s))
        points.append((mean(rows), scale, max_samples, warm))
    torch.cuda.synchronize()
    lines.append(f"{name}, {w}x{h}, {BOUNCES} bounces, target {TARGET_SPP} spp, mean of {seeds} seeds")
    lines.append(f"{'what':<52}{'error':>9}{'spp taken':>11}{'most a pixel':>14}")
    for u, (e, took, most) in uniform.items():
        lines.append(f"{'uniform ' + str(u) + ' spp':<52}{e:>9.5f}{took:>11.3f}{most:>14.1f}")
    for (e, took, most), scale, max_samples, warm in points:
        what = f"adaptive scale 2^{int(np.log2(scale))} max_samples {max_samples} warmup {warm}"
        lines.append(f"{what:<52}{e:>9.5f}{took:>11.3f}{most:>14.1f}")
    best = min(points)
    lines.append(f"best of the grid: scale 2^{int(np.log2(best[1]))}, max_samples {best[2]}, warmup {best[3]}: error {best[0][0]:.5f} with "
                 f"{best[0][1]:.3f} spp against uniform {spp} spp {uniform[spp][0]:.5f} "
                 f"({'better' if best[0][0] < uniform[spp][0] else 'NOT better'} than uniform at the full budget)")
    lines.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="480x270")
    ap.add_argument("--spp", type=int, default=8, help="the total budget, samples a pixel")
    ap.add_argument("--seeds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    w, h = (int(v) for v in args.size.split("x"))
    assert torch.cuda.is_available(), "adaptive_quality needs a GPU"
    rt = G.load_package()
    torch.cuda.set_device(0)
    lines = [f"adaptive against uniform sampling on the GPU ({torch.cuda.get_device_name(0)}): display error (RMS of srgb(aces(0.5 c)), "
             f"three channels) against a {TARGET_SPP} spp target, budget {args.spp} spp", ""]
    for name, scene in scenes(rt, w, h):
        measure(rt, name, scene, w, h, args.spp, args.seeds, lines)
    text = "\n".join(lines)
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
