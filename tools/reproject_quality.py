"""Quality of temporal accumulation (rt_reproject) and of its parameters, measured on the GPU.

  frames   bunny scene, K frames at 5 spp / 6 bounces, each rendered with frame_index 0, along a small camera dolly
           that ends at the scene's set-up camera (tests/reproject_cases.py dolly: 0.07 units and 0.27 degrees per frame)
  target   a 64-frame progressive accumulation at the last camera, with another seed
  error    RMS difference of the viewer's transform srgb(aces(0.5 c)) over the last camera's hit pixels, three channels
           (pixels whose colour is not finite in the last frame or the target have no error to measure and are left out)

    python tools/reproject_quality.py [--size 1920x1080] [--frames 48] [--out profiles/reproject_quality.txt]

Prints the error of the last frame alone, of that frame denoised (rt_denoise), of the accumulated image and of the
accumulated image denoised, then the accumulated image's error over a grid of max_history, sigma_plane and normal_min,
and last the configuration of tests/test_gpu_reproject.py's sanity test (64x36, 8 frames).
"""
import argparse
import itertools
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as G  # noqa: E402
import reproject_cases as C  # noqa: E402

GRID = {"max_history": (8, 16, 32, 64), "sigma_plane": (0.01, 0.03, 0.1), "normal_min": (0.5, 0.9, 0.99)}
SEED, TARGET_SEED = 0xDEADBEEF, 12345


class Sequence:
    """K frames of the dolly with their records and cameras, kept on the device, and the target at the last camera."""

    def __init__(self, rt, w, h, count):
        self.rt, self.w, self.h = rt, w, h
        self.scene = scene = rt.Scene()
        scene.setup("bunny")
        scene.set_viewport(w, h)
        rng = rt.alloc_rng(w * h)
        rt.init_rng_states(rng, w, h, SEED)
        unused = rt.alloc_surface(w, h)
        self.frames = []
        for k in range(count):
            scene.set_camera(*C.dolly(k, count - 1))
            scene.upload(rng.data_ptr())
            surf = rt.alloc_surface(w, h)
            rt.render(scene, surf, unused, w, h, 5, 6, 0)
            self.frames.append((surf, rt.trace_camera(scene, w, h), scene.camera()))
        rt.init_rng_states(rng, w, h, TARGET_SEED)
        scene.upload(rng.data_ptr())
        bufs = [rt.alloc_surface(w, h), rt.alloc_surface(w, h)]
        for f in range(64):
            rt.render(scene, bufs[f & 1], bufs[(f + 1) & 1], w, h, 5, 6, f)
        self.target = bufs[63 & 1]
        last, hits, _ = self.frames[-1]
        finite = lambda s: torch.isfinite(rt.surface_view(s, w)[..., 0:3]).all(dim=-1)
        hit = (rt.hit_fields(hits)["kind"] != rt.HIT_MISS).reshape(h, w)
        self.dropped = int((hit & ~(finite(last) & finite(self.target))).sum())
        self.mask = hit & finite(last) & finite(self.target)
        self.want = self.display(self.target)
        self.slots = [(rt.alloc_surface(w, h), torch.zeros((h, w), device="cuda")) for _ in range(2)]
        self.denoised = rt.alloc_surface(w, h)

    def display(self, surface):
        x = self.rt.surface_view(surface, self.w)[..., 0:3].double() * 0.5
        x = ((x * (2.51 * x + 0.03)) / (x * (2.43 * x + 0.59) + 0.14)).clamp(0.0, 1.0)
        return torch.where(x <= 0.0031308, 12.92 * x, 1.055 * x.pow(1.0 / 2.4) - 0.055)[self.mask]

    def error(self, surface):
        d = self.display(surface) - self.want
        return float((d * d).mean().sqrt())  # a NaN here would show: the accumulated image must be finite on the mask

    def accumulate(self, **kw):
        """(accumulated surface, history) of all frames through rt_reproject with the filter parameters kw."""
        prev = None
        for k, (surf, hits, cam) in enumerate(self.frames):
            out, hist = self.slots[k & 1]
            self.rt.reproject_raw(surf, hits, cam, self.w, self.h, prev=prev, out=out, out_history=hist, **kw)
            prev = (out, hits, hist, cam)
        return out, hist

    def denoise(self, surface):
        return self.rt.denoise(self.scene, surface, self.w, self.h, hits=self.frames[-1][1], out=self.denoised)


def measure(rt, w, h, count, grid):
    s = Sequence(rt, w, h, count)
    last = s.frames[-1][0]
    acc, hist = s.accumulate()
    rows = {"single": s.error(last), "single_denoised": s.error(s.denoise(last)), "accumulated": s.error(acc),
            "accumulated_denoised": s.error(s.denoise(acc)), "mean_history": float(hist[s.mask].mean()),
            "reset": float((hist[s.mask] <= 1).double().mean())}
    points = []
    if grid:
        for point in itertools.product(*GRID.values()):
            kw = dict(zip(GRID, point))
            points.append((s.error(s.accumulate(**kw)[0]), kw))
    return rows, points, int(s.mask.sum()), s.dropped


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1920x1080", metavar="WxH")
    ap.add_argument("--frames", type=int, default=48, help="frames of the dolly (the grid's largest max_history should not exceed it by much)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "reproject_quality needs a GPU"
    rt = G.load_package()
    torch.cuda.set_device(0)
    w, h = (int(v) for v in args.size.split("x"))
    rows, points, n, dropped = measure(rt, w, h, args.frames, grid=True)
    base = rows["single"]
    best = min(points, key=lambda r: r[0])
    lines = [f"rt_reproject on the GPU ({torch.cuda.get_device_name(0)}): display error (RMS of srgb(aces(0.5 c)) over the {n} hit pixels of the",
             f"last camera) of the bunny scene at {w}x{h}; {args.frames} frames at 5 spp / 6 bounces, frame_index 0 each, along a dolly of 0.07 units and",
             "0.27 degrees per frame, against a 64-frame accumulation at the last camera with another seed",
             f"({dropped} hit pixels whose last-frame or target colour is not finite are left out)", "",
             f"last frame alone                         {base:.4f}",
             f"last frame, rt_denoise (defaults)        {rows['single_denoised']:.4f}  ({rows['single_denoised'] / base:.3f} of the last frame's)",
             f"accumulated, defaults {rt.REPROJECT_DEFAULTS}",
             f"                                         {rows['accumulated']:.4f}  ({rows['accumulated'] / base:.3f})",
             f"accumulated, then rt_denoise (defaults)  {rows['accumulated_denoised']:.4f}  ({rows['accumulated_denoised'] / base:.3f})",
             f"with the defaults the history of a hit pixel holds {rows['mean_history']:.2f} frames on average; {100 * rows['reset']:.2f} % of them hold the last frame only",
             f"best grid point {best[1]}   {best[0]:.4f}",
             f"grid: {len(points)} points, errors {min(r[0] for r in points):.4f} to {max(r[0] for r in points):.4f}", "",
             f"{'max_history':>11}{'sigma_plane':>13} | normal_min " + "".join(f"{v:>9g}" for v in GRID["normal_min"])]
    table = {tuple(kw.values()): e for e, kw in points}
    for mh, sp in itertools.product(GRID["max_history"], GRID["sigma_plane"]):
        lines.append(f"{mh:>11}{sp:>13g} |            " + "".join(f"{table[(mh, sp, nm)]:>9.4f}" for nm in GRID["normal_min"]))
    small, _, n_small, _ = measure(rt, 64, 36, 8, grid=False)
    lines += ["", f"the configuration of tests/test_gpu_reproject.py (64x36, 8 frames, defaults, {n_small} pixels): last frame {small['single']:.4f}, "
              f"accumulated {small['accumulated']:.4f}, ratio {small['accumulated'] / small['single']:.3f}"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
