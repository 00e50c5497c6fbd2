"""Quality of the variance-steered filter (rt_moments, rt_reproject on the moments, rt_denoise_variance) and of its two
parameters, measured on the GPU with exactly the protocol of tools/reproject_quality.py: the same dolly, seeds, target
and metric (its Sequence class is used as it is).

    python tools/variance_quality.py [--size 1920x1080] [--frames 48] [--out profiles/variance_quality.txt]

Prints the display error of the last frame alone, of the accumulated image, of the accumulated image through
rt_denoise (these three reproduce profiles/reproject_quality.txt) and through rt_denoise_variance; the same four over
the pixels whose history is shorter than 4 frames (disocclusions) and over those with 16 frames and more (converged);
the grid over sigma_lum and min_history, whose best point (over all hit pixels; ties at the printed precision are
broken by the same grid on the short sequence of tests/test_gpu_variance.py's quality test, 64x36 and 8 frames) is what
the four numbers are reported for and what the library's defaults are set to; how many lanes take the spatial
estimate; and last that short configuration for three seeds.
"""
import argparse
import itertools
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import __graft_entry__ as G  # noqa: E402
import reproject_quality as RQ  # noqa: E402

GRID = {"sigma_lum": (1.0, 2.0, 4.0, 8.0, 16.0), "min_history": (1.0, 2.0, 4.0, 8.0, 16.0)}


class Chain(RQ.Sequence):
    """The sequence with, on top of the accumulated colour, the accumulated moments of the last frame."""

    def __init__(self, rt, w, h, count):
        super().__init__(rt, w, h, count)
        self.moment_slots = [(rt.alloc_surface(w, h), torch.zeros((h, w), device="cuda")) for _ in range(2)]
        self.frame_moments = rt.alloc_surface(w, h)
        self.filtered = rt.alloc_surface(w, h)
        self.variance = torch.zeros((h, w), device="cuda")
        self.scratch = torch.empty((rt.denoise_variance_scratch_bytes(w, h) // 4,), device="cuda")
        self.hit = (rt.hit_fields(self.frames[-1][1])["kind"] != rt.HIT_MISS).reshape(h, w)

    def accumulate_moments(self):
        prev = None
        for k, (surf, hits, cam) in enumerate(self.frames):
            out, hist = self.moment_slots[k & 1]
            self.rt.moments(self.scene, surf, hits, self.w, self.h, out=self.frame_moments)
            self.rt.reproject_raw(self.frame_moments, hits, cam, self.w, self.h, prev=prev, out=out, out_history=hist)
            prev = (out, hits, hist, cam)
        return out

    def filter(self, acc, moments, hist, **kw):
        self.rt.denoise_variance(self.scene, acc, self.w, self.h, hits=self.frames[-1][1], moments=moments, history=hist,
                                 out=self.filtered, out_variance=self.variance, scratch=self.scratch, **kw)
        return self.filtered

    def error_over(self, surface, sub):
        """The display error over the pixels of self.mask that are also in `sub` ([H, W] bool)."""
        d = (self.display(surface) - self.want)[sub[self.mask]]
        return float((d * d).mean().sqrt()) if d.numel() else float("nan")


def best_point(points, tie_break=None):
    """The grid point with the lowest error over all hit pixels, compared at the four decimals the record prints;
    among the points that tie there, the one `tie_break` ({(sigma_lum, min_history): error}) rates lowest."""
    lowest = min(round(r[0], 4) for r in points)
    tied = [r for r in points if round(r[0], 4) == lowest]
    if tie_break is None:
        return min(tied, key=lambda r: r[0]), tied
    return min(tied, key=lambda r: tie_break[(r[3]["sigma_lum"], r[3]["min_history"])]), tied


def measure(rt, w, h, count, params=None, seed=None, tie_break=None):
    """params None: run the grid and report its best point (best_point); else report `params` (sigma_lum, min_history)."""
    if seed is not None:
        RQ.SEED = seed
    s = Chain(rt, w, h, count)
    last = s.frames[-1][0]
    acc, hist = s.accumulate()
    moments = s.accumulate_moments()
    everything = torch.ones_like(s.mask)
    subsets = {"all": everything, "short": hist < 4, "long": hist >= 16}
    points = []
    if params is None:
        for point in itertools.product(*GRID.values()):
            kw = dict(zip(GRID, point))
            f = s.filter(acc, moments, hist, **kw)
            points.append((s.error_over(f, everything), s.error_over(f, subsets["short"]), s.error_over(f, subsets["long"]), kw))
        params = best_point(points, tie_break)[0][3]
    rows = {"params": params}
    for name, sub in subsets.items():
        rows[name] = {"n": int((s.mask & sub).sum()), "single": s.error_over(last, sub), "accumulated": s.error_over(acc, sub),
                      "denoised": s.error_over(s.denoise(acc), sub), "variance": s.error_over(s.filter(acc, moments, hist, **params), sub)}
    rows["mean_history"] = float(hist[s.mask].mean())
    # lanes on the spatial estimate: valid, finite pixels whose history is below min_history (the default's), now and
    # on a first frame (every one of them)
    dflt = params["min_history"]
    rows["spatial_share"] = float((hist[s.hit] < dflt).double().mean())
    blocks = (hist < dflt) & s.hit
    bh, bw = (h + 7) // 8 * 8, (w + 31) // 32 * 32
    padded = torch.zeros((bh, bw), dtype=torch.bool, device="cuda")
    padded[:h, :w] = blocks
    rows["spatial_blocks"] = float(padded.reshape(bh // 8, 8, bw // 32, 32).any(dim=3).any(dim=1).double().mean())
    rows["mean_variance"] = float(s.variance[s.mask].mean())
    return rows, points, s.dropped


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1920x1080", metavar="WxH")
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "variance_quality needs a GPU"
    rt = G.load_package()
    torch.cuda.set_device(0)
    w, h = (int(v) for v in args.size.split("x"))
    # the short sequence of tests/test_gpu_variance.py first: its grid breaks the ties of the long one
    _, short_points, _ = measure(rt, 64, 36, 8)
    short_table = {(r[3]["sigma_lum"], r[3]["min_history"]): r[0] for r in short_points}
    rows, points, dropped = measure(rt, w, h, args.frames, tie_break=short_table)
    best, tied = best_point(points, short_table)
    d = rows["params"]  # the best grid point: what the library's defaults are set to
    lines = [f"rt_denoise_variance on the GPU ({torch.cuda.get_device_name(0)}): display error (RMS of srgb(aces(0.5 c)) over the hit pixels of the",
             f"last camera) of the bunny scene at {w}x{h}; {args.frames} frames at 5 spp / 6 bounces, frame_index 0 each, along a dolly of 0.07 units and",
             "0.27 degrees per frame, against a 64-frame accumulation at the last camera with another seed: the protocol of",
             f"profiles/reproject_quality.txt ({dropped} hit pixels whose last-frame or target colour is not finite are left out).",
             f"rt_reproject with its defaults {rt.REPROJECT_DEFAULTS}; mean history {rows['mean_history']:.2f} frames.",
             f"rt_denoise_variance with sigma_lum {d['sigma_lum']:g}, min_history {d['min_history']:g} (the best grid point, below: the library's defaults).", "",
             f"{'':<44}{'all hit pixels':>16}{'history < 4':>16}{'history >= 16':>16}",
             f"{'pixels':<44}" + "".join(f"{rows[k]['n']:>16}" for k in ("all", "short", "long"))]
    for key, label in (("single", "last frame alone"), ("accumulated", "accumulated"), ("denoised", "accumulated, then rt_denoise (defaults)"),
                       ("variance", "accumulated, then rt_denoise_variance")):
        lines.append(f"{label:<44}" + "".join(f"{rows[k][key]:>16.4f}" for k in ("all", "short", "long")))
    bar, got = rows["all"]["denoised"], rows["all"]["variance"]
    lines += ["", f"the bar, accumulated then rt_denoise (defaults): {bar:.4f}; rt_denoise_variance: {got:.4f} = {got / bar:.3f} of the bar "
              f"({'below' if got < bar else 'NOT below'} it)",
              f"mean filtered variance of the albedo-divided luminance over the hit pixels: {rows['mean_variance']:.3g}",
              f"lanes on the 7x7 spatial estimate at the last frame (history < {d['min_history']:g}): {100 * rows['spatial_share']:.2f} % of the hit pixels, in "
              f"{100 * rows['spatial_blocks']:.2f} % of the 32x8 blocks; on a first frame every hit pixel", "",
              f"best grid point: sigma_lum {best[3]['sigma_lum']:g}, min_history {best[3]['min_history']:g}   {best[0]:.4f} over all hit pixels",
              f"  (the lowest error over all hit pixels at the four decimals printed; {len(tied)} points tie there, and among them the lowest error of",
              "  the short sequence's grid, the last table, decides: 8 frames at 64x36, where the histories are still short)",
              f"grid: {len(points)} points, errors {min(r[0] for r in points):.4f} to {max(r[0] for r in points):.4f}", ""]
    for title, idx, pts in (("all hit pixels", 0, points), ("history < 4", 1, points), ("history >= 16", 2, points),
                            ("64x36, 8 frames", 0, short_points)):
        table = {(kw["sigma_lum"], kw["min_history"]): r[idx] for r in pts for kw in [r[3]]}
        lines.append(f"{title + ':':<16}sigma_lum | min_history " + "".join(f"{v:>9g}" for v in GRID["min_history"]))
        for sl in GRID["sigma_lum"]:
            lines.append(f"{'':<16}{sl:>9g} |             " + "".join(f"{table[(sl, mh)]:>9.4f}" for mh in GRID["min_history"]))
        lines.append("")
    lines.append("the configuration of tests/test_gpu_variance.py (64x36, 8 frames, the same parameters), three seeds of the frames:")
    for seed in (0xDEADBEEF, 1, 2):
        small, _, small_dropped = measure(rt, 64, 36, 8, params=d, seed=seed)
        a = small["all"]
        lines.append(f"  seed {seed:#x}: {a['n']} pixels ({small_dropped} dropped), last frame {a['single']:.4f}, accumulated {a['accumulated']:.4f}, then rt_denoise "
                     f"{a['denoised']:.4f}, then rt_denoise_variance {a['variance']:.4f} = {a['variance'] / a['accumulated']:.3f} of accumulated, "
                     f"{a['variance'] / a['denoised']:.3f} of rt_denoise's")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
