"""Quality of rendering small and upsampling (rt_upsample), measured on the GPU against a converged full-size frame.

  scene    bunny, output 1920x1080 (--size), 6 bounces; frames by rt.render, records by rt.trace_camera
  target   a 64-frame accumulation at 5 spp of the output size, seed 12345
  error    tests/denoise_ref.py's display_error: RMS difference of srgb(aces(0.5 c)) over the hit pixels, three channels
  budget   k = --spp paths per *output* pixel: the full-size frame has k spp, the low frame of scale S has k * S * S

  for each scale S = 2, 3, 4, at the same number of paths:
    (a) full size at k spp + rt_denoise
    (b) low size at k*S*S spp + rt_denoise + rt_upsample
    (c) as (b) with plain bilinear interpolation (torch.nn.functional.interpolate) in rt_upsample's place
    (d) low size at k*S*S spp, no denoiser, + rt_upsample
  and (b) on the grid sigma_plane x normal_power_log2 that picks rt_upsample's defaults.  Every figure is given over
  all hit pixels and over the edge pixels alone: the hit pixels one of whose neighbours 4 output pixels away (the
  largest scale) is a miss, has another material or a normal more than 25 degrees off.  The filter parameters act only
  where the low pixels around an output pixel disagree with it, so the defaults are the grid point with the lowest
  mean error over the three scales on the edge pixels.

    python tools/upsample_quality.py [--size 1920x1080] [--spp 1] [--out profiles/upsample_quality.txt]
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

SCALES = (2, 3, 4)
BOUNCES = 6
GRID = {"sigma_plane": (0.003, 0.01, 0.03, 0.1, 0.3), "normal_power_log2": (0, 3, 5, 7)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--spp", type=int, default=1, help="paths per output pixel")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import rt_testlib as T
    assert torch.cuda.is_available(), "upsample_quality needs a GPU"
    rt = G.load_package()
    W, H = (int(v) for v in args.size.split("x"))
    k = args.spp

    def frames(w, h, seed, spp, count):
        """(scene uploaded for w x h, the accumulation of `count` frames at `spp`); each size has a scene of its own"""
        scene = rt.Scene()
        scene.setup("bunny")
        scene.set_viewport(w, h)
        rng = rt.alloc_rng(w * h)
        rt.init_rng_states(rng, w, h, seed)
        scene.upload(rng.data_ptr())
        bufs = [rt.alloc_surface(w, h), rt.alloc_surface(w, h)]
        for f in range(count):
            rt.render(scene, bufs[f & 1], bufs[(f + 1) & 1], w, h, spp, BOUNCES, f)
        torch.cuda.synchronize()
        return scene, rng, bufs[(count - 1) & 1]

    _, _, target = frames(W, H, 12345, 5, 64)
    scene, rng, noisy = frames(W, H, T.SEED, k, 1)
    hits = rt.trace_camera(scene, W, H)
    finite = lambda s: torch.isfinite(rt.surface_view(s, W)[..., 0:3]).all(dim=-1)
    hit = (rt.hit_fields(hits)["kind"] != rt.HIT_MISS).reshape(H, W) & finite(target)

    def display(surface):
        x = rt.surface_view(surface, W)[..., 0:3].double() * 0.5
        x = ((x * (2.51 * x + 0.03)) / (x * (2.43 * x + 0.59) + 0.14)).clamp(0.0, 1.0)
        return torch.where(x <= 0.0031308, 12.92 * x, 1.055 * x.pow(1.0 / 2.4) - 0.055)

    f = rt.hit_fields(hits)
    kind, material, normal = f["kind"].reshape(H, W), f["material"].reshape(H, W), f["normal"].reshape(H, W, 3)
    edge = torch.zeros_like(hit)
    for dy, dx in ((0, 4), (0, -4), (4, 0), (-4, 0)):
        k2, m2, n2 = (torch.roll(v, (dy, dx), (0, 1)) for v in (kind, material, normal))
        edge |= (k2 == rt.HIT_MISS) | (m2 != material) | ((normal * n2).sum(-1) < 0.9)
    edge &= hit
    shown = display(target)

    def err(surface):
        d = torch.nan_to_num(display(surface), nan=1.0, posinf=1.0, neginf=0.0)  # a pixel that is not finite displays as white
        d = ((d - shown) ** 2).sum(-1)
        return tuple(float((d[m].sum() / (3 * m.sum())).sqrt()) for m in (hit, edge))

    two = lambda e: f"{e[0]:.5f} {e[1]:.5f}"
    lines = [f"rt_upsample quality on the GPU ({torch.cuda.get_device_name(0)}): display error (RMS of srgb(aces(0.5 c)) over the "
             f"{int(hit.sum())} hit pixels",
             f"whose target is finite) of the bunny scene at {W}x{H}, {BOUNCES} bounces, against a 64-frame accumulation at 5 spp with another seed;",
             f"every row of a scale traces the same number of paths: {k} per output pixel; each figure over all hit pixels, then over the "
             f"{int(edge.sum())} edge pixels",
             "command: python tools/upsample_quality.py " + " ".join(sys.argv[1:]), "",
             f"full size, {k} spp, unfiltered                         " + two(err(noisy))]
    a = err(rt.denoise(scene, noisy, W, H, hits=hits))
    lines += [f"(a) full size, {k} spp + rt_denoise                     " + two(a), ""]
    grid = {}
    for s in SCALES:
        assert W % s == 0 and H % s == 0
        lw, lh = W // s, H // s
        low_scene, low_rng, low = frames(lw, lh, T.SEED, k * s * s, 1)
        low_hits = rt.trace_camera(low_scene, lw, lh)
        hits_s = rt.trace_camera(low_scene, W, H)  # the low scene's camera at the output size
        low_filtered = rt.denoise(low_scene, low, lw, lh, hits=low_hits)
        up = lambda surf, **kw: rt.upsample(low_scene, surf, lw, lh, s, low_hits=low_hits, hits=hits_s, **kw)
        b = err(up(low_filtered))
        d = err(up(low))
        img = rt.surface_view(low_filtered, lw).permute(2, 0, 1)[None]
        bil = torch.nn.functional.interpolate(img, size=(H, W), mode="bilinear", align_corners=False)[0].permute(1, 2, 0)
        plain = rt.alloc_surface(W, H)
        rt.surface_view(plain, W).copy_(bil)
        c = err(plain)
        lines += [f"scale {s}: low {lw}x{lh} at {k * s * s} spp",
                  f"  (b) rt_denoise + rt_upsample (defaults)              {two(b)}  ({b[0] / a[0]:.3f} and {b[1] / a[1]:.3f} of (a))",
                  f"  (c) rt_denoise + bilinear interpolation              {two(c)}",
                  f"  (d) rt_upsample alone                                {two(d)}"]
        for point in itertools.product(*GRID.values()):
            grid[(s,) + point] = err(up(low_filtered, **dict(zip(GRID, point))))
    means = {}
    for which, name in ((0, "all hit pixels"), (1, "the edge pixels")):
        lines += ["", f"(b) on the grid over {name}; rows sigma_plane, columns normal_power_log2 x scale, and the mean over the scales",
                  f"{'sigma_plane':>12} | " + " | ".join("".join(f"{'n%d x%d' % (npw, s):>9}" for s in SCALES) + f"{'mean':>9}"
                                                         for npw in GRID["normal_power_log2"])]
        for sp in GRID["sigma_plane"]:
            cells = []
            for npw in GRID["normal_power_log2"]:
                e = [grid[(s, sp, npw)][which] for s in SCALES]
                means[(which, sp, npw)] = sum(e) / len(e)
                cells.append("".join(f"{v:>9.5f}" for v in e) + f"{means[(which, sp, npw)]:>9.5f}")
            lines.append(f"{sp:>12g} | " + " | ".join(cells))
    dflt = (rt.UPSAMPLE_DEFAULTS["sigma_plane"], rt.UPSAMPLE_DEFAULTS["normal_power_log2"])
    for which, name in ((0, "all hit pixels"), (1, "the edge pixels")):
        of = {k[1:]: v for k, v in means.items() if k[0] == which}
        best = min(of, key=of.get)
        lines += ["", f"{name}: best grid point sigma_plane {best[0]:g}, normal_power_log2 {best[1]}: mean {of[best]:.5f}; "
                      f"the defaults (sigma_plane {dflt[0]:g}, normal_power_log2 {dflt[1]}): {of.get(dflt, float('nan')):.5f}; "
                      f"worst point {max(of.values()):.5f}"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
