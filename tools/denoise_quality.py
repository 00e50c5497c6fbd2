"""Quality of the denoiser's parameters, measured on the CPU: the numpy restatement of rt_denoise
(tests/denoise_ref.py) on frames of the CPU oracle (no GPU needed; the GPU computes the same bytes).

  noisy    bunny scene, 96x54, frame 0 at 5 spp, 6 bounces, the tests' seed
  target   the oracle's 64-frame accumulation of the same scene with seed 12345
  hits     tests/query_ref.py's records of the camera's pixel-centre rays
  error    RMS difference of the viewer's transform srgb(aces(0.5 c)) over hit pixels, three channels

    python tools/denoise_quality.py [--out profiles/denoise_quality.txt]
    python tools/denoise_quality.py --gpu 1920x1080 [--out FILE]

Prints the error of the noisy frame, of the defaults and of every point of a small grid around them.
--gpu WxH measures the same grid at a size a user renders, on the GPU: frames by rt.render (same spp, bounces
and seeds), hits by rt.trace_camera, the filter by rt.denoise, the error in float64 on the device.
"""
import argparse
import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as G  # noqa: E402

W, H = 96, 54
GRID = {"iterations": (3, 4, 5, 6), "normal_power_log2": (3, 5, 7), "sigma_plane": (0.01, 0.03, 0.1), "sigma_color": (0.0, 2.0, 8.0, 32.0)}


def report(title, base, default, defaults, rows, hit_count, out):
    best = min(rows, key=lambda r: r[0])
    lines = title + ["", f"noisy frame                      {base:.4f}",
                     f"defaults {defaults}   {default:.4f}  ({default / base:.3f} of the noisy frame's)",
                     f"best grid point {best[1]}   {best[0]:.4f}",
                     f"grid: {len(rows)} points, errors {min(r[0] for r in rows):.4f} to {max(r[0] for r in rows):.4f}", "",
                     f"{'iterations':>10}{'normal_power_log2':>19}{'sigma_plane':>13} | sigma_color " + "".join(f"{s:>9g}" for s in GRID["sigma_color"])]
    table = {tuple(kw.values()): e for e, kw in rows}
    for it, npw, sp in itertools.product(GRID["iterations"], GRID["normal_power_log2"], GRID["sigma_plane"]):
        lines.append(f"{it:>10}{npw:>19}{sp:>13g} |             " + "".join(f"{table[(it, npw, sp, sc)]:>9.4f}" for sc in GRID["sigma_color"]))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as fh:
            fh.write(text)


def on_gpu(size, out):
    import torch
    import rt_testlib as T
    assert torch.cuda.is_available(), "--gpu needs a GPU"
    rt = G.load_package()
    w, h = (int(v) for v in size.split("x"))
    scene = rt.Scene()
    scene.setup("bunny")
    scene.set_viewport(w, h)
    rng = rt.alloc_rng(w * h)

    def frames(seed, count):
        rt.init_rng_states(rng, w, h, seed)
        scene.upload(rng.data_ptr())
        bufs = [rt.alloc_surface(w, h), rt.alloc_surface(w, h)]
        for f in range(count):
            rt.render(scene, bufs[f & 1], bufs[(f + 1) & 1], w, h, 5, 6, f)
        return bufs[(count - 1) & 1]

    noisy, target = frames(T.SEED, 1), frames(12345, 64)
    hits = rt.trace_camera(scene, w, h)
    hit = (rt.hit_fields(hits)["kind"] != rt.HIT_MISS).reshape(h, w)
    # the renderer leaves a few non-finite pixels (bench.py --dump-outputs lists them); they have no error to measure
    finite = lambda s: torch.isfinite(rt.surface_view(s, w)[..., 0:3]).all(dim=-1)
    dropped = int((hit & ~(finite(noisy) & finite(target))).sum())
    hit = hit & finite(noisy) & finite(target)

    def display(surface):
        x = rt.surface_view(surface, w)[..., 0:3].double() * 0.5
        x = ((x * (2.51 * x + 0.03)) / (x * (2.43 * x + 0.59) + 0.14)).clamp(0.0, 1.0)
        return torch.where(x <= 0.0031308, 12.92 * x, 1.055 * x.pow(1.0 / 2.4) - 0.055)[hit]

    want = display(target)
    err = lambda surface: float(((display(surface) - want) ** 2).mean().sqrt())
    scratch = torch.empty((rt.denoise_scratch_bytes(w, h) // 4,), dtype=torch.float32, device="cuda")
    res = rt.alloc_surface(w, h)
    rows = []
    for point in itertools.product(*GRID.values()):
        kw = dict(zip(GRID, point))
        rows.append((err(rt.denoise(scene, noisy, w, h, hits=hits, out=res, scratch=scratch, **kw)), kw))
    default = err(rt.denoise(scene, noisy, w, h, hits=hits, out=res, scratch=scratch))
    title = [f"rt_denoise parameters on the GPU ({torch.cuda.get_device_name(0)}): display error (RMS of srgb(aces(0.5 c)) over the "
             f"{int(hit.sum())} hit pixels) of the bunny scene at {w}x{h},",
             "frame 0 at 5 spp / 6 bounces against a 64-frame accumulation with another seed; frames by rt.render, filter = rt.denoise",
             f"({dropped} hit pixels whose noisy or accumulated colour is not finite are left out)"]
    report(title, err(noisy), default, rt.DENOISE_DEFAULTS, rows, int(hit.sum()), out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--gpu", default=None, metavar="WxH")
    args = ap.parse_args()
    if args.gpu:
        return on_gpu(args.gpu, args.out)
    G._build_module().build_oracle()
    import denoise_ref as D
    import query_ref as Q
    import rt_testlib as T

    osc = T.OracleScene("bunny")
    noisy = osc.render(W, H, 5, 6, frame_index=0, seed=T.SEED)
    rng = T.oracle_rng_frame(12345, W, H)
    target = None
    for f in range(64):
        target = osc.render(W, H, 5, 6, frame_index=f, rng=rng, last=target)
    arrays = osc.arrays()
    hits, _, _ = Q.trace(arrays, Q.camera_rays(osc.camera(W, H), W, H))
    mats = arrays["materials"].view(np.float32).reshape(-1, 16)
    hit = (hits.view(np.uint32)[:, 1] != 0).reshape(H, W)
    err = lambda img: D.display_error(img, target, hit)
    base = err(noisy)
    rows = []
    for point in itertools.product(*GRID.values()):
        kw = dict(zip(GRID, point))
        rows.append((err(D.denoise(noisy, hits, mats, **kw)), kw))
    default = err(D.denoise(noisy, hits, mats, **D.DEFAULTS))
    title = [f"rt_denoise parameters: display error (RMS of srgb(aces(0.5 c)) over the {int(hit.sum())} hit pixels) of the bunny scene at "
             f"{W}x{H},", "frame 0 at 5 spp / 6 bounces against the oracle's 64-frame accumulation with another seed; filter = tests/denoise_ref.py (CPU)"]
    report(title, base, default, D.DEFAULTS, rows, int(hit.sum()), args.out)


if __name__ == "__main__":
    main()
