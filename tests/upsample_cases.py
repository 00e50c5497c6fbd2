"""Hand-made inputs for the upsampler's tests (tests/upsample_ref.py, rt_upsample), built from denoise_cases: a low
frame with its records and the records of the output size as numpy arrays, no scene needed."""
import numpy as np

import denoise_cases as C

F32 = np.float32


def sample_points(low_width, low_height, scale):
    """The output pixel (s*x + s//2, s*y + s//2) each low pixel (x, y) is taken from: ([h, w] rows, [h, w] columns)."""
    ys, xs = np.meshgrid(np.arange(low_height), np.arange(low_width), indexing="ij")
    return scale * ys + scale // 2, scale * xs + scale // 2


def downsample(frame, hits, low_width, low_height, scale):
    """(low frame, low records): the output-size frame [H, W, 4] and records [H*W, 12] at sample_points."""
    py, px = sample_points(low_width, low_height, scale)
    width = low_width * scale
    return frame[py, px].copy(), hits[(py * width + px).reshape(-1)].copy()


def synthetic(low_width, low_height, scale, seed=1):
    """An adversarial pair: (low_surface [h, w, 4], low_hits [h*w, 12], hits [H*W, 12], materials [M, 16]).

    denoise_cases.synthetic(W, H, seed) is the output-size frame and its records; the low frame and records are those
    of sample_points, but a random 20 % of the low pixels take their record from a second synthetic(W, H, seed + 1000)
    instead: other misses, materials and normals on the same position grid, so that low pixels disagree with the
    output pixels around them and all three stages of the upsampler decide pixels."""
    width, height = low_width * scale, low_height * scale
    frame, hits, materials = C.synthetic(width, height, seed)
    _, other, _ = C.synthetic(width, height, seed + 1000)
    low_surface, low_hits = downsample(frame, hits, low_width, low_height, scale)
    _, low_other = downsample(frame, other, low_width, low_height, scale)
    swap = np.random.default_rng(seed + 2000).random(low_width * low_height) < 0.2
    low_hits[swap] = low_other[swap]
    return low_surface, low_hits, hits, materials


def constant(colour, low_width, low_height, alpha=1.0):
    low = np.empty((low_height, low_width, 4), dtype=F32)
    low[..., 0:3], low[..., 3] = colour, alpha
    return low
