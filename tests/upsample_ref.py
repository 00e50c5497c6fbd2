"""Reference for rt_upsample (include/rt_abi.h, csrc/upsample.hip): the upsampler restated in numpy, fp32 throughout.

As in denoise_ref.py every product, sum, difference and quotient is a single numpy float32 operation (no contraction,
IEEE division), dot products are summed in rtm::dot's order, fmaxf is np.fmax, and a tap's contribution is masked with
`w > 0` rather than added as a zero.  One vectorised step per tap, the taps in the kernel's order: j outer, i inner.
The GPU tests compare bytewise against this.

upsample(low_surface, low_hits, hits, materials, scale, ...) -> ([H, W, 4] float32, [H, W] int: the deciding stage)
    low_surface [h, w, 4] float32, the low frame; H, W = scale * h, scale * w
    low_hits    [h*w, 12] float32 rt_hit rows of the low size, record y*w + x
    hits        [H*W, 12] float32 rt_hit rows of the output size
    materials   [M, 16] float32 GPUMaterial rows (albedo in words 0-2); M may be 0
The stage of an output pixel: 1 the bilinear footprint, 2 the 4 x 4 footprint, 3 the nearest low pixel.
"""
import numpy as np

from denoise_ref import F32, albedo, dot, finite3

DEFAULTS = {"normal_power_log2": 0, "sigma_plane": 0.03}


def tags(hits, materials, height, width):
    """0 for a miss, 1 for a hit whose material index is beyond the table, material + 2 otherwise; [H, W] int64."""
    hu = np.ascontiguousarray(hits, dtype=F32).view(np.uint32).reshape(height, width, 12)
    count = np.asarray(materials, dtype=F32).reshape(-1, 16).shape[0]
    material = hu[..., 3].astype(np.int64)
    return np.where(hu[..., 1] == 0, 0, np.where(material < count, material + 2, 1))


def footprint(coords, s):
    """Output coordinates -> (the first low coordinate of the bilinear footprint, the weights of its two taps)."""
    i = 2 * coords + 1 - s
    first = i // (2 * s)  # floor division
    t = (i - 2 * s * first).astype(F32) / F32(2 * s)
    return first, (F32(1) - t, t)


def upsample(low_surface, low_hits, hits, materials, scale, normal_power_log2=DEFAULTS["normal_power_log2"],
             sigma_plane=DEFAULTS["sigma_plane"]):
    low_surface = np.ascontiguousarray(low_surface, dtype=F32)
    lh, lw = low_surface.shape[0:2]
    s = int(scale)
    height, width = lh * s, lw * s
    assert low_surface.shape == (lh, lw, 4) and s in (2, 3, 4)
    assert 0 <= normal_power_log2 <= 8 and sigma_plane > 0
    low_hits = np.ascontiguousarray(low_hits, dtype=F32).reshape(lh, lw, 12)
    hits = np.ascontiguousarray(hits, dtype=F32).reshape(height, width, 12)
    tag_q, tag_p = tags(low_hits, materials, lh, lw), tags(hits, materials, height, width)
    n_q, pos_q = low_hits[..., 4:7], low_hits[..., 8:11]
    n, pos, t = hits[..., 4:7], hits[..., 8:11], hits[..., 0]
    ys, xs = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
    x0, wx = footprint(xs, s)
    y0, wy = footprint(ys, s)
    with np.errstate(all="ignore"):
        c_low = low_surface[..., 0:3] / albedo(low_hits, materials, lh, lw)
        zt = F32(sigma_plane) * t
        total = np.zeros((height, width, 3), dtype=F32)
        wsum = np.zeros((height, width), dtype=F32)

        def tap(qx, qy, base, active):
            nonlocal total, wsum
            inside = (qy >= 0) & (qy < lh) & (qx >= 0) & (qx < lw)
            qy, qx = np.clip(qy, 0, lh - 1), np.clip(qx, 0, lw - 1)
            cq, tq = c_low[qy, qx], tag_q[qy, qx]
            wn = np.fmax(F32(0), dot(n, n_q[qy, qx]))
            for _ in range(normal_power_log2):
                wn = wn * wn
            d = np.abs(dot(n, pos_q[qy, qx] - pos))
            wz = np.fmax(F32(0), F32(1) - d / zt)
            wz = wz * wz
            g = np.where(tag_p == 0, np.where(tq == 0, F32(1), F32(0)), np.where(tq == 0, F32(0), wn * wz)).astype(F32)
            w = g if base is None else base * g
            add = active & inside & finite3(cq) & (w > 0)
            total = np.where(add[..., None], total + cq * w[..., None], total)
            wsum = np.where(add, wsum + w, wsum)

        everywhere = np.ones((height, width), dtype=bool)
        for j in range(2):
            for i in range(2):
                tap(x0 + i, y0 + j, wy[j] * wx[i], everywhere)
        stage = np.where(wsum > 0, 1, 0)
        more = ~(wsum > 0)
        for j in range(4):
            for i in range(4):
                tap(x0 - 1 + i, y0 - 1 + j, None, more)
        stage = np.where(stage == 1, 1, np.where(wsum > 0, 2, 3))
        near_y, near_x = ys // s, xs // s
        c = np.where((wsum > 0)[..., None], total / wsum[..., None], c_low[near_y, near_x])
        assert c.dtype == F32
        out = np.empty((height, width, 4), dtype=F32)
        out[..., 0:3] = c * albedo(hits, materials, height, width)
        out[..., 3] = low_surface[near_y, near_x, 3]
    return out, stage


def bilinear(low_surface, scale):
    """Plain bilinear interpolation with the footprint's weights and clamped taps, float64: what an all-miss frame
    must come out as, up to rounding."""
    low = np.asarray(low_surface, dtype=np.float64)
    lh, lw = low.shape[0:2]
    s = int(scale)
    ys, xs = np.meshgrid(np.arange(lh * s), np.arange(lw * s), indexing="ij")
    x0, wx = footprint(xs, s)
    y0, wy = footprint(ys, s)
    total, wsum = np.zeros((lh * s, lw * s, 3)), np.zeros((lh * s, lw * s))
    for j in range(2):
        for i in range(2):
            qx, qy = x0 + i, y0 + j
            w = wy[j].astype(np.float64) * wx[i].astype(np.float64) * ((qx >= 0) & (qx < lw) & (qy >= 0) & (qy < lh))
            total += low[np.clip(qy, 0, lh - 1), np.clip(qx, 0, lw - 1), 0:3] * w[..., None]
            wsum += w
    return total / wsum[..., None]
