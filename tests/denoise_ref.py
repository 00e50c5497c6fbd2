"""Reference for rt_denoise (include/rt_abi.h, csrc/denoise.hip): the filter restated in numpy, fp32 throughout.

Every product, sum, difference and quotient is a single numpy float32 operation (no contraction, IEEE
division), dot products are summed in rtm::dot's order, fmaxf is np.fmax, and a tap's contribution is masked
with `w > 0` rather than added as a zero (adding +0 to a sum of -0 would change its sign bit).  One vectorised
step per tap, the taps in the kernel's order: dy outer, dx inner.  The GPU tests compare bytewise against this.

denoise(surface, hits, materials, ...) -> [H, W, 4] float32
    surface   [H, W, 4] float32 (row y, pixel x, as rt_render writes it)
    hits      [H*W, 12] float32 rt_hit rows, record y*W + x
    materials [M, 16] float32 GPUMaterial rows (albedo in words 0-2); M may be 0
"""
import numpy as np

F32 = np.float32
FLT_MAX = np.finfo(np.float32).max
H5 = np.array([0.0625, 0.25, 0.375, 0.25, 0.0625], dtype=F32)
ALBEDO_FLOOR = F32(0.015625)
DEFAULTS = {"iterations": 5, "normal_power_log2": 5, "sigma_plane": 0.03, "sigma_color": 8.0}


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def finite3(c):
    return (np.abs(c[..., 0:3]) <= FLT_MAX).all(axis=-1)


def albedo(hits, materials, height, width):
    """The floor-clamped albedo `a` the filter divides and multiplies by, [H, W, 3]."""
    hu = np.ascontiguousarray(hits, dtype=F32).view(np.uint32).reshape(height, width, 12)
    materials = np.asarray(materials, dtype=F32).reshape(-1, 16)
    use = (hu[..., 1] != 0) & (hu[..., 3] < materials.shape[0])
    alb = np.ones((height, width, 3), dtype=F32)
    alb[use] = materials[hu[..., 3][use].astype(np.int64), 0:3]
    return np.fmax(alb, ALBEDO_FLOOR)


def denoise(surface, hits, materials, iterations=DEFAULTS["iterations"], normal_power_log2=DEFAULTS["normal_power_log2"],
            sigma_plane=DEFAULTS["sigma_plane"], sigma_color=DEFAULTS["sigma_color"]):
    surface = np.ascontiguousarray(surface, dtype=F32)
    height, width = surface.shape[0:2]
    assert surface.shape == (height, width, 4)
    assert 1 <= iterations <= 6 and 0 <= normal_power_log2 <= 8 and sigma_plane > 0 and sigma_color >= 0
    hits = np.ascontiguousarray(hits, dtype=F32).reshape(height, width, 12)
    valid = hits.view(np.uint32)[..., 1] != 0
    n, pos, t = hits[..., 4:7], hits[..., 8:11], hits[..., 0]
    sigma_plane, sigma_color = F32(sigma_plane), F32(sigma_color)
    ys, xs = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
    with np.errstate(all="ignore"):
        a = albedo(hits, materials, height, width)
        c = surface[..., 0:3] / a
        zt = sigma_plane * t
        for s in range(iterations):
            step = 1 << s
            sc = sigma_color * F32(2.0 ** -s)
            sc2 = sc * sc
            use_colour = finite3(c) & bool(sigma_color > 0)
            total = np.zeros((height, width, 3), dtype=F32)
            wsum = np.zeros((height, width), dtype=F32)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    qy, qx = ys + dy * step, xs + dx * step
                    inside = (qy >= 0) & (qy < height) & (qx >= 0) & (qx < width)
                    qy, qx = np.clip(qy, 0, height - 1), np.clip(qx, 0, width - 1)
                    cq = c[qy, qx]
                    taken = inside & valid[qy, qx] & finite3(cq)
                    wn = np.fmax(F32(0), dot(n, n[qy, qx]))
                    for _ in range(normal_power_log2):
                        wn = wn * wn
                    d = np.abs(dot(n, pos[qy, qx] - pos))
                    wz = np.fmax(F32(0), F32(1) - d / zt)
                    wz = wz * wz
                    e = cq - c
                    wc = np.where(use_colour, F32(1) / (F32(1) + dot(e, e) / sc2), F32(1)).astype(F32)
                    w = (((H5[dy + 2] * H5[dx + 2]) * wn) * wz) * wc
                    add = valid & taken & (w > 0)
                    total = np.where(add[..., None], total + cq * w[..., None], total)
                    wsum = np.where(add, wsum + w, wsum)
            c = np.where((valid & (wsum > 0))[..., None], total / wsum[..., None], c)
            assert c.dtype == F32
        out = surface.copy()
        out[..., 0:3] = c * a
    return out


# --- the viewer's display transform, for the quality measure only (main.cpp:78-94; float64, not bit-pinned) ---
def display(rgb):
    x = np.asarray(rgb, dtype=np.float64) * 0.5
    x = np.clip((x * (2.51 * x + 0.03)) / (x * (2.43 * x + 0.59) + 0.14), 0.0, 1.0)
    return np.where(x <= 0.0031308, 12.92 * x, 1.055 * np.power(x, 1.0 / 2.4) - 0.055)


def display_error(image, target, mask):
    """RMS difference of srgb(aces(0.5 * c)) over the pixels of `mask` ([H, W] bool), all three channels."""
    d = display(image[..., 0:3])[mask] - display(target[..., 0:3])[mask]
    return float(np.sqrt(np.mean(d * d)))
