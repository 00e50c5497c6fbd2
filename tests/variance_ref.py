"""Reference for rt_moments and rt_denoise_variance (include/rt_abi.h, csrc/denoise_variance.hip): both calls
restated in numpy from the header's text, fp32 throughout.

As in tests/denoise_ref.py every product, sum, difference and quotient is a single numpy float32 operation (no
contraction, IEEE division), dot products are summed in rtm::dot's order, fmaxf is np.fmax, and a tap's contribution
is masked with `w > 0` rather than added as a zero.  One vectorised step per tap, the taps in the header's order: dy
outer, dx inner.  The GPU tests compare bytewise against this.

moments(surface, hits, materials) -> [H, W, 4] float32
denoise_variance(surface, hits, materials, moments=None, history=None, ...) -> ([H, W, 4] float32, [H, W] float32)
    surface   [H, W, 4] float32 (row y, pixel x): the accumulated image
    hits      [H*W, 12] float32 rt_hit rows, record y*W + x
    materials [M, 16] float32 GPUMaterial rows (albedo in words 0-2); M may be 0
    moments   None or [H, W, 4] float32: the accumulated (l, l*l, 0, alpha)
    history   None or [H, W] float32: the frames the accumulated image holds per pixel
"""
import numpy as np

from denoise_ref import ALBEDO_FLOOR, F32, FLT_MAX, H5, albedo, dot, finite3  # noqa: F401  (steps 1 and 2 of rt_denoise's block)

KP = np.array([0.25, 0.5, 0.25], dtype=F32)
TOLERANCE_FLOOR = F32(1e-8)
DEFAULTS = {"iterations": 5, "normal_power_log2": 5, "sigma_plane": 0.03, "sigma_lum": 4.0, "min_history": 4.0}


def lum(c):
    return (F32(0.2126) * c[..., 0] + F32(0.7152) * c[..., 1]) + F32(0.0722) * c[..., 2]


def finite1(v):
    return np.abs(v) <= FLT_MAX


def moments(surface, hits, materials):
    surface = np.ascontiguousarray(surface, dtype=F32)
    height, width = surface.shape[0:2]
    with np.errstate(all="ignore"):
        c = surface[..., 0:3] / albedo(hits, materials, height, width)
        l = lum(c)
        out = np.stack([l, l * l, np.zeros_like(l), surface[..., 3]], axis=-1)
    assert out.dtype == F32
    return out


class Guide:
    """valid(p) and the weights wn and wz of rt_denoise's step 2 between every pixel p and its tap at (dx, dy)."""

    def __init__(self, hits, height, width, normal_power_log2, sigma_plane):
        hits = np.ascontiguousarray(hits, dtype=F32).reshape(height, width, 12)
        self.height, self.width, self.normal_power_log2 = height, width, normal_power_log2
        self.valid = hits.view(np.uint32)[..., 1] != 0
        self.n, self.pos = hits[..., 4:7], hits[..., 8:11]
        self.zt = F32(sigma_plane) * hits[..., 0]
        self.ys, self.xs = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")

    def tap(self, dx, dy):
        """(qy, qx clipped into the image, inside [H, W] bool) of the tap at offset (dx, dy)."""
        qy, qx = self.ys + dy, self.xs + dx
        inside = (qy >= 0) & (qy < self.height) & (qx >= 0) & (qx < self.width)
        return np.clip(qy, 0, self.height - 1), np.clip(qx, 0, self.width - 1), inside

    def weights(self, qy, qx):
        wn = np.fmax(F32(0), dot(self.n, self.n[qy, qx]))
        for _ in range(self.normal_power_log2):
            wn = wn * wn
        d = np.abs(dot(self.n, self.pos[qy, qx] - self.pos))
        wz = np.fmax(F32(0), F32(1) - d / self.zt)
        return wn, wz * wz


def initial_variance(c, g, moments, history, min_history, details=None):
    """Step 1's v_p, [H, W]."""
    height, width = g.height, g.width
    l = lum(c)
    fin = finite3(c)
    hist = np.ones((height, width), dtype=F32) if history is None else np.ascontiguousarray(history, dtype=F32).reshape(height, width)
    temporal = np.zeros((height, width), dtype=bool)
    vt = np.zeros((height, width), dtype=F32)
    if moments is not None:
        moments = np.ascontiguousarray(moments, dtype=F32)
        m1, m2 = moments[..., 0], moments[..., 1]
        temporal = (hist >= F32(min_history)) & finite1(m1) & finite1(m2)
        vt = np.fmax(F32(0), m2 - m1 * m1) / np.fmax(hist, F32(1))
    s1 = np.zeros((height, width), dtype=F32)
    s2 = np.zeros((height, width), dtype=F32)
    ws = np.zeros((height, width), dtype=F32)
    for dy in range(-3, 4):
        for dx in range(-3, 4):
            qy, qx, inside = g.tap(dx, dy)
            lq = l[qy, qx]
            wn, wz = g.weights(qy, qx)
            w = wn * wz
            add = inside & g.valid[qy, qx] & fin[qy, qx] & (w > 0)
            s1 = np.where(add, s1 + lq * w, s1)
            s2 = np.where(add, s2 + (lq * lq) * w, s2)
            ws = np.where(add, ws + w, ws)
    vs = np.where(ws > 0, np.fmax(F32(0), s2 / ws - (s1 / ws) * (s1 / ws)), F32(0))
    v = np.where(g.valid & fin, np.where(temporal, vt, vs), F32(0)).astype(F32)
    if details is not None:
        details.update(temporal=g.valid & fin & temporal, spatial=g.valid & fin & ~temporal)
    return v


def denoise_variance(surface, hits, materials, moments=None, history=None, iterations=DEFAULTS["iterations"],
                     normal_power_log2=DEFAULTS["normal_power_log2"], sigma_plane=DEFAULTS["sigma_plane"],
                     sigma_lum=DEFAULTS["sigma_lum"], min_history=DEFAULTS["min_history"], details=None):
    surface = np.ascontiguousarray(surface, dtype=F32)
    height, width = surface.shape[0:2]
    assert surface.shape == (height, width, 4)
    assert 1 <= iterations <= 6 and 0 <= normal_power_log2 <= 8 and sigma_plane > 0 and sigma_lum > 0 and min_history >= 1
    g = Guide(hits, height, width, normal_power_log2, sigma_plane)
    valid = g.valid
    sl2 = F32(sigma_lum) * F32(sigma_lum)
    with np.errstate(all="ignore"):
        a = albedo(hits, materials, height, width)
        c = surface[..., 0:3] / a
        v = initial_variance(c, g, moments, history, min_history, details)
        if details is not None:
            details["initial_variance"] = v.copy()
        for s in range(iterations):
            step = 1 << s
            vsum = np.zeros((height, width), dtype=F32)
            ksum = np.zeros((height, width), dtype=F32)
            for dy in range(-1, 2):
                for dx in range(-1, 2):
                    qy, qx, inside = g.tap(dx, dy)
                    k = KP[dy + 1] * KP[dx + 1]
                    take = inside & valid[qy, qx]
                    vsum = np.where(take, vsum + v[qy, qx] * k, vsum)
                    ksum = np.where(take, ksum + k, ksum)
            tol = sl2 * (vsum / ksum) + TOLERANCE_FLOOR
            l = lum(c)
            use_lum = finite3(c)
            total = np.zeros((height, width, 3), dtype=F32)
            vs = np.zeros((height, width), dtype=F32)
            wsum = np.zeros((height, width), dtype=F32)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    qy, qx, inside = g.tap(dx * step, dy * step)
                    cq, vq = c[qy, qx], v[qy, qx]
                    taken = inside & valid[qy, qx] & finite3(cq)
                    wn, wz = g.weights(qy, qx)
                    d = l[qy, qx] - l
                    wl = np.where(use_lum, F32(1) / (F32(1) + (d * d) / tol), F32(1)).astype(F32)
                    w = (((H5[dy + 2] * H5[dx + 2]) * wn) * wz) * wl
                    add = valid & taken & (w > 0)
                    total = np.where(add[..., None], total + cq * w[..., None], total)
                    vs = np.where(add, vs + vq * (w * w), vs)
                    wsum = np.where(add, wsum + w, wsum)
            new = valid & (wsum > 0)
            c = np.where(new[..., None], total / wsum[..., None], c)
            v = np.where(new, vs / (wsum * wsum), v)
            assert c.dtype == F32 and v.dtype == F32
        out = surface.copy()
        out[..., 0:3] = c * a
    return out, v
