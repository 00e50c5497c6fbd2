"""Reference for rt_reproject (include/rt_abi.h, csrc/reproject.hip): the specification restated in numpy, fp32
throughout.

Every product, sum, difference and quotient is a single numpy float32 operation (no contraction, IEEE division),
dot and cross products are formed in the header's order, fminf is np.fmin, floorf np.floor on float32, and a tap's
contribution is masked rather than added as a zero.  One vectorised step per tap, the taps in the kernel's order.
The per-frame constants are computed as the host computes them.  The GPU tests compare bytewise against this.

reproject(surface, hits, camera, prev=None, ...) -> (out [H, W, 4] float32, out_history [H, W] float32)
    surface  [H, W, 4] float32 (row y, pixel x): the new frame
    hits     [H*W, 12] float32 rt_hit rows, record y*W + x
    camera   15 floats in GPUCamera's layout (origin, viewport size, aspect, horizontal, vertical, lower-left corner)
    prev     None, or (prev_surface [H, W, 4], prev_hits [H*W, 12], prev_history [H, W], prev_camera)
"""
import numpy as np

F32 = np.float32
FLT_MAX = np.finfo(np.float32).max
DEFAULTS = {"max_history": 32, "sigma_plane": 0.03, "normal_min": 0.9}


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def finite3(c):
    return (np.abs(c[..., 0:3]) <= FLT_MAX).all(axis=-1)


def camera_parts(camera):
    """(O, H, V, L) of 15 GPUCamera floats, each a float32 [3]."""
    c = np.asarray(camera, dtype=F32).reshape(15)
    return c[0:3], c[6:9], c[9:12], c[12:15]


def frame_constants(prev_camera):
    """The host's per-frame constants (O, N, A, B, wn) of the previous camera."""
    O, Hh, V, L = camera_parts(prev_camera)
    w = L - O
    N, A, B = cross(Hh, V), cross(V, w), cross(w, Hh)
    return O, N, A, B, dot(w, N)


def project(hits, camera, prev_camera, width, height):
    """Steps 1 and 2: (fx, fy, valid), each [H, W]; fx and fy float32 as the kernel computes them."""
    hits = np.ascontiguousarray(hits, dtype=F32).reshape(height, width, 12)
    hit = hits.view(np.uint32)[..., 1] != 0
    O, N, A, B, wn = frame_constants(prev_camera)
    co, ch, cv, cl = camera_parts(camera)
    ys, xs = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
    with np.errstate(all="ignore"):
        ux = (xs.astype(F32) + F32(0.5)) / F32(width)
        uy = (ys.astype(F32) + F32(0.5)) / F32(height)
        sky = ((cl + ch * ux[..., None]) + cv * uy[..., None]) - co
        d = np.where(hit[..., None], hits[..., 8:11] - O, sky)
        assert d.dtype == F32
        dn = dot(d, N)
        s = wn / dn
        fx = (dot(d, A) / dn) * F32(width) - F32(0.5)
        fy = (dot(d, B) / dn) * F32(height) - F32(0.5)
        valid = (dn != 0) & (s > 0) & (fx > -1) & (fx < F32(width)) & (fy > -1) & (fy < F32(height))
    assert fx.dtype == F32 and fy.dtype == F32
    return fx, fy, valid


def reproject(surface, hits, camera, prev=None, max_history=DEFAULTS["max_history"], sigma_plane=DEFAULTS["sigma_plane"],
              normal_min=DEFAULTS["normal_min"], details=None):
    surface = np.ascontiguousarray(surface, dtype=F32)
    height, width = surface.shape[0:2]
    assert surface.shape == (height, width, 4)
    assert 1 <= max_history <= 65535 and sigma_plane > 0 and np.isfinite(sigma_plane) and -1 <= normal_min <= 1
    max_history, sigma_plane, normal_min = F32(max_history), F32(sigma_plane), F32(normal_min)
    hits = np.ascontiguousarray(hits, dtype=F32).reshape(height, width, 12)
    cur = surface[..., 0:3]
    cur_finite = finite3(cur)
    out = surface.copy()
    out_history = np.where(cur_finite, F32(1), F32(0)).astype(F32)
    if prev is None:
        return out, out_history
    prev_surface, prev_hits, prev_history, prev_camera = prev
    prev_surface = np.ascontiguousarray(prev_surface, dtype=F32)
    assert prev_surface.shape == surface.shape
    prev_hits = np.ascontiguousarray(prev_hits, dtype=F32).reshape(height, width, 12)
    prev_history = np.ascontiguousarray(prev_history, dtype=F32).reshape(height, width)
    hu, pu = hits.view(np.uint32), prev_hits.view(np.uint32)
    hit, material = hu[..., 1] != 0, hu[..., 3]
    n_p, pos_p, t_p = hits[..., 4:7], hits[..., 8:11], hits[..., 0]
    fx, fy, valid = project(hits, camera, prev_camera, width, height)
    with np.errstate(all="ignore"):
        flx, fly = np.floor(fx), np.floor(fy)
        x0 = np.where(valid, flx, 0).astype(np.int64)  # only a valid projection is converted
        y0 = np.where(valid, fly, 0).astype(np.int64)
        ax, ay = fx - flx, fy - fly
        wx, wy = (F32(1) - ax, ax), (F32(1) - ay, ay)
        plane = sigma_plane * t_p
        total = np.zeros((height, width, 3), dtype=F32)
        hs = np.zeros((height, width), dtype=F32)
        ws = np.zeros((height, width), dtype=F32)
        for k in range(4):
            qx, qy = x0 + (k & 1), y0 + (k >> 1)
            inside = (qx >= 0) & (qx < width) & (qy >= 0) & (qy < height)
            qx, qy = np.clip(qx, 0, width - 1), np.clip(qy, 0, height - 1)
            w = wx[k & 1] * wy[k >> 1]
            cq, hq = prev_surface[qy, qx, 0:3], prev_history[qy, qx]
            qhit = pu[qy, qx, 1] != 0
            agree = (qhit & (pu[qy, qx, 3] == material) & (dot(n_p, prev_hits[qy, qx, 4:7]) >= normal_min)
                     & (np.abs(dot(n_p, prev_hits[qy, qx, 8:11] - pos_p)) <= plane))
            taken = valid & inside & (w > 0) & (hq >= 1) & finite3(cq) & np.where(hit, agree, ~qhit)
            total = np.where(taken[..., None], total + cq * w[..., None], total)
            hs = np.where(taken, hs + hq * w, hs)
            ws = np.where(taken, ws + w, ws)
        has = ws > 0
        pc = total / ws[..., None]
        hl = hs / ws
        n = np.fmin(hl + F32(1), max_history)
        blended = pc + (cur - pc) * (F32(1) / n)[..., None]
        assert blended.dtype == F32 and n.dtype == F32 and pc.dtype == F32
        out[..., 0:3] = np.where((has & cur_finite)[..., None], blended, np.where(has[..., None], pc, cur))
        out_history = np.where(has, np.where(cur_finite, n, np.fmin(hl, max_history)), out_history).astype(F32)
    if details is not None:
        details.update(fx=fx, fy=fy, valid=valid, ws=ws, pc=pc, hl=hl)
    return out, out_history
