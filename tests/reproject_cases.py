"""Hand-made inputs for the tests of rt_reproject (tests/reproject_ref.py): analytic pinhole cameras in GPUCamera's
15-float layout and the first-hit records their pixel-centre rays would give on simple geometry, computed in
float64 and rounded.  No scene needed."""
import numpy as np

from denoise_cases import hit_records

F32 = np.float32


def pinhole(width, height, origin=(0.0, 0.0, 0.0), pixel=1.0 / 16.0, focal=1.0):
    """A camera at `origin` looking along +z: the viewport is `focal` ahead, `pixel` wide per pixel (so a plane at
    depth Z is sampled every pixel * Z / focal), x to the right, y up.  15 floats: origin, viewport size, aspect,
    horizontal, vertical, lower-left corner."""
    o = np.asarray(origin, dtype=np.float64)
    vw, vh = pixel * width, pixel * height
    cam = np.zeros(15, dtype=np.float64)
    cam[0:3], cam[3:5], cam[5] = o, (vw, vh), width / height
    cam[6:9], cam[9:12] = (vw, 0, 0), (0, vh, 0)
    cam[12:15] = o + (-vw / 2, -vh / 2, focal)
    return cam.astype(F32)


def centre_rays(cam, width, height):
    """(origin [3], directions [H, W, 3]) of the pixel-centre rays, float64."""
    c = np.asarray(cam, dtype=np.float64)
    ys, xs = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
    u, v = (xs + 0.5) / width, (ys + 0.5) / height
    d = c[12:15] + c[6:9] * u[..., None] + c[9:12] * v[..., None] - c[0:3]
    return c[0:3], d


def on_plane(cam, width, height, z):
    """Where the pixel-centre rays meet the plane z = const: (positions [H, W, 3], distances [H, W]), float64."""
    o, d = centre_rays(cam, width, height)
    s = (z - o[2]) / d[..., 2]
    pos = o + d * s[..., None]
    return pos, np.linalg.norm(d * s[..., None], axis=-1)


def plane(cam, width, height, z=4.0, material=0):
    """Every pixel hits the fronto-parallel plane z = const (normal 0, 0, -1)."""
    pos, t = on_plane(cam, width, height, z)
    shape = (height, width)
    return hit_records(np.full(shape, 2), np.full(shape, material), np.broadcast_to(np.array([0, 0, -1], F32), pos.shape),
                       pos.astype(F32), t.astype(F32))


def two_planes(cam, width, height, z_near=2.0, z_far=4.0, x_edge=0.0):
    """A foreground plane z = z_near covering x < x_edge (material 1) in front of a background plane z = z_far
    (material 0): a vertical edge.  Returns (hits, [H, W] bool mask of the foreground pixels)."""
    near, t_near = on_plane(cam, width, height, z_near)
    far, t_far = on_plane(cam, width, height, z_far)
    fg = near[..., 0] < x_edge
    pos = np.where(fg[..., None], near, far)
    t = np.where(fg, t_near, t_far)
    return hit_records(np.full(fg.shape, 2), np.where(fg, 1, 0), np.broadcast_to(np.array([0, 0, -1], F32), pos.shape),
                       pos.astype(F32), t.astype(F32)), fg


def all_miss(width, height):
    z = np.zeros((height, width), dtype=np.int64)
    return hit_records(z, z, np.zeros((height, width, 3), F32), np.zeros((height, width, 3), F32), np.zeros((height, width), F32))


def dolly(k, last, step=1.0):
    """Pose k of a small camera dolly through the benchmark scenes that ends, at k == last, at their set-up camera
    (position 0, angles 0 / 180): (position, angle_x, angle_y) for Scene.set_camera.  Per frame the camera moves
    0.07 units and turns 0.27 degrees, times `step`."""
    b = (last - k) * step
    return (-0.05 * b, -0.02 * b, -0.04 * b), 0.1 * b, 180.0 - 0.25 * b


def _rough_frame(g, cam, width, height, z):
    """Records of a rough, tiled surface around z = const: the material decided by the world-space tile a ray lands
    in and sky by the tile of its direction, so that two cameras that look the same way mostly agree about both."""
    pos, _ = on_plane(cam, width, height, z)
    _, d = centre_rays(cam, width, height)
    sky = (np.floor(d[..., 0] / d[..., 2] * 6.0).astype(np.int64) * 5 + np.floor(d[..., 1] / d[..., 2] * 6.0).astype(np.int64) * 3) % 4 == 1
    pos[..., 2] += 0.01 * g.normal(size=pos.shape[0:2])
    tile = np.floor(pos[..., 0] * 2.0).astype(np.int64) * 7 + np.floor(pos[..., 1] * 2.0).astype(np.int64) * 3
    kind = np.where(sky, 0, 1 + tile % 2)
    mat = tile % 3
    v = np.array([0.05, -0.05, -1.0]) + 0.1 * g.normal(size=pos.shape)
    nrm = v / np.linalg.norm(v, axis=-1, keepdims=True)
    t = np.linalg.norm(pos - np.asarray(cam, np.float64)[0:3], axis=-1)
    return kind, mat, nrm.astype(F32), pos.astype(F32), t.astype(F32)


def synthetic(width, height, seed=1):
    """An adversarial pair of frames: a dict with surface [H, W, 4], hits, camera, prev_surface, prev_hits,
    prev_history [H, W], prev_camera and max_history.

    The previous camera stands 2.25 pixel footprints to the left, 1.5 below and a little behind the new one, so
    some columns and rows project outside; about a quarter of each frame is sky.  Where the frame is large enough
    it also holds: NaN, +-inf and 1e30 colours in both images, NaN alphas, histories of 0, NaN, -1, 0.5, fractional
    values and values above max_history, a material index beyond any table, a hit with t = 0, records whose position
    lies behind the previous camera (s <= 0) and in its plane of no projection (dn == 0), and a record of NaNs."""
    g = np.random.default_rng(seed)
    z, px = 5.0, 1.0 / 16.0
    cam = pinhole(width, height, (0.125, -0.25, 0.0), px)
    prev_cam = pinhole(width, height, (0.125 - 2.25 * px * z, -0.25 - 1.5 * px * z, -0.0625), px)
    kind, mat, nrm, pos, t = _rough_frame(g, cam, width, height, z)
    pkind, pmat, pnrm, ppos, pt = _rough_frame(g, prev_cam, width, height, z)
    surface = g.gamma(0.7, 1.5, size=(height, width, 4)).astype(F32)
    prev_surface = g.gamma(0.7, 1.5, size=(height, width, 4)).astype(F32)
    surface[..., 3] = g.random((height, width)).astype(F32)
    prev_history = np.floor(g.uniform(1, 12, size=(height, width))).astype(F32)
    prev_history[g.random((height, width)) < 0.2] += F32(0.375)
    max_history = 8
    if width * height == 1:
        kind[0, 0] = pkind[0, 0] = 2
        pmat[0, 0] = mat[0, 0]
    if width >= 16 and height >= 16:
        cells = g.permutation(width * height)
        at = lambda i: (int(cells[i]) // width, int(cells[i]) % width)
        for i, c in enumerate([(np.nan, 1.0, 2.0), (0.5, np.inf, 0.25), (1e30, 1e30, 1e30), (-np.inf, 0.0, np.nan)]):
            surface[at(i)][0:3] = c
            prev_surface[at(i + 4)][0:3] = c
            prev_surface[at(i + 8)][0:3] = c
        surface[at(12)][3] = np.nan
        prev_surface[at(13)][3] = np.nan
        for i, v in enumerate([0.0, np.nan, -1.0, 0.5, 0.99999994, 1.0, 1e30, np.inf, 70000.0, 0.0, np.nan, 0.5]):
            prev_history[at(20 + i)] = v
        hit_px = np.argwhere(kind != 0)
        pick = [tuple(p) for p in hit_px[g.permutation(len(hit_px))[:8]]]
        mat[pick[0]] = 1 << 20                                   # beyond any table: compared, never looked up
        t[pick[1]] = 0.0                                         # sigma_plane * t = 0: only a tap in the plane passes
        pos[pick[2]] = prev_cam[0:3] + F32([0.5, 0.25, -3.0])    # behind the previous camera: s <= 0
        pos[pick[3]] = prev_cam[0:3] + F32([0.5, 0.25, 0.0])     # d.z == 0: dn == 0
        pos[pick[4]] = prev_cam[0:3]                             # d == 0
        pos[pick[5]] = (np.nan, np.nan, np.nan)
        pos[pick[6]] = (1e30, -1e30, 1e-30)                      # a projection far outside
        nrm[pick[7]] = (np.nan, 0.0, 0.0)
        edge = (height // 2, width - 1)                          # a hit that projects outside: no history ...
        kind[edge] = 2
        surface[edge][0:3] = (np.nan, np.nan, np.nan)            # ... and no colour of its own: history 0
        phit_px = np.argwhere(pkind != 0)
        ppick = [tuple(p) for p in phit_px[g.permutation(len(phit_px))[:3]]]
        pmat[ppick[0]] = 1 << 20
        ppos[ppick[1]] = (np.nan, 1.0, 1.0)
        pnrm[ppick[2]] = (np.inf, 0.0, 0.0)
    return {"surface": surface, "hits": hit_records(kind, mat, nrm, pos, t), "camera": cam,
            "prev_surface": prev_surface, "prev_hits": hit_records(pkind, pmat, pnrm, ppos, pt),
            "prev_history": prev_history, "prev_camera": prev_cam, "max_history": max_history}
