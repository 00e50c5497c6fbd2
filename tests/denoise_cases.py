"""Hand-made inputs for the denoiser's tests (tests/denoise_ref.py, rt_denoise): hit records, material tables
and frames as numpy arrays, no scene needed."""
import numpy as np

F32 = np.float32


def material_table(albedos):
    """[M, 16] float32 GPUMaterial rows with the given albedos (alpha 1, everything else 0)."""
    m = np.zeros((len(albedos), 16), dtype=F32)
    for i, a in enumerate(albedos):
        m[i, 0:3], m[i, 3] = a, 1.0
    return m


def hit_records(kind, material, normal, position, t):
    """[H*W, 12] float32 rt_hit rows from [H, W(, 3)] arrays; a miss is t = 1e30 and zeros, as rt_trace_rays writes it."""
    h, w = kind.shape
    hits = np.zeros((h * w, 12), dtype=F32)
    u = hits.view(np.uint32)
    k = kind.reshape(-1).astype(np.uint32)
    hit = k != 0
    hits[:, 0] = np.where(hit, t.reshape(-1), F32(1e30))
    u[:, 1] = k
    u[:, 3] = np.where(hit, material.reshape(-1).astype(np.uint32), 0)
    hits[:, 4:7] = np.where(hit[:, None], normal.reshape(-1, 3), 0)
    hits[:, 8:11] = np.where(hit[:, None], position.reshape(-1, 3), 0)
    return hits


def plane(width, height, material=0):
    """Every pixel hits the plane z = 5 (normal 0, 0, -1 towards the origin), seen from the origin."""
    ys, xs = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
    pos = np.stack([(xs - width / 2) * 0.1, (ys - height / 2) * 0.1, np.full(xs.shape, 5.0)], axis=-1).astype(F32)
    nrm = np.broadcast_to(np.array([0, 0, -1], dtype=F32), pos.shape)
    t = np.sqrt((pos.astype(np.float64) ** 2).sum(-1)).astype(F32)
    return hit_records(np.full(xs.shape, 2), np.full(xs.shape, material), nrm, pos, t)


def corner(width, height):
    """Two half-planes that meet at a right angle at x = width // 2: z = 5 (normal 0, 0, -1, material 0) on the left,
    x = const (normal -1, 0, 0, material 1) on the right.  Returns (hits, [H, W] bool mask of the left half)."""
    ys, xs = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
    left = xs < width // 2
    edge = (width // 2 - width / 2) * 0.1
    pos = np.stack([np.where(left, (xs - width / 2) * 0.1, edge), (ys - height / 2) * 0.1,
                    np.where(left, 5.0, 5.0 - (xs - width // 2) * 0.1)], axis=-1).astype(F32)
    nrm = np.where(left[..., None], np.array([0, 0, -1], dtype=F32), np.array([-1, 0, 0], dtype=F32)).astype(F32)
    t = np.sqrt((pos.astype(np.float64) ** 2).sum(-1)).astype(F32)
    return hit_records(np.full(xs.shape, 2), np.where(left, 0, 1), nrm, pos, t), left


def synthetic(width, height, seed=1):
    """An adversarial frame: (surface [H, W, 4], hits [H*W, 12], materials [M, 16]).

    About 30 % misses; unit normals, the left half scattered around one direction (so that many taps carry
    weight), the right half uniformly random; positions on a rough surface around z = 5; five materials, one
    with albedo 0 and one with components beyond 1; and, where the frame is large enough, one material index
    beyond the table, a hit with t = 0, and NaN, +inf, -inf and 1e30 colours on hit and on missed pixels."""
    g = np.random.default_rng(seed)
    ys, xs = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
    kind = np.where(g.random((height, width)) < 0.3, 0, g.integers(1, 3, size=(height, width)))
    v = g.normal(size=(height, width, 3))
    v = np.where((xs < width // 2)[..., None], np.array([0.2, -0.1, -1.0]) + 0.25 * v, v)
    nrm = (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(F32)
    pos = np.stack([(xs - width / 2) * 0.1, (ys - height / 2) * 0.1, 5.0 + 0.05 * g.normal(size=xs.shape)], axis=-1).astype(F32)
    t = np.sqrt((pos.astype(np.float64) ** 2).sum(-1)).astype(F32)
    materials = material_table([(0.73, 0.41, 0.2), (0.0, 0.0, 0.0), (1.5, 0.9, 0.01), (0.5, 0.25, 1.0), (0.33, 0.66, 0.99)])
    mat = g.integers(0, materials.shape[0], size=(height, width))
    surface = (g.gamma(0.7, 1.5, size=(height, width, 4))).astype(F32)
    surface[..., 3] = g.random((height, width)).astype(F32)
    if width * height == 1:
        kind[0, 0] = 2
    if width >= 16 and height >= 16:
        hit_px = np.argwhere(kind != 0)
        pick = hit_px[g.permutation(len(hit_px))[:8]]
        mat[tuple(pick[0])] = materials.shape[0] + 7     # beyond the table: albedo 1
        t[tuple(pick[1])] = 0.0                          # sigma_plane * t = 0: every tap's plane weight is 0
        mat[tuple(pick[2])] = 1                          # albedo 0: divided by the floor
        surface[tuple(pick[3])][0:3] = (np.nan, 1.0, 2.0)
        surface[tuple(pick[4])][0:3] = (0.5, np.inf, 0.25)
        surface[tuple(pick[5])][0:3] = (1e30, 1e30, 1e30)
        surface[tuple(pick[6])][0:3] = (-np.inf, 0.0, np.nan)
        surface[tuple(pick[7])][0:3] = (3e38, 1.0, 1.0)  # finite, but not after the division by an albedo < 1
        miss_px = np.argwhere(kind == 0)
        if len(miss_px) >= 2:
            surface[tuple(miss_px[0])][0:3] = (np.nan, np.inf, 1e30)
            surface[tuple(miss_px[1])][3] = np.nan
    return surface, hit_records(kind, mat, nrm, pos, t), materials
