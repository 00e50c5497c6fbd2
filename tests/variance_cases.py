"""Hand-made inputs for the tests of rt_moments and rt_denoise_variance (tests/variance_ref.py): the adversarial
frames of tests/denoise_cases.py with an accumulated-moments surface and a history to go with them.  No scene needed."""
import numpy as np

import denoise_cases as DC
import variance_ref as V

F32 = np.float32


def synthetic(width, height, seed=1):
    """A dict with surface [H, W, 4], hits [H*W, 12], materials [M, 16], moments [H, W, 4] and history [H, W].

    surface, hits and materials are denoise_cases.synthetic's: random normals, positions and materials, about 30 %
    misses and, from 16x16 on, NaN, +-inf and 1e30 colours on hits and misses, a material index beyond the table and a
    hit with t = 0.  The moments are those of a luminance scattered around the surface's own (so the temporal variance
    is of the size of the colour differences), not finite where the colour is not; the history is 0..8 with a few
    fractional values, so that with min_history 4 both estimates occur.  Where there are at least 6 pixels the case
    also holds, on hit pixels where it has them: one moment that is not finite under a finite colour, one m2 < m1*m1
    (the clamp), one history of NaN and one of 0.5 with good moments, and one long history (32)."""
    g = np.random.default_rng(seed + 7919)
    surface, hits, materials = DC.synthetic(width, height, seed=seed)
    with np.errstate(all="ignore"):
        m = V.moments(surface, hits, materials)
        m1 = (m[..., 0] * g.uniform(0.8, 1.2, size=(height, width)).astype(F32)).astype(F32)
        m2 = (m1 * m1 + (g.gamma(0.7, 0.5, size=(height, width)).astype(F32) * (m1 * m1 + F32(0.01)))).astype(F32)
    moments = np.stack([m1, m2, np.zeros_like(m1), surface[..., 3]], axis=-1).astype(F32)
    history = np.floor(g.uniform(0, 9, size=(height, width))).astype(F32)  # 0 to 8
    history[g.random((height, width)) < 0.1] += F32(0.25)
    if width * height >= 6:
        kind = hits.view(np.uint32)[:, 1].reshape(height, width)
        good = np.argwhere((kind != 0) & V.finite3(surface) & np.isfinite(m1) & np.isfinite(m2))
        if len(good) == 0:
            good = np.argwhere(np.ones((height, width), dtype=bool))
        order = g.permutation(len(good))
        pick = [tuple(good[order[i % len(good)]]) for i in range(6)]  # a small frame may reuse a pixel: the first wins last
        history[pick[5]] = 32.0
        history[pick[4]] = 0.5
        history[pick[3]] = np.nan
        moments[pick[2]][0:2], history[pick[2]] = (0.5, np.inf), 7.0
        moments[pick[1]][0:2], history[pick[1]] = (np.nan, 1.0), 6.0
        moments[pick[0]][0:2], history[pick[0]] = (2.0, 3.5), 5.0  # m2 < m1 * m1: the clamp
    return {"surface": surface, "hits": hits, "materials": materials, "moments": moments, "history": history}
