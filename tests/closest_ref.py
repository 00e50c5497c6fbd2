"""Reference for the closest-point queries (rt_closest_point): the rules of include/rt_abi.h restated in numpy, by
brute force -- every sphere and every face for every point, no BVH -- and the lexicographic (d2, kind, id) minimum.

Everything is float32: arrays are float32, constants are np.float32 scalars, every operation is one numpy float32
operation (no promotion, no contraction), and every choice is an np.where select, so a NaN stays a NaN.
closest(arrays, points) returns complete 32-byte rt_nearest records.
"""
import numpy as np

import query_ref as Q

F32 = np.float32
ZERO, ONE = F32(0.0), F32(1.0)


def dot(u, v):
    """(u.x * v.x + u.y * v.y) + u.z * v.z over the last axis."""
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def ratio(n, d):
    with np.errstate(all="ignore"):
        return np.where(d > ZERO, n / d, ZERO).astype(F32)


def sphere_candidates(p, c, rad):
    """p (P, 3), c (S, 3), rad (S,): d2 (P, S), q (P, S, 3)."""
    with np.errstate(all="ignore"):
        v = p[:, None, :] - c[None, :, :]
        length = np.sqrt(dot(v, v))
        s = length - rad[None, :]
        dist = np.where(s < ZERO, -s, s)
        d2 = dist * dist
        k = rad[None, :] / length
        on = c[None, :, :] + v * k[..., None]
        at_centre = c + np.stack([rad, np.zeros_like(rad), np.zeros_like(rad)], axis=1)
        q = np.where((length > ZERO)[..., None], on, np.broadcast_to(at_centre[None, :, :], on.shape))
    return d2.astype(F32), q.astype(F32)


def face_candidates(p, a, ab, ac):
    """p (P, 3), a / ab / ac (F, 3): d2 (P, F), q (P, F, 3), region (P, F)."""
    with np.errstate(all="ignore"):
        ap = p[:, None, :] - a[None, :, :]
        AB, AC = ab[None, :, :], ac[None, :, :]
        d1, d2_ = dot(AB, ap), dot(AC, ap)
        aa, bb, cc = dot(ab, ab)[None, :], dot(ab, ac)[None, :], dot(ac, ac)[None, :]
        d3, d4, d5, d6 = d1 - aa, d2_ - bb, d1 - bb, d2_ - cc
        vc = d1 * d4 - d3 * d2_
        vb = d5 * d2_ - d1 * d6
        va = d3 * d6 - d5 * d4
        e43, e56 = d4 - d3, d5 - d6
        r1 = (d1 <= ZERO) & (d2_ <= ZERO)
        r2 = (d3 >= ZERO) & (d4 <= d3)
        r3 = (vc <= ZERO) & (d1 >= ZERO) & (d3 <= ZERO)
        r4 = (d6 >= ZERO) & (d5 <= d6)
        r5 = (vb <= ZERO) & (d2_ >= ZERO) & (d6 <= ZERO)
        r6 = (va <= ZERO) & (e43 >= ZERO) & (e56 >= ZERO)
        # rule 7, then the earlier rules over it, last to first
        den = (va + vb) + vc
        v = ratio(vb, den)
        w = ratio(vc, den)
        v = np.where(v < ZERO, ZERO, v)
        v = np.where(v > ONE, ONE, v)
        w = np.where(w < ZERO, ZERO, w)
        rest = ONE - v
        w = np.where(w > rest, rest, w)
        region = np.zeros(v.shape, dtype=np.uint32)
        w6 = ratio(e43, e43 + e56)
        v, w, region = np.where(r6, ONE - w6, v), np.where(r6, w6, w), np.where(r6, np.uint32(6), region)
        v, w, region = np.where(r5, ZERO, v), np.where(r5, ratio(d2_, d2_ - d6), w), np.where(r5, np.uint32(5), region)
        v, w, region = np.where(r4, ZERO, v), np.where(r4, ONE, w), np.where(r4, np.uint32(3), region)
        v, w, region = np.where(r3, ratio(d1, d1 - d3), v), np.where(r3, ZERO, w), np.where(r3, np.uint32(4), region)
        v, w, region = np.where(r2, ONE, v), np.where(r2, ZERO, w), np.where(r2, np.uint32(2), region)
        v, w, region = np.where(r1, ZERO, v), np.where(r1, ZERO, w), np.where(r1, np.uint32(1), region)
        v, w = v.astype(F32), w.astype(F32)
        q = (a[None, :, :] + AB * v[..., None]) + AC * w[..., None]
        e = p[:, None, :] - q
        d2 = dot(e, e)
    assert d2.dtype == F32 and q.dtype == F32
    return d2, q, region


def face_records(A):
    """(a, ab, ac) of every face: v0's position and the edges to v1 and v2, read by name (GPUFace: v0, v2, v1)."""
    a = A.vpos[A.faces[:, 0]]
    return a, A.vpos[A.faces[:, 2]] - a, A.vpos[A.faces[:, 1]] - a


def _first_min(d2, r2):
    """Index of the lexicographic (d2, index) minimum among d2 <= r2, or -1."""
    ok = d2 <= r2
    if not ok.any():
        return -1
    m = d2[ok].min()
    return int(np.flatnonzero(ok & (d2 == m))[0])


def closest(arrays, points, details=False, rows=16, block=4096):
    """points: (N, 4) float32 rt_point rows.  Returns (N, 8) float32 rt_nearest rows; with details=True also the
    winner's d2 (N,; NaN on a miss).  `rows` points against `block` faces at a time (arrays that stay in the cache):
    the blocks come in face order, so a later block replaces a point's face only with a strictly smaller d2."""
    A = arrays if isinstance(arrays, Q.Arrays) else Q.Arrays(arrays)
    pts = np.ascontiguousarray(points, dtype=F32).reshape(-1, 4)
    n = pts.shape[0]
    out = np.zeros((n, 8), dtype=F32)
    out_u = out.view(np.uint32)
    out_u[:, 0] = pts[:, 3].view(np.uint32)  # a miss: the radius as passed, zeros
    best_d2 = np.full(n, np.nan, dtype=F32)
    a, ab, ac = face_records(A)
    nf = a.shape[0]
    with np.errstate(all="ignore"):
        r2s = pts[:, 3] * pts[:, 3]
    for i0 in range(0, n, rows):
        p = pts[i0:i0 + rows, 0:3]
        np_ = p.shape[0]
        face = [None] * np_  # (d2, id, q, region)
        for f0 in range(0, nf, block):
            fd2, fq, freg = face_candidates(p, a[f0:f0 + block], ab[f0:f0 + block], ac[f0:f0 + block])
            for j in range(np_):
                f = _first_min(fd2[j], r2s[i0 + j])
                if f >= 0 and (face[j] is None or fd2[j, f] < face[j][0]):
                    face[j] = (fd2[j, f], f0 + f, fq[j, f].copy(), freg[j, f])
        sd2, sq = sphere_candidates(p, A.sph_c, A.sph_r)
        for j in range(np_):
            i = i0 + j
            s = _first_min(sd2[j], r2s[i])
            if s >= 0 and (face[j] is None or sd2[j, s] <= face[j][0]):  # kind 1 before kind 2 on a tie
                out[i, 0] = np.sqrt(sd2[j, s])
                out_u[i, 1:4] = (1, s, np.uint32(A.sph_mat[s].astype(np.uint32)))
                out[i, 4:7] = sq[j, s]
                best_d2[i] = sd2[j, s]
            elif face[j] is not None:
                d2, f, q, reg = face[j]
                out[i, 0] = np.sqrt(d2)
                out_u[i, 1:4] = (2, f, A.faces[f, 3])
                out[i, 4:7] = q
                out_u[i, 7] = reg
                best_d2[i] = d2
    return (out, best_d2) if details else out


def fields(rec):
    u = np.ascontiguousarray(rec, dtype=F32).view(np.uint32).reshape(-1, 8)
    return {"distance": u[:, 0].view(F32), "kind": u[:, 1], "id": u[:, 2], "material": u[:, 3],
            "point": u[:, 4:7].view(F32), "region": u[:, 7]}
