"""Reference for the occlusion queries (rt_occluded) and the AO pass on them (rt_ao).

occluded() is query_ref.trace's `kind != 0`, nothing else: the contract of rt_occluded is stated in terms of
rt_trace_rays' records.  ao_rays() / ao() restate rt_abi.h's AO arithmetic in numpy float32 -- one operation per
numpy call, so nothing is contracted -- with query_ref.normalize (liboracle's glm restatement) and the hash in
Python integers masked to 32 bits.
"""
import numpy as np

import query_ref as Q

F32 = np.float32
M32 = 0xFFFFFFFF


def occluded(arrays, rays):
    """uint8 [N]: whether query_ref.trace reports a hit for each (N, 8) rt_ray row."""
    hits, _, _ = Q.trace(arrays, rays)
    return (hits.view(np.uint32)[:, 1] != 0).astype(np.uint8)


def direction_index(i, k, direction_count):
    return (((i * 0x9E3779B1 + k * 0x85EBCA6B) & M32) >> 8) % direction_count


def ao_rays(hits, w, h, directions, samples, radius, bias):
    """(pixel indices of the valid records [V], rays [V * samples, 8]): ray v * samples + k is sample k of
    valid pixel v."""
    hits = np.ascontiguousarray(hits, dtype=F32).reshape(-1, 12)[:w * h]
    directions = np.ascontiguousarray(directions, dtype=F32).reshape(-1, 4)
    valid = np.nonzero(hits.view(np.uint32)[:, 1] != 0)[0]
    rays = np.zeros((valid.size * samples, 8), dtype=F32)
    bias, radius = F32(bias), F32(radius)
    with np.errstate(all="ignore"):
        for v, i in enumerate(valid):
            n, P = hits[i, 4:7], hits[i, 8:11]
            e = bias * hits[i, 0]
            o = P + n * e
            for k in range(samples):
                s = directions[direction_index(int(i), k, directions.shape[0]), 0:3]
                d0 = n + s
                dd = (d0[0] * d0[0] + d0[1] * d0[1]) + d0[2] * d0[2]
                d = Q.normalize(d0) if dd > F32(1e-6) else n
                r = rays[v * samples + k]
                r[0:3], r[3], r[4:7] = o, radius, d
    return valid, rays


def ao(arrays, hits, w, h, directions, samples, radius, bias):
    """(ao [h * w] float32, per-pixel occluded counts of the valid pixels [V], valid pixel indices [V])."""
    valid, rays = ao_rays(hits, w, h, directions, samples, radius, bias)
    occ = occluded(arrays, rays).reshape(-1, samples).astype(np.int64).sum(axis=1)
    out = np.ones(w * h, dtype=F32)
    out[valid] = (samples - occ).astype(F32) / F32(samples)
    return out, occ, valid
