"""The inputs of the occlusion tests and the reference's answers for them, computed once per process and shared by
tests/test_occlusion_cpu.py (which checks that the cases are what they claim) and tests/test_gpu_occlusion.py
(which compares the GPU against them).  Nothing here needs a GPU."""
import functools

import numpy as np

import occlusion_ref as O
import query_ref as Q
import rt_testlib as T

F32 = np.float32
W, H = 64, 36      # the bunny's pixel-centre rays, as tests/test_gpu_query.py
AW, AH = 32, 18    # the AO frames and bunny4's camera rays
AO_SAMPLES, AO_RADIUS, AO_BIAS, AO_DIRECTIONS = 4, 8.0, 0.001, 64


def kinds(hits):
    return np.ascontiguousarray(hits, dtype=F32).reshape(-1, 12).view(np.uint32)[:, 1]


def unit_vectors(n, seed):
    v = np.random.default_rng(seed).normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32)


@functools.lru_cache(maxsize=None)
def bunny():
    """The bunny's reference arrays, its 64x36 pixel-centre rays and the reference's records for them."""
    osc = T.OracleScene("bunny")
    arrays = Q.Arrays(osc.arrays())
    rays = Q.camera_rays(osc.camera(W, H), W, H)
    hits, _, leaf_size = Q.trace(arrays, rays)
    assert (leaf_size > 8).any()  # rays ending in a big leaf: the wave-cooperative rounds are exercised
    return {"oracle": osc, "arrays": arrays, "rays": rays, "hits": hits}


@functools.lru_cache(maxsize=None)
def incoherent():
    """tests/test_gpu_query.py's 1041 incoherent rays (seed 20240607, every third ray at half its unbounded distance):
    (rays, the reference's records, the records of the same rays unbounded)."""
    b = bunny()
    n = 1041
    ref = b["hits"]
    hit = np.nonzero(kinds(ref) != 0)[0][:n]
    assert hit.size == n
    rays = np.zeros((n, 8), dtype=F32)
    rays[:, 0:3] = ref[hit, 8:11] + ref[hit, 4:7] * F32(0.01)
    rays[:, 3] = F32(1e30)
    rays[:, 4:7] = unit_vectors(n, 20240607)
    free, _, _ = Q.trace(b["arrays"], rays)
    rays[::3, 3] = free[::3, 0] * F32(0.5)
    want = free.copy()
    want[::3], _, _ = Q.trace(b["arrays"], rays[::3])
    return rays, want, free


@functools.lru_cache(maxsize=None)
def tmax_edges():
    """Every second hit ray of incoherent() re-sent with tmax = its hit distance t (the accept is `t < closest`: a
    miss unless something else lies nearer) and with tmax = nextafter(t, inf).  The second need NOT be occluded: a
    rounded hit distance can lie below its own leaf's rounded box entry, which the slab test then culls.
    (rays at t, rays just above t, the reference's bytes for each)."""
    rays, want, _ = incoherent()
    sel = np.nonzero(kinds(want) != 0)[0][::2]
    at, above = rays[sel].copy(), rays[sel].copy()
    at[:, 3] = want[sel, 0]
    above[:, 3] = np.nextafter(want[sel, 0], F32(np.inf))
    arrays = bunny()["arrays"]
    return at, above, O.occluded(arrays, at), O.occluded(arrays, above)


@functools.lru_cache(maxsize=None)
def bunny4():
    """bunny4's reference arrays and the reference's records of its 32x18 pixel-centre rays (a leaf of >= 1024
    triangles is hit: the leaf-tree kernel's ground)."""
    osc = T.OracleScene("bunny4")
    arrays = Q.Arrays(osc.arrays())
    rays = Q.camera_rays(osc.camera(AW, AH), AW, AH)
    hits, _, leaf_size = Q.trace(arrays, rays)
    assert leaf_size.max() >= 1024
    return {"oracle": osc, "arrays": arrays, "rays": rays, "hits": hits}


@functools.lru_cache(maxsize=None)
def ao_directions():
    return T.load_rt().ao_directions(AO_DIRECTIONS)


@functools.lru_cache(maxsize=None)
def ao_case(which):
    """The reference's AO image of `which` ("bunny" or "bunny4") at 32x18 over the reference's own camera records:
    dict(arrays, hits, ao [AH * AW], occ (per valid pixel), valid)."""
    if which == "bunny4":
        arrays, hits = bunny4()["arrays"], bunny4()["hits"]
    else:
        b = bunny()
        arrays = b["arrays"]
        hits, _, _ = Q.trace(arrays, Q.camera_rays(b["oracle"].camera(AW, AH), AW, AH))
    ao, occ, valid = O.ao(arrays, hits, AW, AH, ao_directions(), AO_SAMPLES, AO_RADIUS, AO_BIAS)
    return {"arrays": arrays, "hits": hits, "ao": ao, "occ": occ, "valid": valid}
