"""Scenes, ray sets and reference lists of the rt_trace_hits tests, shared by tests/test_hits_cpu.py and
tests/test_gpu_hits.py.  Everything is deterministic; every reference is computed once per process (hits_ref.trace on
query_ref.Arrays) and left unchanged.

  rays(name)              (arrays, rays (N, 8)) of a named set:
      bunny        the 64x36 pixel-centre rays of the bunny scene
      incoherent   1,041 rays from first hits of those, random unit directions, every third tmax halved
      bunny4       the 32x18 pixel-centre rays of the four-bunny scene (its big leaf has a leaf tree)
      hand         tests/test_gpu_query.py's hand-built scene (two quads, three spheres) and its rays
      box          a closed single-sided box (add_quad x 6) and rays from 512 points around it
      advA, advB   adversarial_cases.py's pinwheel scenes (coplanar triangles with twins: a big leaf / a leaf tree)
                   with every fourth ray of their ray sets
      deck29, deck39, deck62   scene_cases.py's decks (BVHs 29 / 39 / 62 levels deep: the stack-40 and stack-64 builds, and
                   the deepest scene allowed) with the 53x29 pixel-centre rays of their camera, at the deck's apex
  reference(name, k, flags)   hits_ref.trace of that set
  scene(name)             the built (not uploaded) Scene of a named set
"""
import functools

import numpy as np

import adversarial_cases as AC
import closest_cases as CC
import hits_ref as HR
import query_ref as Q
import rt_testlib as T
import scene_cases as SC

F32 = np.float32
W, H = 64, 36
W4, H4 = 32, 18
DECKS = CC.DECKS  # name -> depth
BOX_LO, BOX_HI = np.array([-1.0, -0.5, 2.0]), np.array([1.5, 1.0, 4.0])
DIRECTIONS = ((0.36, 0.48, 0.8), (-0.6, 0.64, -0.48), (0.8, -0.36, 0.48))  # contains()'s


def unit_vectors(n, seed):
    v = np.random.default_rng(seed).normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32)


def box_points(n=512, seed=11):
    """Points uniform in the box grown by half its size (a quarter of the size on every side), and whether each lies
    strictly inside the box (none is within 1e-3 of a face)."""
    size = BOX_HI - BOX_LO
    g = np.random.default_rng(seed)
    pts = np.zeros((0, 3))
    while len(pts) < n:
        p = g.uniform(BOX_LO - 0.25 * size, BOX_HI + 0.25 * size, size=(n, 3))
        near = (np.abs(p - BOX_LO) < 1e-3).any(axis=1) | (np.abs(p - BOX_HI) < 1e-3).any(axis=1)
        pts = np.concatenate([pts, p[~near]])
    pts = pts[:n].astype(F32)
    inside = ((pts > BOX_LO) & (pts < BOX_HI)).all(axis=1)
    return pts, inside


def box_scene():
    rt = T.load_rt()
    s = rt.Scene()
    s.add_material(albedo=(0.5, 0.5, 0.5))
    (x0, y0, z0), (x1, y1, z1) = BOX_LO, BOX_HI
    c = lambda x, y, z: (float(x), float(y), float(z))
    # outward windings: cross(b - a, c - a) points out of the box
    s.add_quad(c(x0, y0, z0), c(x0, y1, z0), c(x1, y1, z0), c(x1, y0, z0), 0)  # z = z0
    s.add_quad(c(x0, y0, z1), c(x1, y0, z1), c(x1, y1, z1), c(x0, y1, z1), 0)  # z = z1
    s.add_quad(c(x0, y0, z0), c(x0, y0, z1), c(x0, y1, z1), c(x0, y1, z0), 0)  # x = x0
    s.add_quad(c(x1, y0, z0), c(x1, y1, z0), c(x1, y1, z1), c(x1, y0, z1), 0)  # x = x1
    s.add_quad(c(x0, y0, z0), c(x1, y0, z0), c(x1, y0, z1), c(x0, y0, z1), 0)  # y = y0
    s.add_quad(c(x0, y1, z0), c(x0, y1, z1), c(x1, y1, z1), c(x1, y1, z0), 0)  # y = y1
    s.set_viewport(16, 16)
    s.build()
    return s


@functools.lru_cache(maxsize=None)
def scene(name):
    rt = T.load_rt()
    if name in ("bunny", "incoherent"):
        return T.product_scene("bunny", W, H)
    if name == "bunny4":
        return T.product_scene("bunny4", W4, H4)
    if name == "hand":
        return CC.hand_scene()
    if name == "box":
        return box_scene()
    if name in ("advA", "advB"):
        return adversarial(name).scene
    if name in DECKS:
        return CC.deck_scene(name)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def adversarial(name):
    rt = T.load_rt()
    with AC.build_options(rt, name == "advB"):
        return AC.build_case(rt, name[-1])


def hand_rays():
    """tests/test_gpu_query.py's own ray table (rays, number of named cases), imported."""
    import test_gpu_query as GQ
    return GQ.handmade_rays()


@functools.lru_cache(maxsize=None)
def rays(name):
    if name == "bunny":
        osc = T.OracleScene("bunny")
        return Q.Arrays(osc.arrays()), Q.camera_rays(osc.camera(W, H), W, H)
    if name == "incoherent":
        A, cam = rays("bunny")
        ref, _, _ = Q.trace(A, cam)
        n = 1041  # not a multiple of 64
        hit = np.nonzero(ref.view(np.uint32)[:, 1] != 0)[0][:n]
        assert hit.size == n
        r = np.zeros((n, 8), dtype=F32)
        r[:, 0:3] = ref[hit, 8:11] + ref[hit, 4:7] * F32(0.01)
        r[:, 3] = F32(1e30)
        r[:, 4:7] = unit_vectors(n, 20240607)
        free, _, _ = Q.trace(A, r[::3])
        r[::3, 3] = np.where(free.view(np.uint32)[:, 1] != 0, free[:, 0] * F32(0.5), F32(1e30))
        return A, r
    if name == "bunny4":
        osc = T.OracleScene("bunny4")
        return Q.Arrays(osc.arrays()), Q.camera_rays(osc.camera(W4, H4), W4, H4)
    if name == "hand":
        return CC.arrays_of(scene("hand")), hand_rays()[0]
    if name == "box":
        pts, _ = box_points()
        r = np.zeros((len(pts), 8), dtype=F32)
        r[:, 0:3], r[:, 3] = pts, F32(1e30)
        r[:, 4:7] = np.array(DIRECTIONS, dtype=F32)[np.arange(len(pts)) % 3]
        return CC.arrays_of(scene("box")), r
    if name in ("advA", "advB"):
        case = adversarial(name)
        base, _ = AC.base_rays(case)
        return case.arrays(), np.ascontiguousarray(base[::4])
    if name in DECKS:
        s, w, h = scene(name), *SC.ROOM_SIZE
        return CC.arrays_of(s), Q.camera_rays(np.frombuffer(bytes(s.camera()), dtype=F32), w, h)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def reference(name, k, flags=0):
    A, r = rays(name)
    return HR.trace(A, r, k, flags)


@functools.lru_cache(maxsize=None)
def deck_pending(name):
    """Per ray of a deck under COUNT_ALL (nothing is cut: the deepest walk), the most entries the kernel's stack holds."""
    A, r = rays(name)
    return HR.trace(A, r, 1, HR.COUNT_ALL, pending=True)[2]


def same_rows(got, want, what, nan_payload_free=False):
    """Bytewise equality of whole (N, K, 12) record buffers, the first difference on failure.  nan_payload_free (the
    adversarial sets, whose non-finite rays give NaN positions): float words that are NaN on both sides may differ in
    payload, which is the ISA's choice (the rule of tests/test_gpu_adversarial.py); everything else stays bytewise."""
    g = np.ascontiguousarray(got, F32).reshape(-1, 12)
    w = np.ascontiguousarray(want, F32).reshape(-1, 12)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    gu, wu = g.view(np.uint32), w.view(np.uint32)
    bad = gu != wu
    if nan_payload_free:
        floats = np.ones(12, dtype=bool)
        floats[1:4] = False
        bad &= ~(np.isnan(g) & np.isnan(w) & floats)
    rows = np.flatnonzero(bad.any(axis=1))
    if rows.size:
        i = int(rows[0])
        k = np.asarray(want).shape[-2] if np.asarray(want).ndim == 3 else 1
        raise AssertionError(f"{what}: {rows.size} of {g.shape[0]} rows differ; first: ray {i // k} row {i % k}\n got  {g[i]} {gu[i, 1:4]}\n"
                             f" want {w[i]} {wu[i, 1:4]}")
