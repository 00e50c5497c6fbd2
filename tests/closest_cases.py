"""Scenes and point sets of the closest-point tests, shared by tests/test_closest_cpu.py and tests/test_gpu_closest.py.
Everything is deterministic: constructed points, fixed seeds.  A scene comes built (host arrays, no device); the GPU
tests upload it.

  hand()            the hand-built scene of tests/test_gpu_query.py (two axis-aligned quads, three spheres; every
                    triangle is a leaf of its own with a flat box) and points placed by construction, by family
  adversarial(name) scenes A, B (leaf tree) and C:above_2p62 (outside the cull's range) of adversarial_cases.py; the
                    points are their rays' origins plus the vertices and edge midpoints of the sliver and degenerate
                    triangles
  product(which)    bunny / bunny4 with 4096 points: a third uniform in the root box, a third on and near the surface
                    (first hits of camera rays from query_ref), a third 2 to 8 box diagonals away; half of all with a
                    finite radius
  deck(name, spheres) scene_cases.py's decks (BVHs 29 / 39 / 62 levels deep: the stack-40 and stack-64 builds, and the
                    deepest scene allowed), as they are or without their sphere, with 64 points: the deck's apex
                    (0, 0, 0) with radius inf, the rest uniform in +-3; every fourth with radius 0.5
"""
import functools

import numpy as np

import adversarial_cases as AC
import query_ref as Q
import rt_testlib as T
import scene_cases as SC

F32 = np.float32
INF = np.inf
SPHERES = [((1.0, 1.0, 3.0), 0.5, 3), ((0.0, 3.0, 0.0), 1.0, 1), ((0.0, 0.0, 0.0), 1.0, 0)]  # test_gpu_query.py's


def arrays_of(scene):
    """query_ref.Arrays of a built Scene, spheres and materials included."""
    a = dict(scene.host_arrays())
    a["spheres"], a["materials"] = scene.spheres().view(np.uint32), scene.materials()
    return Q.Arrays(a)


def same_records(got, want, what):
    """Bytewise equality of whole record buffers; the first difference on failure."""
    g = np.ascontiguousarray(got, F32).view(np.uint32).reshape(-1, 8)
    w = np.ascontiguousarray(want, F32).view(np.uint32).reshape(-1, 8)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.flatnonzero((g != w).any(axis=1))
    if bad.size:
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.size} of {g.shape[0]} records differ; first {i}:\n got  {g[i].view(F32)} {g[i]}\n"
                             f" want {w[i].view(F32)} {w[i]}")


# --- the hand-built scene ---------------------------------------------------------------------------------------------
def hand_scene():
    rt = T.load_rt()
    s = rt.Scene()
    s.add_material(albedo=(0.5, 0.5, 0.5))
    s.add_material(albedo=(0.9, 0.1, 0.1), emissive=(1, 2, 3))
    s.add_material(albedo=(0.1, 0.9, 0.1))
    s.add_material(albedo=(0.1, 0.1, 0.9), emissive=(0.5, 0.25, 0.125))
    s.add_quad((-2, -2, 5), (2, -2, 5), (2, 2, 5), (-2, 2, 5), 1)
    s.add_quad((4, -2, -2), (4, 2, -2), (4, 2, 2), (4, -2, 2), 2)
    for c, r, m in SPHERES:
        s.add_sphere(c, r, m)
    s.set_viewport(16, 16)
    s.build()
    return s


def hand_points(A):
    """(points (N, 4), {family: indices}).  Families: regions, on, above, ties, spheres, radius, nonfinite, random."""
    pts, fam = [], {}

    def put(name, p, radius=INF):
        fam.setdefault(name, []).append(len(pts))
        pts.append((*[float(x) for x in p], float(radius)))

    # over each triangle's interior, beyond each edge and beyond each corner, on both sides of its plane
    for f in range(A.faces.shape[0]):
        v = A.vpos[A.faces[f, 0:3]].astype(np.float64)
        n = np.cross(v[1] - v[0], v[2] - v[0])
        n = n / np.abs(n).max() * 0.25  # the quads are axis-aligned: a dyadic step off the plane
        c = v.mean(axis=0)
        for side in (1.0, -1.0):
            put("regions", (v[0] * 0.5 + v[1] * 0.25 + v[2] * 0.25) + n * side)
            for i in range(3):
                j, k = (i + 1) % 3, (i + 2) % 3
                mid = (v[i] + v[j]) * 0.5
                put("regions", mid + (mid - v[k]) * 0.375 + n * side)
                put("regions", v[i] + (v[i] - c) * 0.5 + n * side)
    # exactly on a vertex, an edge and a face: d2 == 0
    for p in ((2, -2, 5), (0, -2, 5), (1, -1, 5), (4, 2, 2), (4, 0.5, -2), (4, 0.5, -1)):
        put("on", p)
    # straight above a quad, off its diagonal: the leaf's box is flat, so the distance to the box is the distance
    for x, y in ((1.0, -1.0), (1.3, -0.7), (0.9, -1.9), (-1.1, 0.3), (-0.25, 1.75)):
        for z in (5.5, 7.0, 9.125, 5.0 + 2.0 ** -10):
            put("above", (x, y, z))
    for y, z in ((1.0, -1.0), (1.1, -0.3), (1.7, 0.2), (-0.6, 1.9)):
        for x in (4.5, 6.0, 4.0 + 2.0 ** -9):
            put("above", (x, y, z))
    # equidistant: over the quads' diagonals (two faces), and at 0.75 from both the first sphere and the quad behind it
    for p in ((-1, -1, 4.5), (0.5, 0.5, 6.0), (-1.5, -1.5, 5.25), (4.5, 1, 1), (5, -0.5, -0.5)):
        put("ties", p)
    put("ties", (1, 1, 4.25))
    # inside and at the centre of a sphere
    for p in ((0.25, 0, 0), (0, 0, 0), (0, 3, 0), (1, 1, 3.25), (0, 2.5, 0.125), (0.3, 0.4, 0.5)):
        put("spheres", p)
    # radius: 0 on the surface and off it; the exact distance and the float below it; inf, NaN, negative
    below = float(np.nextafter(F32(0.75), F32(0)))
    for p, r in (((2, -2, 5), 0.0), ((1, -1, 4.25), 0.0), ((1, -1, 4.25), 0.75), ((1, -1, 4.25), below), ((1, -1, 4.25), INF),
                 ((1, -1, 4.25), np.nan), ((1, -1, 4.25), -0.75), ((1, -1, 4.25), -below), ((0.25, 0, 0), 0.75),
                 ((0.25, 0, 0), below), ((6, 1, -1), 2.0), ((6, 1, -1), float(np.nextafter(F32(2), F32(0)))), ((30, 30, 30), 1.0),
                 ((30, 30, 30), -INF)):
        put("radius", p, r)
    # NaN and +-inf coordinates
    for val in (np.nan, INF, -INF):
        for k in range(3):
            for r in (INF, 3.0):
                p = [1.0, -1.0, 4.25]
                p[k] = val
                put("nonfinite", p, r)
    put("nonfinite", (np.nan, np.nan, np.nan))
    put("nonfinite", (INF, -INF, INF))
    g = np.random.default_rng(20251021)
    for i in range(121):
        put("random", g.uniform(-4.0, 8.0, size=3), INF if i % 3 else g.uniform(0.5, 3.0))
    out = np.array(pts, dtype=F32)
    assert len(out) % 64 != 0
    return out, {k: np.array(v) for k, v in fam.items()}


@functools.lru_cache(maxsize=None)
def hand():
    s = hand_scene()
    A = arrays_of(s)
    points, families = hand_points(A)
    return {"scene": s, "arrays": A, "points": points, "families": families}


def leaf_boxes(A):
    """face id -> (bmin, bmax) of the leaf that holds it."""
    out = {}
    for node in np.flatnonzero(A.count > 0):
        for f in A.face_indices[A.first[node]:A.first[node] + A.count[node]]:
            out[int(f)] = (A.bmin[node], A.bmax[node])
    return out


def plain_box_d2(p, lo, hi):
    """The squared distance from p to the box, as the textbook states it (fp32, the contract's dot): no slack."""
    p, lo, hi = (np.asarray(x, F32) for x in (p, lo, hi))
    g = np.maximum(np.maximum(lo - p, p - hi), F32(0))
    return (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]


# --- the adversarial scenes -------------------------------------------------------------------------------------------
ADVERSARIAL = ("A", "B", "C:above_2p62")


@functools.lru_cache(maxsize=None)
def adversarial(name):
    """The built case and its points.  Scene B's mirror (its leaf tree) is made under AC.build_options(rt, True): the GPU
    test uploads inside that context."""
    rt = T.load_rt()
    case = AC.build_case(rt, name)
    rays, _ = AC.base_rays(case)
    pts = np.zeros((len(rays), 4), dtype=F32)
    pts[:, 0:3] = rays[:, 0:3]
    pts[:, 3] = INF
    pts[::3, 3] = 16.0
    extra = []
    for t, tag in enumerate(case.tags):
        if tag in ("sliver", "collinear", "repeated"):
            for target in AC._targets(case, t):
                extra.append((*target, INF))
                extra.append((*target, 2.0 ** -10))
    pts = np.concatenate([pts, np.array(extra, dtype=F32)])
    if len(pts) % 64 == 0:
        pts = pts[:-1]
    order = np.random.default_rng(20251022).permutation(len(pts))
    return {"case": case, "scene": case.scene, "arrays": arrays_of(case.scene), "points": np.ascontiguousarray(pts[order]),
            "tree": case.tree}


# --- the decks --------------------------------------------------------------------------------------------------------
DECKS = {"deck29": 29, "deck39": 39, "deck62": 62}  # name -> depth


@functools.lru_cache(maxsize=None)
def deck_scene(name, spheres=True):
    """The built deck.  Spheres are no part of the BVH: without its sphere the deck has the same nodes, and the kernel's
    best is still inf when the walk starts (first_descent_pushes)."""
    case = SC.BY_NAME[name]
    if not spheres:
        case = dict(case, prims=[p for p in case["prims"] if p[0] != "sphere"])
    s = SC.apply_product(T.load_rt(), case)
    s.build()
    return s


@functools.lru_cache(maxsize=None)
def deck(name, spheres=True):
    s = deck_scene(name, spheres)
    pts = np.zeros((64, 4), dtype=F32)
    pts[1:, 0:3] = np.random.default_rng(DECKS[name]).uniform(-3.0, 3.0, size=(63, 3))
    pts[:, 3] = INF
    pts[3::4, 3] = 0.5
    return {"scene": s, "arrays": arrays_of(s), "points": pts}


def first_descent_pushes(rt, A, p, best=INF):
    """The entries rt_closest.hip's walk pushes on its way from the root to the first leaf it reaches, replayed on the
    host node array with closest.h's bound (rt.closest_bound_host): the nearer child first, the other pushed when both
    are within `best` (squared) -- which no leaf has lowered yet."""
    node = pushes = 0
    while A.count[node] == 0:
        l = int(A.first[node])
        bl, br = (rt.closest_bound_host(p, A.bmin[c], A.bmax[c]) for c in (l, l + 1))
        tl, tr = not bl > best, not br > best
        if not (tl or tr):
            break
        pushes += tl and tr
        node = l if tl and (not tr or bl <= br) else l + 1
    return pushes


# --- the product scenes -----------------------------------------------------------------------------------------------
PRODUCT_POINTS = 4096


@functools.lru_cache(maxsize=None)
def product(which):
    s = T.product_scene(which)
    A = arrays_of(s)
    lo, hi = A.bmin[0].astype(np.float64), A.bmax[0].astype(np.float64)
    diag = float(np.linalg.norm(hi - lo))
    g = np.random.default_rng({"bunny": 31, "bunny4": 32}[which])
    n = PRODUCT_POINTS
    n1 = n2 = n // 3
    n3 = n - n1 - n2
    uniform = g.uniform(lo, hi, size=(n1, 3))
    # first hits of 32x18 camera rays: each once as it is (on the surface), then again a little off it along the normal
    osc = T.OracleScene(which)
    hits, _, _ = Q.trace(Q.Arrays(osc.arrays()), Q.camera_rays(osc.camera(32, 18), 32, 18))
    hit = hits[hits.view(np.uint32)[:, 1] != 0]
    assert len(hit) >= 256
    pick = np.concatenate([np.arange(len(hit)), g.integers(len(hit), size=n2)])[:n2]
    off = np.where(np.arange(n2) < len(hit), 0.0, g.uniform(-0.05, 0.05, size=n2))
    surface = hit[pick, 8:11].astype(np.float64) + hit[pick, 4:7].astype(np.float64) * off[:, None]
    d = g.normal(size=(n3, 3))
    far = (lo + hi) * 0.5 + d / np.linalg.norm(d, axis=1, keepdims=True) * (diag * g.uniform(2.0, 8.0, size=(n3, 1)))
    pts = np.zeros((n, 4), dtype=F32)
    pts[:, 0:3] = np.concatenate([uniform, surface, far])
    # half of all with a finite radius around the distance: a fraction of the distance to the nearest of 4096 vertices
    sample = A.vpos[g.choice(len(A.vpos), size=4096, replace=False)].astype(np.float64)
    p64 = pts[:, 0:3].astype(np.float64)
    proxy = np.sqrt(((p64[:, None, :] - sample[None, :, :]) ** 2).sum(axis=2).min(axis=1))
    pts[:, 3] = INF
    finite = g.permutation(n)[:n // 2]
    pts[finite, 3] = (proxy[finite] * g.uniform(0.3, 1.1, size=len(finite))).astype(F32)
    order = g.permutation(n)
    pts = np.ascontiguousarray(pts[order])
    return {"scene": s, "arrays": A, "points": pts, "finite": np.flatnonzero(np.isfinite(pts[:, 3])),
            "sample": np.arange(0, n, n // 64)[:64]}


def twins(A):
    """face id -> the face with the same v0 and the two edges swapped (the loader's second winding), where there is one."""
    a = A.vpos[A.faces[:, 0]]
    b, c = A.vpos[A.faces[:, 2]], A.vpos[A.faces[:, 1]]  # v1, v2 by name
    key = lambda x, y, z: np.ascontiguousarray(np.concatenate([x, y, z], axis=1)).view(np.dtype((np.void, 36)))[:, 0]
    first = {}
    for f, k in enumerate(key(a, b, c).tolist()):
        first.setdefault(k, f)
    return {f: first[k] for f, k in enumerate(key(a, c, b).tolist()) if k in first and first[k] != f}
