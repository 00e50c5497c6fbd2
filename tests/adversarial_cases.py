"""Adversarial scenes and rays for the production traversal's error bounds (csrc/rt_fast.h): shared by
tests/test_adversarial_cpu.py and tests/test_gpu_adversarial.py.  Everything here is deterministic: dyadic
coordinates, fixed seeds.

Scenes (caller-built geometry, no asset):

  A  "pinwheel": K base triangles with the bit-identical fp32 centroid C -- vertices C + a, C + b, C - a - b with
     short dyadic a, b, so both vertex sums are exact and BVH::Subdivide (scene.cpp) can never split them apart --
     each added twice, wound both ways: the (v0, e1, e2) / (v0, e2, e1) pair the mirror's build_twins looks for.
     One leaf of 2K triangles: well-shaped ones with edges from 2^-10 to 2^6, slivers, axis-aligned planes, two
     coplanar overlapping triangles, a collinear one and one with a repeated vertex.  A few axis-aligned
     triangles in small (flat-boxed) leaves nearer and farther, one sphere in front of the leaf and one behind.
  B  the same with K = 160 and rt_build_options.leaf_tree_min = 64: the big leaf gets a leaf tree (MODE 21).
  C  A plus one triangle with a coordinate at, or one float beyond, a gate of the mirror's `fast` flag.

Rays: (N, 8) float32 rt_ray rows in seven families (FAMILIES), shuffled with a fixed seed so that every wave
mixes filtered and exact lanes, hits and misses; N is not a multiple of 64.
"""
import contextlib

import numpy as np

import query_ref as Q
import rt_testlib as T

F32 = np.float32
C = np.array([2.0, -1.0, 64.0])  # the shared centroid
BIG = 1e30

FAMILIES = {1: "boundary", 2: "grazing", 3: "distance sweep", 4: "tmax edges", 5: "ray gates", 6: "non-finite",
            7: "random"}

# (centre, radius, material): [0] lies in front of the big leaf for rays from the near origins, [1] behind it
SPHERES = [((-9.0, 7.0, 26.0), 2.5, 2), ((40.0, 30.0, 110.0), 12.0, 3)]

# separate triangles in small leaves, each in an axis-aligned plane (a flat leaf box); the last one is added twice
EXTRAS = [
    ((1.0, -2.0, 12.0), (3.0, -2.0, 12.0), (1.0, 0.0, 12.0)),
    ((-6.0, 4.0, 20.0), (-6.0, 8.0, 20.0), (-6.0, 4.0, 24.0)),
    ((0.0, -3.0, 30.0), (4.0, -3.0, 30.0), (0.0, -3.0, 34.0)),
    ((50.0, -10.0, 120.0), (50.0, 20.0, 120.0), (50.0, -10.0, 140.0)),
    ((10.0, 10.0, 150.0), (60.0, 10.0, 150.0), (10.0, 60.0, 150.0)),
    ((-20.0, -20.0, 130.0), (30.0, -20.0, 130.0), (-20.0, 30.0, 130.0)),
]

ORIENTATIONS = [((2, 0, 1), (-1, 2, 0)), ((0, 2, -1), (1, -1, 2)), ((1, 1, 0), (-1, 1, 1)), ((1, 0, -2), (0, 1, 1)),
                ((2, 1, 1), (0, -1, 2)), ((1, -2, 0), (1, 1, 1))]

# the special base triangles (a, b, tag); every scene holds all of them
SPECIAL = [
    ((8.0, 0.0, 0.0), (0.0, 2.0 ** -10, 2.0 ** -10), "sliver"),
    ((0.0, 2.0, 2.0), (2.0 ** -11, -2.0 ** -11, 0.0), "sliver"),
    ((16.0, 8.0, 0.0), (0.0, 0.0, 2.0 ** -8), "sliver"),
    ((2.0 ** -4, 0.0, 2.0 ** -4), (0.0, 2.0 ** -18, 0.0), "sliver"),
    ((2.0, 0.0, 0.0), (0.0, 2.0, 0.0), "coplanar"),       # plane z = C.z
    ((1.0, 0.5, 0.0), (-0.5, 1.0, 0.0), "coplanar"),      # the same plane, inside the first
    ((0.0, 4.0, 0.0), (0.0, 0.0, -4.0), "axis"),          # plane x = C.x
    ((0.25, 0.0, 0.0), (0.0, 0.0, 0.5), "axis"),          # plane y = C.y
    ((5.0, 3.0, 1.5), (10.0, 6.0, 3.0), "collinear"),     # C + a, C + 2a, C - 3a
    ((1.5, -0.5, 2.0), (1.5, -0.5, 2.0), "repeated"),     # C + a twice
]


def base_triangles(k, grouped=False):
    """k (a, b, tag) triples: the SPECIAL ones, then well-shaped ones, one orientation and one scale each, the scales
    running over 2^-10 .. 2^4 (edges 2^-10 .. 2^6) and, past the first 15 per orientation, 1.5 times those.
    grouped: the well-shaped ones ordered by orientation, then scale -- a leaf tree splits by normals and then,
    the centroids being equal, in leaf order, so its clusters then hold similar scales and the small ones have
    small boxes, which a cull can miss."""
    well = []
    for i in range(k - len(SPECIAL)):
        o = i % len(ORIENTATIONS)
        (ax, ay, az), (bx, by, bz) = ORIENTATIONS[o]
        step = i // len(ORIENTATIONS)
        # 7 and 15 are coprime: consecutive triangles of one orientation are far apart in scale
        s = 2.0 ** (-10 + (7 * step + 2 * o) % 15) * (1.5 if (step // 15) % 2 else 1.0)
        well.append((o, s, ((ax * s, ay * s, az * s), (bx * s, by * s, bz * s), "well")))
    if grouped:
        well.sort(key=lambda w: w[0:2])
    return list(SPECIAL) + [w[2] for w in well]


def aspect_ratio(a, b):
    """longest edge / the height on it, of the triangle C + a, C + b, C - a - b."""
    a, b = np.asarray(a, float), np.asarray(b, float)
    edges = [a - b, 2 * a + b, a + 2 * b]
    longest = max(np.linalg.norm(e) for e in edges)
    area2 = np.linalg.norm(np.cross(a - b, 2 * a + b))
    return np.inf if area2 == 0 else longest * longest / area2


# the extra triangle of the C variants: one coordinate at, or one float beyond, a gate of mirror.cpp's `fast` flag
def _gate_values():
    hi, lo = F32(2.0 ** 62), F32(2.0 ** -60)
    return {"at_2p62": (float(hi), True), "above_2p62": (float(np.nextafter(hi, F32(np.inf))), False),
            "at_2m60": (float(lo), True), "below_2m60": (float(np.nextafter(lo, F32(0))), False),
            "subnormal": (float(F32(2.0 ** -140)), False)}


# The base triangle whose first winding is added after every other pinwheel triangle: the leaf then holds a twin
# far from its triangle, so a unit's twin can be a candidate at a higher leaf position than triangles that
# later quads offer at the same distance -- the tie rule then has to replace a candidate, not just keep one.
FAR_TWIN = 3

GATES = _gate_values()  # variant -> (the coordinate, whether the scene is still inside the filtered range)


class Case:
    """A built (not uploaded) scene and what the ray builders and the checks need to know about it."""

    def __init__(self, name, scene, bases, tree, faces):
        self.name, self.scene, self.bases, self.tree = name, scene, bases, tree
        self.k = len(bases)
        # face id -> base triangle, and -> winding (0: as listed, 1: the twin); faces 0 .. 2k - 1 are the pinwheel
        self.base_of, self.winding_of = np.zeros(2 * self.k, np.int64), np.zeros(2 * self.k, np.int64)
        for (i, w), f in faces.items():
            self.base_of[f], self.winding_of[f] = i, w
        # pinwheel vertices in float64 (exact: they are short dyadic numbers), original winding
        self.verts = np.array([[C + a, C + b, C - np.asarray(a) - np.asarray(b)] for a, b, _ in bases])
        self.tags = [t for _, _, t in bases]

    def arrays(self):
        """The reference arrays of query_ref.trace (as the `handmade` fixture of test_gpu_query.py builds them)."""
        a = dict(self.scene.host_arrays())
        sph = np.zeros((len(SPHERES), 8), dtype=np.uint32)
        for i, (c, r, m) in enumerate(SPHERES):
            sph[i, 0:4] = np.array([*c, r], dtype=F32).view(np.uint32)
            sph[i, 4] = m
        a["spheres"], a["materials"] = sph, self.scene.materials()
        return Q.Arrays(a)

    def big_leaf(self):
        """(node index, first, count) of the pinwheel's leaf in host_arrays()["nodes"]."""
        nodes = self.scene.host_arrays()["nodes"].view(np.uint32).reshape(-1, 8)
        at = np.flatnonzero(nodes[:, 7] == 2 * self.k)
        assert at.size == 1, f"{self.name}: leaves of {2 * self.k} triangles: {at.size}; leaf sizes {sorted(set(nodes[:, 7].tolist()))}"
        return int(at[0]), int(nodes[at[0], 6]), int(nodes[at[0], 7])


@contextlib.contextmanager
def build_options(rt, tree):
    """rt_build_options.leaf_tree_min = 64 for a tree scene (process-wide; the mirror is built at upload and by
    Scene.mirror), restored afterwards."""
    if tree:
        rt.set_build_options(leaf_tree_min=64)
    try:
        yield
    finally:
        if tree:
            rt.set_build_options()


def build_case(rt, name):
    """name: "A", "B", or "C:<variant>" (a key of GATES).  The scene is built on the host (camera + BVH), not
    uploaded; a tree scene's mirror must be made inside build_options(rt, True)."""
    tree = name == "B"
    bases = base_triangles(160, grouped=True) if tree else base_triangles(24)
    s = rt.Scene()
    s.add_material(albedo=(0.7, 0.7, 0.7), emissive=(0.25, 0.5, 0.125))
    s.add_material(albedo=(0.7, 0.2, 0.2), specular=(0.9, 0.9, 0.9), specular_percent=0.3, roughness=0.2)
    s.add_material(albedo=(0.1, 0.1, 0.1), emissive=(4.0, 3.0, 2.0))
    s.add_material(albedo=(0.2, 0.3, 0.8), emissive=(0.5, 0.25, 0.125))
    faces = {}  # (base, winding) -> face id; winding 0: (p, q, r), 1: (p, r, q), its twin
    late = []
    for i, (a, b, _) in enumerate(bases):
        p, q, r = C + a, C + b, C - np.asarray(a) - np.asarray(b)
        if i == FAR_TWIN:  # this one's first winding goes to the end of the leaf, far from its twin
            late.append((i, p, q, r))
        else:
            faces[i, 0] = len(faces)
            s.add_triangle(p, q, r, 0)
        faces[i, 1] = len(faces)
        s.add_triangle(p, r, q, 1)
    for i, p, q, r in late:
        faces[i, 0] = len(faces)
        s.add_triangle(p, q, r, 0)
    for i, (p, q, r) in enumerate(EXTRAS):
        s.add_triangle(p, q, r, i % 4)
    s.add_triangle(EXTRAS[-1][0], EXTRAS[-1][2], EXTRAS[-1][1], 1)
    for c, r, m in SPHERES:
        s.add_sphere(c, r, m)
    if name.startswith("C:"):
        g = GATES[name[2:]][0]
        if g > 1.0:
            s.add_triangle((g, 0.5, 70.0), (g, 1.0, 70.0), (3.0, 0.5, 72.0), 0)  # centroid past the root's midpoint: a leaf of its own
        else:
            s.add_triangle((g, 3.0, 40.0), (1.0, 3.0, 40.0), (g, 4.0, 41.0), 0)
    s.set_camera((1.5, -0.5, 48.0), 0.0, 180.0)  # looking along +z at the pinwheel, 16 in front of its centre
    s.set_viewport(32, 18)
    s.build()
    return Case(name, s, bases, tree, faces)


def expected_fast(nodes):
    """The scene half of rt_fast.h's range rule on reference nodes ((N, 8) 32-bit words): every bound component
    of every node is 0 or has a magnitude in [2^-60, 2^62]."""
    b = np.abs(np.ascontiguousarray(nodes).view(np.uint32).reshape(-1, 8)[:, 0:6].view(F32))
    return bool(((b == 0) | ((b >= F32(2.0 ** -60)) & (b <= F32(2.0 ** 62)))).all())


# --- rays -------------------------------------------------------------------------------------------------------------
NEAR_ORIGINS = [np.array(o) for o in ((0.5, 0.25, 1.0), (-24.0, 16.0, 8.0), (8.0, -4.0, 160.0), (-40.0, -30.0, 4.0))]


def _ray(o, d, tmax=BIG):
    r = np.zeros(8, dtype=F32)
    r[0:3], r[3], r[4:7] = np.asarray(o, F32), F32(tmax), np.asarray(d, F32)
    return r


def _aim(o, target, tmax=BIG):
    """From o through target: the direction is formed in fp32 from the fp32 origin and target."""
    o32, t32 = np.asarray(o, F32), np.asarray(target, F32)
    return _ray(o32, t32 - o32, tmax)


def _ulps(x, n):
    """x (float32) moved by n floats."""
    x = F32(x)
    for _ in range(abs(n)):
        x = np.nextafter(x, F32(np.inf if n > 0 else -np.inf))
    return x


def _targets(case, tri):
    """The three vertices and three edge midpoints of pinwheel triangle `tri` (exact dyadic points)."""
    v = case.verts[tri]
    return [v[0], v[1], v[2], (v[0] + v[1]) / 2, (v[1] + v[2]) / 2, (v[2] + v[0]) / 2]


def _probe_triangles(case):
    """The base triangles the per-triangle families visit: all of them, or for the tree scene the special ones and
    every tenth of the rest."""
    if case.k <= 32:
        return list(range(case.k))
    n = len(SPECIAL)
    return list(range(n)) + list(range(n, case.k, 10))


def base_rays(case, seed=20250607):
    """Families 1-3 and 5-7 as (rays, family) lists in generation order (family 4 needs the reference's
    distances: tmax_rays)."""
    g = np.random.default_rng(seed)
    rays, fam = [], []

    def put(f, r):
        rays.append(r)
        fam.append(f)

    def unit():
        v = g.normal(size=3)
        return v / np.linalg.norm(v)

    tris = _probe_triangles(case)
    # 1. boundary hits: through every vertex, edge midpoint and the shared centroid, from a general dyadic origin
    #    and along an axis (exact arithmetic: u, v or u + v lands on 0 or det); then the target moved by +-1, +-2
    #    floats in each coordinate
    n = 0
    for t in tris:
        for target in _targets(case, t) + ([C] if t == tris[0] else []):
            o = NEAR_ORIGINS[n % len(NEAR_ORIGINS)]
            put(1, _aim(o, target))
            axis = np.zeros(3)
            axis[n % 3] = 32.0 if (n // 3) % 2 else -32.0
            put(1, _aim(target - axis, target))
            for k in range(3):
                for step in (-2, -1, 1, 2):
                    moved = np.asarray(target, F32).copy()
                    moved[k] = _ulps(moved[k], step)
                    put(1, _aim(o, moved))
            n += 1
    # 2. grazing: an in-plane direction plus a normal part of 10^-1 .. 10^-8 of it, exactly in-plane, along an edge
    for i, t in enumerate(tris):
        v = case.verts[t]
        e = v[1] - v[0]
        nrm = np.cross(v[1] - v[0], v[2] - v[0])
        if not nrm.any():  # degenerate: any direction across the line
            nrm = np.cross(e if e.any() else v[2] - v[0], (0.0, 0.0, 1.0))
        nrm = nrm / np.linalg.norm(nrm)
        inplane = e if e.any() else v[2] - v[0]
        length = np.linalg.norm(inplane)
        inside = C + (v[0] - C) * 0.25  # a point inside the triangle
        for p in (1 + i % 8, 1 + (i + 4) % 8):
            d = inplane + nrm * length * 10.0 ** -p * (1 if i % 2 else -1)
            put(2, _ray(inside - d * 3.0, d))
        put(2, _ray(inside - inplane * 3.0, inplane))
        put(2, _ray(v[0] - inplane * 2.0, inplane))  # along the edge v0 -> v1
    # 3. distance sweep: the same targets from 2^-6 .. 2^12 away, dyadic and random directions; origins on a vertex
    #    and in the plane
    for i, t in enumerate(tris):
        target = _targets(case, t)[i % 6]
        for e in range(-6, 13):
            u = unit() if (e + i) % 2 else np.array([-0.5, 0.25, -1.0]) * (1 if i % 2 else -1)
            put(3, _aim(target + u * 2.0 ** e, target))
        v = case.verts[t]
        put(3, _aim(v[i % 3], C))                                   # origin on a vertex: dist = 0 for that corner
        put(3, _ray(C + (v[0] - C) * 0.5, unit()))                  # origin inside the triangle's plane
    for e in range(-6, 13):  # and the shared centroid, where every triangle of the leaf is hit at nearly one distance
        u = unit() if e % 2 else np.array([0.5, -1.0, 0.25])
        put(3, _aim(C + u * 2.0 ** e, C))
    # 5. ray gates: one direction or origin component at a gate of make_ray and at its float neighbours
    two20, twom40, sub = F32(2.0 ** 20), F32(2.0 ** -40), F32(2.0 ** -140)
    dvals = [_ulps(twom40, -1), twom40, _ulps(twom40, 1), _ulps(two20, -1), two20, _ulps(two20, 1), sub, F32(0.0), F32(-0.0)]
    two62, twom60 = F32(2.0 ** 62), F32(2.0 ** -60)
    ovals = [_ulps(twom60, -1), twom60, _ulps(twom60, 1), _ulps(two62, -1), two62, _ulps(two62, 1), sub, F32(-0.0)]
    other = [np.array(v) for v in ((0.0, 0.5, 1.0), (1.0, 0.0, -0.5), (-0.5, 1.0, 0.0))]
    for k in range(3):
        for sg in (1.0, -1.0):
            for val in dvals:
                d = other[k].astype(F32).copy()
                d[k] = F32(sg) * val
                # the line passes through C: the origin 48 in-plane units (or 2^-14 of a huge component) before it
                back = 48.0 if abs(float(val)) < 2.0 else 2.0 ** -14
                put(5, _ray((C - d.astype(np.float64) * back).astype(F32), d))
            for val in ovals:
                o = (C - other[k] * 48.0).astype(F32)
                o[k] = F32(sg) * val
                put(5, _aim(o, C))
    # 6. non-finite: NaN and +-inf in one origin component, one direction component, in tmax; the zero direction
    o, d = NEAR_ORIGINS[0].astype(F32), (C - NEAR_ORIGINS[0]).astype(F32)
    for val in (np.nan, np.inf, -np.inf):
        for k in range(3):
            o2, d2 = o.copy(), d.copy()
            o2[k] = val
            put(6, _ray(o2, d))
            d2[k] = val
            put(6, _ray(o, d2))
        put(6, _ray(o, d, val))
    put(6, _ray(o, (0.0, 0.0, 0.0)))
    put(6, _ray(C, (0.0, 0.0, 0.0)))
    put(6, _ray(o, (0.0, -0.0, 0.0), 5.0))
    # 7. random directions from random origins around the scene; a few at the two spheres
    for _ in range(280):
        put(7, _ray(C + g.uniform(-70.0, 70.0, size=3), unit() * g.uniform(0.5, 3.0)))
    for c, r, _ in SPHERES:
        for o in NEAR_ORIGINS:
            for _ in range(3):
                put(7, _aim(o, np.array(c) + unit() * r * 0.5))
    return np.array(rays, dtype=F32), np.array(fam)


def tmax_rays(rays, fam, hits, every=24):
    """Family 4 from the reference's records of families 1-3: every `every`-th triangle hit re-sent with tmax = t
    (a miss: strict <), the next float above (a hit) and the next float towards 0; and tmax = 0, -1, +inf.
    Returns (rays, kind) with kind 0: tmax = t, 1: next above, 2: next below, 3: the fixed values."""
    u = hits.view(np.uint32)
    hit = np.flatnonzero((u[:, 1] == 2) & (fam <= 3) & (hits[:, 0] > 0))[::every]
    out, kind = [], []
    for i in hit:
        t = hits[i, 0]
        for k, tm in enumerate((t, np.nextafter(t, F32(np.inf)), np.nextafter(t, F32(0)))):
            r = rays[i].copy()
            r[3] = tm
            out.append(r)
            kind.append(k)
    for i in hit[::4]:
        for tm in (0.0, -1.0, np.inf):
            r = rays[i].copy()
            r[3] = tm
            out.append(r)
            kind.append(3)
    return np.array(out, dtype=F32), np.array(kind)


class RaySet:
    """The shuffled rays of one scene with the reference's records: rays (N, 8), family (N,), want (N, 12),
    tmax_kind (N,; -1 outside family 4), seconds (the reference's time)."""


def ray_set(case, arrays=None, seed=20250607):
    import time
    arrays = arrays if arrays is not None else case.arrays()
    rays, fam = base_rays(case, seed)
    t0 = time.perf_counter()
    hits, _, _ = Q.trace(arrays, rays)
    r4, k4 = tmax_rays(rays, fam, hits)
    h4, _, _ = Q.trace(arrays, r4)
    seconds = time.perf_counter() - t0
    rays, hits = np.concatenate([rays, r4]), np.concatenate([hits, h4])
    fam = np.concatenate([fam, np.full(len(r4), 4)])
    kind = np.concatenate([np.full(len(fam) - len(r4), -1), k4])
    if len(rays) % 64 == 0:  # N is deliberately not a multiple of 64
        rays, hits, fam, kind = rays[:-1], hits[:-1], fam[:-1], kind[:-1]
    order = np.random.default_rng(seed + 1).permutation(len(rays))
    out = RaySet()
    out.rays, out.family, out.want, out.tmax_kind = (np.ascontiguousarray(x[order]) for x in (rays, fam, hits, kind))
    out.seconds = seconds
    return out


def glm_leaf(arrays, node, ray):
    """glm's test (liboracle's oracle_glm_tri_batch) of one ray against every triangle of leaf `node`, in leaf
    order: (accepted mask, (bx, by, t) rows, face ids)."""
    ids, v0, v1, v2 = arrays.leaf(node)
    c = len(ids)
    o = np.ascontiguousarray(np.broadcast_to(ray[0:3], (c, 3)))
    d = np.ascontiguousarray(np.broadcast_to(ray[4:7], (c, 3)))
    hit, out = np.zeros(c, np.int32), np.zeros((c, 3), F32)
    Q._glm().oracle_glm_tri_batch(c, o.ctypes.data, d.ctypes.data, v0.ctypes.data, v1.ctypes.data, v2.ctypes.data,
                                  hit.ctypes.data, out.ctypes.data)
    return hit != 0, out, ids
