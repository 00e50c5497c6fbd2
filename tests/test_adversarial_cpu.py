"""The adversarial scenes and rays of tests/adversarial_cases.py, settled on the CPU: that every case is what it
claims to be (computed with tests/query_ref.py and liboracle's glm predicate only), and the two host-checkable
bounds of the production traversal at the shapes that stress them -- the twin test (rt_fast.h twin_rejected with
mirror.cpp rt_twin_bounds, through rt_twin_check_host) on slivers, mixed scales and |o - v0|_1 from 0 to 2^12,
and the leaf-tree cull (rt_fast.h cluster_cull through rt_cluster_cull_host) on a tree over degenerate, coplanar
and sliver triangles.  tests/test_gpu_adversarial.py then runs the same scenes and rays through the kernels.
"""
import ctypes

import numpy as np
import pytest

import adversarial_cases as AC
import query_ref as Q
import rt_testlib as T
from test_leaf_tree import _subtree_tris, fp32_accepts

F32 = np.float32


@pytest.fixture(scope="module")
def rt():
    return T.load_rt()


@pytest.fixture(scope="module")
def scene_a(rt):
    """Scene A, its reference arrays and its rays with the reference's records (computed once)."""
    case = AC.build_case(rt, "A")
    arrays = case.arrays()
    rs = AC.ray_set(case, arrays)
    print(f"\nscene A: {len(rs.rays)} rays, reference {rs.seconds:.2f} s")
    return case, arrays, rs


@pytest.fixture(scope="module")
def scene_b(rt):
    with AC.build_options(rt, True):
        case = AC.build_case(rt, "B")
        tris, tree, ltris = case.scene.mirror(trees=True)
    return case, tris, tree, ltris


def _fp32_centroid(p, q, r):
    """BVH::Calculate's centroid, in fp32: ((p + q) + r) / 3."""
    p, q, r = (np.asarray(x, F32) for x in (p, q, r))
    return ((p + q) + r) / F32(3.0)


def _slab(bmin, bmax, ray):
    """IntersectAABB (Math.h:50-61) in fp32, as query_ref.trace: (tmin, tmax)."""
    with np.errstate(all="ignore"):
        t1, t2 = (bmin - ray[0:3]) / ray[4:7], (bmax - ray[0:3]) / ray[4:7]
        lo, hi = np.fmin(t1, t2), np.fmax(t1, t2)
    return np.fmax(np.fmax(lo[0], lo[1]), lo[2]), np.fmin(np.fmin(hi[0], hi[1]), hi[2])


# --- the scenes -------------------------------------------------------------------------------------------------------
def _check_pinwheel(case):
    c32 = AC.C.astype(F32)
    for v in case.verts:
        for p, q, r in ((v[0], v[1], v[2]), (v[0], v[2], v[1])):
            assert np.array_equal(np.asarray([p, q, r], F32).astype(np.float64), np.array([p, q, r])), "vertices are fp32 numbers"
            assert _fp32_centroid(p, q, r).tobytes() == c32.tobytes(), (p, q, r)
    node, first, count = case.big_leaf()
    assert count == 2 * case.k
    return node, first, count


def test_pinwheel_scene(rt, scene_a):
    case, arrays, _ = scene_a
    node, first, count = _check_pinwheel(case)
    tags = case.tags
    edges = np.array([[np.linalg.norm(v[i] - v[(i + 1) % 3]) for i in range(3)] for v, t in zip(case.verts, tags) if t == "well"])
    assert edges.min() <= 2.0 ** -8 and edges.max() >= 2.0 ** 5, (edges.min(), edges.max())
    print(f"well-shaped edges {edges.min():.3g} .. {edges.max():.3g}")
    for (a, b, t) in case.bases:
        if t == "sliver":
            assert AC.aspect_ratio(a, b) >= 2.0 ** 12, (a, b, AC.aspect_ratio(a, b))
        if t == "well":
            assert AC.aspect_ratio(a, b) < 8.0, (a, b, AC.aspect_ratio(a, b))
    flat_axes = {k for v, t in zip(case.verts, tags) for k in range(3) if t in ("axis", "coplanar") and np.ptp(v[:, k]) == 0}
    assert flat_axes == {0, 1, 2}, "a triangle in an axis-aligned plane for every axis"
    cop = [v for v, t in zip(case.verts, tags) if t == "coplanar"]
    assert len(cop) == 2 and not np.array_equal(cop[0], cop[1])
    assert np.ptp(cop[0][:, 2]) == 0 and np.ptp(cop[1][:, 2]) == 0 and cop[0][0, 2] == cop[1][0, 2]  # one plane; both hold C
    col = case.verts[tags.index("collinear")]
    assert not np.cross(col[1] - col[0], col[2] - col[0]).any() and len({tuple(p) for p in col}) == 3
    rep = case.verts[tags.index("repeated")]
    assert len({tuple(p) for p in rep}) == 2
    # the mirror: pair, quad and unit records for the leaf, twins found
    quads, units = case.scene.mirror_twins()
    assert len(quads) > 0 and len(units) > 0
    assert len(units) == case.k, "every base triangle found its twin: one unit per pair"
    a = case.scene.host_arrays()
    _, twins = rt.mirror_build_check(a["nodes"].view(np.uint32).reshape(-1, 8), a["face_indices"].view(np.uint32),
                                     a["faces"].view(np.uint32).reshape(-1, 4), a["vertices"].view(F32).reshape(-1, 8))
    assert twins
    nodes = a["nodes"].view(np.uint32).reshape(-1, 8)
    assert (nodes[:, 7] == 0).sum() >= 3, "inner nodes around the big leaf"
    small = nodes[(nodes[:, 7] > 0) & (nodes[:, 7] <= 8)]
    assert len(small) >= 4
    flat = sum(1 for n in small if (n[0:3].view(F32) == n[3:6].view(F32)).any())
    assert flat >= 4, "small leaves with a flat box"
    print(f"scene A: big leaf {count}, quads {len(quads)}, units {len(units)}, nodes {len(nodes)}, depth {case.scene.max_depth()}")


def test_tree_scene(rt, scene_b):
    case, tris, tree, ltris = scene_b
    node, first, count = _check_pinwheel(case)
    assert count == 320
    assert len(tree) > 0 and len(ltris) == count
    assert tris.view(np.uint32)[first, 11] == 2, "the leaf's lead record points at a leaf tree"
    u = tree.view(np.uint32)
    cand = int((u[:, 15] & 1).sum())
    assert cand >= 20, cand
    print(f"scene B: big leaf {count}, tree nodes {len(tree)}, cull candidates {cand}, clusters {int((u[:, 14] != 0xFFFFFFFF).sum())}")


@pytest.mark.parametrize("variant", list(AC.GATES))
def test_gate_scenes_fast_flag(rt, variant):
    """The scene half of the filtered range (rt_fast.h header; mirror.cpp computes it over every node's bounds):
    a bound at 2^62 or 2^-60 keeps the scene inside, the next float beyond, or a subnormal, puts it outside."""
    case = AC.build_case(rt, "C:" + variant)
    _check_pinwheel(case)
    value, inside = AC.GATES[variant]
    nodes = case.scene.host_arrays()["nodes"].view(np.uint32).reshape(-1, 8)
    bounds = nodes[:, 0:6].view(F32)
    assert (bounds == F32(value)).any(), "the gate coordinate is a node bound"
    rest = np.abs(bounds[bounds != F32(value)])
    assert ((rest == 0) | ((rest >= 2.0 ** -6) & (rest <= 2.0 ** 8))).all(), "every other bound is far inside the range"
    assert AC.expected_fast(nodes) == inside, (variant, value)
    quads, units = case.scene.mirror_twins()
    assert len(quads) > 0 and len(units) > 0


def test_plain_scene_is_inside_the_range(scene_a):
    assert AC.expected_fast(scene_a[0].scene.host_arrays()["nodes"])


# --- the rays ---------------------------------------------------------------------------------------------------------
def test_rays_are_what_they_claim(scene_a):
    case, arrays, rs = scene_a
    n = len(rs.rays)
    assert n % 64 != 0
    u = rs.want.view(np.uint32)
    kind, pid = u[:, 1], u[:, 2]
    counts = {f: int((rs.family == f).sum()) for f in AC.FAMILIES}
    assert all(counts.values()), counts
    # every wave mixes the families, hits and misses
    for w in range(0, n - 63, 64):
        assert len(set(rs.family[w:w + 64].tolist())) >= 3 and len(set((kind[w:w + 64] != 0).tolist())) == 2, w
    f14 = rs.family <= 4
    share = float((kind[f14] == 2).mean())
    assert share >= 1 / 3, share
    tri = kind == 2
    pin = tri & (pid < 2 * case.k)
    wind = case.winding_of[np.where(pin, pid, 0)]
    originals, twins = int((pin & (wind == 0)).sum()), int((pin & (wind == 1)).sum())
    assert originals >= 50 and twins >= 50, (originals, twins)
    bx, by = rs.want[:, 7], rs.want[:, 11]
    edge = tri & ((bx == 0) | (by == 0) | (bx + by == 1))
    assert edge.sum() >= 20, int(edge.sum())
    print(f"rays {n}, per family {counts}, triangle hits of families 1-4 {share:.3f}, originals {originals}, twins {twins}, "
          f"exact boundary hits {int(edge.sum())}")
    # tmax edges
    k4 = rs.tmax_kind
    assert (k4 == 0).sum() >= 50
    assert (kind[k4 == 0] == 0).all() and (rs.want[k4 == 0, 0] == rs.rays[k4 == 0, 3]).all(), "tmax = t is a miss (strict <)"
    assert (kind[k4 == 1] == 2).all(), "tmax = the next float above t is a hit"
    assert (rs.want[k4 == 1, 0] < rs.rays[k4 == 1, 3]).all()
    assert (kind[k4 == 2] == 0).all(), "tmax = the next float below t is a miss"
    fixed = k4 == 3
    assert (kind[fixed & (rs.rays[:, 3] <= 0)] == 0).all() and (kind[fixed & np.isinf(rs.rays[:, 3])] == 2).all()


def test_coplanar_tie_is_decided_by_leaf_position(scene_a):
    """At least one ray accepts both coplanar triangles at the same distance, and the record names the earliest
    leaf position among the triangles accepted at that distance (BVHRayHit keeps the first: strict <)."""
    case, arrays, rs = scene_a
    node, first, count = case.big_leaf()
    cop = [i for i, t in enumerate(case.tags) if t == "coplanar"]
    faces = set(np.flatnonzero(np.isin(case.base_of, cop)).tolist())
    u = rs.want.view(np.uint32)
    ties = filtered = 0
    for r in np.flatnonzero((u[:, 1] == 2) & np.isin(u[:, 2], list(faces))):
        acc, out, ids = AC.glm_leaf(arrays, node, rs.rays[r])
        at = acc & (out[:, 2] == rs.want[r, 0])
        got = {int(case.base_of[i]) for i in ids[at]}
        if set(cop) <= got:
            ties += 1
            assert u[r, 2] == ids[np.flatnonzero(at)[0]], (r, ids[at], u[r, 2])
            d = np.abs(rs.rays[r, 4:7])
            filtered += bool(((d >= 2.0 ** -40) & (d <= 2.0 ** 20)).all())
    assert ties >= 1, ties
    print(f"coplanar ties {ties} ({filtered} on rays inside the filtered range)")


def test_spheres_in_front_of_and_behind_the_leaf(scene_a):
    case, arrays, rs = scene_a
    node, _, _ = case.big_leaf()
    u = rs.want.view(np.uint32)
    front = behind = 0
    for r in np.flatnonzero(u[:, 1] == 1):
        tmin, tmax = _slab(arrays.bmin[node], arrays.bmax[node], rs.rays[r])
        # the box test is on the direction as given, the distance along the normalised one
        scale = np.linalg.norm(rs.rays[r, 4:7].astype(np.float64))
        if not (tmax >= tmin and tmax > 0 and np.isfinite(scale) and scale > 0):
            continue
        t = float(rs.want[r, 0])
        front += u[r, 2] == 0 and t < float(tmin) * scale
        behind += u[r, 2] == 1 and t > float(tmax) * scale
    assert front >= 1 and behind >= 1, (front, behind)
    print(f"sphere hits in front of the leaf's box {front}, behind it {behind}")


# --- the bounds -------------------------------------------------------------------------------------------------------
def _normalized(rays):
    """glm::normalize of every direction (liboracle)."""
    d = np.ascontiguousarray(rays[:, 4:7])
    s, out = np.zeros(len(d), F32), np.zeros((len(d), 18), F32)
    Q._glm().oracle_glm_vec_batch(len(d), d.ctypes.data, d.ctypes.data, s.ctypes.data, out.ctypes.data)
    return np.ascontiguousarray(out[:, 0:3])


def test_twin_bound_on_the_pinwheel(rt, scene_a):
    """rt_twin_check_host over every (record of the big leaf, ray of families 1-3): a twin declared rejected never
    passes glm's predicate, and both outcomes occur often enough to exercise both branches of the kernel."""
    case, arrays, rs = scene_a
    _, first, count = case.big_leaf()
    recs = np.ascontiguousarray(case.scene.mirror()[first:first + count])
    pick = rs.family <= 3
    o, nd = np.ascontiguousarray(rs.rays[pick, 0:3]), _normalized(rs.rays[pick])
    assert np.isfinite(nd).all()
    check = rt.lib().rt_twin_check_host
    rp, op, dp = recs.ctypes.data, o.ctypes.data, nd.ctypes.data
    total = decided = bad = 0
    per_tag = {}
    for k in range(count):
        face = int(recs[k, 9:10].view(np.uint32)[0])
        tag = case.tags[case.base_of[face]]
        dec = 0
        for r in range(len(o)):
            b = check(rp + 48 * k, op + 12 * r, dp + 12 * r)
            dec += b & 1
            bad += (b & 3) == 3
        total += len(o)
        decided += dec
        t = per_tag.setdefault(tag, [0, 0])
        t[0] += dec
        t[1] += len(o)
    assert bad == 0, f"{bad} twins declared rejected but accepted by glm's predicate"
    share = decided / total
    print(f"twin test: {total} pairs, decided {share:.3f}, undecided {1 - share:.3f}; decided per kind "
          + ", ".join(f"{k} {v[0] / v[1]:.2f}" for k, v in per_tag.items()))
    assert share >= 0.05 and 1 - share >= 0.05, share


def test_cull_is_sound_on_the_tree(rt, scene_a, scene_b):
    """cluster_cull on every cull-candidate node of scene B's leaf tree against the rays of families 1-4 (scene
    B holds every triangle of scene A, so they are aimed at its vertices, edges and planes too), at the ray's own
    tmax and, where the reference hits, just above that distance -- the bound the cooperative walk tightens to:
    a culled node holds no triangle glm's fp32 test accepts below the bound."""
    _, _, rs = scene_a
    case, tris, tree, ltris = scene_b
    u = tree.view(np.uint32)
    cand = np.flatnonzero(u[:, 15] & 1)
    pick = np.flatnonzero(rs.family <= 4)[::2]
    o, nd = np.ascontiguousarray(rs.rays[pick, 0:3]), _normalized(rs.rays[pick])
    assert np.isfinite(nd).all()
    tmax = rs.rays[pick, 3]
    hit = rs.want.view(np.uint32)[pick, 1] != 0
    above = np.nextafter(rs.want[pick, 0], F32(np.inf))
    cull = rt.lib().rt_cluster_cull_host
    tp, op, dp = tree.ctypes.data, o.ctypes.data, nd.ctypes.data
    tested = culled = 0
    for k in cand:
        recs = ltris[_subtree_tris(tree, k)]
        for r in range(len(pick)):
            for best in ((tmax[r], above[r]) if hit[r] else (tmax[r],)):
                tested += 1
                if cull(op + 12 * r, dp + 12 * r, ctypes.c_float(best), tp + 64 * int(k)):
                    culled += 1
                    assert not fp32_accepts(o[r], nd[r], best, recs).any(), \
                        f"node {k} culled for ray {pick[r]} (family {rs.family[pick[r]]}) at {best} but a triangle is accepted"
    print(f"cull: {len(cand)} candidate nodes, {tested} (node, ray, bound) triples, culled {culled / tested:.3f}")
    assert tested >= 10000
    assert culled >= 0.02 * tested, (culled, tested)


def test_quad_order_replaces_a_candidate_on_a_tie(scene_a):
    """The shared-leaf loop (rt_fast.h quad_test) offers a leaf's triangles quad by quad -- both triangles, then both
    twins -- not in leaf order, and keeps the reference's choice by the (t, position) rule of `offer`.  With the
    far twin of this leaf (adversarial_cases.FAR_TWIN) some rays make that rule replace a candidate by one at the
    same distance and a lower position, fields and all: the sequence is replayed here from the mirror's quad
    records and glm's distances, it must end on the reference's face, and such rays must exist."""
    case, arrays, rs = scene_a
    node, first, count = case.big_leaf()
    quads, _ = case.scene.mirror_twins()
    qu = quads.view(np.uint32)
    order = []  # leaf positions in the order the loop offers them
    for k in range(len(quads)):
        wa, wb = int(qu[k, 24]), int(qu[k, 25])
        order += [p for p in (wa & 0xFFFF, None if wb == 0xFFFFFFFF else wb & 0xFFFF, wa >> 16,
                              None if wb == 0xFFFFFFFF else wb >> 16) if p is not None and p != 0xFFFF]
    assert sorted(order) == list(range(count)) and order != sorted(order)
    u = rs.want.view(np.uint32)
    replaced = 0
    for r in np.flatnonzero((u[:, 1] == 2) & (u[:, 2] < 2 * case.k) & (rs.family != 4) & (rs.rays[:, 3] == F32(AC.BIG))):
        acc, out, ids = AC.glm_leaf(arrays, node, rs.rays[r])
        best, bpos, swaps = F32(AC.BIG), None, 0
        for p in order:
            t = out[p, 2]
            if acc[p] and t >= 0 and (t < best or (t == best and bpos is not None and p < bpos)):
                swaps += bool(t == best)
                best, bpos = t, p
        # (rays whose closest hit lies in this leaf, with nothing nearer before it: the leaf's own answer is the record)
        assert best == rs.want[r, 0] and ids[bpos] == u[r, 2], (r, best, bpos, rs.want[r, 0], u[r, 2])
        replaced += swaps > 0
    print(f"rays whose quad-order walk replaces a candidate at an equal distance: {replaced}")
    assert replaced >= 1, replaced
