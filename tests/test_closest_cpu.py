"""Closest-point queries without a GPU: the structs, the host-side argument checks of rt_closest_point, the host
brute force (rt_closest_point_host) pinned bytewise to the numpy restatement of the contract (tests/closest_ref.py),
the cull's bound on the host, and the conditions on the cases that keep the GPU comparisons of
tests/test_gpu_closest.py from passing by being trivial."""
import ctypes

import numpy as np
import pytest

import adversarial_cases as AC
import closest_cases as CC
import closest_ref as CR
import rt_testlib as T

F32 = np.float32
DUMMY = 0x1000  # non-null, 16-byte aligned, never dereferenced on these paths


def test_symbols_and_binding():
    rt = T.load_rt()
    L = rt.lib()
    for name in ("rt_closest_point", "rt_closest_point_host", "rt_closest_bound_host"):
        assert hasattr(L, name) and name in rt.SIGNATURES
    for name in ("closest_points", "nearest_fields", "closest_points_host", "distance_grid"):
        assert callable(getattr(rt, name))
    assert callable(rt.RayTracer.closest_points)
    f = rt.nearest_fields(np.zeros((3, 8), dtype=F32))
    assert set(f) == {"distance", "kind", "id", "material", "point", "region"} and f["point"].shape == (3, 3)


def test_rt_closest_point_error_paths_without_device():
    rt = T.load_rt()
    L = rt.lib()
    scene = ctypes.byref(rt.GPUScene())

    def refused(word, scene=scene, **kw):
        p = rt.ClosestParams()
        p.points, p.count, p.nearest = DUMMY, 64, DUMMY
        for k, v in kw.items():
            setattr(p, k, v)
        code = L.rt_closest_point(ctypes.byref(p), scene, None)
        msg = L.rt_last_error()
        assert code != 0 and msg.startswith(b"rt_closest_point: ") and word in msg, (kw, code, msg)

    assert L.rt_closest_point(None, scene, None) != 0 and L.rt_last_error() == b"rt_closest_point: null params"
    refused(b"null scene", scene=None)
    refused(b"null nearest", nearest=None)
    refused(b"null points", points=None)
    refused(b"flags", flags=1)
    refused(b"waves_per_simd", waves_per_simd=4)
    refused(b"waves_per_simd", waves_per_simd=8)
    refused(b"negative count", count=-1)
    refused(b"2^31", count=2 ** 31 + 1)
    refused(b"aligned", points=DUMMY + 4)
    refused(b"aligned", nearest=DUMMY + 8)
    # the checks come in this order: a later fault does not hide an earlier one
    refused(b"null nearest", nearest=None, points=None, flags=1)
    refused(b"flags", flags=1, waves_per_simd=4, count=-1)
    refused(b"waves_per_simd", waves_per_simd=4, count=-1, points=DUMMY + 4)
    # a scene that rt_scene_upload did not make is refused once the device-free checks have passed
    refused(b"rt_scene_upload")
    # count 0 returns at once, before the scene is looked at
    p = rt.ClosestParams()
    p.points, p.count, p.nearest = DUMMY, 0, DUMMY
    assert L.rt_closest_point(ctypes.byref(p), scene, None) == 0
    # the host call refuses nulls
    assert L.rt_closest_point_host(None, None, 0, None) != 0 and L.rt_last_error().startswith(b"rt_closest_point_host: ")


# --- the host brute force against the numpy restatement -------------------------------------------------------------
def test_hand_built_scene_host_equals_reference():
    rt = T.load_rt()
    h = CC.hand()
    want = CR.closest(h["arrays"], h["points"])
    CC.same_records(rt.closest_points_host(h["scene"], h["points"]), want, "hand-built scene")


@pytest.mark.parametrize("name", CC.ADVERSARIAL)
def test_adversarial_scene_host_equals_reference(name):
    rt = T.load_rt()
    c = CC.adversarial(name)
    want = CR.closest(c["arrays"], c["points"], rows=256)
    f = CR.fields(want)
    print(name, len(c["points"]), "points; kinds", np.bincount(f["kind"], minlength=3).tolist(), "regions",
          np.bincount(f["region"], minlength=7).tolist())
    assert (np.bincount(f["kind"], minlength=3) > 0).all() and (np.bincount(f["region"], minlength=7) > 0).all()
    CC.same_records(rt.closest_points_host(c["scene"], c["points"]), want, f"adversarial scene {name}")
    if name.startswith("C:"):  # the scene the kernel may not cull in
        nodes = c["scene"].host_arrays()["nodes"]
        assert not AC.expected_fast(nodes)


@pytest.mark.parametrize("which", ["bunny", "bunny4"])
def test_product_scene_host_equals_reference(which):
    rt = T.load_rt()
    c = CC.product(which)
    pts = c["points"][c["sample"]]
    assert len(pts) == 64 and np.isfinite(pts[:, 3]).sum() >= 16 and np.isinf(pts[:, 3]).sum() >= 16
    CC.same_records(rt.closest_points_host(c["scene"], pts), CR.closest(c["arrays"], pts), f"{which}, 64 points")


# --- the cases are not trivial ---------------------------------------------------------------------------------------
def test_hand_built_cases_are_what_they_say():
    h = CC.hand()
    pts, fam = h["points"], h["families"]
    want, d2 = CR.closest(h["arrays"], pts, details=True)
    f = CR.fields(want)
    print("kinds", np.bincount(f["kind"], minlength=3).tolist(), "regions", np.bincount(f["region"], minlength=7).tolist())
    assert (np.bincount(f["kind"], minlength=3) > 0).all()
    assert (np.bincount(f["region"][f["kind"] == 2], minlength=7) > 0).all()  # every region 0..6 wins somewhere
    reg = set(f["region"][fam["regions"]][f["kind"][fam["regions"]] == 2].tolist())
    # region 4, the edge v0v1, is the diagonal the two triangles of a quad share: beyond it the other triangle's
    # interior is nearer, so it wins only straight over the diagonal (the ties family below)
    assert reg == {0, 1, 2, 3, 5, 6}, reg
    assert (d2[fam["on"]] == 0).all() and (f["kind"][fam["on"]] == 2).all()
    # straight above: the face wins at the plain box distance of its flat leaf, for at least one point exactly
    boxes = CC.leaf_boxes(h["arrays"])
    above = fam["above"]
    assert (f["kind"][above] == 2).all()
    plain = np.array([CC.plain_box_d2(pts[i, 0:3], *boxes[int(f["id"][i])]) for i in above], dtype=F32)
    print("above: d2 == plain box distance for", int((d2[above] == plain).sum()), "of", len(above))
    assert (d2[above] == plain).sum() >= 1 and (d2[above] >= plain * F32(1 - 2.0 ** -20)).all()
    # ties: two faces at one distance, the lower index reported; the sphere before the face
    ties = fam["ties"]
    assert (f["kind"][ties[:-1]] == 2).all() and (f["region"][ties[:-1]] == 4).all()
    a, ab, ac = CR.face_records(h["arrays"])
    for i in ties[:-1]:
        fd2, _, _ = CR.face_candidates(pts[i:i + 1, 0:3], a, ab, ac)
        same = np.flatnonzero(fd2[0] == d2[i])
        assert len(same) == 2 and f["id"][i] == same.min(), (i, same)
    last = ties[-1]
    fd2, _, _ = CR.face_candidates(pts[last:last + 1, 0:3], a, ab, ac)
    assert f["kind"][last] == 1 and f["id"][last] == 0 and d2[last] == F32(0.5625) and fd2.min() == F32(0.5625)
    # spheres: inside, and at a centre (the point on +x)
    sp = fam["spheres"]
    assert (f["kind"][sp] == 1).all() and (f["distance"][sp[1:3]] == 1).all()
    assert f["point"][sp[1]].tolist() == [1, 0, 0] and f["point"][sp[2]].tolist() == [1, 3, 0]
    # radius: (kind, distance) of each named case
    r = fam["radius"]
    below = np.nextafter(F32(0.75), F32(0))
    k, dist = f["kind"][r], f["distance"][r]
    assert k.tolist() == [2, 0, 2, 0, 2, 0, 2, 0, 1, 0, 2, 0, 0, 2], k.tolist()
    assert dist[0] == 0 and dist[1] == 0 and dist[2] == F32(0.75) and dist[3] == below and dist[4] == F32(0.75)
    assert np.isnan(dist[5]) and dist[6] == F32(0.75) and dist[7] == -below and dist[10] == 2 and dist[12] == 1
    miss = f["kind"] == 0
    assert (want.view(np.uint32)[miss, 1:] == 0).all() and (want.view(np.uint32)[miss, 0] == pts.view(np.uint32)[miss, 3]).all()
    # non-finite coordinates: a NaN coordinate is a miss at any radius; an infinite one is inf away, so it hits only
    # an infinite radius (d2 = inf <= inf)
    nf = fam["nonfinite"]
    nan = np.isnan(pts[nf, 0:3]).any(axis=1)
    assert (f["kind"][nf][nan] == 0).all()
    inf_r = ~nan & np.isinf(pts[nf, 3])
    assert inf_r.sum() >= 6 and (f["kind"][nf][~nan & ~np.isinf(pts[nf, 3])] == 0).all()
    assert np.isinf(f["distance"][nf][inf_r]).sum() >= 1


@pytest.mark.parametrize("which", ["bunny", "bunny4"])
def test_product_cases_hit_and_miss(which):
    rt = T.load_rt()
    c = CC.product(which)
    pts = c["points"]
    assert len(pts) == CC.PRODUCT_POINTS and len(c["finite"]) == CC.PRODUCT_POINTS // 2
    finite = c["finite"] if which == "bunny" else c["finite"][:512]  # the big scene: a quarter of them is enough
    got = rt.closest_points_host(c["scene"], pts[finite])
    kind = CR.fields(got)["kind"]
    print(which, "finite radius:", int((kind != 0).sum()), "hits,", int((kind == 0).sum()), "misses of", len(finite))
    assert (kind != 0).sum() >= 64 and (kind == 0).sum() >= 64


@pytest.mark.parametrize("name", list(CC.DECKS))
def test_decks_need_their_deep_stacks(name):
    """What tests/test_gpu_closest.py's deck cases lean on, on the host alone.  The BVH is as deep as the deck's name
    says.  From the apex with best = inf both children of every node pass, so the first near-first descent pushes one
    entry per level: exactly `depth`.  That is the kernel's state on the deck without its sphere.  With the sphere
    (5.87 away, offered before the walk) the largest triangles' leaves are out of reach and the same descent pushes
    16 / 21 / 33 entries: deck39 and deck62 still leave rtfast::Stack's 16 LDS entries, deck62 a stack of 30.  deck29
    as built stays inside the LDS entries, so the sphere-less deck is the only case in which the stack-40 build reads
    and writes its private overflow entries, and the only one that fills a stack to its depth: both must stay."""
    rt = T.load_rt()
    depth = CC.DECKS[name]
    with_sphere, plain = CC.deck(name), CC.deck(name, spheres=False)
    apex = with_sphere["points"][0]
    assert apex.tolist() == [0, 0, 0, np.inf] and plain["points"].tobytes() == with_sphere["points"].tobytes()
    assert with_sphere["scene"].max_depth() == plain["scene"].max_depth() == depth
    A = plain["arrays"]
    assert len(A.sph_c) == 0 and np.array_equal(plain["scene"].host_arrays()["nodes"], with_sphere["scene"].host_arrays()["nodes"])
    assert CC.first_descent_pushes(rt, A, apex[0:3]) == depth
    d2, _ = CR.sphere_candidates(apex[None, 0:3], with_sphere["arrays"].sph_c, with_sphere["arrays"].sph_r)
    assert CC.first_descent_pushes(rt, A, apex[0:3], best=d2.min()) == {29: 16, 39: 21, 62: 33}[depth]
    # the host brute force the GPU test compares against is the numpy restatement here too; hits, misses and radii occur
    for c in (with_sphere, plain):
        want = CR.closest(c["arrays"], c["points"])
        CC.same_records(rt.closest_points_host(c["scene"], c["points"]), want, name)
        kind = CR.fields(want)["kind"]
        assert (kind == 2).sum() >= 16 and (kind == 0).sum() >= 4 and (c["points"][:, 3] == 0.5).sum() == 16


def test_bunny_twins_tie_and_the_lower_index_wins():
    rt = T.load_rt()
    c = CC.product("bunny")
    A = c["arrays"]
    pts = c["points"]
    got = rt.closest_points_host(c["scene"], pts)
    f = CR.fields(got)
    twin = CC.twins(A)
    a, ab, ac = CR.face_records(A)
    checked = ties = vertex_ties = 0
    m = float(np.abs(A.bmin[0]).max())
    for i in np.flatnonzero(f["kind"] == 2):
        fid = int(f["id"][i])
        if fid not in twin:
            continue  # the room's own quads have no second winding
        t = twin[fid]
        pair = np.array([fid, t])
        d2, _, _ = CR.face_candidates(pts[i:i + 1, 0:3], a[pair], ab[pair], ac[pair])
        own, other = float(d2[0, 0]), float(d2[0, 1])
        assert np.sqrt(d2[0, 0]) == f["distance"][i]
        # The twin is the same triangle with ab and ac swapped.  At a vertex (v, w in {0, 1}) both windings compute
        # the vertex itself, so they tie bit for bit and the lower index must be the one reported.  On an edge or
        # inside, q = (a + ab v) + ac w rounds in another order for the twin, so its d2 may differ in the last
        # places (within the four roundings of q, 2^-21 m each, times the distance): the winner is then whichever is
        # smaller, and the lower index again where they happen to tie.
        assert own <= other and (own < other or fid < t), (i, fid, t, d2)
        assert other - own <= 2.0 ** -18 * m * np.sqrt(own) + 2.0 ** -36 * m * m, (i, fid, t, d2)
        if f["region"][i] in (1, 2, 3):
            assert own == other and fid < t, (i, fid, t, d2)
            vertex_ties += 1
        ties += own == other
        checked += 1
    print("winners with a twin:", checked, "of", int((f["kind"] == 2).sum()), "; exact ties", ties, "; at a vertex", vertex_ties)
    assert checked >= 64 and ties >= 64 and vertex_ties >= 16


# --- the cull's bound ------------------------------------------------------------------------------------------------
def test_box_bound_never_exceeds_a_computed_distance():
    """closest.h box_bound on the host: for faces with their vertices in a box, the bound is at most the computed d2
    of every one of them -- on boxes far, near, flat and around the point, at scales from 2^-40 to 2^40 -- and on
    the flat leaves of the hand-built scene it is within the axis slack of the distance, not a loose one."""
    rt = T.load_rt()
    g = np.random.default_rng(20251023)
    worst = 0.0
    for trial in range(400):
        scale = 2.0 ** g.integers(-40, 41)
        lo = g.uniform(-1, 1, size=3) * scale
        hi = lo + g.uniform(0, 1, size=3) * scale * 2.0 ** -g.integers(0, 12)
        flat = g.integers(0, 4)
        if flat < 3:
            hi[flat] = lo[flat]
        lo32, hi32 = lo.astype(F32), np.maximum(hi.astype(F32), lo.astype(F32))
        verts = (lo32 + (hi32 - lo32) * g.uniform(0, 1, size=(24, 3, 3)).astype(F32)).astype(F32)
        verts = np.minimum(np.maximum(verts, lo32), hi32)
        verts[0] = [lo32, hi32, lo32]  # box corners, a degenerate face
        verts[1, 1] = [hi32[0], lo32[1], hi32[2]]
        a, ab, ac = verts[:, 0], verts[:, 1] - verts[:, 0], verts[:, 2] - verts[:, 0]
        for where in range(6):
            p = (lo + g.uniform(-3, 4, size=3) * (hi - lo + scale * 2.0 ** -(4 * where))).astype(F32)
            if where == 5:  # straight off one face of the box: the gap is the distance
                p = ((lo + hi) * 0.5).astype(F32)
                p[trial % 3] = hi32[trial % 3] + F32(scale * 2.0 ** -g.integers(0, 20))
            bound = rt.closest_bound_host(p, lo32, hi32)
            d2, _, _ = CR.face_candidates(p[None, :], a, ab, ac)
            # a NaN d2 (products past the fp32 range at the large scales) is never accepted: skipping it is harmless
            ok = (d2[0] >= F32(bound)) | np.isnan(d2[0])
            assert bound >= 0 and ok.all(), (trial, where, p, lo32, hi32, bound, np.nanmin(d2[0]))
            if np.nanmin(d2[0]) > 0:
                worst = max(worst, bound / float(np.nanmin(d2[0])))
    print("largest bound / nearest computed d2:", worst)
    assert worst <= 1.0
    # no bound outside the premises: a point past 2^60 or not finite, a scale below 2^-60
    assert rt.closest_bound_host((2.0 ** 61, 0, 0), (0, 0, 0), (1, 1, 1)) == -1.0
    assert rt.closest_bound_host((np.nan, 0, 0), (0, 0, 0), (1, 1, 1)) == -1.0
    assert rt.closest_bound_host((2.0 ** -70, 0, 0), (0, 0, 0), (2.0 ** -65, 0, 0)) == -1.0
    # the hand-built scene's "above" family: the bound is below the distance by the axis slack and no more
    h = CC.hand()
    boxes = CC.leaf_boxes(h["arrays"])
    want, d2 = CR.closest(h["arrays"], h["points"], details=True)
    ids = CR.fields(want)["id"]
    for i in h["families"]["above"]:
        p = h["points"][i, 0:3]
        bound = F32(rt.closest_bound_host(p, *boxes[int(ids[i])]))
        assert bound <= d2[i] and np.sqrt(bound) >= np.sqrt(d2[i]) - F32(2.0 ** -17) * np.abs(p).max(), (i, bound, d2[i])
