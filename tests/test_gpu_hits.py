"""rt_trace_hits on the GPU (csrc/rt_hits.hip) against tests/hits_ref.py.  Every comparison is bytewise on whole
48-byte records and on the counts: the arithmetic is specified, so no tolerance applies.  (The adversarial sets alone,
whose non-finite rays put NaNs into positions, leave a NaN's payload free, as tests/test_gpu_adversarial.py does.)  The
references are tests/hits_cases.py's, computed once and shared."""
import functools

import numpy as np
import pytest
import torch

import adversarial_cases as AC
import hits_cases as HC
import hits_ref as HR
import rt_testlib as T

pytestmark = pytest.mark.gpu

F32 = np.float32
BACK, FRONT, ALL = HR.CULL_BACK, HR.CULL_FRONT, HR.COUNT_ALL


@functools.lru_cache(maxsize=None)
def uploaded(name):
    """The named scene of hits_cases on the device (queries only: no RNG states) and its rays as a device tensor."""
    rt = T.load_rt()
    s = HC.scene(name)
    with AC.build_options(rt, name == "advB"):  # the mirror is built at upload
        s.upload(0)
    return s, torch.from_numpy(HC.rays(name)[1]).cuda()


def check(name, k, flags=0, waves=0, camera=None):
    """One call against the reference: rows and counts."""
    rt = T.load_rt()
    s, dev = uploaded(name)
    want_hits, want_counts = HC.reference(name, k, flags)
    if camera:
        hits, counts = rt.trace_hits_camera(s, camera[0], camera[1], k, flags=flags, waves_per_simd=waves)
    else:
        hits, counts = rt.trace_hits(s, dev, k, flags=flags, waves_per_simd=waves)
    torch.cuda.synchronize()
    assert tuple(hits.shape) == want_hits.shape and hits.dtype == torch.float32
    assert tuple(counts.shape) == want_counts.shape and counts.dtype == torch.int32
    what = f"{name} K={k} flags={flags} waves={waves} {'camera' if camera else 'rays'}"
    HC.same_rows(hits.cpu().numpy(), want_hits, what, nan_payload_free=name.startswith("adv"))
    assert counts.cpu().numpy().tobytes() == want_counts.tobytes(), what
    return want_hits, want_counts


@pytest.mark.parametrize("waves", [0, 5, 6, 7])
@pytest.mark.parametrize("k", [1, 4, 16])
def test_bunny_camera_and_explicit_rays(k, waves):
    _, counts = check("bunny", k, waves=waves, camera=(HC.W, HC.H))
    check("bunny", k, waves=waves)
    if k == 4:  # truncated and short lists both occur
        assert (counts == 4).sum() == 201 and (counts == 0).sum() == 821 and ((counts > 0) & (counts < 4)).any()
        longer = HC.reference("bunny", 16)[1]
        assert (longer >= 4).sum() == 201 and (longer > 4).sum() == 105


@pytest.mark.parametrize("name", ["bunny", "incoherent"])
def test_one_hit_is_trace_rays(name):
    """K = 1, flags 0: bytewise the library's own rt_trace_rays."""
    rt = T.load_rt()
    s, dev = uploaded(name)
    hits, counts = rt.trace_hits(s, dev, 1)
    first = rt.trace_rays(s, dev)
    torch.cuda.synchronize()
    assert hits.reshape(-1, 12).cpu().numpy().tobytes() == first.cpu().numpy().tobytes()
    kinds = first.cpu().numpy().view(np.uint32)[:, 1]
    assert (counts.cpu().numpy() == (kinds != 0)).all() and {0, 2} <= set(kinds.tolist())
    if name == "incoherent":
        halved = HC.rays(name)[1][::3, 3] < F32(1e30)
        assert halved.any() and (kinds[::3][halved] == 0).all()  # tmax at half the free distance: a miss


@pytest.mark.parametrize("k", [4, 16])
def test_hand_built_scene(k):
    hits, counts = check("hand", k)
    kind, t = hits.view(np.uint32)[:, :, 1], hits[:, :, 0]
    # the cases are what tests/test_gpu_query.py's comments say: the sphere at t = 1, then the quad at 3.5 (on its
    # diagonal: both of its triangles, in face order); tmax between them; tmax before both; from inside the sphere that
    # encloses the origin
    assert kind[8].tolist() == [1, 2, 2, 0][:4] + [0] * (k - 4) and t[8, 0] == 1.0 and t[8, 1] == 3.5 and t[8, 2] == 3.5
    assert counts[8] == 3 and hits.view(np.uint32)[8, 1, 2] < hits.view(np.uint32)[8, 2, 2]
    assert kind[9, :2].tolist() == [1, 0] and counts[9] == 1 and counts[10] == 0 and t[10, 0] == 0.5
    assert kind[18, 0] == 1 and hits.view(np.uint32)[18, 0, 2] == 2 and counts[18] >= 2 and counts[19] == 0
    assert counts.max() >= 3


@pytest.mark.parametrize("k", [4, 16])
def test_leaf_tree_scene(k):
    s, _ = uploaded("bunny4")
    _, tree, _ = s.mirror(trees=True)
    assert tree.shape[0] > 0  # the leaf-tree walk is what runs
    _, counts = check("bunny4", k, camera=(HC.W4, HC.H4))
    check("bunny4", k)
    if k == 4:
        assert (counts == 4).sum() == 102


@pytest.mark.parametrize("flags", [0, ALL])
@pytest.mark.parametrize("k", [4, 16])
@pytest.mark.parametrize("name", list(HC.DECKS))
def test_deep_stacks(name, k, flags):
    """BVHs 29, 39 and 62 levels deep: the stack-40 and stack-64 builds, their private overflow entries in use
    (tests/test_hits_cpu.py test_decks_need_their_deep_stacks)."""
    assert uploaded(name)[0].max_depth() == HC.DECKS[name]
    check(name, k, flags)


@pytest.mark.parametrize("waves", [5, 6, 7])
def test_deep_stack_at_every_occupancy(waves):
    check("deck39", 16, waves=waves)


@pytest.mark.parametrize("name", ["advA", "advB"])
def test_coplanar_twins(name):
    """The pinwheel's coplanar triangles and twins, as one big leaf (A) and as a leaf tree (B): equal distances, which the
    arrival rule decides."""
    s, _ = uploaded(name)
    with AC.build_options(T.load_rt(), name == "advB"):
        _, tree, _ = s.mirror(trees=True)
    assert (len(tree) > 0) == (name == "advB")
    hits, counts = check(name, 16)
    t = hits[:, :, 0]
    ties = sum(int((t[r, 1:counts[r]] == t[r, :counts[r] - 1]).sum()) for r in range(len(t)) if counts[r] > 1)
    assert ties > 50  # the ties are there to be decided
    check(name, 4)


@pytest.mark.parametrize("flags", [BACK, FRONT, ALL, ALL | BACK])
@pytest.mark.parametrize("name", ["bunny", "box"])
def test_flags(name, flags):
    _, counts = check(name, 4, flags)
    if flags == ALL and name == "bunny":
        assert (counts > 4).any()  # the total runs past K
    check(name, 16, flags)


def test_contains_and_signed_distance():
    rt = T.load_rt()
    s, _ = uploaded("box")
    pts, inside = HC.box_points()
    assert 0.15 < inside.mean() < 0.45  # both classes occur
    got = rt.contains(s, torch.from_numpy(pts).cuda(), flags=0)  # single-sided faces: every crossing is one record
    assert got.dtype == torch.bool and (got.cpu().numpy() == inside).all()
    # under one winding a single-sided box counts only the crossings that run along (b - a) x (c - a) of add_quad's
    # corners: with these faces the ways out, so every point inside has one and every point outside none or one
    one_sided = rt.contains(s, torch.from_numpy(pts).cuda()).cpu().numpy()
    assert one_sided[inside].all() and not (one_sided == inside).all()
    size = HC.BOX_HI - HC.BOX_LO
    lo, hi, shape = HC.BOX_LO - 0.25 * size, HC.BOX_HI + 0.25 * size, (6, 5, 7)
    sd = rt.signed_distance_grid(s, lo, hi, shape, flags=0).cpu().numpy()
    d = rt.distance_grid(s, lo, hi, shape).cpu().numpy()
    assert np.abs(sd).tobytes() == d.tobytes() and (d > 0).all()
    ax = [lo[a] + (np.arange(n) + 0.5) * ((hi[a] - lo[a]) / n) for a, n in ((2, 6), (1, 5), (0, 7))]
    z, y, x = np.meshgrid(*ax, indexing="ij")
    cell_inside = ((np.stack([x, y, z], -1) > HC.BOX_LO) & (np.stack([x, y, z], -1) < HC.BOX_HI)).all(-1)
    assert cell_inside.any() and not cell_inside.all() and ((sd < 0) == cell_inside).all()


@pytest.mark.parametrize("count", [1, 63, 64, 65])
def test_partial_waves(count):
    rt = T.load_rt()
    s, dev = uploaded("hand")
    want_hits, want_counts = HC.reference("hand", 4)
    sentinel = float(np.array([0x7FC0BEEF], dtype=np.uint32).view(F32)[0])
    hits = torch.full((count + 64, 4, 12), sentinel, dtype=torch.float32, device="cuda")
    counts = torch.full((count + 64,), 0x5EED, dtype=torch.int32, device="cuda")
    before = hits.cpu().numpy().copy()
    rays = dev[:count].clone()
    out, out_counts = rt.trace_hits(s, rays, 4, hits=hits, counts=counts)
    torch.cuda.synchronize()
    assert out.data_ptr() == hits.data_ptr() and out_counts.data_ptr() == counts.data_ptr()  # in place
    got = hits.cpu().numpy()
    HC.same_rows(got[:count], want_hits[:count], f"{count} rays")
    assert got[count:].tobytes() == before[count:].tobytes()  # rows at and past `count` keep the sentinel
    assert (counts.cpu().numpy()[:count] == want_counts[:count]).all() and (counts.cpu().numpy()[count:] == 0x5EED).all()
    # no counts kept
    hits.fill_(sentinel)
    out, none = rt.trace_hits(s, rays, 4, hits=hits, counts=False)
    torch.cuda.synchronize()
    assert none is None
    HC.same_rows(hits.cpu().numpy()[:count], want_hits[:count], f"{count} rays, no counts")
    assert hits.cpu().numpy()[count:].tobytes() == before[count:].tobytes()


def test_repeatable_on_a_stream():
    rt = T.load_rt()
    s, dev = uploaded("bunny")
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        a, ca = rt.trace_hits(s, dev, 8, stream=st)
        b, cb = rt.trace_hits(s, dev, 8, stream=st)
    st.synchronize()
    assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() and ca.cpu().numpy().tobytes() == cb.cpu().numpy().tobytes()
    HC.same_rows(a.cpu().numpy(), HC.reference("bunny", 8)[0], "non-default stream, K = 8")


def test_layers():
    rt = T.load_rt()
    tracer = rt.RayTracer(HC.W, HC.H, "bunny", spp=1, bounces=1, seed=T.SEED)
    g = tracer.layers(4)
    torch.cuda.synchronize()
    assert tracer.frame_index == 0 and tracer.rng is None
    want_hits, want_counts = HC.reference("bunny", 4)
    u = want_hits.view(np.int32)
    hit = u[:, :, 1] != 0
    assert g["depth"].cpu().numpy().tobytes() == np.where(hit, want_hits[:, :, 0], F32(np.inf)).astype(F32).tobytes()
    assert g["prim"].cpu().numpy().tobytes() == np.where(hit, u[:, :, 2], -1).astype(np.int32).tobytes()
    assert g["kind"].cpu().numpy().tobytes() == np.ascontiguousarray(u[:, :, 1]).tobytes()
    assert g["count"].cpu().numpy().tobytes() == want_counts.tobytes()
    assert tuple(g["depth"].shape) == (HC.H, HC.W, 4) and tuple(g["count"].shape) == (HC.H, HC.W)
