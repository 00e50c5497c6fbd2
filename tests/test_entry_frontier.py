"""The camera rays' entry records (csrc/entry_frontier.h) on the host: the builder the device kernel runs, the key
rule rt_render's cache uses, and a plain fp32 replay of the reference's walk (main_raytracing.cu:33-81) from the
root and from a record (csrc/entry_host.cpp, the test helper library librt_entry_host.so, restates the oracle's aabb_hit / tri_hit).

Structure, for every sub-tile: at most 15 nodes, in the reference's visit order, every expansion through a node
whose box contains its children's, and the record's nodes together with the nodes left out cover every leaf
once.  Replay, for sampled sub-tiles (all of them at 64x36), per pixel the four jitter corners and 8 random
jitters: the same face and the same distance bits from the root and from the record, no node left out passes
IntersectAABB with len = +inf, and the stack the kernel's walk holds from the record stays inside the stack
rt_variant.h choose_variant picks for a frame with a table.
"""
import numpy as np
import pytest

import entry_host
import rt_testlib as T

rt = T.load_rt()

K = 15
U_MIN = np.float32(1.16415321826934814453125e-10)  # Xorwow::uniform of 0 (rt_math.h)
U_MAX = np.float32(1.0)                             # ... of 0xffffffff: rounds to 1.0f


class Case:
    def __init__(self, which, w, h):
        self.scene = T.product_scene(which, w, h)
        self.arrays = self.scene.host_arrays()
        self.cam = self.scene.camera()
        self.w, self.h = w, h
        self.host = entry_host.EntryHost()
        assert self.host.update(self.arrays, self.cam, w, h)
        self.records = self.host.records()
        self.nodes = self.host.nodes()
        self.tx, self.ty = (w + 7) // 8, (h + 7) // 8
        assert self.records.shape == (self.tx * self.ty, 16)


_cases = {}


def case(which, w, h):
    key = (which, w, h)
    if key not in _cases:
        _cases[key] = Case(*key)
    return _cases[key]


def tree_tables(nodes):
    """Per node of the private array reachable from the root: parent, position in the reference's visit order
    (right child first), end of its subtree in that order, leaves below it."""
    u = nodes.view(np.uint32)
    n = nodes.shape[0]
    parent = np.full(n, -1, np.int64)
    pre = np.full(n, -1, np.int64)
    end = np.zeros(n, np.int64)
    leaves = np.zeros(n, np.int64)
    order = []
    stack = [0]
    while stack:
        i = stack.pop()
        pre[i] = len(order)
        order.append(i)
        if u[i, 7] == 0:
            left = int(u[i, 6])
            parent[left] = parent[left + 1] = i
            stack.append(left)
            stack.append(left + 1)
    for i in reversed(order):
        if u[i, 7] != 0:
            end[i], leaves[i] = pre[i] + 1, 1
        else:
            left = int(u[i, 6])
            end[i] = max(end[left], end[left + 1])
            leaves[i] = leaves[left] + leaves[left + 1]
    return parent, pre, end, leaves


def contains_children(nodes, p):
    u = nodes.view(np.uint32)
    left = int(u[p, 6])
    ok = np.isfinite(nodes[[p, left, left + 1], :6]).all()
    for c in (left, left + 1):
        ok = ok and (nodes[c, 0:3] >= nodes[p, 0:3]).all() and (nodes[c, 3:6] <= nodes[p, 3:6]).all()
    return bool(ok)


def check_structure(c):
    parent, pre, end, leaves = tree_tables(c.nodes)
    contained = {}
    fallbacks = 0
    for t in range(c.records.shape[0]):
        rec = c.records[t]
        n = int(rec[0])
        assert 0 <= n <= K
        ids = [int(v) for v in rec[1:1 + n]]
        out = [int(v) for v in c.host.dropped(t % c.tx, t // c.tx)]
        fallbacks += ids == [0]
        # visit order, no node below another
        for a, b in zip(ids, ids[1:]):
            assert pre[a] >= 0 and end[a] <= pre[b], (t, ids)
        # kept and left-out subtrees cover every leaf exactly once
        spans = sorted((pre[i], end[i]) for i in ids + out)
        assert all(s[1] <= nx[0] for s, nx in zip(spans, spans[1:])), (t, spans)
        assert sum(leaves[i] for i in ids + out) == leaves[0], t
        # every node expanded on the way contains its children
        for i in ids + out:
            p = parent[i]
            while p >= 0:
                if p not in contained:
                    contained[p] = contains_children(c.nodes, p)
                assert contained[p], (t, i, p)
                p = parent[p]
    return fallbacks


def rays_of_tiles(c, tiles, seed):
    """Per pixel of the sub-tiles: the four jitter corners, then 8 random jitters."""
    rng = np.random.default_rng(seed)
    px, py, ru, rv = [], [], [], []
    for t in tiles:
        x0, y0 = (t % c.tx) * 8, (t // c.tx) * 8
        for y in range(y0, min(y0 + 8, c.h)):
            for x in range(x0, min(x0 + 8, c.w)):
                j = [(U_MIN, U_MIN), (U_MAX, U_MIN), (U_MIN, U_MAX), (U_MAX, U_MAX)]
                # uniform() of random 32-bit draws, as rt_math.h computes it
                d = rng.integers(0, 2 ** 32, size=(8, 2), dtype=np.uint64).astype(np.float32)
                d = d * np.float32(2.3283064365386963e-10) + np.float32(1.16415321826934814453125e-10)
                j += [(a, b) for a, b in d]
                for a, b in j:
                    px.append(x), py.append(y), ru.append(a), rv.append(b)
    return np.array(px, np.int32), np.array(py, np.int32), np.array(ru, np.float32), np.array(rv, np.float32)


def check_replay(c, tiles, seed):
    r = c.host.replay(*rays_of_tiles(c, tiles, seed))
    assert r.size >= 12 * 16 * len(tiles) // 2
    # rays the kernel starts from their records: make_ray's range (rt_fast.h), restated; a pixel row or column
    # of these cameras has a zero direction component at one jitter corner, and those start at the root
    d, o = np.abs(r["direction"]), np.abs(np.array(list(c.cam.origin), np.float32))
    want = ((d >= 2.0 ** -40) & (d <= 2.0 ** 20)).all(axis=1) & ((o == 0) | ((o >= 2.0 ** -60) & (o <= 2.0 ** 62))).all()
    assert np.array_equal(r["qualifies"] == 1, want) and want.mean() > 0.9
    assert np.array_equal(r["visits_root"][~want], r["visits_entry"][~want])
    assert (r["dropped_hit"] == 0).all()
    assert np.array_equal(r["face_root"], r["face_entry"])
    assert np.array_equal(r["t_root"].view(np.uint32), r["t_entry"].view(np.uint32))
    assert (r["face_root"] != 0xffffffff).any()
    # Stack depth.  The root walk holds at most one pending sibling per level; from the record the lane starts with
    # up to K entries, so under a record node it can hold (K - 1) more.  choose_variant's choice (rt_variant.h), restated: the stack
    # instantiation for depth + 2 + (K - 1).
    depth = c.scene.max_depth()
    assert int(r["stack_root"].max()) <= depth + 1
    need = depth + 2 + (K - 1)
    stack = 30 if need <= 30 else 40 if need <= 40 else 64
    assert need <= 64 and int(r["stack_entry"].max()) <= min(depth + 1 + (K - 1), stack), (depth, int(r["stack_entry"].max()))
    assert int(r["stack_entry"].max()) >= 1
    return r


def test_bunny_64x36_every_tile():
    c = case("bunny", 64, 36)
    assert check_structure(c) < c.records.shape[0]
    r = check_replay(c, range(c.records.shape[0]), 1)
    # the point of it: fewer nodes popped per camera ray
    assert r["visits_entry"].sum() < 0.7 * r["visits_root"].sum()


@pytest.mark.parametrize("w,h,step", [(256, 144, 7), (250, 141, 5)])
def test_bunny_viewports(w, h, step):
    c = case("bunny", w, h)
    check_structure(c)
    n = c.records.shape[0]
    # a sample of sub-tiles, with the last column and the last row (partial sub-tiles at 250x141)
    tiles = sorted(set(range(0, n, step)) | {c.tx - 1, n - 1, n - c.tx, (c.ty // 2) * c.tx + c.tx - 1})
    check_replay(c, tiles, 2)


def test_bunny4_nodes():
    c = case("bunny4", 256, 144)
    check_structure(c)
    check_replay(c, range(3, c.records.shape[0], 71), 3)  # (a 12,318-triangle leaf: few rays)


def _camera(origin, lower_left, horizontal, vertical):
    cam = rt.GPUCamera()
    for i in range(3):
        cam.origin[i], cam.lower_left_corner[i] = origin[i], lower_left[i]
        cam.horizontal[i], cam.vertical[i] = horizontal[i], vertical[i]
    return cam


def test_camera_in_a_face_plane_falls_back():
    c = case("bunny", 64, 36)
    cam = rt.GPUCamera.from_buffer_copy(bytes(c.cam))
    cam.origin[0] = float(c.nodes[0, 3])  # the root box's x-max face plane
    host = entry_host.EntryHost()
    assert host.update(c.arrays, cam, 64, 36)
    rec = host.records()
    assert (rec[:, 0] == 1).all() and (rec[:, 1:] == 0).all()
    # the unchanged camera does expand
    assert (c.records[:, 0] != 1).any() or (c.records[:, 1] != 0).any()


def test_zero_direction_component_starts_at_the_root():
    c = case("bunny", 64, 36)
    # d.x = (-0.5 + 2 uvx) - 0.5 is exactly 0 at uvx = 0.5: pixel 31 with ru = 1.0f
    cam = _camera((0.5, 1.0, 3.0), (-0.5, 0.0, 2.0), (2.0, 0.0, 0.0), (0.0, 2.0, 0.0))
    host = entry_host.EntryHost()
    assert host.update(c.arrays, cam, 64, 36)
    ys = np.arange(36, dtype=np.int32)
    r = host.replay(np.full(36, 31, np.int32), ys, np.full(36, U_MAX), np.full(36, 0.5, np.float32))
    assert (r["direction"][:, 0] == 0.0).all()
    assert (r["qualifies"] == 0).all()
    assert np.array_equal(r["visits_root"], r["visits_entry"]) and np.array_equal(r["face_root"], r["face_entry"])
    # its neighbours, with a non-zero component, do start from their records and agree
    r = host.replay(np.full(36, 30, np.int32), ys, np.full(36, 0.25, np.float32), np.full(36, 0.5, np.float32))
    assert (r["qualifies"] == 1).all() and (r["dropped_hit"] == 0).all()
    assert np.array_equal(r["face_root"], r["face_entry"])
    assert np.array_equal(r["t_root"].view(np.uint32), r["t_entry"].view(np.uint32))


def test_key_and_build_counter():
    c = case("bunny", 64, 36)
    host = entry_host.EntryHost()
    assert host.update(c.arrays, c.cam, 64, 36) and host.builds == 1
    first = host.records()
    assert not host.update(c.arrays, c.cam, 64, 36) and host.builds == 1  # same key: no rebuild
    assert np.array_equal(first, host.records())
    moved = rt.GPUCamera.from_buffer_copy(bytes(c.cam))
    moved.origin[0] += 0.25
    moved.lower_left_corner[0] += 0.25
    assert host.update(c.arrays, moved, 64, 36) and host.builds == 2  # camera
    assert not np.array_equal(first, host.records())
    assert host.update(c.arrays, moved, 72, 40) and host.builds == 3  # viewport
    assert host.records().shape[0] == 9 * 5
    assert host.update(c.arrays, c.cam, 64, 36) and host.builds == 4
    assert np.array_equal(first, host.records())  # a function of the key alone
    other = {k: v.copy() for k, v in c.arrays.items()}  # another node array (a copy at another address): a new mirror generation
    assert host.update(other, c.cam, 64, 36) and host.builds == 5
    assert np.array_equal(first, host.records())


def test_option_validated():
    d = rt.build_options()
    assert d.entry_frontier == 0  # an opt-in: profiles/entry_ab.txt
    try:
        with pytest.raises(rt.RTError, match="build_options"):
            rt.set_build_options(entry_frontier=2)
        rt.set_build_options(entry_frontier=1)
        assert rt.build_options().entry_frontier == 1
    finally:
        rt.set_build_options()
    assert rt.build_options().entry_frontier == 0
