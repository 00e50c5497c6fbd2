"""rt_trace_hits without a device: the kernel's list code (csrc/hit_list.h through rt_hit_list_host) against a stable
sort, the reference's own properties (tests/hits_ref.py, which the GPU tests compare against), the refusals that need
no device as a table of exact messages, and the ctypes layout of rt_hits_params against the header's numbers."""
import ctypes

import numpy as np
import pytest

import hits_cases as HC
import hits_ref as HR
import query_ref as Q
import rt_testlib as T

F32 = np.float32
NAN, INF = float("nan"), float("inf")


# --- the list -----------------------------------------------------------------------------------------------------------
def sequences():
    g = np.random.default_rng(5)
    few = g.integers(0, 6, size=40).astype(F32) * F32(0.5)  # many ties
    mixed = g.uniform(-1, 8, size=64).astype(F32)
    mixed[::7] = F32(NAN)
    mixed[3::11] = F32(-0.0)
    mixed[5::13] = F32(0.0)
    mixed[8::17] = F32(6.0)  # == tmax below
    return {
        "ties": few,
        "descending": np.arange(30, 0, -1).astype(F32),
        "ascending": np.arange(30).astype(F32),
        "runs": np.concatenate([np.arange(10, 0, -1), np.arange(10), np.arange(10, 0, -1)]).astype(F32),
        "mixed": mixed,
        "zeros": np.array([0.0, -0.0, 0.0, -0.0, 1.0, -0.0], dtype=F32),
        "all_refused": np.array([NAN, -1.0, -INF, 6.0, 7.0, INF], dtype=F32),
        "empty": np.zeros(0, dtype=F32),
        "short": np.array([2.0, 1.0], dtype=F32),
    }


@pytest.mark.parametrize("count_all", [False, True])
@pytest.mark.parametrize("k", [1, 4, 5, 16])
@pytest.mark.parametrize("name", list(sequences()))
def test_list_against_stable_sort(name, k, count_all):
    rt = T.load_rt()
    t = sequences()[name]
    payload = np.arange(100, 100 + len(t), dtype=np.uint32)
    tmax = F32(6.0)
    got_t, got_p, total = rt.hit_list_host(t, payload, k, tmax, count_all)
    with np.errstate(invalid="ignore"):
        valid = np.flatnonzero((t >= 0) & (t < tmax))  # a NaN fails both
    order = valid[np.argsort(t[valid], kind="stable")][:k]  # -0.0 and 0.0 tie: arrival decides
    assert got_p.tolist() == payload[order].tolist(), (name, k)
    assert got_t.tobytes() == t[order].tobytes()  # the bits as offered, a -0.0 included
    # the total: every offer below tmax under COUNT_ALL; otherwise the rule's own count, offer by offer
    lst = HR.HitList(k, tmax, count_all)
    for x, p in zip(t, payload):
        lst.offer(x, 2, int(p))
    assert [e[2] for e in lst.entries] == got_p.tolist()
    assert total == lst.total
    if count_all:
        assert total == len(valid)


@pytest.mark.parametrize("k", [1, 4, 16])
def test_list_nan_tmax_and_infinite_tmax(k):
    rt = T.load_rt()
    t = np.array([3.0, 1.0, NAN, 2.0, 1.0, INF], dtype=F32)
    p = np.arange(6, dtype=np.uint32)
    for count_all in (False, True):
        got_t, got_p, total = rt.hit_list_host(t, p, k, NAN, count_all)
        assert len(got_t) == 0 and len(got_p) == 0 and total == 0  # nothing is < NaN
        got_t, got_p, total = rt.hit_list_host(t, p, k, INF, count_all)
        assert got_p.tolist() == [1, 4, 3, 0][:k]  # inf is not < inf
        assert total == (4 if count_all else {1: 2, 4: 4, 16: 4}[k])


def test_list_refuses_bad_arguments():
    rt = T.load_rt()
    for k in (0, 17, -1):
        with pytest.raises(rt.RTError, match="rt_hit_list_host"):
            rt.hit_list_host([1.0], [1], k, 5.0)


# --- the reference's own properties -----------------------------------------------------------------------------------------
def test_k1_is_the_closest_hit():
    for name in ("bunny", "incoherent", "hand"):
        A, rays = HC.rays(name)
        want, _, _ = Q.trace(A, rays)
        got, counts = HC.reference(name, 1)
        HC.same_rows(got, want, f"{name}: K = 1 against query_ref.trace")
        assert (counts == (want.view(np.uint32)[:, 1] != 0)).all()


def test_bunny_lists_are_what_the_tests_assume():
    """The figures the GPU tests lean on: truncated and short lists both occur, no NaN arises."""
    _, counts = HC.reference("bunny", 16, HR.COUNT_ALL)
    assert counts.min() == 0 and counts.max() == 9
    h4, c4 = HC.reference("bunny", 4)
    assert int((c4 == 4).sum()) == 201 and int((c4 == 0).sum()) == 821 and ((c4 > 0) & (c4 < 4)).any()
    assert not np.isnan(HC.reference("bunny", 16)[0]).any()
    _, c44 = HC.reference("bunny4", 4)
    assert HC.reference("bunny4", 16, HR.COUNT_ALL)[1].max() == 10 and int((c44 == 4).sum()) == 102


@pytest.mark.parametrize("name", ["bunny", "bunny4", "hand", "advA", "box"])
def test_lists_are_sorted_and_padded_with_misses(name):
    _, rays = HC.rays(name)
    for k in (4, 16):
        hits, counts = HC.reference(name, k)
        u = hits.view(np.uint32)
        for r in range(len(hits)):
            n = counts[r]
            assert (u[r, :n, 1] != 0).all() and (u[r, n:, 1:] == 0).all()
            assert hits[r, n:, 0].tobytes() == np.full(k - n, rays[r, 3], F32).tobytes()
            t = hits[r, :n, 0]
            assert (t[1:] >= t[:-1]).all() and (t >= 0).all() and (t < rays[r, 3]).all()


@pytest.mark.parametrize("name", ["bunny", "advA"])
def test_cull_flags_split_the_triangle_records(name):
    """For K = 16 on rays whose unflagged list is not full, CULL_BACK and CULL_FRONT together hold exactly its triangle
    records, and both hold all its sphere records."""
    both, cb = HC.reference(name, 16)
    back, _ = HC.reference(name, 16, HR.CULL_BACK)
    front, _ = HC.reference(name, 16, HR.CULL_FRONT)
    checked = 0
    for r in np.flatnonzero(cb < 16):
        rows = lambda h: {x.tobytes() for x in h[r] if x.view(np.uint32)[1] == 2}
        spheres = lambda h: {x.tobytes() for x in h[r] if x.view(np.uint32)[1] == 1}
        assert rows(back) | rows(front) == rows(both) and not (rows(back) & rows(front)), r
        assert spheres(back) == spheres(front) == spheres(both)
        checked += len(rows(both))
    assert checked > 100


@pytest.mark.parametrize("name", ["bunny", "hand", "box"])
def test_count_all_totals(name):
    for k in (1, 4):
        hits, counts = HC.reference(name, k)
        all_hits, totals = HC.reference(name, k, HR.COUNT_ALL)
        assert (totals >= counts).all() and (k > 1 or (totals > k).any())
        # the totals do not depend on K, and with the bound held at tmax the kept rows are the first K of the K = 16 list
        assert (totals == HC.reference(name, 16, HR.COUNT_ALL)[1]).all()
        assert all_hits.tobytes() == HC.reference(name, 16, HR.COUNT_ALL)[0][:, :k].tobytes()


def test_box_parity_is_containment():
    """The closed single-sided box: the COUNT_ALL total is odd exactly for the points inside, in each direction."""
    A, rays = HC.rays("box")
    pts, inside = HC.box_points()
    assert 0.15 < inside.mean() < 0.45
    for d in HC.DIRECTIONS:
        r = rays.copy()
        r[:, 4:7] = np.array(d, dtype=F32)
        _, totals = HR.trace(A, r, 1, HR.COUNT_ALL)
        assert ((totals & 1) == inside).all(), d


@pytest.mark.parametrize("name", list(HC.DECKS))
def test_decks_need_their_deep_stacks(name):
    """What tests/test_gpu_hits.py's deck cases lean on, on the reference alone: the BVH is as deep as the deck's name
    says (29: the stack-40 build, 39 and 62: the stack-64 build), and under COUNT_ALL at least 16 rays hold more entries
    at once than rtfast::Stack keeps in LDS (16) -- for deck39 and deck62 more than the next smaller build has at all
    (30, 40).  The lists are full, short and empty in turn."""
    depth = HC.DECKS[name]
    assert HC.scene(name).max_depth() == depth
    pending = HC.deck_pending(name)
    print(name, "most entries held:", int(pending.max()), "; rays above 16 / 30 / 40:",
          [int((pending > n).sum()) for n in (16, 30, 40)])
    assert (pending > 16).sum() >= 16
    assert depth != 39 or (pending > 30).sum() >= 16
    assert depth != 62 or (pending > 40).sum() >= 16
    _, c16 = HC.reference(name, 16)
    _, totals = HC.reference(name, 16, HR.COUNT_ALL)
    assert (c16 == 16).sum() == 49 and (c16 >= 8).sum() == 545 and (c16 == 0).sum() == 833
    assert totals.max() == {29: 36, 39: 41, 62: 52}[depth]


# --- the refusals that need no device ---------------------------------------------------------------------------------------
D = 0x1000  # non-null, 16-byte aligned, never dereferenced on these paths
DEFAULTS = dict(rays=D, hits=D, counts=D + 0x100000, count=64, max_hits=4)
WAVES = "waves_per_simd must be 0 (default), 5, 6 or 7"
UPLOAD = ("this GPUScene was not uploaded by rt_scene_upload (a foreign scene has no private mirror to query; foreign "
          "scenes are not supported here)")
BITS, BOTH = "unknown flag bits", "RT_HITS_CULL_BACK and RT_HITS_CULL_FRONT exclude each other"
RESERVED, MAXH = "reserved must be 0", "max_hits must be 1..16"
CAMERA, NEG, RAYS31 = "camera mode needs width, height > 0", "negative count", "more than 2^31 rays in one call"
RH16, C4 = "rays and hits must be 16-byte aligned", "counts must be 4-byte aligned"
# (parameter overrides or None for null params, scene given, message after "rt_trace_hits: " or None for success): the
# single faults in the header's order of checks, then rows with two faults that pin the order
TABLE = [
    (None, True, "null params"), ({}, False, "null scene"), (dict(hits=None), True, "null hits"),
    (dict(flags=8), True, BITS), (dict(flags=0x80000000), True, BITS), (dict(flags=3), True, BOTH), (dict(flags=7), True, BOTH),
    (dict(reserved=1), True, RESERVED), (dict(waves_per_simd=4), True, WAVES), (dict(waves_per_simd=8), True, WAVES),
    (dict(max_hits=0), True, MAXH), (dict(max_hits=17), True, MAXH), (dict(max_hits=-1), True, MAXH),
    (dict(rays=None, width=0, height=4), True, CAMERA), (dict(rays=None, width=4, height=-1), True, CAMERA),
    (dict(count=-1), True, NEG), (dict(count=2 ** 31 + 1), True, RAYS31),
    (dict(rays=None, width=65536, height=65536), True, RAYS31), (dict(rays=D + 4), True, RH16), (dict(hits=D + 8), True, RH16),
    (dict(counts=D + 2), True, C4), (dict(count=0), True, None), (dict(count=0, counts=None), True, None),
    ({}, True, UPLOAD), (dict(counts=None), True, UPLOAD), (dict(count=2 ** 31), True, UPLOAD),
    (dict(flags=1), True, UPLOAD), (dict(flags=2 | 4), True, UPLOAD), (dict(max_hits=16), True, UPLOAD),
    (None, False, "null params"), (dict(hits=None), False, "null scene"), (dict(hits=None, flags=8), True, "null hits"),
    (dict(flags=8 | 3), True, BITS), (dict(flags=3, reserved=1), True, BOTH), (dict(reserved=1, waves_per_simd=4), True, RESERVED),
    (dict(waves_per_simd=8, max_hits=0), True, WAVES), (dict(max_hits=17, rays=None, width=0), True, MAXH),
    (dict(rays=None, width=0, hits=D + 8), True, CAMERA), (dict(count=-1, rays=D + 4), True, NEG),
    (dict(count=2 ** 31 + 1, counts=D + 2), True, RAYS31), (dict(rays=D + 4, counts=D + 2), True, RH16),
    (dict(count=0, counts=D + 2), True, C4), (dict(count=0, hits=D + 4), True, RH16),
]


@pytest.mark.parametrize("overrides, with_scene, message", TABLE, ids=lambda v: None if isinstance(v, (dict, bool)) else v)
def test_refusal(overrides, with_scene, message):
    rt = T.load_rt()
    L = rt.lib()
    p = None
    if overrides is not None:
        p = rt.HitsParams()
        for k, v in {**DEFAULTS, **overrides}.items():
            setattr(p, k, v)
    scene = ctypes.byref(rt.GPUScene()) if with_scene else None
    code = L.rt_trace_hits(ctypes.byref(p) if p is not None else None, scene, None)
    if message is None:
        assert code == 0
    else:
        assert code != 0 and L.rt_last_error() == ("rt_trace_hits: " + message).encode(), (overrides, code, L.rt_last_error())


def test_params_layout():
    rt = T.load_rt()
    P = rt.HitsParams
    assert ctypes.sizeof(P) == 56
    want = {"rays": 0, "count": 8, "width": 16, "height": 20, "hits": 24, "counts": 32, "max_hits": 40, "flags": 44,
            "waves_per_simd": 48, "reserved": 52}
    assert {name: getattr(P, name).offset for name, _ in P._fields_} == want
    assert (rt.HITS_MAX, rt.RT_HITS_CULL_BACK, rt.RT_HITS_CULL_FRONT, rt.RT_HITS_COUNT_ALL) == (16, 1, 2, 4)
    assert ctypes.sizeof(rt.Hit) == 48 and ctypes.sizeof(rt.Ray) == 32
