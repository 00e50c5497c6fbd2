"""Caller-built scenes (tests/scene_cases.py) on the host: the product's scene arrays against the oracle's
builder byte for byte, the conditions that make each case worth rendering -- asserted on the oracle alone,
before tests/test_gpu_user_scenes.py launches anything --, the kernel chooser on either side of every stack
boundary, the oracle's refusal of BVHs deeper than the traversal stack, and the oracle's frames against
tests/golden/user_scenes.json (tools/make_user_scenes_golden.py).  No GPU work.
"""
import hashlib
import json
import os

import numpy as np
import pytest

import query_ref as Q
import rt_testlib as T
import scene_cases as C
from test_variant_cpu import choose

MIN_PIXELS = 16
ALL = C.CASES + C.REFUSED
DECKS = [c for c in C.CASES if "depth" in c["expect"]]
ids = lambda cases: [c["name"] for c in cases]
STACKS = (30, 40, 64)
MAX_DEPTH = 62  # rt_variant.h kMaxBvhDepth, oracle O_MAX_DEPTH


def product(case):
    s = C.apply_product(T.load_rt(), case)
    s.build()
    return s


def mirror_state(s):
    """(arrays_complete, has_tree, fast) of the mirror the scene would upload: what rt_render passes the chooser."""
    quads, units = s.mirror_twins()
    _, tree, _ = s.mirror(trees=True)
    b = np.abs(s.host_arrays()["nodes"].view(np.float32).reshape(-1, 8)[:, :6])
    fast = bool(np.all((b == 0) | ((b >= 2.0 ** -60) & (b <= 2.0 ** 62))))  # mirror.cpp rt_build_mirror
    return len(quads) > 0 and len(units) > 0, len(tree) > 0, fast


def default_variant(rt, s, want_entry=0, tune=0):
    complete, tree, fast = mirror_state(s)
    return choose(rt, tune=tune, arrays_complete=complete, has_tree=tree, depth=s.max_depth(), want_entry=want_entry and fast)


@pytest.mark.parametrize("case", ALL, ids=ids(ALL))
def test_host_arrays_equal_the_oracles(case):
    s = product(case)
    o, code = C.apply_oracle(case)
    assert code == (2 if case["expect"].get("refused") else 0)
    p, a = s.host_arrays(), o.arrays()
    for k in ("vertices", "faces", "nodes", "face_indices"):
        assert p[k].shape == a[k].shape and np.array_equal(p[k], a[k]), k
    assert s.max_depth() == a["max_depth"]
    assert np.array_equal(s.materials().view(np.uint8).reshape(-1), a["materials"]), "materials"
    # a sphere record's last 12 bytes are padding
    ps, os_ = s.spheres().view(np.uint32), a["spheres"].view(np.uint32).reshape(-1, 8)
    assert ps.shape == os_.shape and np.array_equal(ps[:, :5], os_[:, :5]), "spheres"
    cam = np.frombuffer(bytes(s.camera()), dtype=np.float32)
    assert np.array_equal(cam.view(np.uint32), o.camera(case["width"], case["height"]).view(np.uint32)), "camera"


@pytest.mark.parametrize("case", C.CASES, ids=ids(C.CASES))
def test_viewport_is_ragged(case):
    w, h = case["width"], case["height"]
    assert w % 16 and h % 16 and (w * h) % 64


@pytest.fixture(scope="module")
def first_hits():
    cache = {}

    def get(case):
        if case["name"] not in cache:
            o = C.oracle_frames(case)
            hits, _, _ = Q.trace(o["arrays"], Q.camera_rays(o["camera"], case["width"], case["height"]))
            cache[case["name"]] = hits.view(np.uint32)
        return cache[case["name"]]
    return get


@pytest.mark.parametrize("case", C.CASES, ids=ids(C.CASES))
def test_case_is_not_trivial(case, first_hits):
    """Every material the case is about is the first hit of >= 16 pixel-centre rays (every material, unless the case
    names the ones its pose can see); the poses' own conditions."""
    e = case["expect"]
    h = first_hits(case)
    kind, prim, material = h[:, 1], h[:, 2], h[:, 3]
    per = np.bincount(material[kind != 0].astype(np.int64), minlength=len(case["materials"]))
    seen = e.get("seen", range(len(case["materials"])))
    short = {m: int(per[m]) for m in seen if per[m] < MIN_PIXELS}
    assert not short, f"materials seen by fewer than {MIN_PIXELS} pixels: {short}"
    if "hits" in e:
        assert int((kind != 0).sum()) == e["hits"]
        o = C.oracle_frames(case)
        assert int(o["stats"][5]) == 0 and int(o["stats"][7]) == 0, "the jittered rays hit nothing either"
    if "inside" in e:
        inside = (kind == 1) & (prim == e["inside"])
        assert int(inside.sum()) >= MIN_PIXELS
        c, r = C.room_sphere(e["inside"])
        assert sum((a - b) ** 2 for a, b in zip(case["camera"][0], c)) < r * r, "the camera is inside that sphere"
    if case["name"] == "room_on_wall":
        assert case["camera"][0][0] == C.ROOM_LO[0] and np.all(h[:, 0].view(np.float32) == 0.0), "every ray hits its own wall at t = 0"


@pytest.mark.parametrize("case", C.CASES, ids=ids(C.CASES))
def test_default_kernel_is_the_one_the_case_is_built_for(case):
    rt = T.load_rt()
    s = product(case)
    v = default_variant(rt, s)
    assert v["mode"] == (17 | 128 if case["expect"]["lean"] else 17) and v["needs_plugin"] == 0
    assert default_variant(rt, s, tune=3 << 16)["mode"] == 17, "the XCD run length set explicitly: the general kernel"
    assert mirror_state(s)[2] == bool(case["expect"].get("fast", 1))


@pytest.mark.parametrize("case", DECKS, ids=ids(DECKS))
def test_deck_depth_and_stack_use(case):
    """The BVH is exactly as deep as the case says; >= 16 pixels' walks hold `depth` or more pending entries (the top
    of the stack and its overflow part are used); no walk holds more than the stack the chooser picks can take."""
    rt = T.load_rt()
    d = case["expect"]["depth"]
    o = C.oracle_frames(case)
    assert o["arrays"]["max_depth"] == d
    assert int((o["pending"] >= d).sum()) >= MIN_PIXELS
    assert int(o["stats"][7]) == int(o["pending"].max())
    s = product(case)
    for want_entry in (0, 1):
        v = default_variant(rt, s, want_entry=want_entry)
        assert int(o["pending"].max()) <= v["stack"] - 1, (v, int(o["pending"].max()))
    assert int(o["pending"].max()) <= (28 if d + 2 <= 28 else 40 if d + 2 <= 40 else 64) - 1  # rt_ref.hip launch_variant


@pytest.mark.parametrize("depth,stack,stack_entry,use_entry", [
    (26, 30, 64, 1), (27, 30, 64, 1), (28, 30, 64, 1), (29, 40, 64, 1), (38, 40, 64, 1), (39, 64, 64, 1),
    (48, 64, 64, 1), (49, 64, 64, 0), (62, 64, 64, 0)])
def test_chooser_at_the_stack_boundaries(depth, stack, stack_entry, use_entry):
    """variant_stack: depth + 2 (+ 14 with an entry record) <= 30 / 40 / 64; depth 48 is the last with an entry record."""
    rt = T.load_rt()
    assert depth in C.DECK_DEPTHS
    v = choose(rt, arrays_complete=1, depth=depth)
    assert (v["mode"], v["stack"], v["use_entry"]) == (17 | 128, stack, 0) and stack >= depth + 2
    e = choose(rt, arrays_complete=1, depth=depth, want_entry=1)
    assert (e["mode"], e["stack"], e["use_entry"]) == (17 | 128, stack_entry if use_entry else stack, use_entry)
    assert e["stack"] >= depth + 2 + (14 if use_entry else 0)
    g = choose(rt, arrays_complete=0, depth=depth, want_entry=1)
    assert (g["mode"], g["stack"], g["use_entry"]) == (17, stack, 0), "only the lean kernels read entry records"


def test_depth_limit_is_one_number():
    assert T.oracle().oracle_max_depth_limit() == MAX_DEPTH == max(C.DECK_DEPTHS) == STACKS[-1] - 2
    text = open(os.path.join(T.ROOT, "cuda-raytracing_amd", "csrc", "rt_variant.h")).read()
    assert f"constexpr int kMaxBvhDepth = {MAX_DEPTH};" in text
    assert min(C.REFUSED_DEPTHS) == MAX_DEPTH + 1


@pytest.mark.parametrize("case", C.REFUSED, ids=ids(C.REFUSED))
def test_oracle_refuses_deeper_trees(case):
    o, code = C.apply_oracle(case)
    assert code == 2 and o.arrays()["max_depth"] == case["expect"]["depth"] > MAX_DEPTH
    out = np.full((case["height"], case["width"], 4), 7.0, dtype=np.float32)
    st = np.zeros(8, dtype=np.uint64)
    code = T.oracle().oracle_render(o.h, case["width"], case["height"], 1, 1, 0, T.SEED, None, None, out.ctypes.data, 0,
                                    case["height"], 1, st.ctypes.data)
    assert code != 0 and np.all(out == 7.0) and not st.any(), "a refused scene is never walked"


def test_oracle_refuses_a_scene_without_triangles():
    o = T.OracleScene(None)
    o.add_sphere((0.0, 0.0, 5.0), 1.0, o.add_material(C.material_floats(C.mat(albedo=(0.5, 0.5, 0.5)))))
    assert o.finish() == 1


def test_product_host_refuses_nothing_at_build_time():
    """The host BVH and mirror of a too-deep deck build (the refusal is the entry points': tests/test_gpu_user_scenes.py),
    and report the depth rt_render compares with the limit."""
    for case in C.REFUSED:
        s = product(case)
        assert s.max_depth() == case["expect"]["depth"]
        assert len(s.mirror()) == len(s.host_arrays()["face_indices"]) // 4


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def test_golden_covers_the_cases():
    gold = json.load(open(os.path.join(T.GOLDEN, "user_scenes.json")))
    assert sorted(gold) == sorted(c["name"] for c in C.CASES)


@pytest.mark.parametrize("case", C.CASES, ids=ids(C.CASES))
def test_oracle_reproduces_the_golden_frames(case):
    g = json.load(open(os.path.join(T.GOLDEN, "user_scenes.json")))[case["name"]]
    assert g["size"] == [case["width"], case["height"]] and (g["spp"], g["bounces"]) == (case["spp"], case["bounces"])
    o = C.oracle_frames(case)
    assert len(g["rows"]) == C.FRAMES == len(o["frames"])
    for f, (rows, img) in enumerate(zip(g["rows"], o["frames"])):
        bad = [y for y in range(case["height"]) if sha(img[y]) != rows[y]]
        assert not bad, f"frame {f}: rows {bad} differ from tests/golden/user_scenes.json"
    assert sha(o["rng"]) == g["rng"], "final RNG states"
