"""Adaptive sampling without a GPU: the four structs against the header, the host-side refusals that need no device as
a table of exact rt_last_error texts (rows with two faults pin the order of the checks), the planner's scratch size,
and self-checks of the reference planner (tests/adaptive_ref.py) the GPU tests compare the device against."""
import ctypes
import os
import re

import numpy as np
import pytest

import adaptive_ref as A
import rt_testlib as T

F32 = np.float32
D = 0x1000  # non-null, 16-byte aligned, never dereferenced on these paths
NAN, INF = float("nan"), float("inf")
STRUCTS = {"rt_sample_pixels_params": ("SamplePixelsParams", 80), "rt_sample_priority_params": ("SamplePriorityParams", 40),
           "rt_sample_plan_params": ("SamplePlanParams", 80), "rt_sample_resolve_params": ("SampleResolveParams", 40)}


@pytest.mark.parametrize("name", list(STRUCTS))
def test_struct_layout(name):
    rt = T.load_rt()
    text = open(os.path.join(T.ROOT, "include", "rt_abi.h")).read()
    cls, want_size = getattr(rt, STRUCTS[name][0]), STRUCTS[name][1]
    size = int(re.search(r"sizeof\(%s\) == (\d+)" % name, text).group(1))
    offsets = dict((k, int(v)) for k, v in re.findall(r"offsetof\(%s, (\w+)\) == (\d+)" % name, text))
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = [n for decl in body.split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip().replace("*", " "))]
    fields = [f for f, _ in cls._fields_]
    assert size == want_size == ctypes.sizeof(cls)
    assert declared == fields, (declared, fields)
    assert set(offsets) == set(fields)  # the header pins every offset
    for k, off in offsets.items():
        assert getattr(cls, k).offset == off, k


def test_symbols_and_binding():
    rt = T.load_rt()
    for name in ("rt_sample_pixels", "rt_sample_priority", "rt_sample_plan", "rt_sample_plan_scratch_bytes", "rt_sample_resolve"):
        assert hasattr(rt.lib(), name) and name in rt.SIGNATURES
    for name in ("sample_pixels", "sample_priority", "sample_plan", "sample_plan_scratch_bytes", "sample_resolve",
                 "AdaptiveSampler"):
        assert callable(getattr(rt, name))
    assert callable(rt.RayTracer.adaptive)
    for name in ("warmup", "step", "image", "counts", "reset"):
        assert callable(getattr(rt.AdaptiveSampler, name))


# ----------------------------------------------------------------------------------------------------------------------
# refusals
# ----------------------------------------------------------------------------------------------------------------------
DEFAULTS = {
    "rt_sample_pixels": ("SamplePixelsParams", dict(pixels=D, samples=D, count=64, rng=D, accum=D, accum_pitch=256, moments=D,
                                                    width=16, height=4, bounces=6)),
    "rt_sample_priority": ("SamplePriorityParams", dict(accum=D, accum_pitch=256, moments=D, priority=D + 0x10000, width=16,
                                                        height=4)),
    "rt_sample_plan": ("SamplePlanParams", dict(priority=D, width=16, height=4, budget=256, min_samples=1, max_samples=64,
                                                scale=1.0, pixels=D + 0x1000, samples=D + 0x2000, total=D + 0x3000,
                                                scratch=D + 0x10000, scratch_bytes=1 << 20)),
    "rt_sample_resolve": ("SampleResolveParams", dict(accum=D, accum_pitch=256, out=D + 0x10000, out_pitch=256, width=16,
                                                      height=4)),
}
WAVES = "waves_per_simd must be 0 (default), 5, 6 or 7"
UPLOAD = ("this GPUScene was not uploaded by rt_scene_upload (a foreign scene has no private mirror to query; foreign "
          "scenes are not supported here)")
FLAGS, RESERVED, NEG, RAYS31 = "flags must be 0", "reserved must be 0", "negative count", "more than 2^31 rays in one call"
WH, PIX30 = "width and height must be > 0", "more than 2^30 pixels"
NOPIX, BOUNCES = "null pixels needs count == width * height", "bounces must be >= 0"
PITCH, PITCH16 = "accum_pitch smaller than width * 16", "accum_pitch must be a multiple of 16"
OPITCH, OPITCH16 = "out_pitch smaller than width * 16", "out_pitch must be a multiple of 16"
A16, RM8, P4, S2 = ("accum must be 16-byte aligned", "rng and moments must be 8-byte aligned", "pixels must be 4-byte aligned",
                    "samples must be 2-byte aligned")
MAXS, MINS = "max_samples must be 1..4095", "min_samples must be 0..max_samples"
SCALE, BUDGET = "scale must be > 0 and finite", "budget smaller than min_samples * width * height"
SCRATCH = "scratch too small (rt_sample_plan_scratch_bytes)"
# (call, parameter overrides or None for null params, scene given, message after "call: " or None for success); in
# each block the single faults in the call's order of checks, then the rows with two
TABLE = [("rt_sample_pixels", kw, s, m) for kw, s, m in [
    (None, True, "null params"), ({}, False, "null scene"), (dict(samples=None), True, "null samples"),
    (dict(rng=None), True, "null rng"), (dict(accum=None), True, "null accum"), (dict(flags=1), True, FLAGS),
    (dict(reserved=1), True, RESERVED), (dict(waves_per_simd=4), True, WAVES), (dict(waves_per_simd=8), True, WAVES),
    (dict(count=-1), True, NEG), (dict(count=2 ** 31 + 1), True, RAYS31), (dict(width=0), True, WH), (dict(height=-1), True, WH),
    (dict(width=65536, height=32768), True, PIX30), (dict(pixels=None, count=63), True, NOPIX), (dict(bounces=-1), True, BOUNCES),
    (dict(accum_pitch=255), True, PITCH), (dict(accum_pitch=264), True, PITCH16), (dict(accum=D + 8), True, A16),
    (dict(rng=D + 4), True, RM8), (dict(moments=D + 4), True, RM8), (dict(pixels=D + 2), True, P4), (dict(samples=D + 1), True, S2),
    (dict(count=0), True, None), (dict(count=0, pixels=None, width=0), True, WH), ({}, True, UPLOAD),
    (dict(pixels=None), True, UPLOAD), (dict(moments=None), True, UPLOAD), (dict(bounces=0), True, UPLOAD),
    (dict(count=2 ** 31), True, UPLOAD),
    (None, False, "null params"), (dict(samples=None), False, "null scene"), (dict(samples=None, rng=None), True, "null samples"),
    (dict(rng=None, accum=None), True, "null rng"), (dict(accum=None, flags=1), True, "null accum"),
    (dict(flags=1, reserved=1), True, FLAGS), (dict(reserved=1, waves_per_simd=4), True, RESERVED),
    (dict(waves_per_simd=8, count=-1), True, WAVES), (dict(count=-1, width=0), True, NEG),
    (dict(count=2 ** 31 + 1, height=0), True, RAYS31), (dict(width=0, bounces=-1), True, WH),
    (dict(width=65536, height=32768, pixels=None), True, PIX30), (dict(pixels=None, count=1, bounces=-1), True, NOPIX),
    (dict(bounces=-1, accum_pitch=8), True, BOUNCES), (dict(accum_pitch=8, accum=D + 8), True, PITCH),
    (dict(accum_pitch=264, accum=D + 8), True, PITCH16), (dict(accum=D + 8, rng=D + 4), True, A16),
    (dict(moments=D + 4, pixels=D + 2), True, RM8), (dict(pixels=D + 2, samples=D + 1), True, P4),
    (dict(count=0, samples=D + 1), True, S2),
]] + [("rt_sample_priority", kw, None, m) for kw, m in [
    (None, "null params"), (dict(accum=None), "null accum"), (dict(moments=None), "null moments"),
    (dict(priority=None), "null priority"), (dict(width=0), WH), (dict(height=-3), WH), (dict(width=65536, height=32768), PIX30),
    (dict(accum_pitch=240), PITCH), (dict(accum_pitch=264), PITCH16), (dict(accum=D + 8), A16),
    (dict(moments=D + 4), "moments must be 8-byte aligned"), (dict(priority=D + 0x10002), "priority must be 4-byte aligned"),
    (dict(priority=D + 256 * 3 + 252), "priority must not overlap accum"),
    (dict(moments=D + 0x8000, priority=D + 0x8000 + 508), "priority must not overlap moments"),
    (dict(accum=None, width=0), "null accum"), (dict(width=0, accum_pitch=8), WH), (dict(accum_pitch=8, accum=D + 8), PITCH),
    (dict(accum=D + 8, moments=D + 4), A16), (dict(moments=D + 4, priority=D + 0x10002), "moments must be 8-byte aligned"),
]] + [("rt_sample_plan", kw, None, m) for kw, m in [
    (None, "null params"), (dict(priority=None), "null priority"), (dict(pixels=None), "null pixels"),
    (dict(samples=None), "null samples"), (dict(scratch=None), "null scratch"), (dict(width=0), WH), (dict(height=0), WH),
    (dict(width=65536, height=32768, budget=2 ** 40), PIX30), (dict(reserved=2), RESERVED), (dict(max_samples=0), MAXS),
    (dict(max_samples=4096), MAXS), (dict(min_samples=-1), MINS), (dict(min_samples=65), MINS), (dict(scale=0.0), SCALE),
    (dict(scale=-1.0), SCALE), (dict(scale=NAN), SCALE), (dict(scale=INF), SCALE), (dict(budget=63), BUDGET),
    (dict(budget=-1, min_samples=0), BUDGET), (dict(scratch=D + 0x10008), "scratch must be 16-byte aligned"),
    (dict(total=D + 0x3004), "total must be 8-byte aligned"), (dict(priority=D + 2), "priority and pixels must be 4-byte aligned"),
    (dict(pixels=D + 0x1002), "priority and pixels must be 4-byte aligned"), (dict(samples=D + 0x2001), "samples must be 2-byte aligned"),
    (dict(scratch_bytes=1000), SCRATCH), (dict(scratch_bytes=0), SCRATCH),
    (dict(pixels=D + 252), "priority must not overlap pixels"), (dict(samples=D + 254), "priority must not overlap samples"),
    (dict(total=D + 248), "priority must not overlap total"), (dict(samples=D + 0x1000 + 254), "pixels must not overlap samples"),
    (dict(total=D + 0x2000 + 120), "samples must not overlap total"), (dict(pixels=D + 0x10000 + 16), "pixels must not overlap scratch"),
    (dict(total=D + 0x10000), "total must not overlap scratch"),
    (dict(priority=None, width=0), "null priority"), (dict(width=0, reserved=1), WH), (dict(reserved=1, max_samples=0), RESERVED),
    (dict(max_samples=0, min_samples=-1), MAXS), (dict(min_samples=65, scale=0.0), MINS), (dict(scale=NAN, budget=0), SCALE),
    (dict(budget=0, scratch=D + 0x10008), BUDGET), (dict(scratch=D + 0x10008, scratch_bytes=0), "scratch must be 16-byte aligned"),
    (dict(samples=D + 0x2001, scratch_bytes=0), "samples must be 2-byte aligned"), (dict(scratch_bytes=0, pixels=D + 252), SCRATCH),
]] + [("rt_sample_resolve", kw, None, m) for kw, m in [
    (None, "null params"), (dict(accum=None), "null accum"), (dict(out=None), "null out"), (dict(width=-1), WH),
    (dict(width=65536, height=32768), PIX30), (dict(accum_pitch=16), PITCH), (dict(accum_pitch=264), PITCH16),
    (dict(accum=D + 4), A16), (dict(out_pitch=255), OPITCH), (dict(out_pitch=264), OPITCH16),
    (dict(out=D + 0x10004), "out must be 16-byte aligned"), (dict(out=D), "out must not overlap accum"),
    (dict(out=D + 256 * 3 + 240), "out must not overlap accum"),
    (dict(accum=None, out=None), "null accum"), (dict(out=None, width=0), "null out"), (dict(accum=D + 4, out_pitch=0), A16),
    (dict(out_pitch=0, out=D + 4), OPITCH), (dict(out_pitch=264, out=D + 4), OPITCH16),
]]


@pytest.mark.parametrize("call, overrides, with_scene, message", TABLE,
                         ids=lambda v: None if isinstance(v, (dict, bool)) or v is None else v)
def test_refusal(call, overrides, with_scene, message):
    rt = T.load_rt()
    L = rt.lib()
    p = None
    if overrides is not None:
        cls, defaults = DEFAULTS[call]
        p = getattr(rt, cls)()
        for k, v in {**defaults, **overrides}.items():
            setattr(p, k, v)
    args = [ctypes.byref(p) if p is not None else None]
    if with_scene is not None:  # rt_sample_pixels takes a scene
        args.append(ctypes.byref(rt.GPUScene()) if with_scene else None)
    code = getattr(L, call)(*args, None)
    if message is None:
        assert code == 0
    else:
        assert code != 0 and L.rt_last_error() == (call + ": " + message).encode(), (overrides, code, L.rt_last_error())


def test_scratch_bytes():
    rt = T.load_rt()
    f = rt.sample_plan_scratch_bytes
    for w, h in [(0, 0), (0, 5), (5, 0), (-1, 5), (5, -1), (-3, -3)]:
        assert f(w, h) == 0
    sizes = [1, 2, 7, 8, 9, 63, 64, 65, 1000, 1920, 4096, 32768]
    for w in sizes:
        for h in sizes:
            here = f(w, h)
            assert here >= 16 + 28 * w * h + 65536 and here % 16 == 0
            assert f(w + 1, h) >= here and f(w, h + 1) >= here
    assert f(32768, 32768) >= 28 * 2 ** 30  # no 32-bit arithmetic on the way


# ----------------------------------------------------------------------------------------------------------------------
# the reference itself
# ----------------------------------------------------------------------------------------------------------------------
SIZES = [(8, 8), (9, 7), (53, 29), (1, 1)]


priorities, KINDS, PLANS = A.priorities, A.KINDS, A.PLANS


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("w, h", SIZES)
def test_reference_plan_properties(w, h, kind):
    P = w * h
    prio = priorities(kind, P)
    order = A.subtile_order(w, h)
    rank = np.empty(P, dtype=np.int64)
    rank[order] = np.arange(P)
    for kw in PLANS:
        budget = max(int(kw["budget_spp"] * P), kw["min_samples"] * P)
        pixels, samples, total = A.plan(prio, w, h, budget, kw["min_samples"], kw["max_samples"], kw["scale"])
        assert pixels.dtype == np.int32 and samples.dtype == np.uint16 and pixels.shape == samples.shape == (P,)
        assert np.array_equal(np.sort(pixels), np.arange(P)), "a permutation of the pixels"
        s = samples.astype(np.int64)
        assert (np.diff(s) <= 0).all(), "counts are non-increasing"
        assert total == int(s.sum()) <= budget
        assert (s >= kw["min_samples"]).all() and (s <= kw["max_samples"]).all()
        same = np.diff(s) == 0
        assert (np.diff(rank[pixels])[same] > 0).all(), "sub-tile order inside a count class"
        if kind in ("zero",):
            assert (s == kw["min_samples"]).all()
        if kind == "hot":
            hot = P // 2
            assert pixels[0] == hot or P == 1 or s[0] == s[-1]
            assert s[0] == min(kw["max_samples"], kw["min_samples"] + budget - kw["min_samples"] * P)


def test_subtile_order():
    assert A.subtile_order(1, 1).tolist() == [0]
    o = A.subtile_order(9, 7)
    assert o[:8].tolist() == list(range(8)) and o[8] == 9 and o[55] == 6 * 9 + 7  # the full sub-tile: 7 rows of 8
    assert o[56:].tolist() == [8 + 9 * y for y in range(7)]                        # the one-pixel-wide sub-tile
    o = A.subtile_order(17, 10)
    assert o.size == 170 and o[64] == 8 and o[128] == 16 and o[136] == 8 * 17 and o[137] == 8 * 17 + 1 and o[152] == 8 * 17 + 8


def test_quantise_and_priority_edges():
    q = A.quantise(np.array([np.nan, np.inf, -np.inf, -1.0, 0.0, 0.999, 1.0, 65534.5, 65535.0, 1e30], dtype=F32), 1.0)
    assert q == [65535, 65535, 0, 0, 0, 0, 1, 65534, 65535, 65535]
    acc = np.zeros((6, 4), dtype=F32)
    mom = np.zeros((6, 2), dtype=F32)
    acc[:, 3] = [0, 1, 2, 4, 4, np.nan]
    mom[2], mom[3], mom[4] = (2.0, 2.0), (np.inf, 1.0), (2.0, 3.0)
    p = A.priority(acc, mom)
    assert np.isposinf(p[[0, 1, 3, 5]]).all() and p[2] == 0.0
    m1, m2 = F32(0.5), F32(0.75)
    assert p[4] == ((m2 - m1 * m1) / F32(4.0)) / (m1 * m1 + F32(1e-4))
    r = A.resolve(np.array([[2, 4, 6, 2], [1, 1, 1, 0.5], [3, 3, 3, np.nan], [0, 0, 0, 0]], dtype=F32))
    assert r.tolist() == [[1, 2, 3, 1], [0, 0, 0, 1], [0, 0, 0, 1], [0, 0, 0, 1]]


@pytest.mark.parametrize("name", ["room_closed", "room_open_sky"])
def test_chain_tables_and_sums_are_the_oracles(name):
    """The two facts behind the GPU comparison: an entry chain_tables fills is the full per-offset table's, and
    chain_sums over it is the oracle's own frame (undivided) with the oracle's draw count."""
    import radiance_ref as R
    import scene_cases as C
    case = C.BY_NAME[name]
    w, h, bounces, spp = case["width"], case["height"], case["bounces"], case["spp"]
    P = w * h
    o, code = C.apply_oracle(case)
    assert code == 0
    states = T.oracle_rng_frame(T.SEED, w, h)
    sparse = A.chain_tables("cpu:" + name, o, w, h, bounces, states, spp)
    full = R.frame_tables("cpu:" + name, o, w, h, bounces, states, A.table_entries(spp, bounces))
    assert sparse.shape == full.shape
    filled = ~np.isnan(sparse[:, :, 3])
    assert (filled.sum(axis=1) == spp).all() and filled[:, 0].all()
    assert np.array_equal(sparse[filled].view(np.uint32), full[filled].view(np.uint32))
    counts = np.full(P, spp)
    for tables in (sparse, full):
        acc, mom, off = A.chain_sums(tables, counts, bounces)
        want, want_off = R.chain_frame(full, spp)
        assert np.array_equal(off, want_off) and (acc[:, 3] == spp).all()
        assert np.array_equal((acc[:, 0:3] / F32(spp)).astype(F32).view(np.uint32), want[:, 0:3].view(np.uint32))
        frame = C.oracle_frames(case)["frames"][0].reshape(P, 4)
        assert np.array_equal((acc[:, 0:3] / F32(spp)).astype(F32).view(np.uint32), np.ascontiguousarray(frame[:, 0:3]).view(np.uint32))
        assert (mom[:, 0] > 0).any() and (mom[:, 1] >= 0).all()
    # counts that differ, in two parts, from the first part's offsets: the same sums as in one go
    a = np.arange(P) % (spp + 1)
    acc1, mom1, off1 = A.chain_sums(sparse, a, bounces)
    acc2, mom2, off2 = A.chain_sums(sparse, spp - a, bounces, offsets=off1, accum=acc1, moments=mom1)
    acc, mom, off = A.chain_sums(sparse, counts, bounces)
    assert np.array_equal(acc2, acc) and np.array_equal(mom2, mom) and np.array_equal(off2, off)
    with pytest.raises(AssertionError, match="too short"):
        A.chain_sums(sparse, counts + 1, bounces)
