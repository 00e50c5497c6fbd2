"""Adaptive sampling on the GPU (csrc/rt_adaptive.hip, csrc/sample_plan.hip), bit for bit: no tolerance, no pixel exempt.

1. rt_sample_pixels against the CPU oracle's per-offset sample table followed along each pixel's chain
   (adaptive_ref.chain_sums): accumulator, moments and final states of a shuffled list with counts from {0, 1, 2, 3, 5}.
2. Against the renderer: pixels = NULL with a uniform count n gives rt_render's spp n surface times n, and its states.
3. Splitting: counts a then b in two calls = a + b in one call = any permutation of the list.
4. Edges: list lengths, entries outside the frame, canaries, untouched pixels, row padding, bounces = 0.
5. Occupancies, a stream, refusals.  6. rt_sample_priority, rt_sample_plan, rt_sample_resolve against adaptive_ref as
   exact arrays.  7. AdaptiveSampler and RayTracer.adaptive end to end.
"""
import ctypes

import numpy as np
import pytest
import torch

import adaptive_ref as A
import radiance_ref as R
import rt_testlib as T
import scene_cases as C

pytestmark = pytest.mark.gpu

F32, U32 = np.float32, np.uint32
PRODUCT = {"bunny": (64, 36, 6), "bunny4": (64, 36, 6)}  # width, height, bounces
ORACLE_CASES = ["room_closed", "room_open_sky", "spheres70", "deck62", "bunny", "bunny4"]
VALUES = np.array([0, 1, 2, 3, 5])
MAX_TOTAL = int(VALUES.max())  # the longest chain of test 1
GUARD = 3  # guard rows / records around every buffer
CANARY_F, CANARY_U = F32(-7.5), 0xC0FFEE11


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    torch.cuda.set_device(0)
    return T.load_rt()


_SETUPS = {}


def setup(rt, name):
    """{"scene", "oracle", "w", "h", "bounces", "states": the frame's initial states uint32 [w * h, 6]}."""
    got = _SETUPS.get(name)
    if got is None:
        if name in PRODUCT:
            w, h, bounces = PRODUCT[name]
            s = rt.Scene()
            s.setup(name)
            s.set_viewport(w, h)
            o = T.OracleScene(name)
        else:
            case = C.BY_NAME[name]
            w, h, bounces = case["width"], case["height"], case["bounces"]
            s = C.apply_product(rt, case)
            o, code = C.apply_oracle(case)
            assert code == 0
        s.upload(0)  # rt_sample_pixels takes its states from the caller
        got = _SETUPS[name] = {"name": name, "scene": s, "oracle": o, "w": w, "h": h, "bounces": bounces,
                               "states": T.oracle_rng_frame(T.SEED, w, h)}
    return got


def tables(su, max_total=MAX_TOTAL):
    return A.chain_tables("adaptive:" + su["name"], su["oracle"], su["w"], su["h"], su["bounces"], su["states"], max_total)


def hashed_counts(P, salt=0):
    """A count from VALUES for every pixel, by a fixed hash of the pixel index."""
    p = np.arange(P, dtype=np.uint64) + np.uint64(salt)
    return VALUES[((p * np.uint64(2654435761)) >> np.uint64(7)) % np.uint64(VALUES.size)].astype(np.int64)


def same_words(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    g, w = got.view(U32), want.view(U32)
    nan = np.isnan(got) & np.isnan(want) if got.dtype == F32 else np.zeros(got.shape, bool)
    differing = (g != w) & ~nan
    if differing.any():
        k = tuple(int(v[0]) for v in np.nonzero(differing))
        pytest.fail(f"{what}: {int(differing.reshape(got.shape[0], -1).any(axis=-1).sum())} of {got.shape[0]} rows differ; "
                    f"first at {k}: got {got[k]!r} ({g[k]:#010x}), want {want[k]!r} ({w[k]:#010x})")


class Frame:
    """Device buffers of one frame with guards around each: the states, the pitched accumulator (its row padding is
    guard too), the moments.  `accum0` [P, 4] / `moments0` [P, 2] are the initial contents; the states are the frame's."""

    def __init__(self, rt, su, accum0=None, moments0=None, moments=True):
        self.rt, self.w, self.h = rt, su["w"], su["h"]
        w, h, P = self.w, self.h, su["w"] * su["h"]
        host = np.full((P + 2 * GUARD, R.STATE_WORDS), CANARY_U, dtype=U32)
        host[GUARD:GUARD + P] = R.pack_states(su["states"]).view(U32).reshape(P, R.STATE_WORDS)
        self.rng_all = torch.from_numpy(host.reshape(-1).view(np.int32).copy()).cuda()
        self.rng = self.rng_all[GUARD * R.STATE_WORDS:(GUARD + P) * R.STATE_WORDS]
        row = rt.alloc_surface(w, 1).shape[1]
        host = np.full((h + 2 * GUARD, row), CANARY_F, dtype=F32)
        host[GUARD:GUARD + h, :w * 4] = (np.zeros((P, 4), dtype=F32) if accum0 is None else accum0).reshape(h, w * 4)
        self.accum_all = torch.from_numpy(host).cuda()
        self.accum = self.accum_all[GUARD:GUARD + h]
        self.moments_all = self.moments = None
        if moments:
            host = np.full((P + 2 * GUARD, 2), CANARY_F, dtype=F32)
            host[GUARD:GUARD + P] = np.zeros((P, 2), dtype=F32) if moments0 is None else moments0
            self.moments_all = torch.from_numpy(host).cuda()
            self.moments = self.moments_all[GUARD:GUARD + P]

    def read(self):
        """(accum [P, 4], moments [P, 2] or None, states uint32 [P, 6]) after checking every guard and the unused words."""
        w, h, P = self.w, self.h, self.w * self.h
        a = self.accum_all.cpu().numpy()
        assert (a[:GUARD] == CANARY_F).all() and (a[GUARD + h:] == CANARY_F).all(), "rows around the accumulator were written"
        assert (a[GUARD:GUARD + h, w * 4:] == CANARY_F).all(), "row padding of the accumulator was written"
        r = self.rng_all.cpu().numpy().view(U32).reshape(-1, R.STATE_WORDS)
        assert (r[:GUARD] == CANARY_U).all() and (r[GUARD + P:] == CANARY_U).all(), "states around the frame's were written"
        assert not r[GUARD:GUARD + P, 6:].any(), "the unused words of the states were written"
        m = None
        if self.moments_all is not None:
            m = self.moments_all.cpu().numpy()
            assert (m[:GUARD] == CANARY_F).all() and (m[GUARD + P:] == CANARY_F).all(), "moments around the frame's were written"
            m = m[GUARD:GUARD + P].copy()
        return a[GUARD:GUARD + h, :w * 4].reshape(P, 4).copy(), m, r[GUARD:GUARD + P, :6].copy()


def guarded_list(pixels, samples):
    """Device (pixels int32 [n], samples int16 [n]) slices with guard entries around them, and a check of the guards."""
    n = len(samples)
    hp = np.full(n + 2 * GUARD, 0x5A5A5A5, dtype=np.int32)
    hs = np.full(n + 2 * GUARD, 0x7A7A, dtype=np.uint16)
    hp[GUARD:GUARD + n], hs[GUARD:GUARD + n] = pixels, samples
    dp, ds = torch.from_numpy(hp).cuda(), torch.from_numpy(hs.view(np.int16)).cuda()

    def unchanged():
        assert np.array_equal(dp.cpu().numpy(), hp) and np.array_equal(ds.cpu().numpy().view(np.uint16), hs), "the list was written"
    return dp[GUARD:GUARD + n], ds[GUARD:GUARD + n], unchanged


def sample(rt, su, frame, pixels, samples, **kw):
    """rt.sample_pixels of host lists (pixels None: the uniform form) into `frame`."""
    if pixels is None:
        ds = torch.from_numpy(np.asarray(samples, dtype=np.uint16).view(np.int16).copy()).cuda()
        dp, unchanged = None, lambda: None
    else:
        dp, ds, unchanged = guarded_list(np.asarray(pixels, dtype=np.int32), np.asarray(samples, dtype=np.uint16))
    kw.setdefault("bounces", su["bounces"])
    rt.sample_pixels(su["scene"], su["w"], su["h"], ds, frame.rng, frame.accum, pixels=dp, moments=frame.moments, **kw)
    torch.cuda.synchronize()
    unchanged()


def check_frame(frame, want, what):
    accum, moments, states = frame.read()
    same_words(accum, want[0], what + ": accumulator")
    if moments is not None:
        same_words(moments, want[1], what + ": moments")
    same_words(states, np.asarray(want[2], dtype=U32), what + ": states")


def chained(su, counts, accum0=None, moments0=None, max_total=MAX_TOTAL):
    """(accum, moments, final states) the oracle's chains give for `counts` more samples from the initial states."""
    acc, mom, off = A.chain_sums(tables(su, max_total), counts, su["bounces"], accum=accum0, moments=moments0)
    return acc, mom, R.xorwow_advance(su["states"], off)


def initial(P):
    """Accumulators and moments that are not zero: what the calls add to must survive."""
    p = np.arange(P)
    acc = np.stack([(p % 7) * 0.25, (p % 5) * 0.5, (p % 3) * 1.5, 3.0 + (p % 4)], axis=1).astype(F32)
    mom = np.stack([(p % 11) * 0.125, (p % 13) * 0.375], axis=1).astype(F32)
    return acc, mom


# --- 1. the oracle ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ORACLE_CASES)
def test_shuffled_list_against_the_oracle_chain(rt, name):
    su = setup(rt, name)
    P = su["w"] * su["h"]
    assert su["bounces"] == 6
    counts = hashed_counts(P)
    assert set(np.unique(counts)) == set(VALUES.tolist())
    t = tables(su)
    t = t[~np.isnan(t[:, :, 3])]  # the entries the chains visit
    assert t.shape[0] == P * MAX_TOTAL and (t[:, 3] > 2).any() and (t[:, 0:3] != 0).any(), "a table of misses in the dark proves nothing"
    order = np.random.default_rng(5).permutation(P)
    acc0, mom0 = initial(P)
    frame = Frame(rt, su, acc0, mom0)
    sample(rt, su, frame, order, counts[order])
    check_frame(frame, chained(su, counts, acc0, mom0), f"{name}: a shuffled list of {int(counts.sum())} samples")


# --- 2. the renderer --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 4])
@pytest.mark.parametrize("name", ["room_open_sky", "bunny"])
def test_uniform_rounds_are_the_renderers_frames(rt, name, n):
    su = setup(rt, name)
    w, h, s = su["w"], su["h"], su["scene"]
    P = w * h
    frame_rng = rt.alloc_rng(P)
    rt.init_rng_states(frame_rng, w, h, T.SEED)
    s.upload(frame_rng.data_ptr())
    try:
        surface = rt.alloc_surface(w, h)
        rt.render(s, surface, None, w, h, n, su["bounces"], frame_index=0)
        torch.cuda.synchronize()
        want = rt.surface_view(surface, w).cpu().numpy().reshape(P, 4)
        want_rng = frame_rng.cpu().numpy().view(U32).reshape(-1, R.STATE_WORDS)[:, :6]
    finally:
        s.upload(0)
    frame = Frame(rt, su)
    sample(rt, su, frame, None, np.full(P, n))
    accum, moments, states = frame.read()
    assert (want[:, 0:3] != 0).any()
    same_words((accum[:, 0:3] / F32(n)).astype(F32), want[:, 0:3].copy(), f"{name}: accum.rgb / {n} against rt_render at spp {n}")
    assert (accum[:, 3] == F32(n)).all()
    same_words(states, want_rng.copy(), f"{name}: states after {n} samples against rt_render's")


# --- 3. splitting -----------------------------------------------------------------------------------------------------
def test_split_and_permuted_lists_agree(rt):
    su = setup(rt, "room_closed")
    P = su["w"] * su["h"]
    a, b = hashed_counts(P), hashed_counts(P, salt=977)
    assert (a != b).any() and ((a > 0) & (b > 0)).any()
    acc0, mom0 = initial(P)
    ident = np.arange(P)
    once = Frame(rt, su, acc0, mom0)
    sample(rt, su, once, ident, a + b)
    want = once.read()
    twice = Frame(rt, su, acc0, mom0)
    sample(rt, su, twice, ident, a)
    sample(rt, su, twice, ident[::-1], b[::-1])
    check_frame(twice, want, "a then b against a + b")
    order = np.random.default_rng(11).permutation(P)
    shuffled = Frame(rt, su, acc0, mom0)
    sample(rt, su, shuffled, order, (a + b)[order])
    check_frame(shuffled, want, "a permuted list against the identity list")
    check_frame(once, chained(su, a + b, acc0, mom0, max_total=10), "a + b against the oracle's chains")


# --- 4. edges ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", [0, 1, 63, 64, 65])
def test_list_lengths_outside_entries_and_canaries(rt, length):
    su = setup(rt, "room_closed")
    P = su["w"] * su["h"]
    r = np.random.default_rng(100 + length)
    pixels = r.permutation(P)[:length].astype(np.int64)
    samples = VALUES[r.integers(1, VALUES.size, size=length)]
    if length >= 63:  # entries outside the frame, asking for samples: nothing is rendered for them
        pixels[[5, 40, 62]] = [-1, P, 2 ** 31 - 1]
        pixels[7] = -2 ** 31
    counts = np.zeros(P, dtype=np.int64)
    inside = (pixels >= 0) & (pixels < P)
    counts[pixels[inside]] = samples[inside]
    acc0, mom0 = initial(P)
    frame = Frame(rt, su, acc0, mom0)
    if length == 0:
        empty = torch.zeros((0,), dtype=torch.int16, device="cuda")
        rt.sample_pixels(su["scene"], su["w"], su["h"], empty, frame.rng, frame.accum, pixels=torch.zeros((0,), dtype=torch.int32,
                         device="cuda"), moments=frame.moments)
        # count 0 returns at once even where the other checks would look at the scene
        p = rt.SamplePixelsParams()
        p.pixels, p.samples, p.rng, p.accum, p.accum_pitch, p.width, p.height = 16, 16, 16, 16, su["w"] * 16, su["w"], su["h"]
        assert rt.lib().rt_sample_pixels(ctypes.byref(p), ctypes.byref(rt.GPUScene()), None) == 0
        torch.cuda.synchronize()
    else:
        sample(rt, su, frame, pixels, samples)
    want = chained(su, counts, acc0, mom0)
    # pixels outside the list: byte-identical accumulator, moments and state
    untouched = counts == 0
    assert untouched.sum() >= P - length
    same_words(want[0][untouched], acc0[untouched], "the reference leaves unlisted pixels alone")
    check_frame(frame, want, f"a list of {length}")


def test_zero_samples_read_and_write_nothing(rt):
    su = setup(rt, "room_closed")
    P = su["w"] * su["h"]
    acc0, mom0 = initial(P)
    frame = Frame(rt, su, acc0, mom0)
    pixels = np.full(200, 2 ** 30, dtype=np.int64)  # never read: their samples are 0
    pixels[100] = 17
    samples = np.zeros(200, dtype=np.int64)
    samples[100] = 2
    sample(rt, su, frame, pixels, samples)
    counts = np.zeros(P, dtype=np.int64)
    counts[17] = 2
    check_frame(frame, chained(su, counts, acc0, mom0), "one live entry among zeros")


@pytest.mark.parametrize("moments", [True, False])
def test_zero_bounces(rt, moments):
    su = setup(rt, "room_closed")
    P = su["w"] * su["h"]
    counts = hashed_counts(P)
    acc0, mom0 = initial(P)
    frame = Frame(rt, su, acc0, mom0, moments=moments)
    order = np.random.default_rng(3).permutation(P)
    sample(rt, su, frame, order, counts[order], bounces=0)
    acc = acc0.copy()
    for k in range(int(counts.max())):  # (0, 0, 0) and 1.0f per sample, one at a time
        rows = counts > k
        acc[rows, 0:3] = (acc[rows, 0:3] + F32(0.0)).astype(F32)
        acc[rows, 3] = (acc[rows, 3] + F32(1.0)).astype(F32)
    check_frame(frame, (acc, mom0, R.xorwow_advance(su["states"], 2 * counts)), "bounces = 0: two draws a sample")


def test_without_moments(rt):
    su = setup(rt, "room_closed")
    P = su["w"] * su["h"]
    counts = hashed_counts(P)
    frame = Frame(rt, su, moments=False)
    sample(rt, su, frame, np.arange(P), counts)
    check_frame(frame, chained(su, counts), "moments = NULL")


# --- 5. occupancy, stream, refusals -----------------------------------------------------------------------------------
@pytest.mark.parametrize("wps", [5, 6, 7])
@pytest.mark.parametrize("name", ["room_closed", "bunny4"])
def test_waves_per_simd(rt, name, wps):
    su = setup(rt, name)
    P = su["w"] * su["h"]
    counts = hashed_counts(P)
    order = np.random.default_rng(5).permutation(P)
    frame = Frame(rt, su)
    sample(rt, su, frame, order, counts[order], waves_per_simd=wps)
    check_frame(frame, chained(su, counts), f"{name} at {wps} waves per SIMD")


def test_on_a_stream(rt):
    su = setup(rt, "room_closed")
    P = su["w"] * su["h"]
    counts = hashed_counts(P)
    frame = Frame(rt, su)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    sample(rt, su, frame, np.arange(P), counts, stream=stream)
    check_frame(frame, chained(su, counts), "on a non-default stream")


def untouched_buffers(rt, su):
    frame = Frame(rt, su, *initial(su["w"] * su["h"]))
    before = frame.read()
    return frame, lambda: check_frame(frame, before, "a refused call")


def test_foreign_scene_is_refused(rt):
    su = setup(rt, "room_closed")
    P = su["w"] * su["h"]
    f = rt.GPUScene()
    ctypes.pointer(f)[0] = su["scene"].gpu.contents
    other_nodes = torch.zeros((64,), dtype=torch.float32, device="cuda")  # another address: no mirror is registered for it
    f.gpu_bvh_nodes = other_nodes.data_ptr()
    frame, unchanged = untouched_buffers(rt, su)
    samples = torch.ones((P,), dtype=torch.int16, device="cuda")
    with pytest.raises(rt.RTError, match="rt_sample_pixels: this GPUScene was not uploaded by rt_scene_upload"):
        rt.sample_pixels(f, su["w"], su["h"], samples, frame.rng, frame.accum, moments=frame.moments)
    torch.cuda.synchronize()
    unchanged()


@pytest.mark.parametrize("case", C.REFUSED, ids=[c["name"] for c in C.REFUSED])
def test_too_deep_bvh_is_refused(rt, case):
    s = C.apply_product(rt, case)
    s.upload(0)
    w, h = case["width"], case["height"]
    rng, accum = rt.alloc_rng(w * h), rt.alloc_surface(w, h)
    samples = torch.ones((w * h,), dtype=torch.int16, device="cuda")
    text = f"rt_sample_pixels: the scene's BVH is {case['expect']['depth']} levels deep; the traversal stack holds depth <= 62"
    with pytest.raises(rt.RTError, match=text):
        rt.sample_pixels(s, w, h, samples, rng, accum)
    torch.cuda.synchronize()
    assert not bool(accum.any()) and not bool(rng.any())


def test_short_and_overlapping_buffers_are_refused(rt):
    su = setup(rt, "room_closed")
    w, h, s = su["w"], su["h"], su["scene"]
    P = w * h
    L = rt.lib()
    frame, unchanged = untouched_buffers(rt, su)
    pixels = torch.arange(P, dtype=torch.int32, device="cuda")
    samples = torch.ones((P,), dtype=torch.int16, device="cuda")
    pitch = frame.accum.stride(0) * 4
    big = torch.zeros((h * pitch // 4 + P * 12,), dtype=torch.float32, device="cuda")  # room for an accumulator, then states

    def refused(word, **kw):
        p = rt.SamplePixelsParams()
        p.pixels, p.samples, p.count, p.rng = pixels.data_ptr(), samples.data_ptr(), P, frame.rng.data_ptr()
        p.accum, p.accum_pitch, p.moments = frame.accum.data_ptr(), pitch, frame.moments.data_ptr()
        p.width, p.height, p.bounces = w, h, 1
        for k, v in kw.items():
            setattr(p, k, v)
        code = L.rt_sample_pixels(ctypes.byref(p), ctypes.cast(s.gpu, ctypes.c_void_p), None)
        msg = L.rt_last_error()
        assert code != 0 and msg.startswith(b"rt_sample_pixels: ") and word in msg, (kw, code, msg)

    # (torch's tensors are carved out of larger allocations: a certainly short buffer is an allocation of its own)
    small = ctypes.c_void_p()
    assert L.rt_malloc(ctypes.byref(small), 64) == 0
    try:
        refused(b"pixels too small", count=2 ** 31)
        for name in ("pixels", "samples", "rng", "accum", "moments"):  # the order of the checks
            refused(name.encode() + b" too small", **{name: small.value})
        refused(b"samples too small", samples=small.value, rng=small.value, accum=small.value)
        refused(b"accum too small", accum_pitch=1 << 40)
    finally:
        assert L.rt_free(small) == 0
    last_row = big.data_ptr() + (h - 1) * pitch + w * 16
    refused(b"accum overlaps rng", accum=big.data_ptr(), rng=last_row - 8)
    refused(b"accum overlaps moments", accum=big.data_ptr(), moments=last_row - 8)
    refused(b"accum overlaps pixels", accum=big.data_ptr(), pixels=last_row - 4)
    refused(b"accum overlaps samples", accum=big.data_ptr(), samples=last_row - 2)
    torch.cuda.synchronize()
    unchanged()
    assert not bool(big.any())


# --- 6. priority, plan, resolve ---------------------------------------------------------------------------------------
PLAN_SIZES = [(8, 8), (9, 7), (53, 29), (64, 36)]


def device_plan(rt, prio, w, h, budget, **kw):
    """rt.sample_plan of host priorities with guards around every output -> (pixels, samples uint16, total int)."""
    P = w * h
    d_prio = torch.from_numpy(np.ascontiguousarray(prio, dtype=F32)).cuda()
    px = torch.full((P + 2 * GUARD,), 0x5A5A5A5, dtype=torch.int32, device="cuda")
    sm = torch.full((P + 2 * GUARD,), 0x7A7A, dtype=torch.int16, device="cuda")
    tot = torch.full((3,), -99, dtype=torch.int64, device="cuda")
    rt.sample_plan(d_prio, w, h, budget, pixels=px[GUARD:GUARD + P], samples=sm[GUARD:GUARD + P], total=tot[1:2], **kw)
    torch.cuda.synchronize()
    px, sm, tot = px.cpu().numpy(), sm.cpu().numpy().view(np.uint16), tot.cpu().numpy()
    assert (px[:GUARD] == 0x5A5A5A5).all() and (px[GUARD + P:] == 0x5A5A5A5).all(), "entries around pixels were written"
    assert (sm[:GUARD] == 0x7A7A).all() and (sm[GUARD + P:] == 0x7A7A).all(), "entries around samples were written"
    assert tot[0] == -99 and tot[2] == -99, "words around total were written"
    assert np.array_equal(d_prio.cpu().numpy().view(U32), np.ascontiguousarray(prio, dtype=F32).view(U32)), "priority was written"
    return px[GUARD:GUARD + P], sm[GUARD:GUARD + P], int(tot[1])


def check_plan(rt, prio, w, h, kw, what):
    P = w * h
    budget = max(int(kw["budget_spp"] * P), kw["min_samples"] * P)
    rest = {k: v for k, v in kw.items() if k != "budget_spp"}
    want = A.plan(prio, w, h, budget, kw["min_samples"], kw["max_samples"], kw["scale"])
    got = device_plan(rt, prio, w, h, budget, **rest)
    assert got[2] == want[2], (what, "total", got[2], want[2])
    assert np.array_equal(got[1], want[1]), (what, "samples")
    assert np.array_equal(got[0], want[0]), (what, "pixels")


@pytest.mark.parametrize("kind", A.KINDS)
@pytest.mark.parametrize("w, h", PLAN_SIZES)
def test_plan_against_the_reference(rt, w, h, kind):
    prio = A.priorities(kind, w * h)
    for kw in A.PLANS:
        check_plan(rt, prio, w, h, kw, f"{kind} {w}x{h} {kw}")


def test_plan_with_a_budget_beyond_64_bits_of_product(rt):
    """q * B overflows 64 bits here; the device's split quotient must still be the exact one."""
    w, h = 9, 7
    prio = A.priorities("random", w * h)
    for budget in (2 ** 62, 2 ** 63 - 1, 2 ** 50 + 12345):
        want = A.plan(prio, w, h, budget, 0, 4095, 20000.0)
        got = device_plan(rt, prio, w, h, budget, min_samples=0, max_samples=4095, scale=20000.0)
        assert got[2] == want[2] and np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0]), budget
    # a Q so small that B / Q is huge, and shares that stay below the cap
    prio = np.zeros(w * h, dtype=F32)
    prio[[3, 40]] = [1.0, 3.0]
    want = A.plan(prio, w, h, 1000, 0, 4095, 1.0)
    got = device_plan(rt, prio, w, h, 1000, min_samples=0, max_samples=4095, scale=1.0)
    assert want[1][:2].tolist() == [750, 250] and got[2] == want[2] == 1000
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0])


_WARM = {}


def warm_frame(rt):
    """room_open_sky after a uniform round of 3 samples: (su, Frame, accum, moments), once."""
    if not _WARM:
        su = setup(rt, "room_open_sky")
        frame = Frame(rt, su)
        sample(rt, su, frame, None, np.full(su["w"] * su["h"], 3))
        accum, moments, _ = frame.read()
        _WARM["got"] = (su, frame, accum, moments)
    return _WARM["got"]


def priority_cases(P):
    """Accumulators and moments with every branch of rt_sample_priority among ordinary values."""
    r = np.random.default_rng(21)
    acc = np.zeros((P, 4), dtype=F32)
    acc[:, 3] = r.integers(0, 6, size=P)
    lum = r.random((P, 8)).astype(F32) ** 3
    mom = np.stack([lum.sum(axis=1), (lum * lum).sum(axis=1)], axis=1).astype(F32)
    k = min(P, 12)
    rows = r.permutation(P)[:k]
    acc[rows, 3] = np.array([np.nan, np.inf, -1.0, 1.5, 2.0, 1e30, 4, 4, 4, 4, 4, 0.0], dtype=F32)[:k]
    mom[rows[6:10]] = np.array([[np.inf, 1], [1, np.nan], [-np.inf, 2], [0, 0]], dtype=F32)[:max(0, k - 6)]
    return acc, mom


@pytest.mark.parametrize("w, h", PLAN_SIZES)
def test_priority_and_resolve_against_the_reference(rt, w, h):
    P = w * h
    acc, mom = priority_cases(P)
    acc[:, 0:3] = np.random.default_rng(2).random((P, 3)).astype(F32) * 9
    d_acc = rt.alloc_surface(w, h)
    d_acc.fill_(float(CANARY_F))
    rt.surface_view(d_acc, w).copy_(torch.from_numpy(acc.reshape(h, w, 4)))
    d_mom = torch.from_numpy(mom).cuda()
    out = torch.full((P + 2 * GUARD,), float(CANARY_F), dtype=torch.float32, device="cuda")
    rt.sample_priority(d_acc, d_mom, w, h, out=out[GUARD:GUARD + P])
    image = rt.alloc_surface(w, h)
    image.fill_(float(CANARY_F))
    rt.sample_resolve(d_acc, w, h, out=image)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[:GUARD] == CANARY_F).all() and (got[GUARD + P:] == CANARY_F).all()
    want = A.priority(acc, mom)
    assert np.isposinf(want).any() and np.isfinite(want).any() and (want[np.isfinite(want)] > 0).any()
    same_words(got[GUARD:GUARD + P].copy(), want, f"priority {w}x{h}")
    same_words(rt.surface_view(image, w).cpu().numpy().reshape(P, 4), A.resolve(acc), f"resolve {w}x{h}")
    assert bool((image[:, w * 4:] == float(CANARY_F)).all()), "row padding of the resolved image was written"
    with pytest.raises(rt.RTError, match="rt_sample_resolve: out must not overlap accum"):
        rt.sample_resolve(d_acc, w, h, out=d_acc)


def test_priority_and_plan_of_a_real_warm_up(rt):
    su, frame, accum, moments = warm_frame(rt)
    w, h = su["w"], su["h"]
    prio = rt.sample_priority(frame.accum, frame.moments, w, h)
    torch.cuda.synchronize()
    want = A.priority(accum, moments)
    assert np.isfinite(want).all() and len(np.unique(want)) > 100, "a warm-up of 3 samples knows every pixel"
    same_words(prio.cpu().numpy(), want, "priority of a warm-up")
    for kw in (dict(budget_spp=2, min_samples=0, max_samples=8, scale=65536.0),
               dict(budget_spp=3, min_samples=1, max_samples=64, scale=4096.0)):
        check_plan(rt, want, w, h, kw, f"warm-up {kw}")
        budget = int(kw["budget_spp"] * w * h)
        samples = A.plan(want, w, h, budget, kw["min_samples"], kw["max_samples"], kw["scale"])[1]
        assert len(np.unique(samples)) >= 3, "the plan tells pixels apart"


# --- 7. end to end ----------------------------------------------------------------------------------------------------
def test_adaptive_sampler_end_to_end(rt):
    su = setup(rt, "room_open_sky")
    w, h = su["w"], su["h"]
    P = w * h
    sampler = rt.AdaptiveSampler(su["scene"], w, h, bounces=su["bounces"], seed=T.SEED)
    sampler.warmup(2)
    spent = []
    for _ in range(2):
        sampler.step(1.5, max_samples=3, scale=65536.0)
        spent.append(int(sampler.total.cpu()[0]))
    torch.cuda.synchronize()
    counts = sampler.counts().cpu().numpy().reshape(P)
    accum = rt.surface_view(sampler.accum, w).cpu().numpy().reshape(P, 4)
    budget = int(round(1.5 * P))
    assert all(0 < s <= budget for s in spent), (spent, budget)
    assert counts.sum() == 2 * P + sum(spent) and counts.min() >= 2 and counts.max() <= 8
    assert counts.min() < counts.max(), "the rounds told pixels apart"
    icounts = counts.astype(np.int64)
    assert (icounts == counts).all()
    want = chained(su, icounts, max_total=8)
    same_words(accum, want[0], "the sampler's accumulator against the oracle's chains with its own counts")
    same_words(sampler.moments.cpu().numpy(), want[1], "the sampler's moments")
    same_words(sampler.rng.cpu().numpy().view(U32).reshape(P, R.STATE_WORDS)[:, :6].copy(), want[2], "the sampler's states")
    same_words(rt.surface_view(sampler.image(), w).cpu().numpy().reshape(P, 4), A.resolve(accum), "the sampler's image")
    # the list of the last round is the reference's plan of the priorities before it
    listed = np.zeros(P, dtype=np.int64)
    listed[sampler.pixels.cpu().numpy()] = sampler.samples.cpu().numpy().view(np.uint16)
    assert listed.sum() == spent[1]
    sampler.reset()
    torch.cuda.synchronize()
    assert not bool(sampler.accum.any()) and not bool(sampler.moments.any())
    same_words(sampler.rng.cpu().numpy().view(U32).reshape(P, R.STATE_WORDS)[:, :6].copy(), su["states"], "reset states")


def test_raytracer_adaptive_leaves_the_frame_alone(rt):
    w, h = 64, 36
    tr = rt.RayTracer(w, h, scene="bunny", spp=2, bounces=3, seed=T.SEED)
    tr.process()
    torch.cuda.synchronize()
    frame, last, states, index = tr.surface.clone(), tr.last_frame.clone(), tr.rng.clone(), tr.frame_index
    sampler = tr.adaptive(2, 1.0, warmup=2, max_samples=4, scale=65536.0)
    image = sampler.image()
    torch.cuda.synchronize()
    assert torch.equal(tr.surface, frame) and torch.equal(tr.last_frame, last) and torch.equal(tr.rng, states)
    assert tr.frame_index == index
    view = rt.surface_view(image, w).cpu().numpy()
    counts = sampler.counts().cpu().numpy()
    assert np.isfinite(view).all() and (view[:, :, 3] == 1).all() and (view[:, :, 0:3] > 0).any()
    assert counts.min() >= 2 and 2 * w * h < counts.sum() <= 4 * w * h
    # the warm-up is the renderer's own frame: the same seed, the same states, the same two samples a pixel
    again = rt.AdaptiveSampler(tr.scene, w, h, bounces=3, seed=T.SEED)
    again.warmup(2)
    torch.cuda.synchronize()
    first = rt.surface_view(again.image(), w).cpu().numpy()
    assert np.array_equal(first[:, :, 0:3], rt.surface_view(frame, w).cpu().numpy()[:, :, 0:3])
