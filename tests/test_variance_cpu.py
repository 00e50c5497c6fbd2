"""The variance-steered filter without a GPU: the host-side argument checks of rt_moments and rt_denoise_variance,
their structs and symbols, and hand-computed properties of the numpy restatement the GPU tests compare against
(tests/variance_ref.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

import denoise_cases as DC
import variance_cases as C
import variance_ref as V
import rt_testlib as T

F32 = np.float32
DUMMY = 0x10000  # non-null, 16-byte aligned, never dereferenced on these paths
W, H = 8, 4


def refusals(rt, call, make):
    L = rt.lib()

    def refused(word, **kw):
        p = make()
        for k, v in kw.items():
            setattr(p, k, v)
        code = getattr(L, call)(ctypes.byref(p), None)
        msg = L.rt_last_error()
        assert code != 0 and call.encode() in msg and word in msg, (kw, code, msg)

    assert getattr(L, call)(None, None) != 0 and b"null params" in L.rt_last_error()
    return refused


def test_moments_error_paths_without_device():
    rt = T.load_rt()

    def make():
        p = rt.MomentsParams()
        p.surface, p.hits, p.materials, p.out = DUMMY, 2 * DUMMY, 3 * DUMMY, 4 * DUMMY
        p.pitch = p.out_pitch = W * 16
        p.width, p.height, p.material_count = W, H, 1
        return p

    refused = refusals(rt, "rt_moments", make)
    refused(b"null surface", surface=None)
    refused(b"null hits", hits=None)
    refused(b"null out", out=None)
    refused(b"null materials", materials=None)
    refused(b"material_count", material_count=-1)
    refused(b"width", width=0)
    refused(b"height", height=-3)
    refused(b"RT_DENOISE_MAX_HEIGHT", height=131073, width=1)
    refused(b"RT_DENOISE_MAX_PIXELS", width=65536, height=32768, pitch=65536 * 16, out_pitch=65536 * 16)
    refused(b"pitch", pitch=W * 16 - 16)
    refused(b"out_pitch", out_pitch=W * 16 - 16)
    refused(b"multiples of 16", out_pitch=W * 16 + 4)
    refused(b"aligned", surface=DUMMY + 4)
    refused(b"aligned", out=4 * DUMMY + 8)
    refused(b"flags", flags=1)
    refused(b"out must not overlap surface", out=DUMMY)                       # out == surface
    refused(b"out must not overlap surface", out=DUMMY + W * 16 * (H - 1))    # its first row on the surface's last
    refused(b"out must not overlap hits", out=2 * DUMMY + 48 * W * H - 16)


def test_denoise_variance_error_paths_without_device():
    rt = T.load_rt()
    L = rt.lib()
    need = L.rt_denoise_variance_scratch_bytes(W, H)
    assert need < DUMMY

    def make():
        p = rt.DenoiseVarianceParams()
        p.surface, p.hits, p.materials, p.moments, p.history = DUMMY, 2 * DUMMY, 3 * DUMMY, 4 * DUMMY, 5 * DUMMY
        p.out, p.out_variance, p.scratch = 6 * DUMMY, 7 * DUMMY, 8 * DUMMY
        p.pitch = p.out_pitch = p.moments_pitch = W * 16
        p.width, p.height, p.material_count = W, H, 1
        p.scratch_bytes = need
        p.iterations = p.normal_power_log2 = rt.DENOISE_DEFAULT
        p.sigma_plane = p.sigma_lum = p.min_history = rt.DENOISE_DEFAULT
        return p

    refused = refusals(rt, "rt_denoise_variance", make)
    refused(b"null surface", surface=None)
    refused(b"null hits", hits=None)
    refused(b"null out", out=None)
    refused(b"null scratch", scratch=None)
    refused(b"null materials", materials=None)
    refused(b"material_count", material_count=-1)
    refused(b"width", width=0)
    refused(b"height", height=-3)
    refused(b"RT_DENOISE_MAX_HEIGHT", height=131073, width=1)
    refused(b"RT_DENOISE_MAX_PIXELS", width=65536, height=32768)
    refused(b"pitch", pitch=W * 16 - 16)
    refused(b"out_pitch", out_pitch=W * 16 - 16)
    refused(b"moments_pitch", moments_pitch=W * 16 - 16)
    refused(b"moments_pitch", moments_pitch=0)
    refused(b"multiples of 16", pitch=W * 16 + 4)
    refused(b"multiples of 16", moments_pitch=W * 16 + 8)
    refused(b"16-byte aligned", surface=DUMMY + 4)
    refused(b"16-byte aligned", moments=4 * DUMMY + 8)
    refused(b"16-byte aligned", scratch=8 * DUMMY + 4)
    refused(b"4-byte aligned", history=5 * DUMMY + 2)
    refused(b"4-byte aligned", out_variance=7 * DUMMY + 1)
    refused(b"scratch too small", scratch_bytes=need - 1)
    refused(b"scratch too small", scratch_bytes=0)
    refused(b"flags", flags=1)
    refused(b"reserved", reserved=1)
    refused(b"iterations", iterations=0)
    refused(b"iterations", iterations=7)
    refused(b"iterations", iterations=-2)
    refused(b"normal_power_log2", normal_power_log2=9)
    refused(b"normal_power_log2", normal_power_log2=-2)
    refused(b"sigma_plane", sigma_plane=0.0)
    refused(b"sigma_plane", sigma_plane=float("nan"))
    refused(b"sigma_lum", sigma_lum=0.0)
    refused(b"sigma_lum", sigma_lum=-0.5)
    refused(b"sigma_lum", sigma_lum=float("inf"))
    refused(b"sigma_lum", sigma_lum=float("nan"))
    refused(b"min_history", min_history=0.5)
    refused(b"min_history", min_history=0.0)
    refused(b"min_history", min_history=float("inf"))
    refused(b"min_history", min_history=float("nan"))
    out_bytes = W * 16 * H
    refused(b"out must not overlap scratch", out=8 * DUMMY + need - 16)
    refused(b"out must not overlap scratch", scratch=6 * DUMMY + out_bytes - 16)
    refused(b"out must not overlap hits", out=2 * DUMMY)
    refused(b"out must not overlap moments", out=4 * DUMMY)          # out == moments
    refused(b"out must not overlap moments", moments=6 * DUMMY + out_bytes - 16)
    refused(b"out must not overlap history", history=6 * DUMMY + 4)
    refused(b"out_variance must not overlap out", out_variance=6 * DUMMY + out_bytes - 4)
    refused(b"out_variance must not overlap scratch", out_variance=8 * DUMMY)
    # what is allowed is not refused by these checks: every message above names an argument, and a call that passes
    # them all would launch, so the allowed forms are exercised on the GPU (tests/test_gpu_variance.py)


def test_scratch_size():
    rt = T.load_rt()
    n = rt.denoise_variance_scratch_bytes
    assert n(1, 1) > 0 and n(0, 5) == 0 and n(5, -1) == 0 and n(0, 0) == 0 and n(-1, -1) == 0
    sizes = [(1, 1), (5, 3), (16, 16), (37, 19), (64, 36), (1920, 1080), (4096, 2160), (32768, 32768)]
    for (w, h) in sizes:
        assert w * h * 68 <= n(w, h) <= w * h * 72 + 16  # the guide, two colour-and-variance buffers, alpha
        assert n(w + 1, h) >= n(w, h) and n(w, h + 1) >= n(w, h) and n(w + 1, h + 1) > n(w, h)
        assert n(w, h) % 16 == 0
    row = [n(w, 7) for w in range(0, 70)]
    assert row == sorted(row)


@pytest.mark.parametrize("struct,mirror", [("rt_moments_params", "MomentsParams"),
                                           ("rt_denoise_variance_params", "DenoiseVarianceParams")])
def test_header_symbols_and_layout(struct, mirror):
    rt = T.load_rt()
    L = rt.lib()
    for name in ("rt_moments", "rt_denoise_variance", "rt_denoise_variance_scratch_bytes"):
        assert hasattr(L, name) and name in rt.SIGNATURES
    for name in ("moments", "denoise_variance", "denoise_variance_raw", "denoise_variance_scratch_bytes"):
        assert callable(getattr(rt, name))
    assert callable(rt.RayTracer.filtered) and callable(rt.VarianceAccumulator.push)
    cls = getattr(rt, mirror)
    text = open(os.path.join(T.ROOT, "include", "rt_abi.h")).read()
    m = re.search(r"sizeof\(%s\) == (\d+)" % struct, text)
    assert m and int(m.group(1)) == ctypes.sizeof(cls)
    pinned = dict((k, int(v)) for k, v in re.findall(r"offsetof\(%s, (\w+)\) == (\d+)" % struct, text))
    fields = [f for f, _ in cls._fields_]
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = [n for decl in body.split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip().replace("*", " "))]
    assert declared == fields, (declared, fields)
    assert set(pinned) == set(fields)  # every offset is pinned
    for k, off in pinned.items():
        assert getattr(cls, k).offset == off, k


def test_defaults_agree():
    """The defaults are written down in the kernel's unit, the Python binding, the reference and the header: one set,
    and sigma_lum and min_history are the point profiles/variance_quality.txt names."""
    rt = T.load_rt()
    assert rt.DENOISE_VARIANCE_DEFAULTS == V.DEFAULTS
    src = open(os.path.join(T.ROOT, "cuda-raytracing_amd", "csrc", "denoise_variance.hip")).read()
    got = {"iterations": int(re.search(r"DEFAULT_ITERATIONS = (\d+);", src).group(1)),
           "normal_power_log2": int(re.search(r"DEFAULT_NORMAL_POWER_LOG2 = (\d+);", src).group(1)),
           "sigma_plane": float(re.search(r"DEFAULT_SIGMA_PLANE = ([\d.]+)f;", src).group(1)),
           "sigma_lum": float(re.search(r"DEFAULT_SIGMA_LUM = ([\d.]+)f;", src).group(1)),
           "min_history": float(re.search(r"DEFAULT_MIN_HISTORY = ([\d.]+)f;", src).group(1))}
    assert got == V.DEFAULTS
    header = open(os.path.join(T.ROOT, "include", "rt_abi.h")).read()
    assert float(re.search(r"float sigma_lum;\s*/\* > 0, finite \(([\d.]+)\)", header).group(1)) == V.DEFAULTS["sigma_lum"]
    assert float(re.search(r"float min_history;\s*/\* >= 1, finite \(([\d.]+)\)", header).group(1)) == V.DEFAULTS["min_history"]
    record = open(os.path.join(T.ROOT, "profiles", "variance_quality.txt")).read()
    m = re.search(r"best grid point: sigma_lum ([\d.]+), min_history ([\d.]+)", record)
    assert m and (float(m.group(1)), float(m.group(2))) == (V.DEFAULTS["sigma_lum"], V.DEFAULTS["min_history"])


# --- properties of the reference --------------------------------------------------------------------------------
PW, PH = 23, 17
COLOUR = np.array([0.7, 0.3, 1.1, 0.25], dtype=F32)
MATS = DC.material_table([(0.6, 0.5, 0.9), (0.2, 0.8, 0.4)])


def test_moments_by_hand():
    surf = np.broadcast_to(COLOUR, (PH, PW, 4)).copy()
    m = V.moments(surf, DC.plane(PW, PH), MATS)
    c = COLOUR[0:3] / np.array([0.6, 0.5, 0.9], dtype=F32)
    l = (F32(0.2126) * c[0] + F32(0.7152) * c[1]) + F32(0.0722) * c[2]
    want = np.array([l, l * l, 0.0, COLOUR[3]], dtype=F32)
    assert m.dtype == F32 and m.tobytes() == np.broadcast_to(want, (PH, PW, 4)).tobytes()
    surf[3, 4, 1] = np.nan
    m = V.moments(surf, DC.plane(PW, PH), MATS)
    assert np.isnan(m[3, 4, 0:2]).all() and m[3, 4, 2] == 0 and m[3, 4, 3] == COLOUR[3] and np.isfinite(np.delete(m.reshape(-1, 4), 3 * PW + 4, 0)).all()


@pytest.mark.parametrize("iterations", [1, 3, 6])
@pytest.mark.parametrize("with_moments", [False, True])
def test_constant_image_is_a_fixed_point_with_variance_zero(iterations, with_moments):
    """A weighted mean sum(x * w_i) / sum(w_i) of equal values x is x bit for bit when x is a power of two: every
    x * w_i is exact, so the numerator's partial sums are x times the denominator's, roundings included.  The colour
    is therefore a power of two times the albedo in each channel, and the image comes back bytewise.  The temporal
    variance of (l, l*l) is m2 - m1*m1 = 0 exactly.  The spatial one is E[l^2] - E[l]^2 of 49 equal samples of weight
    1 (same normal, same plane) in fp32: each mean carries at most 50 roundings of 2^-24, so it is 0 up to
    2 * 50 * 2^-24 * l^2 and is asserted below 2^-17 * l^2; the passes only shrink it."""
    colour = np.array([0, 0, 0, 0.25], dtype=F32)
    colour[0:3] = MATS[0, 0:3] * np.array([2, 0.5, 4], dtype=F32)
    surf = np.broadcast_to(colour, (PH, PW, 4)).copy()
    hits = DC.plane(PW, PH)
    moments = history = None
    if with_moments:
        moments = V.moments(surf, hits, MATS)
        history = np.full((PH, PW), 8, dtype=F32)
    det = {}
    out, var = V.denoise_variance(surf, hits, MATS, moments=moments, history=history, iterations=iterations, details=det)
    assert out.dtype == F32 and var.dtype == F32 and var.shape == (PH, PW)
    assert out.tobytes() == surf.tobytes()
    assert det["temporal"].all() if with_moments else det["spatial"].all()
    l = float(V.lum(np.array([2, 0.5, 4], dtype=F32)))
    print(f"{iterations} passes, moments {with_moments}: largest variance {float(var.max()):.3g} (l*l = {l * l:.3g})")
    assert (var >= 0).all() and float(var.max()) <= (0.0 if with_moments else 2.0 ** -17 * l * l)
    assert float(det["initial_variance"].max()) <= (0.0 if with_moments else 2.0 ** -17 * l * l)


def test_zero_variance_tolerance_by_hand():
    """v = 0 everywhere and one pixel brighter than the rest: with two pixels only, the weights can be written down.
    tol = 1e-8f, wl = 1 / (1 + d*d / 1e-8f) for the neighbour, 1 for the pixel itself."""
    w, h = 2, 1
    hits = DC.plane(w, h)
    mats = DC.material_table([(1.0, 1.0, 1.0)])
    surf = np.array([[[1.0, 1.0, 1.0, 0.5], [1.0, 1.0, 1.0 + 2.0 ** -10, 0.75]]], dtype=F32)
    moments = V.moments(surf, hits, mats)  # variance 0
    history = np.full((h, w), 4, dtype=F32)
    det = {}
    out, var = V.denoise_variance(surf, hits, mats, moments=moments, history=history, iterations=1, normal_power_log2=0,
                                  sigma_plane=1e6, min_history=4, details=det)
    assert det["temporal"].all() and (det["initial_variance"] == 0).all()
    l0 = (F32(0.2126) * F32(1) + F32(0.7152) * F32(1)) + F32(0.0722) * surf[0, 0, 2]
    l1 = (F32(0.2126) * F32(1) + F32(0.7152) * F32(1)) + F32(0.0722) * surf[0, 1, 2]
    d = l1 - l0
    assert d != 0
    wl = F32(1) / (F32(1) + (d * d) / F32(1e-8))
    assert 0 < wl < 0.75  # d is about 7e-5, d*d about 5e-9: of the tolerance floor's size, the weight well inside (0, 1)
    # the plane's two pixels have the same normal and lie in each other's tangent plane: wn = wz = 1 exactly
    h2, h3 = F32(0.375), F32(0.25)
    w_self, w_other = (((h2 * h2) * F32(1)) * F32(1)) * F32(1), (((h2 * h3) * F32(1)) * F32(1)) * wl
    for p, q in ((0, 1), (1, 0)):
        want = (surf[0, p, 2] * w_self + surf[0, q, 2] * w_other) / (w_self + w_other)
        assert out[0, p, 2] == want and out[0, p, 0] == 1 and out[0, p, 3] == surf[0, p, 3]
    assert (var == 0).all()
    # the same with a wide tolerance (a large variance): the neighbour counts almost fully
    moments[..., 1] = moments[..., 0] * moments[..., 0] + F32(4.0)
    out2, var2 = V.denoise_variance(surf, hits, mats, moments=moments, history=history, iterations=1, normal_power_log2=0,
                                    sigma_plane=1e6, min_history=4)
    assert abs(out2[0, 0, 2] - out2[0, 1, 2]) < abs(out[0, 0, 2] - out[0, 1, 2])
    assert (var2 > 0).all() and (var2 < 1.0).all()  # (4 / 4 frames) filtered over two taps: below 1


@pytest.mark.parametrize("with_moments", [False, True])
def test_single_valid_pixel_among_misses_is_unchanged(with_moments):
    """Its only tap is itself, with weight w = h[2] * h[2] = 9/64: c' = (c * w) / w.  That is c bit for bit when
    c * 9 is exact, so the pixel's colour has short mantissas here (for a full mantissa the two roundings may leave
    one unit in the last place, in rt_denoise as well); the misses around it are random and come back bytewise."""
    g = np.random.default_rng(5)
    surf = g.gamma(0.7, 1.5, size=(PH, PW, 4)).astype(F32)
    surf[8, 11, 0:3] = (0.75, 1.5, 0.3125)
    kind = np.zeros((PH, PW), dtype=np.int64)
    kind[8, 11] = 2
    z3 = np.zeros((PH, PW, 3), F32)
    nrm = z3.copy()
    nrm[8, 11] = (0, 0, -1)
    pos = z3.copy()
    pos[8, 11] = (0.1, 0.2, 5.0)
    hits = DC.hit_records(kind, np.zeros((PH, PW), dtype=np.int64), nrm, pos, np.full((PH, PW), 5.0, F32))
    mats = DC.material_table([(1.0, 1.0, 1.0)])  # albedo 1: c * a / a is c
    moments = history = None
    if with_moments:
        moments = g.gamma(0.7, 1.5, size=(PH, PW, 4)).astype(F32)
        moments[8, 11, 0:2] = (1.0, 3.0)
        history = np.full((PH, PW), 4, dtype=F32)
    for it in (1, 6):
        out, var = V.denoise_variance(surf, hits, mats, moments=moments, history=history, iterations=it)
        assert out.tobytes() == surf.tobytes()
        # the only tap is the pixel itself: v' = v * w*w / (w*w), its own variance up to that rounding -- (3 - 1) / 4 = 0.5,
        # or 0 from the spatial estimate over one sample
        want = 0.5 if with_moments else 0.0
        assert var[8, 11] == pytest.approx(want, rel=1e-6) and (np.delete(var.reshape(-1), 8 * PW + 11) == 0).all()


def test_both_estimates_occur_in_every_case_and_the_clamp_clamps():
    for (w, h) in [(5, 3), (16, 16), (37, 19), (130, 9)]:
        case = C.synthetic(w, h, seed=w * 131 + h)
        det = {}
        V.denoise_variance(case["surface"], case["hits"], case["materials"], moments=case["moments"], history=case["history"],
                           iterations=1, details=det)
        assert det["temporal"].any() and det["spatial"].any(), (w, h)
        m = case["moments"]
        with np.errstate(all="ignore"):
            clamped = det["temporal"] & (m[..., 1] < m[..., 0] * m[..., 0])
        assert clamped.any() and (det["initial_variance"][clamped] == 0).all()
        assert (~np.isfinite(m[..., 0:2])).any() and np.isnan(case["history"]).any()
        if w >= 16 and h >= 16:
            kind = case["hits"].view(np.uint32)[:, 1].reshape(h, w)
            assert (kind == 0).any() and (~np.isfinite(case["surface"][..., 0:3])).any()
            assert (case["hits"].view(np.uint32)[:, 3] >= case["materials"].shape[0]).any()
            assert ((case["hits"][:, 0] == 0) & (kind.reshape(-1) != 0)).any()
        if w * h >= 256:
            assert set(np.floor(case["history"][np.isfinite(case["history"])]).astype(int).tolist()) >= set(range(0, 9))


def test_history_steers_the_tolerance():
    """The point of the feature, on the restatement: the same noisy plane and the same moments are smoothed less when
    the history says they are converged (variance / 32) than when it says they are fresh (variance / 1)."""
    g = np.random.default_rng(9)
    surf = (COLOUR * g.uniform(0.5, 1.5, size=(PH, PW, 1))).astype(F32)
    surf[..., 3] = COLOUR[3]
    hits = DC.plane(PW, PH)
    m = V.moments(surf, hits, MATS)
    m[..., 1] = m[..., 1] + F32(0.05)
    res = {}
    for n in (1, 32):
        out, var = V.denoise_variance(surf, hits, MATS, moments=m, history=np.full((PH, PW), n, F32), min_history=1, sigma_lum=1.0)
        res[n] = float(out[..., 0].std())
        assert (var >= 0).all() and out[..., 3].tobytes() == surf[..., 3].tobytes()
    assert res[1] < res[32] < float(surf[..., 0].std())
