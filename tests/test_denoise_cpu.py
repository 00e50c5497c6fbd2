"""The denoiser without a GPU: rt_denoise's host-side argument checks, its structs and symbols, properties of the
numpy restatement the GPU tests compare against (tests/denoise_ref.py), and the quality of the committed
defaults on a 5-spp frame of the bunny scene."""
import ctypes
import os
import re

import numpy as np
import pytest

import denoise_cases as C
import denoise_ref as D
import query_ref as Q
import rt_testlib as T

F32 = np.float32
# A constant colour comes back within relative 2^-19 = 32 x 2^-24, for every number of passes: a pass is a weighted
# mean of at most 25 nearly equal values, about 27 rounding units of 2^-24 in the worst case; the reference's own
# deviations, printed by the tests, are 3 to 9 units.
BOUND = 2.0 ** -19


def test_error_paths_without_device():
    rt = T.load_rt()
    L = rt.lib()
    dummy = 0x1000  # non-null, 16-byte aligned, never dereferenced on these paths
    w, h = 8, 4

    def params(**kw):
        p = rt.DenoiseParams()
        p.surface, p.hits, p.materials, p.out, p.scratch = dummy, dummy, dummy, dummy, dummy
        p.pitch = p.out_pitch = w * 16
        p.width, p.height, p.material_count = w, h, 1
        p.scratch_bytes = L.rt_denoise_scratch_bytes(w, h)
        p.iterations = p.normal_power_log2 = rt.DENOISE_DEFAULT
        p.sigma_plane = p.sigma_color = rt.DENOISE_DEFAULT
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def refused(word, **kw):
        code = L.rt_denoise(ctypes.byref(params(**kw)), None)
        msg = L.rt_last_error()
        assert code != 0 and word in msg, (kw, code, msg)

    assert L.rt_denoise(None, None) != 0 and b"null params" in L.rt_last_error()
    refused(b"null surface", surface=None)
    refused(b"null hits", hits=None)
    refused(b"null out", out=None)
    refused(b"null scratch", scratch=None)
    refused(b"null materials", materials=None)
    refused(b"width", width=0)
    refused(b"height", height=-3)
    refused(b"RT_DENOISE_MAX_HEIGHT", height=131073, width=1)
    refused(b"RT_DENOISE_MAX_PIXELS", width=65536, height=32768)
    refused(b"pitch", pitch=w * 16 - 16)
    refused(b"out_pitch", out_pitch=w * 16 - 16)
    refused(b"multiples of 16", pitch=w * 16 + 4)
    refused(b"aligned", surface=dummy + 4)
    refused(b"scratch too small", scratch_bytes=L.rt_denoise_scratch_bytes(w, h) - 1)
    refused(b"scratch too small", scratch_bytes=0)
    refused(b"flags", flags=1)
    refused(b"iterations", iterations=0)
    refused(b"iterations", iterations=7)
    refused(b"iterations", iterations=-2)
    refused(b"normal_power_log2", normal_power_log2=9)
    refused(b"normal_power_log2", normal_power_log2=-2)
    refused(b"sigma_plane", sigma_plane=-0.5)
    refused(b"sigma_plane", sigma_plane=0.0)
    refused(b"sigma_plane", sigma_plane=float("nan"))
    refused(b"sigma_color", sigma_color=-0.5)
    refused(b"sigma_color", sigma_color=float("inf"))
    refused(b"material_count", material_count=-1)


def test_scratch_size():
    rt = T.load_rt()
    n = rt.denoise_scratch_bytes
    assert n(1, 1) > 0 and n(0, 5) == 0 and n(5, -1) == 0
    sizes = [(1, 1), (5, 3), (16, 16), (37, 19), (64, 36), (1920, 1080), (4096, 2160), (32768, 32768)]
    for (w, h) in sizes:
        assert n(w, h) >= w * h * 48  # the guide and two colour buffers at the least
        assert n(w + 1, h) >= n(w, h) and n(w, h + 1) >= n(w, h) and n(w + 1, h + 1) > n(w, h)
        assert n(w, h) % 16 == 0


def test_header_symbols_and_layout():
    rt = T.load_rt()
    L = rt.lib()
    for name in ("rt_denoise", "rt_denoise_scratch_bytes"):
        assert hasattr(L, name) and name in rt.SIGNATURES
    for name in ("denoise", "denoise_raw", "denoise_scratch_bytes"):
        assert callable(getattr(rt, name))
    assert callable(rt.RayTracer.denoised)
    text = open(os.path.join(T.ROOT, "include", "rt_abi.h")).read()
    m = re.search(r"sizeof\(rt_denoise_params\) == (\d+)", text)
    assert m and int(m.group(1)) == ctypes.sizeof(rt.DenoiseParams)
    pinned = dict((k, int(v)) for k, v in re.findall(r"offsetof\(rt_denoise_params, (\w+)\) == (\d+)", text))
    fields = [f for f, _ in rt.DenoiseParams._fields_]
    # the struct's members in the header, in order, are the mirror's
    body = re.search(r"typedef struct rt_denoise_params \{(.*?)\} rt_denoise_params;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = [n for decl in body.split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip().replace("*", " "))]
    assert declared == fields, (declared, fields)
    assert set(pinned) >= set(fields) - {"surface", "height"}
    for k, off in pinned.items():
        assert getattr(rt.DenoiseParams, k).offset == off, k
    assert re.search(r"#define RT_DENOISE_DEFAULT \(-1\)", text) and rt.DENOISE_DEFAULT == -1
    # the height limit keeps every launch grid (a row of blocks per 4 pixel rows at the least) within 65,535 rows
    assert int(re.search(r"#define RT_DENOISE_MAX_HEIGHT (\d+)", text).group(1)) // 4 <= 65535
    assert int(re.search(r"#define RT_DENOISE_MAX_PIXELS (\d+)", text).group(1)) == 1 << 30


def test_defaults_agree():
    """The defaults are written down in the kernel's unit, the Python binding and the reference: one set."""
    rt = T.load_rt()
    assert rt.DENOISE_DEFAULTS == D.DEFAULTS
    src = open(os.path.join(T.ROOT, "cuda-raytracing_amd", "csrc", "denoise.hip")).read()
    got = {"iterations": int(re.search(r"DEFAULT_ITERATIONS = (\d+);", src).group(1)),
           "normal_power_log2": int(re.search(r"DEFAULT_NORMAL_POWER_LOG2 = (\d+);", src).group(1)),
           "sigma_plane": float(re.search(r"DEFAULT_SIGMA_PLANE = ([\d.]+)f;", src).group(1)),
           "sigma_color": float(re.search(r"DEFAULT_SIGMA_COLOR = ([\d.]+)f;", src).group(1))}
    assert got == D.DEFAULTS


# --- properties of the reference --------------------------------------------------------------------------------
W, H = 23, 17
COLOUR = np.array([0.7, 0.3, 1.1, 0.25], dtype=F32)
MATS = C.material_table([(0.6, 0.5, 0.9), (0.2, 0.8, 0.4)])


def rel(got, want):
    return float(np.max(np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.abs(want.astype(np.float64))))


@pytest.mark.parametrize("iterations", [1, 2, 3, 4, 5, 6])
def test_constant_colour_over_a_plane(iterations):
    surf = np.broadcast_to(COLOUR, (H, W, 4)).copy()
    out = D.denoise(surf, C.plane(W, H), MATS, iterations=iterations)
    assert out.dtype == F32 and out.shape == surf.shape
    worst = rel(out[..., 0:3], surf[..., 0:3])
    print(f"{iterations} passes: worst relative deviation {worst:.3g} = {worst * 2 ** 24:.2f} x 2^-24")
    assert worst <= BOUND
    assert out[..., 3].tobytes() == surf[..., 3].tobytes()


def test_all_miss_image_comes_back_bytewise():
    g = np.random.default_rng(5)
    surf = g.gamma(0.7, 1.5, size=(H, W, 4)).astype(F32)
    surf[2, 3, 0], surf[4, 5, 1], surf[6, 7, 2], surf[8, 9, 3] = np.nan, np.inf, -0.0, np.nan
    surf[1, 1] = (1e-42, 1e30, -np.inf, 3.0)  # a denormal too
    hits = C.hit_records(np.zeros((H, W), dtype=np.int64), np.zeros((H, W), dtype=np.int64), np.zeros((H, W, 3), F32),
                         np.zeros((H, W, 3), F32), np.zeros((H, W), F32))
    assert D.denoise(surf, hits, MATS).tobytes() == surf.tobytes()
    assert D.denoise(surf, hits, MATS[:0], iterations=1).tobytes() == surf.tobytes()


def test_nan_pixel_among_finite_neighbours_comes_back_finite():
    surf = np.broadcast_to(COLOUR, (H, W, 4)).copy()
    surf[8, 11, 0:3] = (np.nan, 1.0, np.inf)
    surf[0, 0, 1] = np.nan  # a corner: 9 taps inside the image
    for it in (1, 5):
        out = D.denoise(surf, C.plane(W, H), MATS, iterations=it)
        assert np.isfinite(out).all()
        # ... and its neighbours never took it in: they are what they would be without it
        clean = D.denoise(np.broadcast_to(COLOUR, (H, W, 4)).copy(), C.plane(W, H), MATS, iterations=it)
        assert rel(out[..., 0:3], clean[..., 0:3]) <= BOUND


@pytest.mark.parametrize("kw", [{}, {"normal_power_log2": 0}, {"sigma_color": 0.0}, {"iterations": 1}])
def test_perpendicular_half_planes_do_not_mix(kw):
    hits, left = C.corner(W, H)
    other = np.array([2.5, 0.05, 0.4, 0.75], dtype=F32)
    surf = np.where(left[..., None], COLOUR, other).astype(F32)
    out = D.denoise(surf, hits, MATS, **kw)
    assert rel(out[..., 0:3], surf[..., 0:3]) <= BOUND
    assert out[..., 3].tobytes() == surf[..., 3].tobytes()


def test_the_filter_filters():
    """Noise over a plane is reduced (so the properties above are not those of the identity)."""
    g = np.random.default_rng(9)
    surf = (COLOUR * g.uniform(0.5, 1.5, size=(H, W, 1))).astype(F32)
    out = D.denoise(surf, C.plane(W, H), MATS, sigma_color=0.0)
    assert out[..., 0].std() < 0.35 * surf[..., 0].std()


# --- quality of the committed defaults -----------------------------------------------------------------------------
QW, QH = 96, 54


@pytest.fixture(scope="module")
def bunny_frames():
    osc = T.OracleScene("bunny")
    noisy = osc.render(QW, QH, 5, 6, frame_index=0, seed=T.SEED)
    rng = T.oracle_rng_frame(12345, QW, QH)
    target = None
    for f in range(64):
        target = osc.render(QW, QH, 5, 6, frame_index=f, rng=rng, last=target)
    arrays = osc.arrays()
    hits, _, _ = Q.trace(arrays, Q.camera_rays(osc.camera(QW, QH), QW, QH))
    mats = arrays["materials"].view(F32).reshape(-1, 16)
    return noisy, target, hits, mats


def test_quality_of_the_defaults(bunny_frames):
    noisy, target, hits, mats = bunny_frames
    hit = (hits.view(np.uint32)[:, 1] != 0).reshape(QH, QW)
    assert hit.sum() > QW * QH // 2
    before = D.display_error(noisy, target, hit)
    after = D.display_error(D.denoise(noisy, hits, mats), target, hit)
    print(f"display error over {int(hit.sum())} hit pixels: noisy {before:.4f}, denoised {after:.4f}, ratio {after / before:.3f}")
    assert after <= 0.6 * before
