"""rt_upsample without a device: the ABI, the host-side refusals as a table in the style of test_image_errors_cpu.py
(the exact rt_last_error text of each, single faults in the call's order of checks, then rows with two faults that pin
which check comes first; the pointers are dummies that nothing dereferences on these paths), and properties of the numpy
restatement tests/upsample_ref.py that the GPU tests compare against."""
import ctypes
import os
import re

import numpy as np
import pytest

import denoise_cases as C
import rt_testlib as T
import upsample_cases as UC
import upsample_ref as U

F32 = np.float32


# --- the ABI ----------------------------------------------------------------------------------------------------
def test_header_symbols_and_layout():
    rt = T.load_rt()
    L = rt.lib()
    for name in ("rt_upsample", "rt_upsample_scratch_bytes"):
        assert hasattr(L, name) and name in rt.SIGNATURES
    for name in ("upsample", "upsample_raw", "upsample_scratch_bytes"):
        assert callable(getattr(rt, name))
    assert callable(rt.RayTracer.upsampled)
    text = open(os.path.join(T.ROOT, "include", "rt_abi.h")).read()
    m = re.search(r"sizeof\(rt_upsample_params\) == (\d+)", text)
    assert m and int(m.group(1)) == ctypes.sizeof(rt.UpsampleParams)
    pinned = dict((k, int(v)) for k, v in re.findall(r"offsetof\(rt_upsample_params, (\w+)\) == (\d+)", text))
    fields = [f for f, _ in rt.UpsampleParams._fields_]
    body = re.search(r"typedef struct rt_upsample_params \{(.*?)\} rt_upsample_params;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = [n for decl in body.split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip().replace("*", " "))]
    assert declared == fields, (declared, fields)
    assert set(pinned) == set(fields)
    for k, off in pinned.items():
        assert getattr(rt.UpsampleParams, k).offset == off, k
    assert re.search(r"#define RT_UPSAMPLE_DEFAULT \(-1\)", text) and rt.UPSAMPLE_DEFAULT == -1
    assert re.search(r"#define RT_UPSAMPLE_MAX_HEIGHT RT_DENOISE_MAX_HEIGHT\b", text)
    assert re.search(r"#define RT_UPSAMPLE_MAX_PIXELS RT_DENOISE_MAX_PIXELS\b", text)


def test_scratch_size():
    rt = T.load_rt()
    n = rt.upsample_scratch_bytes
    assert n(1, 1) > 0 and n(0, 5) == 0 and n(5, -1) == 0 and n(-3, -3) == 0 and n(0, 0) == 0
    for (w, h) in [(1, 1), (5, 3), (16, 16), (37, 19), (64, 36), (960, 540), (1920, 1080), (16384, 16384)]:
        assert n(w + 1, h) >= n(w, h) and n(w, h + 1) >= n(w, h) and n(w + 1, h + 1) > n(w, h)
        assert n(w, h) % 16 == 0


def test_defaults_agree():
    """The defaults are written down in the kernel's unit, the Python binding and the reference: one set."""
    rt = T.load_rt()
    assert rt.UPSAMPLE_DEFAULTS == U.DEFAULTS
    src = open(os.path.join(T.ROOT, "cuda-raytracing_amd", "csrc", "upsample.hip")).read()
    got = {"normal_power_log2": int(re.search(r"DEFAULT_NORMAL_POWER_LOG2 = (\d+);", src).group(1)),
           "sigma_plane": float(re.search(r"DEFAULT_SIGMA_PLANE = ([\d.]+)f;", src).group(1))}
    assert got == U.DEFAULTS


# --- the refusal table ------------------------------------------------------------------------------------------
# distinct buffers 1 MiB apart, all 16-byte aligned; the low frame is 8 x 4 pixels, the scale 2, both pitches tight
LS, LH, H, O, S, MA = (0x100000 * i for i in range(1, 7))
LW, LHT, SCALE = 8, 4, 2
LROW, OROW = LW * 16, LW * SCALE * 16
LN, N = LW * LHT, LW * LHT * SCALE * SCALE
OUT_BYTES = LHT * SCALE * OROW
NAN, INF = float("nan"), float("inf")
DEFAULT = dict(low_surface=LS, low_pitch=LROW, low_hits=LH, low_width=LW, low_height=LHT, scale=SCALE, hits=H, out=O,
               out_pitch=OROW, scratch=S, scratch_bytes=LN * 48, normal_power_log2=-1, sigma_plane=-1.0)
LOW_SIZE, SCALES = "low_width and low_height must be > 0", "scale must be 2, 3 or 4"
TALL, PIX = "height above RT_UPSAMPLE_MAX_HEIGHT", "more than RT_UPSAMPLE_MAX_PIXELS pixels"
NEG_MC, NO_MAT = "negative material_count", "null materials with material_count > 0"
LPITCH, OPITCH, PITCH16 = "low_pitch smaller than low_width * 16", "out_pitch smaller than width * 16", "pitches must be multiples of 16"
A16 = "low_surface, low_hits, hits, materials, out and scratch must be 16-byte aligned"
SCRATCH, FLAGS, RESERVED = "scratch too small (rt_upsample_scratch_bytes)", "flags must be 0", "reserved must be 0"
NPOW, SPLANE = ("%s (or RT_UPSAMPLE_DEFAULT)" % s for s in ("normal_power_log2 must be 0..8", "sigma_plane must be > 0 and finite"))
TALL_OUT = dict(low_width=1, low_height=65537)             # 131,074 rows
WIDE_OUT = dict(low_width=16384, low_height=16385)         # 2^30 + 2^16 pixels
HUGE_OUT = dict(low_width=1 << 30, low_height=1, scale=4)  # a width of 2^32: the output size is not computed in 32 bits
ONE_MAT = dict(materials=MA, material_count=1)


def overlaps(name):
    return "out must not overlap " + name


TABLE = [
    # single faults, in the order of the checks
    (None, "null params"), (dict(low_surface=None), "null low_surface"), (dict(low_hits=None), "null low_hits"),
    (dict(hits=None), "null hits"), (dict(out=None), "null out"), (dict(scratch=None), "null scratch"),
    (dict(low_width=0), LOW_SIZE), (dict(low_height=-1), LOW_SIZE), (dict(scale=1), SCALES), (dict(scale=5), SCALES),
    (dict(scale=0), SCALES), (dict(scale=-2), SCALES), (TALL_OUT, TALL), (dict(low_width=1, low_height=32769, scale=4), TALL),
    (WIDE_OUT, PIX), (HUGE_OUT, PIX), (dict(material_count=-1), NEG_MC), (dict(material_count=1), NO_MAT),
    (dict(low_pitch=LROW - 16), LPITCH), (dict(out_pitch=OROW - 16), OPITCH), (dict(out_pitch=LROW), OPITCH),
    (dict(low_pitch=LROW + 8), PITCH16), (dict(out_pitch=OROW + 4), PITCH16), (dict(low_surface=LS + 4), A16),
    (dict(low_hits=LH + 8), A16), (dict(hits=H + 2), A16), (dict(out=O + 1), A16), (dict(scratch=S + 4), A16),
    (dict(materials=MA + 4), A16), (dict(materials=MA + 8, material_count=1), A16),
    (dict(scratch_bytes=LN * 48 - 1), SCRATCH), (dict(scratch_bytes=0), SCRATCH),
    (dict(out=LS), overlaps("low_surface")), (dict(out=LS + LHT * LROW - 16), overlaps("low_surface")),
    (dict(out=LS - OUT_BYTES + 16), overlaps("low_surface")), (dict(out=LH), overlaps("low_hits")),
    (dict(out=LH + LN * 48 - 16), overlaps("low_hits")), (dict(out=H), overlaps("hits")),
    (dict(out=H + N * 48 - 16), overlaps("hits")), (dict(out=H - OUT_BYTES + 16), overlaps("hits")),
    (dict(out=S), overlaps("scratch")), (dict(out=S + LN * 48 - 16), overlaps("scratch")),
    (dict(ONE_MAT, out=MA), overlaps("materials")), (dict(ONE_MAT, out=MA + 48), overlaps("materials")),
    (dict(ONE_MAT, out=MA - OUT_BYTES + 16), overlaps("materials")),
    (dict(flags=1), FLAGS), (dict(flags=-1), FLAGS), (dict(reserved=1), RESERVED), (dict(normal_power_log2=-2), NPOW),
    (dict(normal_power_log2=9), NPOW), (dict(sigma_plane=0.0), SPLANE), (dict(sigma_plane=-0.5), SPLANE),
    (dict(sigma_plane=INF), SPLANE), (dict(sigma_plane=NAN), SPLANE),
    # out begins where a buffer ends, or ends where it begins: no overlap there, so the next check is reached
    (dict(out=S + LN * 48, flags=1), FLAGS), (dict(out=H - OUT_BYTES, flags=1), FLAGS), (dict(ONE_MAT, out=MA + 64, flags=1), FLAGS),
    (dict(out=MA, flags=1), FLAGS),  # no material table: nothing to overlap
    # two faults: the earlier check reports
    (dict(low_surface=None, low_hits=None), "null low_surface"), (dict(low_hits=None, hits=None), "null low_hits"),
    (dict(hits=None, out=None), "null hits"), (dict(out=None, scratch=None), "null out"), (dict(scratch=None, low_width=0), "null scratch"),
    (dict(low_width=0, scale=5), LOW_SIZE), (dict(TALL_OUT, scale=1), SCALES), (dict(TALL_OUT, material_count=-1), TALL),
    (dict(WIDE_OUT, material_count=-1), PIX), (dict(low_width=16384, low_height=65537), TALL),  # too tall and too many pixels
    (dict(material_count=-1, low_pitch=0), NEG_MC), (dict(material_count=1, low_pitch=0), NO_MAT),
    (dict(low_pitch=0, out_pitch=0), LPITCH), (dict(out_pitch=0, low_pitch=LROW + 8), OPITCH),
    (dict(low_pitch=LROW + 8, low_surface=LS + 4), PITCH16), (dict(hits=H + 4, scratch_bytes=0), A16),
    (dict(scratch_bytes=0, out=LS), SCRATCH), (dict(out=LS, flags=1), overlaps("low_surface")),
    (dict(out=LH, low_surface=LH), overlaps("low_surface")), (dict(out=H, low_hits=H), overlaps("low_hits")),
    (dict(out=S, hits=S), overlaps("hits")), (dict(ONE_MAT, out=MA, scratch=MA), overlaps("scratch")),
    (dict(flags=1, reserved=1), FLAGS), (dict(reserved=1, normal_power_log2=9), RESERVED),
    (dict(normal_power_log2=9, sigma_plane=NAN), NPOW),
]


@pytest.mark.parametrize("overrides, message", TABLE, ids=lambda v: None if isinstance(v, dict) else v)
def test_refusal(overrides, message):
    rt = T.load_rt()
    L = rt.lib()
    p = None
    if overrides is not None:
        p = rt.UpsampleParams()
        for k, v in {**DEFAULT, **overrides}.items():
            setattr(p, k, v)
    code = L.rt_upsample(ctypes.byref(p) if p is not None else None, None)
    assert code == 1 and L.rt_last_error() == ("rt_upsample: " + message).encode(), (overrides, code, L.rt_last_error())


# --- properties of the reference --------------------------------------------------------------------------------
LOW = (23, 17)
MATS = C.material_table([(0.6, 0.5, 0.9), (0.2, 0.8, 0.4)])
SYNTHETIC = [((5, 3), 2), ((37, 19), 2), ((22, 3), 3), ((17, 2), 4), ((19, 17), 3)]
# A pixel of constant input: 4 products wy*wx*g and c*w, 6 additions (3 into each sum), 3 divisions (by a_q, by wsum,
# tx) and 1 product by a_P, each within half an ulp; to first order their relative errors add up to 14 half ulps, and
# the bound leaves one ulp for the result's own binade.
ULPS = 8


def ulps(got, want):
    want = np.broadcast_to(np.asarray(want, dtype=F32), got.shape)
    return float(np.max(np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)))


@pytest.mark.parametrize("scale", [2, 3, 4])
def test_constant_colour_over_a_plane(scale):
    lw, lh = LOW
    hits = C.plane(lw * scale, lh * scale)
    colour = np.array([0.7, 0.3, 1.1, 0.25], dtype=F32)
    low = UC.constant(colour[0:3], lw, lh, alpha=colour[3])
    _, low_hits = UC.downsample(np.zeros((lh * scale, lw * scale, 4), F32), hits, lw, lh, scale)
    out, stage = U.upsample(low, low_hits, hits, MATS, scale)
    assert (stage == 1).all()
    worst = ulps(out[..., 0:3], colour[0:3])
    print("scale", scale, "worst error", worst, "ulps")
    assert worst <= ULPS
    assert (out[..., 3] == colour[3]).all()


@pytest.mark.parametrize("scale", [2, 3, 4])
def test_perpendicular_half_planes_do_not_mix(scale):
    lw, lh = LOW
    hits, left = C.corner(lw * scale, lh * scale)
    frame = np.where(left[..., None], F32(1), F32(3)).astype(F32).repeat(4, axis=-1)
    low, low_hits = UC.downsample(frame, hits, lw, lh, scale)
    assert (low[..., 0] == 1).any() and (low[..., 0] == 3).any()
    out, stage = U.upsample(low, low_hits, hits, MATS, scale)
    rgb = out[..., 0:3]
    print("scale", scale, "left", np.unique(rgb[left]), "right", np.unique(rgb[~left]), "stages", np.bincount(stage.reshape(-1)))
    # nothing of the other half's colour: a mixture would lie between the two
    assert ulps(rgb[left], F32(1)) <= ULPS and ulps(rgb[~left], F32(3)) <= ULPS


@pytest.mark.parametrize("scale", [2, 3, 4])
def test_all_miss_frame_is_bilinear(scale):
    lw, lh = LOW
    g = np.random.default_rng(scale)
    low = g.random((lh, lw, 4)).astype(F32) + F32(0.5)
    miss = np.zeros((lh, lw), dtype=np.int64)
    zeros3 = np.zeros((lh, lw, 3), F32)
    low_hits = C.hit_records(miss, miss, zeros3, zeros3, np.zeros((lh, lw), F32))
    big = np.zeros((lh * scale, lw * scale), dtype=np.int64)
    zeros3 = np.zeros((lh * scale, lw * scale, 3), F32)
    hits = C.hit_records(big, big, zeros3, zeros3, zeros3[..., 0])
    out, stage = U.upsample(low, low_hits, hits, MATS, scale)
    assert (stage == 1).all()
    want = U.bilinear(low, scale)
    # the same sums in fp32, all terms positive: bilinear() takes the same rounded weights, whose errors cancel between
    # sum and wsum; what is left to first order is 1 product c*w, 3 additions in each sum and 1 division, 8 half ulps
    assert np.max(np.abs(out[..., 0:3] - want) / want) <= ULPS * 2.0 ** -24
    # an interior pixel of scale 2 has the weights 9/16, 3/16, 3/16, 1/16
    if scale == 2:
        x, y = 5, 7  # low (2, 3) is its nearest; the footprint starts at low (2, 3) with tx = ty = 1/4
        w = np.array([[9, 3], [3, 1]]) / 16.0
        assert np.allclose(out[y, x, 0:3], (low[3:5, 2:4, 0:3].astype(np.float64) * w[..., None]).sum(axis=(0, 1)), rtol=1e-6, atol=0)


@pytest.mark.parametrize("low_size, scale", SYNTHETIC, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else "x%d" % v)
def test_every_stage_decides_pixels(low_size, scale):
    lw, lh = low_size
    low, low_hits, hits, materials = UC.synthetic(lw, lh, scale, seed=lw * 131 + lh)
    out, stage = U.upsample(low, low_hits, hits, materials, scale)
    share = np.bincount(stage.reshape(-1), minlength=4)[1:4] / stage.size
    print(low_size, scale, "stage shares", share)
    assert set(np.unique(stage)) <= {1, 2, 3}
    assert (share >= 0.01).all(), share
    # alpha is the nearest low pixel's, bytewise
    ys, xs = np.meshgrid(np.arange(lh * scale), np.arange(lw * scale), indexing="ij")
    assert out[..., 3].tobytes() == low[ys // scale, xs // scale, 3].tobytes()
    # stage 3 passes the nearest low pixel's colour through, finite or not
    third = stage == 3
    a_low = U.albedo(low_hits, materials, lh, lw)
    a = U.albedo(hits, materials, lh * scale, lw * scale)
    with np.errstate(all="ignore"):
        want = ((low[..., 0:3] / a_low)[ys // scale, xs // scale] * a)[third]
    assert out[..., 0:3][third].tobytes() == want.tobytes()
