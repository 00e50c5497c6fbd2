"""The host-side refusals of the image-space entry points (rt_denoise, rt_moments, rt_denoise_variance, rt_reproject,
rt_tonemap_srgb8) that need no device, as one table in the style of test_batch_errors_cpu.py: the exact rt_last_error
text of each, and rows with two faults at once that pin which check comes first.  Every row is refused before any
launch; the pointers are dummies that nothing dereferences on these paths."""
import ctypes

import pytest

import rt_testlib as T

# distinct buffers 1 MiB apart, all 16-byte aligned; the frame is 8 x 4 pixels with a tight pitch
S, H, O, C, M, HI, V, MA, PS, PH, PHI, OH = (0x100000 * i for i in range(1, 13))
W, HT, ROW = 8, 4, 8 * 16
N = W * HT
NAN, INF = float("nan"), float("inf")
IMAGE = dict(surface=S, pitch=ROW, width=W, height=HT, hits=H, out=O, out_pitch=ROW)
FILTER = dict(iterations=-1, normal_power_log2=-1, sigma_plane=-1.0)
DEFAULTS = {
    "rt_denoise": ("DenoiseParams", dict(IMAGE, **FILTER, scratch=C, scratch_bytes=N * 64, sigma_color=-1.0)),
    "rt_moments": ("MomentsParams", dict(IMAGE)),
    "rt_denoise_variance": ("DenoiseVarianceParams", dict(IMAGE, **FILTER, scratch=C, scratch_bytes=N * 68, moments=M,
                                                          moments_pitch=ROW, history=HI, out_variance=V, sigma_lum=-1.0,
                                                          min_history=-1.0)),
    "rt_reproject": ("ReprojectParams", dict(IMAGE, out_history=OH, prev_surface=PS, prev_pitch=ROW, prev_hits=PH,
                                             prev_history=PHI, max_history=-1, sigma_plane=-1.0, normal_min=-1.0)),
}
WH, TALL, PIX = "width and height must be > 0", "height above RT_%s_MAX_HEIGHT", "more than RT_%s_MAX_PIXELS pixels"
NEG_MC, NO_MAT = "negative material_count", "null materials with material_count > 0"
PITCH, OPITCH, MPITCH, PPITCH = ("%s smaller than width * 16" % n for n in ("pitch", "out_pitch", "moments_pitch", "prev_pitch"))
PITCH16, FLAGS, RESERVED = "pitches must be multiples of 16", "flags must be 0", "reserved must be 0"
D16 = "surface, hits, materials, out and scratch must be 16-byte aligned"
M16 = "surface, hits, materials and out must be 16-byte aligned"
V16 = "surface, hits, materials, moments, out and scratch must be 16-byte aligned"
V4 = "history and out_variance must be 4-byte aligned"
R16 = "surface, hits, prev_surface, prev_hits and out must be 16-byte aligned"
R4 = "prev_history and out_history must be 4-byte aligned"
SCRATCH = "scratch too small (rt_%s_scratch_bytes)"
ITER, NPOW = ("%s (or RT_DENOISE_DEFAULT)" % s for s in ("iterations must be 1..6", "normal_power_log2 must be 0..8"))
SPLANE, SCOLOR, SLUM, MINH = ("%s (or RT_DENOISE_DEFAULT)" % s for s in (
    "sigma_plane must be > 0 and finite", "sigma_color must be >= 0 and finite", "sigma_lum must be > 0 and finite",
    "min_history must be >= 1 and finite"))
MAXH, RPLANE, NMIN = ("%s (or RT_REPROJECT_DEFAULT)" % s for s in (
    "max_history must be 1..65535", "sigma_plane must be > 0 and finite", "normal_min must be in [-1, 1]"))
PREVS = "prev_surface, prev_hits and prev_history must be all NULL or all non-NULL"
NO_PREV = dict(prev_surface=None, prev_hits=None, prev_history=None)
TALL_FRAME, WIDE_FRAME = dict(width=1, height=131073), dict(width=32768, height=32769)  # the latter: 2^30 + 2^15 pixels


def overlaps(a, b):
    return "%s must not overlap %s" % (a, b)


# (call, parameter overrides or None for null params, message after "call: "); in each block the single faults in the
# call's order of checks, then the rows with two
TABLE = [("rt_denoise", kw, m) for kw, m in [
    (None, "null params"), (dict(surface=None), "null surface"), (dict(hits=None), "null hits"), (dict(out=None), "null out"),
    (dict(scratch=None), "null scratch"), (dict(width=0), WH), (dict(height=-1), WH), (TALL_FRAME, TALL % "DENOISE"),
    (WIDE_FRAME, PIX % "DENOISE"), (dict(material_count=-1), NEG_MC), (dict(material_count=1), NO_MAT),
    (dict(pitch=ROW - 16), PITCH), (dict(out_pitch=ROW - 16), OPITCH), (dict(pitch=ROW + 8), PITCH16),
    (dict(out_pitch=ROW + 4), PITCH16), (dict(surface=S + 4), D16), (dict(hits=H + 8), D16), (dict(out=O + 1), D16),
    (dict(scratch=C + 2), D16), (dict(materials=MA + 4, material_count=1), D16), (dict(materials=MA + 4), D16),
    (dict(scratch_bytes=N * 64 - 1), SCRATCH % "denoise"), (dict(flags=1), FLAGS), (dict(iterations=0), ITER),
    (dict(iterations=7), ITER), (dict(normal_power_log2=-2), NPOW), (dict(normal_power_log2=9), NPOW),
    (dict(sigma_plane=0.0), SPLANE), (dict(sigma_plane=INF), SPLANE), (dict(sigma_plane=NAN), SPLANE),
    (dict(sigma_color=-0.5), SCOLOR), (dict(sigma_color=INF), SCOLOR), (dict(sigma_color=NAN), SCOLOR),
    (dict(surface=None, hits=None), "null surface"), (dict(hits=None, out=None), "null hits"),
    (dict(out=None, scratch=None), "null out"), (dict(scratch=None, width=0), "null scratch"),
    (dict(width=0, height=131073), WH), (dict(TALL_FRAME, material_count=-1), TALL % "DENOISE"),
    (dict(WIDE_FRAME, material_count=-1), PIX % "DENOISE"), (dict(material_count=-1, pitch=0), NEG_MC),
    (dict(material_count=1, pitch=0), NO_MAT), (dict(pitch=0, out_pitch=0), PITCH), (dict(out_pitch=0, surface=S + 4), OPITCH),
    (dict(pitch=ROW + 8, surface=S + 4), PITCH16), (dict(surface=S + 4, scratch_bytes=0), D16),
    (dict(scratch_bytes=0, flags=1), SCRATCH % "denoise"), (dict(flags=1, iterations=0), FLAGS),
    (dict(iterations=0, normal_power_log2=9), ITER), (dict(normal_power_log2=9, sigma_plane=0.0), NPOW),
    (dict(sigma_plane=NAN, sigma_color=NAN), SPLANE),
]] + [("rt_moments", kw, m) for kw, m in [
    (None, "null params"), (dict(surface=None), "null surface"), (dict(hits=None), "null hits"), (dict(out=None), "null out"),
    (dict(width=-1), WH), (dict(height=0), WH), (TALL_FRAME, TALL % "DENOISE"), (WIDE_FRAME, PIX % "DENOISE"),
    (dict(material_count=-1), NEG_MC), (dict(material_count=2), NO_MAT), (dict(pitch=ROW - 16), PITCH),
    (dict(out_pitch=ROW - 16), OPITCH), (dict(pitch=ROW + 8), PITCH16), (dict(out_pitch=ROW + 4), PITCH16),
    (dict(surface=S + 4), M16), (dict(hits=H + 8), M16), (dict(out=O + 1), M16), (dict(materials=MA + 2), M16),
    (dict(flags=2), FLAGS), (dict(out=S), overlaps("out", "surface")), (dict(out=S + (HT - 1) * ROW + ROW - 16), overlaps("out", "surface")),
    (dict(out=H), overlaps("out", "hits")), (dict(out=H + N * 48 - 16), overlaps("out", "hits")),
    (dict(out=H - HT * ROW + 16), overlaps("out", "hits")),
    (dict(surface=None, out=None), "null surface"), (dict(out=None, width=0), "null out"), (dict(width=0, height=131073), WH),
    (dict(TALL_FRAME, material_count=-1), TALL % "DENOISE"), (dict(WIDE_FRAME, material_count=1), PIX % "DENOISE"),
    (dict(material_count=-1, pitch=0), NEG_MC), (dict(material_count=1, out_pitch=0), NO_MAT), (dict(pitch=0, out_pitch=0), PITCH),
    (dict(out_pitch=0, pitch=ROW + 8), OPITCH), (dict(out_pitch=ROW + 8, out=O + 4), PITCH16), (dict(hits=H + 4, flags=1), M16),
    (dict(flags=1, out=S), FLAGS), (dict(surface=H, out=H), overlaps("out", "surface")),
    # out ends where surface begins: no overlap there, so the hits check is reached
    (dict(surface=H + N * 48 - 16, out=H + N * 48 - 16 - HT * ROW), overlaps("out", "hits")),
]] + [("rt_denoise_variance", kw, m) for kw, m in [
    (None, "null params"), (dict(surface=None), "null surface"), (dict(hits=None), "null hits"), (dict(out=None), "null out"),
    (dict(scratch=None), "null scratch"), (dict(width=0), WH), (dict(height=-1), WH), (TALL_FRAME, TALL % "DENOISE"),
    (WIDE_FRAME, PIX % "DENOISE"), (dict(material_count=-1), NEG_MC), (dict(material_count=1), NO_MAT),
    (dict(pitch=ROW - 16), PITCH), (dict(out_pitch=ROW - 16), OPITCH), (dict(moments_pitch=ROW - 16), MPITCH),
    (dict(pitch=ROW + 8), PITCH16), (dict(out_pitch=ROW + 4), PITCH16), (dict(moments_pitch=ROW + 8), PITCH16),
    (dict(surface=S + 4), V16), (dict(hits=H + 8), V16), (dict(out=O + 1), V16), (dict(scratch=C + 2), V16),
    (dict(materials=MA + 4), V16), (dict(moments=M + 8), V16), (dict(history=HI + 2), V4), (dict(out_variance=V + 1), V4),
    (dict(scratch_bytes=N * 68 - 1), SCRATCH % "denoise_variance"), (dict(flags=1), FLAGS), (dict(reserved=1), RESERVED),
    (dict(iterations=0), ITER), (dict(iterations=7), ITER), (dict(normal_power_log2=-2), NPOW), (dict(normal_power_log2=9), NPOW),
    (dict(sigma_plane=0.0), SPLANE), (dict(sigma_plane=INF), SPLANE), (dict(sigma_plane=NAN), SPLANE),
    (dict(sigma_lum=0.0), SLUM), (dict(sigma_lum=INF), SLUM), (dict(sigma_lum=NAN), SLUM), (dict(min_history=0.5), MINH),
    (dict(min_history=INF), MINH), (dict(min_history=NAN), MINH),
    (dict(out=C), overlaps("out", "scratch")), (dict(out=C + N * 68 - 16), overlaps("out", "scratch")),
    (dict(out=H), overlaps("out", "hits")), (dict(out=H + N * 48 - 16), overlaps("out", "hits")),
    (dict(out=M), overlaps("out", "moments")), (dict(out=HI), overlaps("out", "history")),
    (dict(out=HI + N * 4 - 16), overlaps("out", "history")), (dict(out_variance=O), overlaps("out_variance", "out")),
    (dict(out_variance=O + HT * ROW - 4), overlaps("out_variance", "out")), (dict(out_variance=C), overlaps("out_variance", "scratch")),
    (dict(out_variance=C + N * 68 - 4), overlaps("out_variance", "scratch")),
    # a null moments surface: its pitch is not looked at, and nothing overlaps it
    (dict(moments=None, moments_pitch=0, flags=1), FLAGS), (dict(moments=None, moments_pitch=8, flags=1), FLAGS),
    (dict(moments=None, history=None, out_variance=None, out=C), overlaps("out", "scratch")),
    (dict(scratch=None, hits=None), "null hits"), (dict(scratch=None, width=0), "null scratch"),
    (dict(WIDE_FRAME, material_count=-1), PIX % "DENOISE"), (dict(material_count=1, pitch=0), NO_MAT),
    (dict(pitch=0, out_pitch=0, moments_pitch=0), PITCH), (dict(out_pitch=0, moments_pitch=0), OPITCH),
    (dict(moments_pitch=0, pitch=ROW + 8), MPITCH), (dict(moments_pitch=ROW + 8, moments=M + 8), PITCH16),
    (dict(moments=M + 8, history=HI + 2), V16), (dict(out_variance=V + 2, scratch_bytes=0), V4),
    (dict(scratch_bytes=0, flags=1), SCRATCH % "denoise_variance"), (dict(flags=1, reserved=1), FLAGS),
    (dict(reserved=1, iterations=0), RESERVED), (dict(iterations=7, normal_power_log2=9), ITER),
    (dict(normal_power_log2=9, sigma_plane=NAN), NPOW), (dict(sigma_plane=0.0, sigma_lum=0.0), SPLANE),
    (dict(sigma_lum=NAN, min_history=0.0), SLUM), (dict(min_history=0.0, out=C), MINH),
    (dict(out=C, hits=C), overlaps("out", "scratch")), (dict(out=H, moments=H), overlaps("out", "hits")),
    (dict(out=M, history=M), overlaps("out", "moments")), (dict(out=HI, out_variance=HI), overlaps("out", "history")),
    # out begins where the scratch (the hits, the history) end: no overlap there, so the later check is reached
    (dict(out=C + N * 68, out_variance=C), overlaps("out_variance", "scratch")),
    (dict(out=C + N * 68, out_variance=C + N * 68), overlaps("out_variance", "out")),
    (dict(out=H + N * 48, out_variance=H + N * 48), overlaps("out_variance", "out")),
    (dict(out=HI + N * 4, out_variance=C), overlaps("out_variance", "scratch")),
]] + [("rt_reproject", kw, m) for kw, m in [
    (None, "null params"), (dict(surface=None), "null surface"), (dict(hits=None), "null hits"), (dict(out=None), "null out"),
    (dict(out_history=None), "null out_history"), (dict(prev_surface=None), PREVS), (dict(prev_hits=None), PREVS),
    (dict(prev_history=None), PREVS), (dict(prev_surface=None, prev_hits=None), PREVS),
    (dict(prev_hits=None, prev_history=None), PREVS), (dict(prev_surface=None, prev_history=None), PREVS), (dict(width=0), WH),
    (dict(height=-1), WH), (TALL_FRAME, TALL % "REPROJECT"), (WIDE_FRAME, PIX % "REPROJECT"), (dict(pitch=ROW - 16), PITCH),
    (dict(out_pitch=ROW - 16), OPITCH), (dict(prev_pitch=ROW - 16), PPITCH), (dict(pitch=ROW + 8), PITCH16),
    (dict(out_pitch=ROW + 4), PITCH16), (dict(prev_pitch=ROW + 8), PITCH16), (dict(surface=S + 4), R16), (dict(hits=H + 8), R16),
    (dict(out=O + 1), R16), (dict(prev_surface=PS + 2), R16), (dict(prev_hits=PH + 4), R16), (dict(out_history=OH + 2), R4),
    (dict(prev_history=PHI + 1), R4), (dict(flags=1), FLAGS), (dict(max_history=0), MAXH), (dict(max_history=65536), MAXH),
    (dict(sigma_plane=0.0), RPLANE), (dict(sigma_plane=INF), RPLANE), (dict(sigma_plane=NAN), RPLANE),
    (dict(normal_min=-1.5), NMIN), (dict(normal_min=1.5), NMIN), (dict(normal_min=NAN), NMIN),
    (dict(out=PS), overlaps("out", "prev_surface")), (dict(out=PS + HT * ROW - 16), overlaps("out", "prev_surface")),
    (dict(out_history=PHI), overlaps("out_history", "prev_history")),
    (dict(out_history=PHI + N * 4 - 4), overlaps("out_history", "prev_history")),
    # without a previous frame: prev_pitch is not looked at
    (dict(NO_PREV, prev_pitch=0, flags=1), FLAGS), (dict(NO_PREV, prev_pitch=8, flags=1), FLAGS),
    (dict(out=None, out_history=None), "null out"), (dict(out_history=None, prev_hits=None), "null out_history"),
    (dict(prev_hits=None, width=0), PREVS), (dict(width=0, height=131073), WH), (dict(TALL_FRAME, pitch=0), TALL % "REPROJECT"),
    (dict(WIDE_FRAME, pitch=0), PIX % "REPROJECT"), (dict(pitch=0, out_pitch=0, prev_pitch=0), PITCH),
    (dict(out_pitch=0, prev_pitch=0), OPITCH), (dict(prev_pitch=0, pitch=ROW + 8), PPITCH),
    (dict(prev_pitch=ROW + 8, prev_hits=PH + 4), PITCH16), (dict(prev_hits=PH + 4, prev_history=PHI + 2), R16),
    (dict(out_history=OH + 2, flags=1), R4), (dict(flags=1, max_history=0), FLAGS), (dict(max_history=0, sigma_plane=0.0), MAXH),
    (dict(sigma_plane=NAN, normal_min=NAN), RPLANE), (dict(normal_min=2.0, out=PS), NMIN),
    (dict(out=PS, out_history=PHI), overlaps("out", "prev_surface")),
    # out ends where prev_surface begins: no overlap there, so the history check is reached
    (dict(out=PS - HT * ROW, out_history=PHI), overlaps("out_history", "prev_history")),
]]
# rt_tonemap_srgb8(surface, pitch, width, height, out_rgb, stream): one message for every refusal
TONEMAP = [dict(surface=None), dict(out_rgb=None), dict(width=0), dict(width=-1), dict(height=0), dict(height=-3),
           dict(pitch=ROW - 1), dict(pitch=0), dict(surface=None, out_rgb=None, width=0)]


@pytest.mark.parametrize("call, overrides, message", TABLE, ids=lambda v: None if isinstance(v, dict) else v)
def test_refusal(call, overrides, message):
    rt = T.load_rt()
    L = rt.lib()
    p = None
    if overrides is not None:
        cls, defaults = DEFAULTS[call]
        p = getattr(rt, cls)()
        for k, v in {**defaults, **overrides}.items():
            setattr(p, k, v)
    code = getattr(L, call)(ctypes.byref(p) if p is not None else None, None)
    assert code == 1 and L.rt_last_error() == (call + ": " + message).encode(), (overrides, code, L.rt_last_error())


@pytest.mark.parametrize("overrides", TONEMAP, ids=lambda v: "-".join(v))
def test_tonemap_refusal(overrides):
    L = T.load_rt().lib()
    a = {**dict(surface=S, pitch=ROW, width=W, height=HT, out_rgb=O), **overrides}
    code = L.rt_tonemap_srgb8(a["surface"], a["pitch"], a["width"], a["height"], a["out_rgb"], None)
    assert code == 1 and L.rt_last_error() == b"rt_tonemap_srgb8: bad arguments", (overrides, code, L.rt_last_error())
