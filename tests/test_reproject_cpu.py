"""Temporal reprojection without a GPU: rt_reproject's host-side argument checks, its struct and symbols, and
properties of the numpy restatement the GPU tests compare against (tests/reproject_ref.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

import reproject_cases as C
import reproject_ref as R
import rt_testlib as T

F32 = np.float32
W, H = 23, 17
U = 2.0 ** -24  # one rounding of a value below 1
# An unmoved camera's projection lands within 2^-19 x width pixels of the pixel's own centre.  u = dot(d, A) / dn
# is built from the rounded record (the float64 position rounded to fp32, then minus O: 2 roundings per component),
# the constants N, A, B (3 roundings per component) and wn, two dot products (5 roundings each) and a division: no
# more than 16 roundings, each at most 2^-24 of a term that is itself at most |dn| here (the viewport is centred, so
# |d.x A.x| <= dn / 2 and d.z A.z = dn / 2), hence |du| <= 16 x 2^-24.  Times width, one more rounding, minus 0.5,
# another: below 2^-19 x width.  The reference's own worst, printed by the tests, is 1 to 2 x 2^-24 x width.
BOUND_PX = 2.0 ** -19 * max(W, H)


def test_error_paths_without_device():
    rt = T.load_rt()
    L = rt.lib()
    w, h = 8, 4
    ptr = {"surface": 0x1000, "hits": 0x2000, "prev_surface": 0x3000, "prev_hits": 0x4000, "prev_history": 0x5000,
           "out": 0x6000, "out_history": 0x7000}  # non-null, aligned, apart, never dereferenced on these paths

    def params(**kw):
        p = rt.ReprojectParams()
        for k, v in ptr.items():
            setattr(p, k, v)
        p.pitch = p.prev_pitch = p.out_pitch = w * 16
        p.width, p.height = w, h
        p.camera = p.prev_camera = rt._as_camera(C.pinhole(w, h))
        p.max_history = rt.REPROJECT_DEFAULT
        p.sigma_plane = p.normal_min = rt.REPROJECT_DEFAULT
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def refused(word, **kw):
        code = L.rt_reproject(ctypes.byref(params(**kw)), None)
        msg = L.rt_last_error()
        assert code != 0 and word in msg, (kw, code, msg)

    assert L.rt_reproject(None, None) != 0 and b"null params" in L.rt_last_error()
    refused(b"null surface", surface=None)
    refused(b"null hits", hits=None)
    refused(b"null out", out=None)
    refused(b"null out_history", out_history=None)
    for missing in (("prev_surface",), ("prev_hits",), ("prev_history",), ("prev_surface", "prev_hits"),
                    ("prev_surface", "prev_history"), ("prev_hits", "prev_history")):
        refused(b"all NULL or all non-NULL", **{k: None for k in missing})
    refused(b"width", width=0)
    refused(b"height", height=-3)
    refused(b"RT_REPROJECT_MAX_HEIGHT", height=131073, width=1)
    refused(b"RT_REPROJECT_MAX_PIXELS", width=65536, height=32768)
    refused(b"pitch", pitch=w * 16 - 16)
    refused(b"out_pitch", out_pitch=w * 16 - 16)
    refused(b"prev_pitch", prev_pitch=w * 16 - 16)
    for k in ("pitch", "prev_pitch", "out_pitch"):
        refused(b"multiples of 16", **{k: w * 16 + 4})
    for k in ("surface", "hits", "prev_surface", "prev_hits", "out"):
        refused(b"16-byte aligned", **{k: ptr[k] + 4})
    for k in ("prev_history", "out_history"):
        refused(b"4-byte aligned", **{k: ptr[k] + 2})
    refused(b"flags", flags=1)
    for v in (0, -2, 65536):
        refused(b"max_history", max_history=v)
    for v in (0.0, -0.5, float("nan"), float("inf")):
        refused(b"sigma_plane", sigma_plane=v)
    for v in (-1.5, 1.5, float("nan"), float("inf")):
        refused(b"normal_min", normal_min=v)
    refused(b"out must not overlap prev_surface", out=ptr["prev_surface"])
    refused(b"out must not overlap prev_surface", out=ptr["prev_surface"] + 16 * w * (h - 1))
    refused(b"out_history must not overlap prev_history", out_history=ptr["prev_history"])
    refused(b"out_history must not overlap prev_history", out_history=ptr["prev_history"] + 4 * (w * h - 1))
    # a prev pitch is not looked at without a previous frame, but the rest still is
    refused(b"flags", prev_surface=None, prev_hits=None, prev_history=None, prev_pitch=3, flags=2)


def test_header_symbols_and_layout():
    rt = T.load_rt()
    L = rt.lib()
    assert hasattr(L, "rt_reproject") and "rt_reproject" in rt.SIGNATURES
    for name in ("reproject_raw", "TemporalAccumulator"):
        assert callable(getattr(rt, name))
    assert callable(rt.RayTracer.reprojected) and callable(rt.TemporalAccumulator.push) and callable(rt.TemporalAccumulator.reset)
    text = open(os.path.join(T.ROOT, "include", "rt_abi.h")).read()
    m = re.search(r"sizeof\(rt_reproject_params\) == (\d+)", text)
    assert m and int(m.group(1)) == ctypes.sizeof(rt.ReprojectParams)
    pinned = dict((k, int(v)) for k, v in re.findall(r"offsetof\(rt_reproject_params, (\w+)\) == (\d+)", text))
    fields = [f for f, _ in rt.ReprojectParams._fields_]
    body = re.search(r"typedef struct rt_reproject_params \{(.*?)\} rt_reproject_params;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = [n for decl in body.split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip().replace("*", " "))]
    assert declared == fields, (declared, fields)
    assert declared == ["surface", "pitch", "hits", "prev_surface", "prev_pitch", "prev_hits", "prev_history", "out",
                        "out_pitch", "out_history", "camera", "prev_camera", "width", "height", "max_history",
                        "sigma_plane", "normal_min", "flags"]
    assert set(pinned) == set(fields)
    for k, off in pinned.items():
        assert getattr(rt.ReprojectParams, k).offset == off, k
    assert re.search(r"#define RT_REPROJECT_DEFAULT \(-1\)", text) and rt.REPROJECT_DEFAULT == -1
    assert re.search(r"#define RT_REPROJECT_MAX_HEIGHT RT_DENOISE_MAX_HEIGHT\b", text)
    assert re.search(r"#define RT_REPROJECT_MAX_PIXELS RT_DENOISE_MAX_PIXELS\b", text)


def test_defaults_agree():
    """The defaults are written down in the kernel's unit, the Python binding and the reference: one set, and it
    cites the measurement it was chosen from."""
    rt = T.load_rt()
    assert rt.REPROJECT_DEFAULTS == R.DEFAULTS
    src = open(os.path.join(T.ROOT, "cuda-raytracing_amd", "csrc", "reproject.hip")).read()
    got = {"max_history": int(re.search(r"DEFAULT_MAX_HISTORY = (\d+);", src).group(1)),
           "sigma_plane": float(re.search(r"DEFAULT_SIGMA_PLANE = ([\d.]+)f;", src).group(1)),
           "normal_min": float(re.search(r"DEFAULT_NORMAL_MIN = ([\d.]+)f;", src).group(1))}
    assert got == R.DEFAULTS
    assert "profiles/reproject_quality.txt" in src
    assert os.path.exists(os.path.join(T.ROOT, "profiles", "reproject_quality.txt"))


# --- properties of the reference --------------------------------------------------------------------------------
def colours(seed, lo=0.5, hi=1.5):
    g = np.random.default_rng(seed)
    img = g.uniform(lo, hi, size=(H, W, 4)).astype(F32)
    img[..., 3] = g.random((H, W)).astype(F32)
    return img


def history(k):
    return np.full((H, W), k, dtype=F32)


GENERIC = C.pinhole(W, H, (0.3, -0.2, 0.1), pixel=0.07)


def test_identity_camera_projects_onto_the_own_centre():
    hits = C.plane(GENERIC, W, H)
    fx, fy, valid = R.project(hits, GENERIC, GENERIC, W, H)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    worst = max(float(np.abs(fx.astype(np.float64) - xs).max()), float(np.abs(fy.astype(np.float64) - ys).max()))
    print(f"identity camera, {W}x{H}: worst distance from the own centre {worst:.3g} px = {worst / (U * max(W, H)):.2f} x 2^-24 x width")
    assert valid.all() and worst <= BOUND_PX


@pytest.mark.parametrize("k, max_history", [(4, 32), (5, 32), (64, 32), (1, 1), (31.5, 32)])
def test_identity_camera_is_a_running_mean(k, max_history):
    hits = C.plane(GENERIC, W, H)
    cur, prev = colours(1), colours(2)
    out, oh = R.reproject(cur, hits, GENERIC, (prev, hits, history(k), GENERIC), max_history=max_history)
    assert out.dtype == F32 and oh.dtype == F32 and out.shape == cur.shape and oh.shape == (H, W)
    n = min(k + 1, max_history)
    # hl = sum(k w) / sum(w): exactly k when k is a power of two (scaling by it commutes with every rounding), else
    # within the 4 products, 3 sums and the division of hl, 8 x 2^-24 relative, plus the rounding of hl + 1
    hist_bound = 0.0 if k in (1, 4, 64) else 9 * U * (k + 1)
    worst_h = float(np.abs(oh.astype(np.float64) - n).max())
    # pc is the bilinear blend of the four pixels around a point at most BOUND_PX off the centre: at most
    # 2 x BOUND_PX x (the range of the colours, 1) from the centre's colour, plus the blend's 16 roundings of values
    # below 1.5 and the mean's 4 of values below 3
    col_bound = 2 * BOUND_PX * 1.0 + 16 * U * 1.5 + 4 * U * 3
    want = prev[..., 0:3].astype(np.float64) + (cur[..., 0:3].astype(np.float64) - prev[..., 0:3]) / n
    worst_c = float(np.abs(out[..., 0:3] - want).max())
    print(f"k {k}, max {max_history}: history off by {worst_h:.3g} (bound {hist_bound:.3g}), colour off the running mean by "
          f"{worst_c:.3g} = {worst_c / U:.1f} x 2^-24 (bound {col_bound:.3g})")
    assert worst_h <= hist_bound and worst_c <= col_bound
    assert out[..., 3].tobytes() == cur[..., 3].tobytes()


@pytest.mark.parametrize("m", [1, 3, -2])
def test_lateral_shift_brings_the_previous_image_back_shifted(m):
    """Pixel 1/16 and depth 4: a footprint of 0.25 on the plane, every coordinate exact in fp32.  The camera moves m
    footprints to the right, so new pixel x sees what the previous pixel x + m saw."""
    cam0, cam1 = C.pinhole(W, H), C.pinhole(W, H, (0.25 * m, 0.0, 0.0))
    hits0, hits1 = C.plane(cam0, W, H), C.plane(cam1, W, H)
    cur, prev = colours(3), colours(4)
    out, oh = R.reproject(cur, hits1, cam1, (prev, hits0, history(4), cam0))
    xs = np.arange(W)
    seen = (xs + m >= 0) & (xs + m < W)
    fx, _, _ = R.project(hits1, cam1, cam0, W, H)
    worst_px = float(np.abs(fx[:, seen].astype(np.float64) - (xs[seen] + m)).max())
    shifted = prev[:, np.clip(xs + m, 0, W - 1), 0:3].astype(np.float64)
    want = shifted + (cur[..., 0:3].astype(np.float64) - shifted) / 5.0
    worst_c = float(np.abs(out[:, seen, 0:3] - want[:, seen]).max())
    col_bound = 2 * BOUND_PX * 1.0 + 16 * U * 1.5 + 4 * U * 3  # as for the unmoved camera
    print(f"shift {m}: projection off by {worst_px:.3g} px (bound {BOUND_PX:.3g}), colour by {worst_c:.3g} (bound {col_bound:.3g})")
    assert worst_px <= BOUND_PX and worst_c <= col_bound
    assert (oh[:, seen] == 5).all()
    # the revealed columns: the new frame itself, history 1
    assert (~seen).sum() == abs(m)
    assert out[:, ~seen].tobytes() == cur[:, ~seen].tobytes() and (oh[:, ~seen] == 1).all()


@pytest.mark.parametrize("same_material", [False, True])
def test_disoccluded_background_resets(same_material):
    """A foreground plane at depth 2 left of x = 0 before a background at depth 4; the camera moves 3 background
    footprints (6 foreground ones) to the right.  New background pixel x saw the previous pixel x + 3, which for
    the three pixels next to the edge held the foreground."""
    cam0, cam1 = C.pinhole(W, H), C.pinhole(W, H, (0.75, 0.0, 0.0))
    hits0, fg0 = C.two_planes(cam0, W, H)
    hits1, fg1 = C.two_planes(cam1, W, H)
    if same_material:  # then the tangent-plane test alone must tell them apart
        for h in (hits0, hits1):
            h.view(np.uint32)[:, 3] = 0
    prev = colours(5)
    prev[fg0] = (100.0, 100.0, 100.0, 1.0)
    cur = colours(6)
    out, oh = R.reproject(cur, hits1, cam1, (prev, hits0, history(4), cam0))
    xs = np.broadcast_to(np.arange(W), (H, W))
    bg1 = ~fg1
    landed_on_fg = bg1 & (xs + 3 < W) & fg0[:, np.clip(np.arange(W) + 3, 0, W - 1)]
    assert landed_on_fg.sum() == 3 * H and fg1.any() and bg1.any()
    assert (oh[landed_on_fg] == 1).all() and out[landed_on_fg].tobytes() == cur[landed_on_fg].tobytes()
    assert (out[bg1][:, 0:3] < 2.0).all()          # no background pixel took foreground colour
    kept = bg1 & (xs + 3 < W) & ~landed_on_fg
    assert kept.any() and (oh[kept] == 5).all()    # the rest of the background kept its history
    # the foreground moved 6 pixels: what is still in view kept its history and its colour
    fg_kept = fg1 & (xs + 6 < W)
    assert fg_kept.any() and (oh[fg_kept] == 5).all() and (out[fg_kept][:, 0:3] > 50.0).all()


def test_sky_keeps_its_history_under_translation():
    """Direction-only reprojection: a camera that only moves sees the same sky in every pixel."""
    cam0, cam1 = GENERIC, C.pinhole(W, H, (5.3, 2.0, -7.0), pixel=0.07)
    miss = C.all_miss(W, H)
    cur, prev = colours(7), colours(8)
    out, oh = R.reproject(cur, miss, cam1, (prev, miss, history(4), cam0))
    fx, fy, valid = R.project(miss, cam1, cam0, W, H)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    worst = max(float(np.abs(fx.astype(np.float64) - xs).max()), float(np.abs(fy.astype(np.float64) - ys).max()))
    print(f"sky under translation: worst distance from the own centre {worst:.3g} px (bound {BOUND_PX:.3g})")
    assert valid.all() and worst <= BOUND_PX and (oh == 5).all()
    # ... and a hit record in the previous frame is never taken by a sky pixel
    out2, oh2 = R.reproject(cur, miss, cam1, (prev, C.plane(cam0, W, H), history(4), cam0))
    assert (oh2 == 1).all() and out2.tobytes() == cur.tobytes()


def test_non_finite_values():
    hits = C.plane(GENERIC, W, H)
    cur, prev, hist = colours(9), colours(10), history(4)
    cur[3, 4, 0:3] = (np.nan, 1.0, np.inf)        # healed by its history
    prev[6, 7, 1] = np.nan                         # never taken
    prev[8, 9, 0:3] = (1e30, -np.inf, 0.0)
    hist[10, 11], hist[2, 2] = 0.0, 0.5
    hist[11:14, 12:15] = 0.0                       # no history at (13, 12) nor in any neighbour a sliver could come from
    hist[12, 13] = np.nan
    cur[12, 13, 2] = np.nan                        # NaN now and nothing to heal it with
    out, oh = R.reproject(cur, hits, GENERIC, (prev, hits, hist, GENERIC))
    assert np.isfinite(out[3, 4]).all() and oh[3, 4] == 4
    assert float(np.abs(out[3, 4, 0:3] - prev[3, 4, 0:3]).max()) <= 2 * BOUND_PX + 20 * U * 1.5
    for (y, x) in ((6, 7), (8, 9), (10, 11), (2, 2)):
        # the own centre carries all but 2 x BOUND_PX of the weight: without it the history is dropped or, where a
        # neighbour's sliver is taken, the neighbour's -- never the refused value
        assert np.isfinite(out[y, x]).all() and oh[y, x] in (1, 5)
    assert oh[12, 13] == 0 and out[12, 13].tobytes() == cur[12, 13].tobytes()
    finite = np.isfinite(out[..., 0:3]).all(axis=-1)
    assert (~finite).sum() == 1 and (oh[finite] >= 1).all()
    # the next frame ignores the pixel that stayed poisoned, and nothing else became non-finite
    cur2 = colours(11)
    out2, oh2 = R.reproject(cur2, hits, GENERIC, (out, hits, oh, GENERIC))
    # (its own tap is refused; a neighbour's sliver, one frame old, may be taken)
    assert np.isfinite(out2).all() and (oh2 >= 1).all() and oh2[12, 13] in (1, 2)


def test_alpha_and_null_prev():
    case = C.synthetic(37, 19, seed=4)
    cur = case["surface"]
    prev = (case["prev_surface"], case["prev_hits"], case["prev_history"], case["prev_camera"])
    out, oh = R.reproject(cur, case["hits"], case["camera"], prev, max_history=case["max_history"])
    assert np.isnan(cur[..., 3]).any() and out[..., 3].tobytes() == cur[..., 3].tobytes()
    assert (oh > 1).mean() > 0.3 and (oh == 1).any() and (oh == 0).any() and (oh <= case["max_history"]).all()
    first, fh = R.reproject(cur, case["hits"], case["camera"], None)
    assert first.tobytes() == cur.tobytes()
    finite = np.isfinite(cur[..., 0:3]).all(axis=-1)
    assert (~finite).any() and (fh[finite] == 1).all() and (fh[~finite] == 0).all()


def test_synthetic_case_covers_what_it_promises():
    w, h = 37, 19
    case = C.synthetic(w, h, seed=w * 131 + h)
    d = {}
    prev = (case["prev_surface"], case["prev_hits"], case["prev_history"], case["prev_camera"])
    out, oh = R.reproject(case["surface"], case["hits"], case["camera"], prev, max_history=case["max_history"], details=d)
    kind = case["hits"].view(np.uint32)[:, 1].reshape(h, w)
    with np.errstate(all="ignore"):
        O, N, A, B, wn = R.frame_constants(case["prev_camera"])
        pos = case["hits"][:, 8:11].reshape(h, w, 3)
        dn = R.dot(pos - O, N)
        assert ((kind != 0) & (dn == 0)).any() and ((kind != 0) & (wn / dn < 0)).any() and np.isnan(d["fx"]).any()
    assert (~d["valid"]).mean() > 0.05 and d["valid"].mean() > 0.5
    assert ((kind == 0) & (oh > 1)).any() and ((kind != 0) & (oh > 1)).any() and ((kind != 0) & d["valid"] & (oh == 1)).any()
    ph = case["prev_history"]
    assert np.isnan(ph).any() and (ph == 0).any() and (ph > case["max_history"]).any()
    fin = ph[np.isfinite(ph)]
    assert (fin != np.floor(fin)).any()
    assert (case["hits"][:, 0] == 0).any() and (case["hits"].view(np.uint32)[:, 3] >= 1 << 20).any()
