"""rt_radiance without a GPU: the struct, the host-side argument checks, the panorama ray table, and the two facts
that make the GPU comparisons of tests/test_gpu_radiance.py mean something -- radiance_ref's XORWOW step is the
oracle's, and the oracle's per-offset sample table, followed along each pixel's chain, is the oracle's own frame."""
import ctypes
import os
import re

import numpy as np
import pytest

import radiance_ref as R
import rt_testlib as T
import scene_cases as C

F32, U32 = np.float32, np.uint32
DUMMY = 0x1000  # non-null, 16-byte aligned, never dereferenced on these paths
# the caller-built cases tests/test_gpu_radiance.py checks against the table
TABLE_CASES = ["room_closed", "room_tilted", "room_inside_sphere", "spheres70", "deck62", "deck29_plain"]
CHAIN_ENTRIES = 14  # a sample draws at most 2 + 4 * 6 = 26 numbers: 14 entries cover the two samples of a case


def test_struct_layout():
    rt = T.load_rt()
    text = open(os.path.join(T.ROOT, "include", "rt_abi.h")).read()
    name, cls = "rt_radiance_params", rt.RadianceParams
    size = int(re.search(r"sizeof\(%s\) == (\d+)" % name, text).group(1))
    offsets = dict((k, int(v)) for k, v in re.findall(r"offsetof\(%s, (\w+)\) == (\d+)" % name, text))
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = [n for decl in body.split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip().replace("*", " "))]
    fields = [f for f, _ in cls._fields_]
    assert size == 48 == ctypes.sizeof(cls)
    assert declared == fields, (declared, fields)
    assert set(offsets) == set(fields)  # the header pins every offset
    for k, off in offsets.items():
        assert getattr(cls, k).offset == off, k


def test_symbols_and_binding():
    rt = T.load_rt()
    assert hasattr(rt.lib(), "rt_radiance") and "rt_radiance" in rt.SIGNATURES
    for name in ("radiance", "ray_rng", "panorama_rays", "panorama"):
        assert callable(getattr(rt, name))
    assert callable(rt.RayTracer.panorama)


def test_error_paths_without_device():
    rt = T.load_rt()
    L = rt.lib()
    scene = ctypes.byref(rt.GPUScene())

    def params(**kw):
        p = rt.RadianceParams()
        p.rays, p.rng, p.radiance, p.count, p.bounces, p.samples = DUMMY, DUMMY, DUMMY, 64, 6, 1
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def refused(word, scene=scene, **kw):
        code = L.rt_radiance(ctypes.byref(params(**kw)), scene, None)
        msg = L.rt_last_error()
        assert code != 0 and msg.startswith(b"rt_radiance: ") and word in msg, (kw, code, msg)

    assert L.rt_radiance(None, scene, None) != 0 and L.rt_last_error() == b"rt_radiance: null params"
    refused(b"null scene", scene=None)
    refused(b"null rays", rays=None)
    refused(b"null rng", rng=None)
    refused(b"null radiance", radiance=None)
    refused(b"flags", flags=1)
    refused(b"waves_per_simd", waves_per_simd=4)
    refused(b"waves_per_simd", waves_per_simd=8)
    refused(b"negative count", count=-1)
    refused(b"2^31", count=2 ** 31 + 1)
    refused(b"bounces", bounces=-1)
    refused(b"samples", samples=0)
    refused(b"samples", samples=2 ** 24 + 1)
    refused(b"aligned", rays=DUMMY + 8)
    refused(b"aligned", radiance=DUMMY + 4)
    refused(b"aligned", rng=DUMMY + 4)
    # the scene comes after them: a GPUScene nobody uploaded is a foreign one
    refused(b"not uploaded by rt_scene_upload")
    # count 0 returns at once, before the scene is looked at
    assert L.rt_radiance(ctypes.byref(params(count=0)), scene, None) == 0


def test_panorama_rays():
    rt = T.load_rt()
    w, h = 96, 48
    origin = (1.5, -2.0, 0.25)
    rays = rt.panorama_rays(origin, w, h)
    assert rays.shape == (w * h, 8) and rays.dtype == F32
    assert (rays[:, 0:3] == np.array(origin, dtype=F32)).all() and (rays[:, 3] == F32(rt.RAY_TMAX)).all() and (rays[:, 7] == 0).all()
    d = rays[:, 4:7].astype(np.float64)
    # unit length to within 2 ulp of 1 (three components rounded to fp32: |error| <= 3 * 2^-25 < 2 * 2^-23)
    assert np.abs(np.sqrt((d * d).sum(axis=1)) - 1.0).max() <= 2 * 2.0 ** -23
    grid = rays.reshape(h, w, 8)
    # the two centre columns straddle +z: x = -+sin(pi / W) cos(theta), z > 0; the first column looks along -z
    assert (grid[:, w // 2 - 1, 4] < 0).all() and (grid[:, w // 2, 4] > 0).all()
    assert np.array_equal(grid[:, w // 2 - 1, 4], -grid[:, w // 2, 4]) and (grid[:, w // 2, 6] > 0).all()
    mid = grid[h // 2, w // 2, 4:7].astype(np.float64)
    assert abs(mid[2] - np.cos(np.pi / w) * np.cos(np.pi / (2 * h))) < 1e-7
    assert (grid[:, 0, 6] < 0).all()
    # row 0 is the bottom: y grows with the row, from -cos(pi / 2H) to its negative
    assert (np.diff(grid[:, 0, 5].astype(np.float64)) > 0).all() and np.allclose(grid[:, :, 5], grid[:, :1, 5])
    assert abs(float(grid[0, 0, 5]) + np.cos(np.pi / (2 * h))) < 1e-7 and grid[h - 1, 0, 5] == -grid[0, 0, 5]
    # x grows to the right of +z (the renderer's image has -x on the right at angle_y = 180; a panorama is its own map)
    assert (grid[h // 2, w // 2 :, 4] > 0).all() and (grid[h // 2, : w // 2, 4] < 0).all()


def test_xorwow_advance_is_the_oracles_step():
    states = np.stack([T.oracle_rng_state(T.SEED, sub) for sub in (0, 1, 77, 1536)])
    n, skip = 40, [0, 1, 2, 26, 31]
    draws = np.zeros((len(states), n), dtype=F32)
    for k, s in enumerate(states):
        buf = (ctypes.c_float * n)()
        T.oracle().oracle_rng_draws((ctypes.c_uint32 * 6)(*[int(v) for v in s]), n, buf)
        draws[k] = np.array(buf[:], dtype=F32)
    assert np.array_equal(R.uniforms(states, n), draws), "curand_uniform of the restated step"
    for j in skip:
        adv = R.xorwow_advance(states, j)
        assert np.array_equal(R.uniforms(adv, n - j), draws[:, j:]), f"advanced by {j}"
    # a per-row count
    per_row = np.array([3, 0, 11, 26])
    adv = R.xorwow_advance(states, per_row)
    for k, j in enumerate(per_row):
        assert np.array_equal(R.uniforms(adv[k : k + 1], n - j)[0], draws[k, j:])
    assert np.array_equal(states, np.stack([T.oracle_rng_state(T.SEED, sub) for sub in (0, 1, 77, 1536)])), "inputs left alone"


@pytest.mark.parametrize("name", TABLE_CASES)
def test_table_chain_is_the_oracles_frame(name):
    """Following each pixel's sample chain through the table reproduces oracle_render's frame 0 and its final states:
    the table is a sound yardstick for single samples, and jittered_camera_rays' inputs (draws 2i, 2i + 1) are the
    ones the table's rows were computed from."""
    case = C.BY_NAME[name]
    w, h = case["width"], case["height"]
    want = C.oracle_frames(case)
    o, code = C.apply_oracle(case)
    assert code == 0
    states = T.oracle_rng_frame(T.SEED, w, h)
    tables = R.frame_tables(name, o, w, h, case["bounces"], states, CHAIN_ENTRIES)
    frame, draws = R.chain_frame(tables, case["spp"])
    got, ref = frame.reshape(h, w, 4), want["frames"][0]
    nan_g, nan_r = np.isnan(got), np.isnan(ref)
    differing = (nan_g != nan_r) | (~nan_g & ~nan_r & (got.view(U32) != ref.view(U32)))
    assert not differing.any(), f"{int(differing.any(axis=2).sum())} pixels differ"
    assert (draws % 2 == 0).all() and (tables[:, :, 3] >= 2).all() and (tables[:, :, 3] <= 2 + 4 * case["bounces"]).all()
    # frame 1 of oracle_frames advanced the states further; frame 0's end is the chain's end, which a fresh
    # single-frame render of the same pixels confirms
    rng = states.copy()
    o.render(w, h, case["spp"], case["bounces"], frame_index=0, rng=rng)
    assert np.array_equal(R.xorwow_advance(states, draws), rng)
    # the cases exercise the shading: some samples hit nothing, some end early, some run to the bounce limit
    d = tables[:, :4, 3]
    assert (d > 2).any() and (d < 2 + 4 * case["bounces"]).any()


def test_jittered_camera_rays_are_pixel_rays():
    """With jitter 0.5 the rays are rt_trace_rays' camera-mode rays (query_ref.camera_rays, same arithmetic)."""
    import query_ref as Q
    case = C.BY_NAME["room_tilted"]
    w, h = case["width"], case["height"]
    cam = C.oracle_frames(case)["camera"]
    half = np.full(w * h, 0.5, dtype=F32)
    got = R.jittered_camera_rays(cam, w, h, half, half)
    want = Q.camera_rays(cam, w, h)
    assert np.array_equal(got[:, 0:3], want[:, 0:3]) and np.array_equal(got[:, 4:7], want[:, 4:7])
