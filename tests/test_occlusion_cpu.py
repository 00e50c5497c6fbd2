"""Occlusion queries and AO without a GPU: the structs, the host-side argument checks of rt_occluded and rt_ao, the
direction table, and the conditions on the CPU reference that keep the GPU comparisons of
tests/test_gpu_occlusion.py from passing by being trivial."""
import ctypes
import os

import numpy as np
import pytest

import occlusion_cases as OC
import occlusion_ref as O
import rt_testlib as T

F32 = np.float32
DUMMY = 0x1000  # non-null, 16-byte aligned, never dereferenced on these paths


def test_symbols_and_binding():
    rt = T.load_rt()
    L = rt.lib()
    for name in ("rt_occluded", "rt_ao", "rt_ao_scratch_bytes"):
        assert hasattr(L, name) and name in rt.SIGNATURES
    for name in ("occluded", "ao_directions", "ambient_occlusion"):
        assert callable(getattr(rt, name))
    assert callable(rt.RayTracer.ao)


def test_rt_occluded_error_paths_without_device():
    rt = T.load_rt()
    L = rt.lib()
    scene = ctypes.byref(rt.GPUScene())

    def refused(word, scene=scene, **kw):
        p = rt.OcclusionParams()
        p.rays, p.count, p.occluded = DUMMY, 64, DUMMY
        for k, v in kw.items():
            setattr(p, k, v)
        code = L.rt_occluded(ctypes.byref(p), scene, None)
        msg = L.rt_last_error()
        assert code != 0 and msg.startswith(b"rt_occluded: ") and word in msg, (kw, code, msg)

    assert L.rt_occluded(None, scene, None) != 0 and L.rt_last_error() == b"rt_occluded: null params"
    refused(b"null scene", scene=None)
    refused(b"null occluded", occluded=None)
    refused(b"null rays", rays=None)
    refused(b"flags", flags=1)
    refused(b"waves_per_simd", waves_per_simd=4)
    refused(b"waves_per_simd", waves_per_simd=8)
    refused(b"negative count", count=-1)
    refused(b"2^31", count=2 ** 31 + 1)
    refused(b"aligned", rays=DUMMY + 4)
    # count 0 returns at once, before the scene is looked at
    p = rt.OcclusionParams()
    p.rays, p.count, p.occluded = DUMMY, 0, DUMMY
    assert L.rt_occluded(ctypes.byref(p), scene, None) == 0


def test_rt_ao_error_paths_without_device():
    rt = T.load_rt()
    L = rt.lib()
    scene = ctypes.byref(rt.GPUScene())

    def params(**kw):
        p = rt.AoParams()
        p.hits, p.directions, p.ao = DUMMY, DUMMY, DUMMY
        p.width, p.height, p.direction_count, p.samples = 8, 4, 64, 4
        p.radius, p.bias = 8.0, 0.001
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def refused(word, scene=scene, **kw):
        code = L.rt_ao(ctypes.byref(params(**kw)), scene, None)
        msg = L.rt_last_error()
        assert code != 0 and msg.startswith(b"rt_ao: ") and word in msg, (kw, code, msg)

    assert L.rt_ao(None, scene, None) != 0 and L.rt_last_error() == b"rt_ao: null params"
    refused(b"null scene", scene=None)
    refused(b"null ao", ao=None)
    refused(b"null hits", hits=None)
    refused(b"null directions", directions=None)
    refused(b"flags", flags=1)
    refused(b"waves_per_simd", waves_per_simd=4)
    refused(b"waves_per_simd", waves_per_simd=8)
    refused(b"width", width=0)
    refused(b"height", height=-1)
    refused(b"2^30", width=65536, height=32768)
    refused(b"samples", samples=0)
    refused(b"samples", samples=65)
    refused(b"direction_count", direction_count=0)
    refused(b"direction_count", direction_count=65537)
    refused(b"radius", radius=0.0)
    refused(b"radius", radius=-1.0)
    refused(b"radius", radius=float("nan"))
    refused(b"bias", bias=-1.0)
    refused(b"bias", bias=float("inf"))
    refused(b"aligned", hits=DUMMY + 4)
    refused(b"aligned", directions=DUMMY + 8)
    # scratch one byte short, wherever the call needs any
    for (w, h, s) in [(8, 4, 4), (1920, 1080, 64)]:
        need = L.rt_ao_scratch_bytes(w, h, s)
        if need:
            refused(b"scratch too small", width=w, height=h, samples=s, scratch=DUMMY, scratch_bytes=need - 1)


def test_ao_scratch_bytes():
    rt = T.load_rt()
    n = rt.ao_scratch_bytes
    assert n(0, 5, 4) == 0 and n(5, -1, 4) == 0 and n(5, 5, 0) == 0 and n(-1, -1, -1) == 0
    for (w, h, s) in [(1, 1, 1), (5, 3, 2), (64, 36, 8), (1920, 1080, 8), (32768, 32768, 64)]:
        assert n(w + 1, h, s) >= n(w, h, s) and n(w, h + 1, s) >= n(w, h, s) and n(w, h, min(s + 1, 64)) >= n(w, h, s)


def test_ao_directions():
    rt = T.load_rt()
    d = rt.ao_directions(64)
    assert d.shape == (64, 4) and d.dtype == np.float32 and (d[:, 3] == 0).all()
    length = np.sqrt((d[:, 0:3].astype(np.float64) ** 2).sum(axis=1))
    assert np.abs(length - 1.0).max() <= 1e-6
    assert np.abs(d[:, 0:3].astype(np.float64).mean(axis=0)).max() < 0.05  # spread over the sphere, not a cap
    assert rt.ao_directions().shape == (256, 4)
    assert len({tuple(r) for r in d.tolist()}) == 64


def test_hash_is_32_bit():
    # the product wraps at 2^32 before the shift: Python integers must be masked
    assert O.direction_index(3, 2, 64) == (((3 * 0x9E3779B1 + 2 * 0x85EBCA6B) % 2 ** 32) >> 8) % 64
    seen = {O.direction_index(i, k, 64) for i in range(576) for k in range(4)}
    assert len(seen) == 64  # every table entry is used at the test size


# --- the conditions on the reference that the GPU comparisons rest on ------------------------------------------------
def test_incoherent_classes():
    rays, want, free = OC.incoherent()
    k, kf = OC.kinds(want), OC.kinds(free)
    print("unbounded: misses", int((kf == 0).sum()), "hits", int((kf != 0).sum()), "; halved third misses",
          int((k[::3] == 0).sum()))
    assert (k[::3] == 0).all() and (want[::3, 0] == rays[::3, 3]).all()  # half the free distance: nothing in reach
    assert (kf == 0).sum() >= 64 and (kf != 0).sum() >= 64 and (k[::3] == 0).sum() >= 64
    assert (k != 0).sum() >= 64 and (k == 0).sum() >= 64
    assert O.occluded(OC.bunny()["arrays"], rays[:40]).tolist() == (k[:40] != 0).astype(np.uint8).tolist()


def test_tmax_edges():
    at, above, occ_at, occ_above = OC.tmax_edges()
    print("tmax = t:", int(occ_at.sum()), "of", len(at), "occluded; tmax = nextafter(t):", int(occ_above.sum()))
    assert len(at) >= 128
    # at its own distance a hit is not accepted (`t < closest`), so whatever is occluded there has a second surface
    # nearer; just above it most rays are occluded, and not all of them (a distance below its leaf's box entry)
    assert occ_above.sum() >= 64 and occ_above.sum() > occ_at.sum()
    assert (occ_at == 0).sum() >= 64


@pytest.mark.parametrize("which", ["bunny", "bunny4"])
def test_ao_reference_is_not_trivial(which):
    c = OC.ao_case(which)
    n = OC.AW * OC.AH
    counts = np.bincount(c["occ"], minlength=OC.AO_SAMPLES + 1)
    print(which, "valid pixels %.1f %%" % (100.0 * len(c["valid"]) / n), "occluded rays %.1f %%" %
          (100.0 * c["occ"].sum() / (len(c["valid"]) * OC.AO_SAMPLES)), "per-pixel counts", counts.tolist())
    assert 0.5 <= len(c["valid"]) / n <= 0.8
    assert len(counts) == OC.AO_SAMPLES + 1 and (counts >= 10).all()
    miss = np.ones(n, dtype=bool)
    miss[c["valid"]] = False
    assert (c["ao"][miss].view(np.uint32) == 0x3F800000).all()
    assert set(np.unique(c["ao"]).tolist()) == {0.0, 0.25, 0.5, 0.75, 1.0}
    # the rays are what rt_abi.h says: origin off the surface along the normal, unit directions in the normal's hemisphere
    valid, rays = O.ao_rays(c["hits"], OC.AW, OC.AH, OC.ao_directions(), OC.AO_SAMPLES, OC.AO_RADIUS, OC.AO_BIAS)
    nrm = np.repeat(c["hits"][valid, 4:7], OC.AO_SAMPLES, axis=0).astype(np.float64)
    d = rays[:, 4:7].astype(np.float64)
    assert np.abs(np.sqrt((d * d).sum(axis=1)) - 1.0).max() < 1e-6 and ((d * nrm).sum(axis=1) > -1e-6).all()
    assert (rays[:, 3] == F32(OC.AO_RADIUS)).all()


def test_render_image_ao_row_order(tmp_path):
    """tools/render_image.py --ao: the AO image comes in record order (row 0 = the bottom of the frame); the PFM keeps
    that order, the PPM runs top to bottom like the beauty frame's (whose rows tonemap flips)."""
    import sys
    import torch
    sys.path.insert(0, os.path.join(T.ROOT, "tools"))
    import render_image
    rt = T.load_rt()
    h, w = 5, 3
    ao = torch.tensor([0.0, 0.25, 0.5, 0.75, 1.0])[:, None].expand(h, w).contiguous()  # bottom row closed, top row open
    pfm, ppm = render_image.ao_outputs(ao)
    assert tuple(pfm.shape) == (h, w * 4) and pfm.dtype == torch.float32
    assert tuple(ppm.shape) == (h, w, 3) and ppm.dtype == torch.uint8
    rt.write_pfm(str(tmp_path / "ao.pfm"), pfm, w, h)
    rt.write_ppm(str(tmp_path / "ao.ppm"), ppm)
    raw = open(tmp_path / "ao.ppm", "rb").read()
    head = raw.split(b"\n", 3)
    assert head[0] == b"P6" and head[1].split() == [b"3", b"5"] and head[2] == b"255"
    rows = np.frombuffer(head[3], dtype=np.uint8).reshape(h, w, 3)
    assert rows[0].tolist() == [[255] * 3] * w and rows[-1].tolist() == [[0] * 3] * w  # PPM: first row = top of the frame
    assert rows[:, 0, 0].tolist() == [255, 191, 128, 64, 0]
    data = open(tmp_path / "ao.pfm", "rb").read()
    body = np.frombuffer(data[len(data) - h * w * 3 * 4:], dtype=np.float32).reshape(h, w, 3)
    assert body[:, 0, 0].tolist() == [0.0, 0.25, 0.5, 0.75, 1.0]  # PFM: first row = bottom of the frame
    # the two files show the same picture: PPM row r is PFM row h - 1 - r
    assert (rows[:, :, 0] == (body[::-1, :, 0] * 255.0 + 0.5).astype(np.uint8)).all()
