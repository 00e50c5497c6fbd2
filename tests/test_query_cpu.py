"""Ray queries without a GPU: the C-ABI structs and symbols, rt_trace_rays' host-side argument checks, and
the Python reference of the GPU tests (tests/query_ref.py) pinned to the CPU oracle's own traversal."""
import ctypes
import os
import re

import numpy as np
import pytest

import query_ref as Q
import rt_testlib as T

W, H = 64, 36


def test_struct_layouts():
    rt = T.load_rt()
    assert ctypes.sizeof(rt.Ray) == 32 and ctypes.sizeof(rt.Hit) == 48 and ctypes.sizeof(rt.TraceParams) == 40
    assert [getattr(rt.Ray, f).offset for f in ("origin", "tmax", "direction", "reserved")] == [0, 12, 16, 28]
    assert [getattr(rt.Hit, f).offset for f in ("t", "kind", "id", "material", "normal", "bx", "position", "by")] == \
        [0, 4, 8, 12, 16, 28, 32, 44]
    assert [getattr(rt.TraceParams, f).offset for f in ("rays", "count", "width", "height", "hits", "flags",
                                                        "waves_per_simd")] == [0, 8, 16, 20, 24, 32, 36]
    # the header fixes the same numbers
    text = open(os.path.join(T.ROOT, "include", "rt_abi.h")).read()
    assert re.search(r"sizeof\(rt_ray\) == 32", text) and re.search(r"sizeof\(rt_hit\) == 48", text)


def test_symbols_exported_and_bound():
    rt = T.load_rt()
    L = rt.lib()
    for name in ("rt_trace_rays", "rt_scene_materials"):
        assert hasattr(L, name) and name in rt.SIGNATURES
    for name in ("trace_rays", "trace_camera", "hit_fields"):
        assert callable(getattr(rt, name))
    assert callable(rt.RayTracer.gbuffer) and callable(rt.Scene.materials)


def test_error_paths_without_device():
    rt = T.load_rt()
    L = rt.lib()
    scene = rt.GPUScene()
    dummy = 0x1000  # a non-null, 16-byte aligned address that is never dereferenced on these paths

    def call(p, s=scene):
        return L.rt_trace_rays(ctypes.byref(p) if p is not None else None, ctypes.byref(s) if s is not None else None, None)

    def params(**kw):
        p = rt.TraceParams()
        p.rays, p.hits, p.count = dummy, dummy, 64
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    assert call(None) != 0 and b"null params" in L.rt_last_error()
    assert call(params(), None) != 0 and b"null scene" in L.rt_last_error()
    assert call(params(hits=None)) != 0 and b"null hits" in L.rt_last_error()
    assert call(params(count=-1)) != 0 and b"negative" in L.rt_last_error()
    assert call(params(count=(1 << 31) + 1)) != 0 and b"2^31" in L.rt_last_error()
    assert call(params(flags=1)) != 0 and b"flags" in L.rt_last_error()
    assert call(params(waves_per_simd=4)) != 0 and b"waves_per_simd" in L.rt_last_error()
    assert call(params(rays=None, width=0, height=4)) != 0 and b"camera" in L.rt_last_error()
    assert call(params(rays=dummy + 4)) != 0 and b"aligned" in L.rt_last_error()
    assert call(params(count=0)) == 0
    # a GPUScene that rt_scene_upload did not fill has no private mirror: refused, and the message says so
    assert call(params()) != 0 and b"rt_scene_upload" in L.rt_last_error()


def test_scene_materials():
    rt = T.load_rt()
    s = rt.Scene()
    s.add_material(albedo=(0.25, 0.5, 0.75), emissive=(1, 2, 3), roughness=0.5)
    s.add_material(albedo=(1, 0, 0))
    m = s.materials()
    assert m.shape == (2, 16) and m.dtype == np.float32
    assert m[0, 0:3].tolist() == [0.25, 0.5, 0.75] and m[0, 4:7].tolist() == [1, 2, 3] and m[0, 12] == 0.5
    assert m[1, 0:3].tolist() == [1, 0, 0]
    bunny = T.product_scene("bunny").materials()
    want = T.OracleScene("bunny").arrays()["materials"].view(np.float32).reshape(-1, 16)
    assert bunny.tobytes() == want.tobytes()


@pytest.fixture(scope="module")
def pinned():
    """query_ref on the oracle's own frame-0 sample rays of the 64x36 bunny frame, and that frame."""
    osc = T.OracleScene("bunny")
    arrays = osc.arrays()
    rays = Q.camera_rays(osc.camera(W, H), W, H, jitter=Q.frame_jitter(T.SEED, W, H))
    hits, counters, leaf_size = Q.trace(arrays, rays)
    frame, stats = osc.render(W, H, 1, 1, stats=True)
    return arrays, hits, counters, leaf_size, frame, stats


def test_reference_counters_equal_the_oracles(pinned):
    _, _, c, _, _, st = pinned
    want = dict(zip(("seg", "nodes", "tris", "tacc", "sacc", "hits", "misses"), (int(v) for v in st[:7])))
    print("query_ref", c, "oracle", want)
    assert want["seg"] == W * H
    for k in ("nodes", "tris", "tacc", "sacc", "hits", "misses"):
        assert c[k] == want[k], k


def test_reference_hits_carry_the_oracles_materials(pinned):
    arrays, hits, _, _, frame, _ = pinned
    mats = arrays["materials"].view(np.float32).reshape(-1, 16)
    kind, mat = hits.view(np.int32)[:, 1], hits.view(np.int32)[:, 3]
    hit = kind != 0
    assert hit.sum() > W * H // 2 and (~hit).sum() > 0
    rgb = frame.reshape(-1, 4)[:, 0:3]
    # one sample, one bounce: a hit pixel's colour is its material's emission and nothing else
    assert rgb[hit].tobytes() == np.ascontiguousarray(mats[mat[hit], 4:7]).tobytes()
    assert len(set(mat[hit].tolist())) > 2


def test_reference_reaches_a_big_leaf(pinned):
    """The GPU tests are to exercise the wave-cooperative big-leaf rounds: at least one of these rays must end
    on a face of a leaf of more than 8 triangles (rtfast::BIG)."""
    _, _, _, leaf_size, _, _ = pinned
    assert (leaf_size > 8).any(), leaf_size.max()
