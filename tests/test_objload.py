"""OBJ input (cuda-raytracing_amd/csrc/objload.cpp) against the assimp 3.3 import of the
reference's data/stanford-bunny.obj (assets/bunny_mesh.bin, made by tools/make_assets.py):
the reference's Scene::AddLoadedScene (RayTracing/Scene.cpp:75-132) receives the same vertex
positions, vertex order and faces bit for bit, and normals within a few ulps (the smoothing
sum's order follows assimp's internal sort of tied SpatialSort entries, not reproduced).

The OBJ is the reference's own file, kept xz-compressed as tests/golden/stanford-bunny.obj.xz
(tools/make_assets.py fixtures) and unpacked into the test's temporary directory.  CPU only.
"""
import lzma
import os

import numpy as np
import pytest

import rt_testlib as T

OBJ_XZ = os.path.join(T.GOLDEN, "stanford-bunny.obj.xz")


@pytest.fixture
def obj_path(tmp_path):
    path = tmp_path / "stanford-bunny.obj"
    with lzma.open(OBJ_XZ) as src:
        path.write_bytes(src.read())
    return str(path)


def _scene(rt, path):
    s = rt.Scene()
    s.add_loaded_scene(path, np.eye(4, dtype=np.float32).reshape(-1).tolist(), 0)
    s.build()
    a = s.host_arrays()
    v = np.frombuffer(a["vertices"].tobytes(), dtype=np.float32).reshape(-1, 8)
    f = np.frombuffer(a["faces"].tobytes(), dtype=np.uint32).reshape(-1, 4)
    return v, f


def test_obj_matches_assimp_import(obj_path):
    rt = T.load_rt()
    va, fa = _scene(rt, os.path.join(T.ROOT, "assets", "bunny_mesh.bin"))
    vo, fo = _scene(rt, obj_path)
    assert va.shape == vo.shape and fa.shape == fo.shape
    # AddLoadedScene: the indexed (smooth) copy first, then the flat copies
    assert np.array_equal(fa, fo)
    assert np.array_equal(va[:, 0:3], vo[:, 0:3])  # positions (transformed) bit for bit
    assert np.array_equal(va[:, 6:8], vo[:, 6:8])
    d = np.abs(va[:, 3:6] - vo[:, 3:6])  # smooth normals (unnormalised, x the transform)
    scale = np.abs(va[:, 3:6]).max()
    assert d.max() <= 4e-7 * max(1.0, scale), d.max()
