"""Sky input: the product's C++ DDS reader (csrc/scene.cpp load_cube, which
restates utils/image/DDSLoader.cpp:135-371 and the face slicing of utils/CUDATexture.cpp:187-220)
loads the reference's own data/sunset_uncompressed.dds through rt_scene_set_environment_file, and
its level-0 texels equal assets/sunset_cube128.bin byte for byte (the asset the tests, smoke()
and the benchmark render with; made by tools/make_assets.py).

The DDS file (2 MB: header, then per face level 0 and mips 1-7) is put together in the test's
temporary directory from tests/golden/sunset_dds_mips.npz (its header and every face's mips 1-7,
tools/make_assets.py fixtures) and the level-0 texels the asset holds, so the reader's header
parsing, mip skipping and face order are tested wherever the suite runs; the rebuilt file must
have the SHA-256 of the reference's.  CPU.
"""
import hashlib
import os

import numpy as np
import pytest

import rt_testlib as T

DDS_SHA256 = "6826b5e7b53c17682adf8538804dc7967f629c5e2ee31c602e9e9e780c29ae9e"  # data/sunset_uncompressed.dds
MIPS = os.path.join(T.GOLDEN, "sunset_dds_mips.npz")
ASSET = os.path.join(T.ASSETS, "sunset_cube128.bin")


def _env(rt, path):
    s = rt.Scene()
    s.set_environment(path)
    return s.environment()


@pytest.fixture
def dds_path(tmp_path):
    z = np.load(MIPS)  # data only: no pickle
    level0 = np.fromfile(ASSET, dtype=np.uint8, offset=12).reshape(6, -1)
    path = tmp_path / "sunset_uncompressed.dds"
    path.write_bytes(z["header"].tobytes() + np.concatenate([level0, z["mips"]], axis=1).tobytes())
    return str(path)


def test_dds_reader_matches_asset(dds_path):
    rt = T.load_rt()
    assert os.path.getsize(dds_path) == 128 + 6 * 16 * sum((128 >> m) ** 2 for m in range(8))
    assert hashlib.sha256(open(dds_path, "rb").read()).hexdigest() == DDS_SHA256
    dds = _env(rt, dds_path)
    asset = _env(rt, ASSET)
    assert dds.shape == asset.shape == (6, 128, 128, 4)
    assert np.array_equal(dds.view(np.uint32), asset.view(np.uint32))
    # faces differ from each other (+X,-X,+Y,-Y,+Z,-Z order kept, not six copies of one face)
    assert len({dds[f].tobytes() for f in range(6)}) == 6
    # the mips behind each face are other data than its level 0 (a reader that did not skip them would
    # take face 1 from face 0's mips): mip 1 is not the first quarter of level 0
    z = np.load(MIPS)
    assert not np.array_equal(z["mips"][0, : 16 * 64 * 64], np.fromfile(ASSET, dtype=np.uint8, offset=12)[: 16 * 64 * 64])


def test_environment_file_errors():
    rt = T.load_rt()
    s = rt.Scene()
    assert s.environment() is None
    with pytest.raises(rt.RTError):
        s.set_environment(os.path.join(T.ASSETS, "does_not_exist.dds"))
    with pytest.raises(rt.RTError):
        s.set_environment(os.path.join(T.ASSETS, "bunny_mesh.bin"))  # not a cube map
