"""bench.py's reading of rocprofv3 output (CPU): the render kernel is found under its namespaced,
templated name, and a probe dispatch of the other occupancy variant does not mix into the
counters of the production frames.  (Round 3 moved the kernels into `namespace rtk`; the old
name filter silently found no rows and the bench line lost its PMC roofline.)"""
import csv
import os

import bench

W6 = "void rtk::render_fast_kernel_w6<30, false, 17>(rtk::RenderArgs)"
W5 = "void rtk::render_fast_kernel_w5<30, false, 17>(rtk::RenderArgs)"
OTHER = "(anonymous namespace)::init_rng_kernel(rt_rng_state*, unsigned int const*)"


def test_short_names():
    assert bench._short(W6) == "render_fast_kernel_w6<30, false, 17>"
    assert bench._short(OTHER) == "init_rng_kernel"


def _write(path, header, rows):
    with open(path, "w", newline="") as fh:
        w = csv.writer(fh, quoting=csv.QUOTE_NONNUMERIC)
        w.writerow(header)
        w.writerows(rows)


def test_read_pmc_pass_picks_the_production_variant(tmp_path):
    d = tmp_path / "pass0"
    os.makedirs(d)
    rows = [[OTHER, "SQ_INSTS_VALU", 1.0], [W5, "SQ_INSTS_VALU", 99.0]]
    rows += [[W6, "SQ_INSTS_VALU", v] for v in (10.0, 12.0, 14.0)]
    _write(d / "pmc_counter_collection.csv", ["Kernel_Name", "Counter_Name", "Counter_Value"], rows)
    trace = [[OTHER, 0, 5], [W5, 0, 7_000_000]] + [[W6, 100, 100 + 16_000_000] for _ in range(3)]
    _write(d / "pmc_kernel_trace.csv", ["Kernel_Name", "Start_Timestamp", "End_Timestamp"], trace)
    vals, kernel, dur = bench.read_pmc_pass(str(d))
    assert kernel == "render_fast_kernel_w6<30, false, 17>"
    assert vals == {"SQ_INSTS_VALU": [10.0, 12.0, 14.0]}
    assert dur == [0.016] * 3


def test_read_pmc_pass_empty(tmp_path):
    assert bench.read_pmc_pass(str(tmp_path)) == ({}, None, [])


def test_dump_outputs_whole_frame_and_seeded_sample(tmp_path, monkeypatch):
    """--dump-outputs (CPU part): a frame within the size limit is written whole, bit for bit, as float32,
    its non-finite components as 0 with their place and kind in frame_nonfinite.npy, so both files are
    finite and together give the frame back; a larger frame as the same sorted, duplicate-free sample of
    its pixels on every call."""
    import numpy as np
    import torch

    img = torch.arange(9 * 7 * 4, dtype=torch.float32).reshape(9, 7, 4)
    img[2, 3, 1] = float("nan")
    img[4, 0, 0], img[4, 0, 3] = float("inf"), float("-inf")
    img[8, 6, :] = float("nan")
    bench.dump_outputs(str(tmp_path / "whole"), img)
    assert sorted(os.listdir(tmp_path / "whole")) == ["frame.npy", "frame_nonfinite.npy"]
    a = np.load(tmp_path / "whole" / "frame.npy")
    codes = np.load(tmp_path / "whole" / "frame_nonfinite.npy")
    assert a.dtype == codes.dtype == np.float32 and a.shape == (9, 7, 4) and codes.shape == (9, 7)
    assert np.isfinite(a).all() and np.isfinite(codes).all()
    assert codes[2, 3] == 1 * 4 and codes[4, 0] == 2 + 3 * 64 and codes[8, 6] == 1 + 4 + 16 + 64
    assert np.count_nonzero(codes) == 3
    # the two arrays give the frame back: the finite components bit for bit, the others by kind
    kind = codes.astype(np.int64)[..., None] // 4 ** np.arange(4) % 4
    back = np.where(kind == 0, a, np.array([0, np.nan, np.inf, -np.inf], dtype=np.float32)[kind])
    assert np.array_equal(back, img.numpy(), equal_nan=True)
    assert np.array_equal(a[kind == 0].view(np.uint32), img.numpy()[kind == 0].view(np.uint32)) and (a[kind != 0] == 0).all()

    assert bench.dump_sample(1920 * 1080) is None  # the headline frame (33 + 8 MB) is written whole
    idx = bench.dump_sample(3840 * 2160)  # config 3's 133 MB frame
    assert idx.size * 20 + 256 <= 64 * 10 ** 6 and idx.size >= 3840 * 2160 // 4
    assert (np.diff(idx) > 0).all() and idx[0] >= 0 and idx[-1] < 3840 * 2160
    assert np.array_equal(idx, bench.dump_sample(3840 * 2160))

    small = bench.dump_sample(63, max_bytes=20 * 20)  # room for 20 of the 63 pixels
    assert small.size == 20
    monkeypatch.setattr(bench, "dump_sample", lambda pixels: small)
    bench.dump_outputs(str(tmp_path / "sample"), img)
    s = np.load(tmp_path / "sample" / "frame.npy")
    sc = np.load(tmp_path / "sample" / "frame_nonfinite.npy")
    assert s.dtype == np.float32 and s.shape == (20, 4) and sc.shape == (20,)
    assert np.array_equal(s, a.reshape(-1, 4)[small]) and np.array_equal(sc, codes.reshape(-1)[small])
