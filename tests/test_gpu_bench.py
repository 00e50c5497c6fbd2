"""The benchmark line proves itself: a bench.py --full run re-renders the frames it timed unsharded,
in plain tile order, and compares the final surface bit for bit (`check_equal`), so the exact launch
shape behind the headline number -- cost-ordered tiles, the measured lane map, the occupancy the probe
picks -- is checked at full size on every run (RayTracing/RayTracing.cpp:231-233: each frame lerps
into the last one, so the final surface carries every frame's pixels).  At N > 1 the compared frame is
the gathered one, and the line carries the per-frame gather time (tests/test_gpu_multi.py
test_bench_two_ranks_without_launcher).
"""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(args, timeout=240):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True,
                       timeout=timeout, cwd=ROOT)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert lines, f"exit {r.returncode}: {r.stderr[-3000:]}"
    return r.returncode, json.loads(lines[-1])


@pytest.mark.gpu
def test_bench_cfg2_line_is_bit_exact():
    """The headline workload (config 2) with the bench's own defaults: the line says check_equal."""
    rc, line = _bench(["--config", "cfg2", "--steps", "2", "--warmup", "1", "--full", "--no-pmc", "--no-cpu-baseline"])
    assert rc == 0, line
    assert line["check_equal"] is True
    assert line["check"]["frames"] == 3
    assert line["plan"]["kind"].startswith("cost")
    # frame 0 of the exact timed launch shape against the oracle's own full frame (row hashes + RNG states)
    assert line["check_oracle_fixture"]["equal"] is True, line["check_oracle_fixture"]


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_last_frame(tmp_path):
    """A plain run (no --full) prints the headline fields and none of the extra legs, and --dump-outputs
    writes the frame of its last timed step: config 1 (256x256, 1 spp), 1 warm-up + 2 timed frames, equals
    the same three progressive frames rendered here in plain tile order, bit for bit."""
    import numpy as np
    import torch

    import rt_testlib as T

    out = tmp_path / "outputs"
    rc, line = _bench(["--gpus", "1", "--config", "cfg1", "--steps", "2", "--warmup", "1", "--dump-outputs", str(out)])
    assert rc == 0, line
    assert line["unit"] == "Mrays/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["steps"] == 2 and line["value"] > 0 and line["ms_per_step"] > 0
    # value = segments / elapsed and ms_per_step = elapsed / steps describe the same timed interval (the line
    # rounds ms_per_step to 3 decimals, value to 2 and segments_per_step to 1)
    rounding = 0.0005 / line["ms_per_step"] + 0.005 / line["value"] + 0.05 / line["config"]["segments_per_step"]
    assert line["value"] == pytest.approx(line["config"]["segments_per_step"] / line["ms_per_step"] / 1e3, rel=1.01 * rounding)
    for leg in ("roofline", "cpu_baseline", "check_equal", "check", "check_oracle_fixture"):
        assert leg not in line, leg
    assert sorted(os.listdir(out)) == ["frame.npy", "frame_nonfinite.npy"]
    got, got_codes = np.load(out / "frame.npy"), np.load(out / "frame_nonfinite.npy")
    assert got.dtype == got_codes.dtype == np.float32 and got.shape == (256, 256, 4) and got_codes.shape == (256, 256)
    assert np.isfinite(got).all() and np.isfinite(got_codes).all()

    rt = T.load_rt()
    w, h, spp, bounces = 256, 256, 1, 1
    s = rt.Scene()
    s.setup("bunny")
    s.set_viewport(w, h)
    rng = rt.alloc_rng(w * h)
    rt.init_rng_states(rng, w, h, T.SEED)
    s.upload(rng.data_ptr())
    bufs = [rt.alloc_surface(w, h), rt.alloc_surface(w, h)]
    for i in range(3):
        rt.render(s, bufs[i & 1], bufs[(i + 1) & 1], w, h, spp, bounces, i)
    torch.cuda.synchronize()
    import bench

    want, want_codes = bench.split_nonfinite(rt.surface_view(bufs[0], w).cpu().numpy())
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and np.array_equal(got_codes, want_codes)
    assert line["image_finite"] == (not got_codes.any())

