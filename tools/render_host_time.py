#!/usr/bin/env python3
"""Host time of rt_render itself: the wall time of the call while the stream is already busy, so nothing it enqueues
can start and the clock sees only the host side (argument checks, mirror lookup, variant choice, the launch).
    python tools/render_host_time.py [--rounds 40] [--calls 16]
Each round enqueues one heavy frame (1280 x 720, 4 spp), then times `calls` consecutive rt_render calls of a 64 x 36
frame on the same stream through ctypes with parameters filled beforehand, then synchronises.  Prints the median and
the 10th / 90th percentile over all timed calls in microseconds, and one JSON line.  For refactors of the launch path:
run it for both builds alternately in one session (profiles/render_split_timing.txt)."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rt_testlib as T  # noqa: E402


def params(rt, surface, last, w, h, spp):
    p = rt.RenderParams()
    p.surface, p.surface_last_frame, p.width, p.height, p.pitch = surface.data_ptr(), last.data_ptr(), w, h, surface.shape[1] * 4
    p.spp, p.bounces, p.shard_count = spp, 6, 1
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--calls", type=int, default=16)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    rt = T.load_rt()
    W, H, w, h = 1280, 720, 64, 36
    s = rt.Scene()
    s.setup("bunny")
    s.set_viewport(W, H)
    rng = rt.alloc_rng(W * H)
    rt.init_rng_states(rng, W, H, T.SEED)
    s.upload(rng.data_ptr())
    big = params(rt, rt.alloc_surface(W, H), rt.alloc_surface(W, H), W, H, 4)
    small = params(rt, rt.alloc_surface(w, h), rt.alloc_surface(w, h), w, h, 1)
    render, scene = rt.lib().rt_render, ctypes.cast(s.gpu, ctypes.c_void_p)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    bp, sp = ctypes.byref(big), ctypes.byref(small)
    times = []
    for r in range(a.rounds + 2):
        assert render(bp, scene, stream) == 0, rt.lib().rt_last_error()
        for _ in range(a.calls):
            t0 = time.perf_counter_ns()
            code = render(sp, scene, stream)
            t1 = time.perf_counter_ns()
            assert code == 0, rt.lib().rt_last_error()
            if r >= 2:  # two rounds of warm-up
                times.append((t1 - t0) / 1000.0)
        torch.cuda.synchronize()
    t = np.array(times)
    res = {"metric": "rt_render_host_us", "median": round(float(np.median(t)), 2), "p10": round(float(np.percentile(t, 10)), 2),
           "p90": round(float(np.percentile(t, 90)), 2), "calls": int(t.size)}
    print("rt_render host time, busy stream: median %.2f us  p10 %.2f  p90 %.2f  (%d calls)" % (res["median"], res["p10"], res["p90"], t.size))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
