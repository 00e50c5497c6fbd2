#!/usr/bin/env python3
"""Which kernel the four ray-batch entry points launch (rt_trace_rays, rt_occluded, rt_ao, rt_radiance): every
occupancy and stack size gives the same bits, so the bit-exact tests cannot see a launch ladder that picks the wrong one.

  rocprofv3 --kernel-trace --output-format csv -d DIR -o run -- python tools/batch_dispatch_check.py run > expected.txt
  python tools/batch_dispatch_check.py compare expected.txt DIR      (no GPU; prints the table, exit 1 on a difference)

`run` calls each entry point with 65 rays (rt_ao: 8 x 9 pixels) at waves_per_simd 5, 6 and 7 on scenes that between
them get stacks 30 / 40 / 64 and MODE 17 / 145 / 21 (tests/scene_cases.py decks, tests/adversarial_cases.py case B), and
prints before each call the kernel it must launch: the stack and mode of rt_variant_host for that scene, the occupancy
asked for."""
import csv
import glob
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
BATCH = re.compile(r"(?:query|occlusion|ao|radiance)_kernel_w\d<\d+, \d+>")


def run():
    import numpy as np
    import torch
    import adversarial_cases as A
    import rt_testlib as T
    import scene_cases as SC
    from test_variant_cpu import choose
    rt = T.load_rt()
    k = torch.arange(65, dtype=torch.float32, device="cuda")
    rays = torch.zeros((65, 8), dtype=torch.float32, device="cuda")
    rays[:, 3], rays[:, 4], rays[:, 5], rays[:, 6] = 1e30, (k % 9 - 4) / 16, (k // 9 - 3) / 16, 1 - 2 * (k % 2)
    rays[:, 4:7] /= rays[:, 4:7].norm(dim=1, keepdim=True)
    for name in ("deck28", "deck38", "deck39", "deck29_plain", "B"):
        with A.build_options(rt, name == "B"):
            s = A.build_case(rt, "B").scene if name == "B" else SC.apply_product(rt, SC.BY_NAME[name])
            s.upload(0)  # queried only: no renderer RNG
            nodes = s.host_arrays()["nodes"].view(np.uint32).reshape(-1, 8)
            has_tree, big_leaves = len(s.mirror(trees=True)[1]) > 0, bool((nodes[:, 7] > 8).any())  # big: the lean arrays exist
            v = choose(rt, has_tree=has_tree, arrays_complete=big_leaves, depth=s.max_depth())
        for w in (5, 6, 7):
            def expect(kernel):
                print("%s  %s_w%d<%d, %d>" % (name, kernel, w, v["stack"], v["mode"]), flush=True)
            expect("query_kernel")
            rt.trace_rays(s, rays, waves_per_simd=w)
            expect("query_kernel")
            hits = rt.trace_camera(s, 8, 9, waves_per_simd=w)
            expect("occlusion_kernel")
            rt.occluded(s, rays, waves_per_simd=w)
            expect("ao_kernel")
            rt.ambient_occlusion(s, hits, 8, 9, radius=4.0, samples=2, waves_per_simd=w)
            expect("radiance_kernel")
            rt.radiance(s, rays, rt.ray_rng(65, 7), bounces=2, waves_per_simd=w)
        torch.cuda.synchronize()


def compare(expected_file, trace_dir):
    want = [ln.split("  ", 1) for ln in open(expected_file).read().splitlines() if BATCH.search(ln)]
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    rows = [r for f in files for r in csv.DictReader(open(f))]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    got = [m.group(0) for m in (BATCH.search(r["Kernel_Name"]) for r in rows) if m]
    bad = len(want) != len(got)
    for i, (scene, kernel) in enumerate(want):
        ran = got[i] if i < len(got) else "(nothing)"
        bad |= ran != kernel
        print("%-13s expected %-32s traced %-32s %s" % (scene, kernel, ran, "same" if ran == kernel else "DIFFERS"))
    print("%d launches expected, %d batch kernels in the trace: %s" % (len(want), len(got), "DIFFERENT" if bad else "all the same"))
    return 1 if bad else 0


if __name__ == "__main__":
    if sys.argv[1:2] == ["run"]:
        run()
    elif sys.argv[1:2] == ["compare"] and len(sys.argv) == 4:
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
