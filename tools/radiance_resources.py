#!/usr/bin/env python3
"""The compiler's resource usage of every kernel of one HIP unit, as a table: the unit compiled with build.py's own
command plus -Rpass-analysis=kernel-resource-usage into a temporary object (the build's objects are left alone).
Needs no GPU.

    python tools/radiance_resources.py rt_radiance.hip > profiles/radiance_resources.txt
    python tools/radiance_resources.py rt_hits.hip cap > profiles/hits_resources.txt
    python tools/radiance_resources.py rt_closest.hip v > profiles/closest_resources.txt

A further argument labels the kernels' second template integer where it is not a MODE (the walk units' <STACK, V>:
rt_hits.hip's list capacity, rt_closest.hip's unused 0).

(tools/kernel_resources.py reads registers and spills from a built object's metadata; this one also has the
compiler's LDS and occupancy figures and labels the rows by MODE and stack.)
"""
import importlib.util
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = [("VGPRs", "vgpr"), ("VGPRs Spill", "vspill"), ("TotalSGPRs", "sgpr"), ("SGPRs Spill", "sspill"),
          ("ScratchSize [bytes/lane]", "scratch"), ("LDS Size [bytes/block]", "lds"), ("Occupancy [waves/SIMD]", "occ")]


def build_module():
    spec = importlib.util.spec_from_file_location("rt_build", os.path.join(ROOT, "cuda-raytracing_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def remarks(unit):
    """[(mangled kernel name, {field: int})] in the compiler's order."""
    b = build_module()
    _, cmd = b._hip_job(unit)
    with tempfile.TemporaryDirectory() as td:
        cmd = cmd[:cmd.index("-o")] + ["-Rpass-analysis=kernel-resource-usage", "-o", os.path.join(td, "x.o")]
        text = subprocess.run(cmd, check=True, capture_output=True, text=True).stderr
    out, cur = [], None
    for ln in text.split("\n"):
        m = re.search(r"remark:\s+(.*?):\s+(\S+) \[-Rpass-analysis", ln)
        if not m:
            continue
        key, val = m.group(1).strip(), m.group(2)
        if key == "Function Name":
            cur = {}
            out.append((val, cur))
        elif cur is not None and val.isdigit():
            cur[key] = int(val)
    return out


def main():
    unit = sys.argv[1] if len(sys.argv) > 1 else "rt_radiance.hip"
    cols = (sys.argv[2] if len(sys.argv) > 2 else "mode", "stack")
    rows = []
    for name, f in remarks(unit):
        m = re.search(r"([a-z_]+_w\d)ILi(\d+)ELi(\d+)E", name)  # the mangled kernel<STACK, MODE>
        label = (m.group(1), int(m.group(3)), int(m.group(2))) if m else (name, 0, 0)
        rows.append((label, f))
    rows.sort(key=lambda r: (r[0][1], r[0][2], r[0][0]))
    print(f"# {unit}: -Rpass-analysis=kernel-resource-usage with the build's flags (tools/radiance_resources.py); no GPU involved")
    print(f"{'kernel':<24}{cols[0]:>5}{cols[1]:>6}" + "".join(f"{short:>9}" for _, short in FIELDS))
    for (kernel, mode, stack), f in rows:
        print(f"{kernel:<24}{mode:>5}{stack:>6}" + "".join(f"{f.get(key, -1):>9}" for key, _ in FIELDS))


if __name__ == "__main__":
    main()
