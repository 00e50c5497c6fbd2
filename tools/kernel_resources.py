"""Registers / LDS / spills / scratch and instruction counts of the kernels in a HIP object (code-object metadata and
build.disassemble), or of two builds of one object side by side:
    python tools/kernel_resources.py cuda-raytracing_amd/build/rt_fast_prod.hip.o [filter]
    python tools/kernel_resources.py OLD/denoise.hip.o NEW/denoise.hip.o --compare"""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_equal import build_module  # noqa: E402

LLVM_BIN = "/opt/rocm/lib/llvm/bin"
FIELDS = ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")


def resources(obj, fields=("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")):
    """[(kernel, the metadata `fields`...)] in the object's order; FIELDS adds SGPRs and LDS bytes."""
    with tempfile.TemporaryDirectory() as td:
        fat, co = os.path.join(td, "fat.bin"), os.path.join(td, "dev.co")
        subprocess.run([f"{LLVM_BIN}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", obj, os.path.join(td, "x.o")],
                       check=True, capture_output=True)
        subprocess.run([f"{LLVM_BIN}/clang-offload-bundler", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                        f"--input={fat}", f"--output={co}", "--unbundle"], check=True, capture_output=True)
        notes = subprocess.run([f"{LLVM_BIN}/llvm-readelf", "--notes", co], check=True, capture_output=True, text=True).stdout
    out = []
    for blk in re.split(r"\n\s+- \.agpr_count", notes)[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        out.append((name,) + tuple(int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1)) for k in fields))
    return out


def instructions(obj):
    """{symbol: [instruction text]} of the object's device code, encodings and addresses dropped."""
    B = build_module()
    per = {}
    for _, text, _, kernel in B.parse_disassembly(B.disassemble(obj))[1]:
        per.setdefault(kernel, []).append(text)
    return per


def line(name, r, count):
    v, s, lds, vs, ss, priv = r
    return f"{name[:64]:64s} vgpr {v:3d} sgpr {s:3d} lds {lds:6d} B vgpr_spill {vs:4d} sgpr_spill {ss:4d} scratch {priv:4d} B  {count:5d} instructions"


def compare(old, new):
    ro, rn = ({r[0]: r[1:] for r in resources(o, FIELDS)} for o in (old, new))
    io, inew = instructions(old), instructions(new)
    print("symbols: " + ("the same set" if sorted(io) == sorted(inew) else f"DIFFER: {sorted(set(io) ^ set(inew))}"))
    for name in rn:
        same = io.get(name) == inew[name]
        print(line(name, rn[name], len(inew[name])) + ("  same code" if same else ""))
        if not same and name in ro:
            print(line("  was", ro[name], len(io[name])) + f"  ({100.0 * (len(inew[name]) - len(io[name])) / len(io[name]):+.2f} % instructions)")


if __name__ == "__main__":
    if "--compare" in sys.argv:
        compare(sys.argv[1], sys.argv[2])
    else:
        flt = sys.argv[2] if len(sys.argv) > 2 else ""
        counts = instructions(sys.argv[1])
        for r in resources(sys.argv[1], FIELDS):
            if flt in r[0]:
                print(line(r[0], r[1:], len(counts.get(r[0], []))))
