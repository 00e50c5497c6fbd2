#!/usr/bin/env python3
"""Whether two builds hold the same device code: tools/isa_equal.py OLD_BUILD_DIR NEW_BUILD_DIR compares the gfx950
disassembly (build.disassemble) of every *.hip.o of build.py's HIP_SOURCES and EXP_SOURCES line for line, but for the
`file format` line, which names a temporary file.  One line per object: name, kernel count, `same` or the first
differing kernel; exit status 1 on any difference.  For refactors that claim to leave the kernels alone: no GPU involved."""
import importlib.util
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_module():
    spec = importlib.util.spec_from_file_location("rt_build", os.path.join(ROOT, "cuda-raytracing_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def compare(old, new):
    """(kernel count of `new`, None or a description of the first difference) of two disassemblies."""
    a, b = ([ln for ln in d.split("\n") if "file format" not in ln] for d in (old, new))  # that line names the temporary
    symbols = [ln for ln in b if re.match(r"^[0-9a-f]+ <\S+>:$", ln)]
    kernel = "(before the first symbol)"
    for i in range(max(len(a), len(b))):
        la, lb = (a[i] if i < len(a) else "<end>"), (b[i] if i < len(b) else "<end>")
        if la != lb:
            return len(symbols), "DIFFERS at line %d in %s: %r -> %r" % (i + 2, kernel, la.strip(), lb.strip())
        m = re.match(r"^[0-9a-f]+ <(\S+)>:$", lb)
        if m:
            kernel = m.group(1)
    return len(symbols), None


def main(old_dir, new_dir):
    B = build_module()
    bad = 0
    for src in B.HIP_SOURCES + B.EXP_SOURCES:
        objs = [os.path.join(d, src + ".o") for d in (old_dir, new_dir)]
        missing = [o for o in objs if not os.path.exists(o)]
        if missing:
            print("%-24s MISSING %s" % (src + ".o", missing[0]))
            bad += 1
            continue
        n, diff = compare(B.disassemble(objs[0]), B.disassemble(objs[1]))
        print("%-24s %4d kernels  %s" % (src + ".o", n, diff or "same"))
        bad += diff is not None
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
