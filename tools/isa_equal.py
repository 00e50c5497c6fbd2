#!/usr/bin/env python3
"""Whether two builds hold the same device code: tools/isa_equal.py OLD_BUILD_DIR NEW_BUILD_DIR compares the gfx950
disassembly (build.disassemble) of every *.hip.o of build.py's HIP_SOURCES and EXP_SOURCES line for line, but for the
`file format` line, which names a temporary file.  One line per object: name, kernel count, `same` or the first
differing kernel; then the kernels that moved to another unit, compared by symbol; exit status 1 on any difference.  For refactors that claim to leave the kernels alone: no GPU involved."""
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


def by_symbol(old_objs, new_objs):
    """For a refactor that moves kernels between units: every kernel of the old objects that its own unit no longer
    holds, looked up by symbol in the new ones and compared on instruction text (addresses dropped) and on registers,
    LDS, spills and scratch.  Prints one line per moved kernel; returns how many are missing or differ."""
    import kernel_resources as K
    def body(ins):  # what follows a kernel's last s_endpgm is padding up to the next symbol, which depends on the neighbour
        return ins[:len(ins) - ins[::-1].index("s_endpgm")] if "s_endpgm" in ins else ins

    def code(objs):  # {object with device code: ({symbol: instructions}, {kernel: resources})}
        ins = {o: {s: body(i) for s, i in K.instructions(o).items()} for o in objs}
        return {os.path.basename(o): (i, {r[0]: r[1:] for r in K.resources(o, K.FIELDS)}) for o, i in ins.items() if i}
    old, new = code(old_objs), code(new_objs)
    bad = 0
    for o, (ins, res) in old.items():
        stayed = new.get(o, ({}, {}))[0]
        for sym in [s for s in res if s not in stayed]:
            homes = [n for n in new if sym in new[n][1]]
            same = len(homes) == 1 and new[homes[0]][0][sym] == ins[sym] and new[homes[0]][1][sym] == res[sym]
            print("  %-62s %s -> %s  %s" % (sym[:62], o, homes[0] if homes else "NOWHERE",
                                            "same instructions and resources %s" % (res[sym],) if same else "DIFFERS"))
            bad += not same
    return bad


def main(old_dir, new_dir):
    B = build_module()
    bad = 0
    for src in B.HIP_SOURCES + B.EXP_SOURCES:
        objs = [os.path.join(d, src + ".o") for d in (old_dir, new_dir)]
        if not os.path.exists(objs[0]) and os.path.exists(objs[1]):
            print("%-24s new unit" % (src + ".o"))
            continue
        missing = [o for o in objs if not os.path.exists(o)]
        if missing:
            print("%-24s MISSING %s" % (src + ".o", missing[0]))
            bad += 1
            continue
        old, new = B.disassemble(objs[0]), B.disassemble(objs[1])
        n, diff = compare(old, new)
        if diff and not B.parse_disassembly(new)[1]:
            print("%-24s %4d kernels  every kernel left the unit (by symbol below)" % (src + ".o", n))
            continue
        print("%-24s %4d kernels  %s" % (src + ".o", n, diff or "same"))
        bad += diff is not None
    objs = lambda d: [os.path.join(d, f) for f in sorted(os.listdir(d)) if f.endswith(".hip.o")]
    print("kernels that changed units:")
    bad += by_symbol(objs(old_dir), objs(new_dir))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
