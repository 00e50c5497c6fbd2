"""Static comparison of a lean render kernel with the general one it replaces (profiles/lean_static.txt):
code length, spill counts and scratch from the code-object metadata of the built objects, and, from the
compiler's assembly of the same sources with build.py's flags, what sits inside the `trace` loop (loop
depth >= 2: the segment loop is depth 1): IEEE fp32 division expansions (one v_div_fmas_f32 each) and reloads
of spilled scalars (v_readlane_b32 from a VGPR that holds them: the target of a v_writelane_b32 with a constant
lane whose source is an SGPR).

    python tools/lean_static.py [--pairs w7:30:17,w6:40:17,...]     (waves : stack : general MODE)
Run after build(); prints the table."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cuda-raytracing_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import build  # noqa: E402
from kernel_resources import resources  # noqa: E402

LLVM_BIN = build.LLVM_BIN
LEAN = 128


def kernel_sizes(obj):
    """{kernel symbol: code bytes} of the gfx950 code object inside a HIP object."""
    with tempfile.TemporaryDirectory() as td:
        fat, co = os.path.join(td, "fat.bin"), os.path.join(td, "dev.co")
        subprocess.run([f"{LLVM_BIN}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", obj, os.path.join(td, "x.o")],
                       check=True, capture_output=True)
        subprocess.run([f"{LLVM_BIN}/clang-offload-bundler", "--type=o", f"--targets=hipv4-amdgcn-amd-amdhsa--{build.ARCH}",
                        f"--input={fat}", f"--output={co}", "--unbundle"], check=True, capture_output=True)
        syms = subprocess.run([f"{LLVM_BIN}/llvm-readelf", "-sW", co], check=True, capture_output=True, text=True).stdout
    out = {}
    for ln in syms.split("\n"):
        f = ln.split()
        if len(f) >= 8 and f[3] == "FUNC":
            out[f[7]] = int(f[2], 0) if f[2].startswith("0x") else int(f[2])
    return out


def object_figures(obj):
    """{kernel symbol: dict(code, sgpr_spill, vgpr_spill, scratch, vgpr)} from the built object."""
    size = kernel_sizes(obj)
    return {name: dict(code=size.get(name, 0), vgpr=v, vgpr_spill=vs, sgpr_spill=ss, scratch=priv)
            for name, v, vs, ss, priv in resources(obj)}


def assembly(src):
    """The device assembly of csrc/<src> with build.py's flags (loop-depth annotations included)."""
    asm = os.path.join(tempfile.gettempdir(), f"lean_static_{src}.s")
    obj, cmd = build._hip_job(src)
    cmd = [c for c in cmd if c != "-fPIC"]
    i = cmd.index("-c")
    cmd = cmd[:i] + ["--cuda-device-only", "-S"] + cmd[i:]
    cmd[cmd.index("-o") + 1] = asm
    subprocess.run(cmd, check=True, capture_output=True)
    return open(asm).read()


def loop_figures(txt, sym):
    """In-loop (depth >= 2) division expansions and spilled-scalar reloads of kernel `sym`."""
    start = txt.index("\n" + sym + ":")
    body = txt[start:txt.index(".end_amdhsa_kernel", start)]
    spill_regs = set(re.findall(r"^\s+v_writelane_b32 (v\d+), s\d+, \d+", body, re.M))
    depth, divs, reloads, all_reloads, all_divs = 0, 0, 0, 0, 0
    for ln in body.split("\n"):
        if re.match(r"^(\.LBB\S+|; %bb\.\d+):", ln):
            m = re.search(r"Depth=(\d+)", ln)
            depth = int(m.group(1)) if m else 0
            continue
        if ln.strip().startswith(";") and "Loop Header: Depth=" in ln:
            depth = int(re.search(r"Depth=(\d+)", ln).group(1))
            continue
        m = re.match(r"\s+(\S+)\s+(.*)", ln)
        if not m:
            continue
        op, rest = m.group(1), m.group(2)
        if op == "v_div_fmas_f32":
            all_divs += 1
            divs += depth >= 2
        elif op == "v_readlane_b32":
            r = re.match(r"s\d+, (v\d+), \d+", rest)
            if r and r.group(1) in spill_regs:
                all_reloads += 1
                reloads += depth >= 2
    return dict(loop_divs=divs, loop_reloads=reloads, divs=all_divs, reloads=all_reloads, spill_vgprs=sorted(spill_regs))


def symbol(waves, stack, mode):
    return f"_ZN3rtk21render_fast_kernel_w{waves}ILi{stack}ELb0ELi{mode}EEEvNS_10RenderArgsE"


def main():
    pairs = "w7:30:17,w6:30:17,w5:30:17"
    if "--pairs" in sys.argv:
        pairs = sys.argv[sys.argv.index("--pairs") + 1]
    objs = {s: object_figures(os.path.join(build.BUILD, s + ".o")) for s in ("rt_fast_prod.hip", "rt_fast_lean.hip")}
    asms = {s: assembly(s) for s in objs}
    cols = ("code", "sgpr_spill", "vgpr_spill", "scratch", "loop_divs", "loop_reloads", "divs", "reloads")
    print(f"{'kernel':28s}" + "".join(f"{c:>13s}" for c in cols) + "  spill VGPRs")
    for p in pairs.split(","):
        w, stack, mode = p.split(":")
        for src, md in (("rt_fast_prod.hip", int(mode)), ("rt_fast_lean.hip", int(mode) | LEAN)):
            sym = symbol(w[1:], stack, md)
            fig = dict(objs[src][sym])
            fig.update(loop_figures(asms[src], sym))
            print(f"{w + '<' + stack + ',false,' + str(md) + '>':28s}" + "".join(f"{fig[c]:13d}" for c in cols) + "  " +
                  ",".join(fig["spill_vgprs"]))


if __name__ == "__main__":
    main()
