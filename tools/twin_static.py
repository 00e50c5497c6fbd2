"""Static price of the twin decision in the big-leaf loops of a lean render kernel (profiles/twin_hoist_static.txt):
the shared-leaf quad loop and the cooperative unit-chunk loop are found as the loops that hold instructions the
compiler attributes (.loc of a -gline-tables-only build, same machine code) to quad_test / unit_test, and their
instructions are counted by kind (tools/salu_map.py classify), those attributed to the twin decision -- the
twin_* functions and the |o - v0|_1 sums -- apart.  "every iteration" leaves out the basic blocks of the rare path
(a hit, or a twin tested itself): those that hold an instruction of offer / tri_offer / pair_t or of a division.

    python tools/twin_static.py [kernel-substring] [--src rt_fast_lean.hip]
"""
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cuda-raytracing_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import build  # noqa: E402
import salu_map  # noqa: E402


TWIN_FNS = ("twin_rejected_pre", "twin_rejected", "twin_fold", "twin_limits", "twin_decide", "add_each", "twin_visit",
            "twin_visit_dn", "twin_visit_from", "ld_twin_leaf")


def function_lines(path):
    """{function name: (first line, last line)} of the top-level functions of rt_fast.h named below."""
    names = TWIN_FNS + ("quad_test", "unit_test", "pair_eval", "coop_units", "tri_ok", "tri_ok_folded", "offer",
                        "tri_offer", "pair_t")
    src = open(path).read().split("\n")
    out = {}
    for i, ln in enumerate(src):
        m = re.search(r"\b(" + "|".join(names) + r")\(", ln)
        if m and m.group(1) not in out and not ln.startswith((" ", "\t", "//")) and not ln.rstrip().endswith(";"):
            j = i
            while not src[j].startswith("}"):
                j += 1
            out[m.group(1)] = (i + 1, j + 1)
    return out


def compile_asm(src):
    asm = os.path.join(tempfile.gettempdir(), f"twin_static_{src}.s")
    obj, cmd = build._hip_job(src)
    cmd = [c for c in cmd if c != "-fPIC"]
    i = cmd.index("-c")
    cmd = cmd[:i] + ["--cuda-device-only", "-S", "-gline-tables-only"] + cmd[i:]
    cmd[cmd.index("-o") + 1] = asm
    subprocess.run(cmd, check=True, capture_output=True)
    return asm


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    src = "rt_fast_lean.hip"
    if "--src" in sys.argv:
        src = sys.argv[sys.argv.index("--src") + 1]
        args.remove(src)
    want = args[0] if args else "render_fast_kernel_w7ILi30ELb0ELi145E"
    fl = function_lines(os.path.join(build.CSRC, "rt_fast.h"))
    txt = open(compile_asm(src)).read()
    sym, ins = salu_map.scan(txt, want)
    # the basic block of every instruction, in scan's order
    body = txt[txt.index("\n" + sym + ":"):]
    body = body[:body.find(".end_amdhsa_kernel")]
    blocks, blk = [], 0
    for ln in body.split("\n"):
        if re.match(r"^(\.LBB\S+|; %bb\.\d+):", ln):
            blk += 1
        elif re.match(r"^\s+([sv]_\S+.*?|global_\S+.*?|buffer_\S+.*?|scratch_\S+.*?|flat_\S+.*?|ds_\S+.*?)\s*(?:;.*)?$", ln) \
                and not ln.strip().startswith("s_code_end"):
            blocks.append(blk)
    assert len(blocks) == len(ins)

    def owner(loc):
        f, _, n = loc.partition(":")
        if f != "rt_fast.h" or not n.isdigit():
            return None
        hits = [k for k, (a, b) in fl.items() if a <= int(n) <= b]
        return min(hits, key=lambda k: fl[k][1] - fl[k][0]) if hits else None

    dn_line = None  # pair_eval's |o - v0|_1 line, part of the twin decision
    for i, ln in enumerate(open(os.path.join(build.CSRC, "rt_fast.h")).read().split("\n")):
        if "E.dn =" in ln:
            dn_line = i + 1
    twin_fns = TWIN_FNS
    print(f"{sym}: {len(ins)} instructions")
    for title, fn in (("shared-leaf quad loop", "quad_test"), ("cooperative unit-chunk loop", "unit_test")):
        headers = collections.Counter(h for k, loc, d, h, _ in ins if d >= 2 and owner(loc) == fn)
        if not headers:
            print(f"{title}: no loop holds {fn}")
            continue
        hdr = headers.most_common(1)[0][0]
        tot, twin, by_fn = collections.Counter(), collections.Counter(), collections.defaultdict(collections.Counter)
        rare = {b for (kind, loc, d, h, text), b in zip(ins, blocks)
                if h == hdr and (owner(loc) in ("offer", "tri_offer", "pair_t") or text.startswith(("v_div_", "v_rcp_")))}
        every, every_twin = collections.Counter(), collections.Counter()
        for (kind, loc, d, h, text), b in zip(ins, blocks):
            if h != hdr:
                continue
            tot[kind] += 1
            o = owner(loc)
            by_fn[o or "other"][kind] += 1
            is_twin = o in twin_fns or (dn_line is not None and loc == f"rt_fast.h:{dn_line}")
            twin[kind] += is_twin
            if b not in rare:
                every[kind] += 1
                every_twin[kind] += is_twin
        kinds = [k for k in salu_map.KINDS if tot[k]]
        print(f"{title} (loop {hdr}):")
        print("  all            " + " ".join(f"{k}={tot[k]}" for k in kinds))
        print("  twin decision  " + " ".join(f"{k}={twin[k]}" for k in kinds if twin[k]))
        if fn == "quad_test":  # (unit_test offers a hit before its twin test: its blocks do not separate)
            print("  every iteration            " + " ".join(f"{k}={every[k]}" for k in kinds if every[k]))
            print("  every iteration, twin part " + " ".join(f"{k}={every_twin[k]}" for k in kinds if every_twin[k]))
        for f, cnt in sorted(by_fn.items(), key=lambda kv: -sum(kv[1].values())):
            print(f"    {f:<18s}" + " ".join(f"{k}={cnt[k]}" for k in kinds if cnt[k]))


if __name__ == "__main__":
    main()
