"""The lean production kernels against the general ones they replace, from the code-object metadata of the
built objects (tools/lean_static.py; no GPU): the lean variant exists to drop code and to stop carrying scalars
across the traversal, so at every occupancy and stack size its code is shorter and it spills fewer scalar
registers, no more vector registers, and uses no more scratch -- above all the kernel the benchmark runs,
render_fast_kernel_w7<30, false, 17 | 128> against <30, false, 17>.  (The counts inside the trace loop need
the compiler's assembly, a minute per unit: profiles/lean_static.txt records them.)
"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import lean_static  # noqa: E402

LEAN = lean_static.LEAN


@pytest.fixture(scope="module")
def figures():
    build = lean_static.build
    return {s: lean_static.object_figures(os.path.join(build.BUILD, s + ".o")) for s in ("rt_fast_prod.hip", "rt_fast_lean.hip")}


def pair(figures, waves, stack, mode):
    g = figures["rt_fast_prod.hip"][lean_static.symbol(waves, stack, mode)]
    l = figures["rt_fast_lean.hip"][lean_static.symbol(waves, stack, mode | LEAN)]
    return g, l


@pytest.mark.parametrize("stack", [30, 40, 64])
@pytest.mark.parametrize("waves", [5, 6, 7])
def test_lean_below_general(figures, waves, stack):
    g, l = pair(figures, waves, stack, 17)
    print(f"w{waves}<{stack},17> general {g}  lean {l}")
    assert 0 < l["code"] < g["code"]
    assert l["sgpr_spill"] < g["sgpr_spill"]
    assert l["vgpr_spill"] <= g["vgpr_spill"]
    assert l["scratch"] <= g["scratch"]


def test_benchmark_kernel(figures):
    g, l = pair(figures, 7, 30, 17)
    print(f"general {g}  lean {l}")
    assert 0 < l["code"] < g["code"]
    assert l["sgpr_spill"] < g["sgpr_spill"]
    assert l["vgpr_spill"] <= g["vgpr_spill"]
    assert l["scratch"] <= g["scratch"]
    assert l["vgpr"] <= 72  # 7 waves per SIMD: 512 / 7 registers, in units of 8
