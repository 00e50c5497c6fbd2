"""The one chooser of the render kernel variant (csrc/rt_variant.h choose_variant, through rt_variant_host)
against the decisions of the code it replaced.

tests/golden/variant_table.npz is the table of parent commit a7b51e5 ("Entry frontier for camera rays: exact,
measured, shipped switched off"): its needs_experimental, lean_mode, launch_prod, launch_fast (with
launch_fast_ab's forwarding to its second unit), the entry-frontier condition of rt_render and the stack rule,
copied verbatim into a host program with the launchers stubbed to record (family, mode), run over the full
cross product of RT_TUNE bits 0 (one the kernel reads), 4, 5, 7, 8, 12 x stats, lane_cost, refill, has_tree,
screens, arrays_complete, want_entry x depth in {-1, 0, 14, 15, 24, 25, 28, 29, 38, 39, 48, 49, 75} (either side of
every boundary of depth + 2 (+ 14) <= 30 / 40 / 64), without lane_cost + refill, which rt_render refuses:
79,872 rows.  Families are numbered as rt_variant.h's enum.
"""
import os

import numpy as np
import pytest

import rt_testlib as T

INPUTS = ["tune", "stats", "lane_cost", "refill", "has_tree", "screens", "arrays_complete", "depth", "want_entry"]
OUTPUTS = ["family", "mode", "stack", "needs_plugin", "use_entry"]
FAMILIES = ["prod", "lean", "timing", "stats", "ab", "ab2", "refill", "screen"]  # rt_variant.h Family
PLUGIN = {FAMILIES.index(f) for f in ("ab", "ab2", "refill", "screen")}


def golden():
    g = np.load(os.path.join(T.ROOT, "tests", "golden", "variant_table.npz"))
    return {k: g[k].astype(np.int32) for k in INPUTS + OUTPUTS}


def choose(rt, **inputs):
    """rt_variant_host for one frame: {output name: value}."""
    i = np.array([int(inputs.get(k, 0)) for k in INPUTS], dtype=np.int32)
    o = np.zeros(len(OUTPUTS), dtype=np.int32)
    rt.lib().rt_variant_host(i.ctypes.data, o.ctypes.data)
    return dict(zip(OUTPUTS, o.tolist()))


@pytest.fixture(scope="module")
def table():
    """The golden table and the chooser's outputs for every row of it."""
    rt = T.load_rt()
    g = golden()
    n = len(g["tune"])
    assert n == 79872, "the full cross product, no row dropped"
    ins = np.ascontiguousarray(np.stack([g[k] for k in INPUTS], axis=1))
    outs = np.zeros((n, len(OUTPUTS)), dtype=np.int32)
    fn = rt.lib().rt_variant_host
    a, b, sa, sb = ins.ctypes.data, outs.ctypes.data, ins.strides[0], outs.strides[0]
    for r in range(n):
        fn(a + r * sa, b + r * sb)
    return rt, g, ins, outs


def test_chooser_reproduces_the_parent(table):
    _, g, ins, outs = table
    want = np.stack([g[k] for k in OUTPUTS], axis=1)
    bad = np.flatnonzero((outs != want).any(axis=1))
    first = [(dict(zip(INPUTS, ins[r].tolist())), want[r].tolist(), outs[r].tolist()) for r in bad[:5]]
    assert bad.size == 0, f"{bad.size} of {len(want)} rows differ (inputs, parent, chooser): {first}"


def test_plugin_families_need_the_plugin(table):
    _, g, _, outs = table
    for src in (outs[:, [0, 3]], np.stack([g["family"], g["needs_plugin"]], axis=1)):
        in_plugin = np.isin(src[:, 0], sorted(PLUGIN))
        assert in_plugin.any() and (src[in_plugin, 1] == 1).all()
    # kept as found: a refill request is refused without the plugin even where a statistics / timing kernel of the
    # product would render the frame and ignore it
    over = (g["needs_plugin"] == 1) & ~np.isin(g["family"], sorted(PLUGIN))
    assert over.any() and (g["refill"][over] == 1).all()


def test_every_chosen_mode_is_instantiated(table):
    """Every (family, mode) of the table is in the mode list its family's unit is built from (rt_render.h), and
    every list entry is chosen by some row: no variant is compiled that no frame can reach."""
    rt, g, _, _ = table
    has = rt.lib().rt_family_has_mode_host
    chosen = sorted(set(zip(g["family"].tolist(), g["mode"].tolist())))
    assert len(chosen) == 19
    for fam, mode in chosen:
        assert has(fam, mode) == 1, f"{FAMILIES[fam]} does not instantiate MODE {mode}"
    listed = sorted((f, m) for f in range(len(FAMILIES)) for m in range(256) if has(f, m))
    assert listed == chosen
    assert has(len(FAMILIES), 17) == 0 and has(-1, 17) == 0


def test_query_variant(table):
    """rt_trace_rays calls the chooser with tune 0: MODE 17 | 128 with every array, 17 without, 21 with leaf trees."""
    rt = table[0]
    assert choose(rt, arrays_complete=1, depth=20)["mode"] == 17 | 128
    assert choose(rt, arrays_complete=0, depth=20)["mode"] == 17
    v = choose(rt, arrays_complete=1, has_tree=1, depth=29)
    assert (v["mode"], v["stack"], v["needs_plugin"], v["use_entry"]) == (21, 40, 0, 0)
