"""Every ctypes structure of the binding against include/rt_abi.h, twice: against what a C++ compiler makes of the
header (sizeof and offsetof of every struct and field), and against the header's text (field names in order, the
sizes and offsets its static_asserts pin).  No GPU and no HIP: g++ on the header alone."""
import ctypes
import os
import subprocess

import pytest

import rt_testlib as T

HEADER = os.path.join(T.ROOT, "include", "rt_abi.h")
rt = T.load_rt()

# C name -> (ctypes class, sizeof in bytes)
STRUCTS = {
    "GPUCamera": (rt.GPUCamera, 60), "GPUMaterial": (rt.GPUMaterial, 64), "GPUScene": (rt.GPUScene, 136),
    "rt_build_options": (rt.BuildOptions, 32), "rt_render_params": (rt.RenderParams, 168),
    "rt_ray": (rt.Ray, 32), "rt_hit": (rt.Hit, 48), "rt_trace_params": (rt.TraceParams, 40),
    "rt_occlusion_params": (rt.OcclusionParams, 32), "rt_ao_params": (rt.AoParams, 72),
    "rt_radiance_params": (rt.RadianceParams, 48),
    "rt_point": (rt.Point, 16), "rt_nearest": (rt.Nearest, 32), "rt_closest_params": (rt.ClosestParams, 32),
    "rt_hits_params": (rt.HitsParams, 56),
    "rt_denoise_params": (rt.DenoiseParams, 96), "rt_reproject_params": (rt.ReprojectParams, 224),
    "rt_moments_params": (rt.MomentsParams, 64), "rt_denoise_variance_params": (rt.DenoiseVarianceParams, 136),
    "rt_upsample_params": (rt.UpsampleParams, 104),
    "rt_sample_pixels_params": (rt.SamplePixelsParams, 80), "rt_sample_priority_params": (rt.SamplePriorityParams, 40),
    "rt_sample_plan_params": (rt.SamplePlanParams, 80), "rt_sample_resolve_params": (rt.SampleResolveParams, 40),
}
# the structs whose static_assert in the header must pin the offset of every field
EVERY_OFFSET_PINNED = ("rt_point", "rt_nearest", "rt_closest_params", "rt_occlusion_params", "rt_ao_params")
NO_STATIC_ASSERT = ("rt_render_params", "rt_build_options")  # the header states no size for these: the compiler check does


def c_fields(cls):
    """The field names the header declares too: `_pad` stands in ctypes for the padding that alignas makes in C."""
    return [name for name, _ in cls._fields_ if name != "_pad"]


def test_the_table_covers_the_binding():
    classes = {v for v in vars(rt).values() if isinstance(v, type) and issubclass(v, ctypes.Structure)}
    assert classes == {cls for cls, _ in STRUCTS.values()}
    assert set(EVERY_OFFSET_PINNED) <= set(STRUCTS)


def test_against_the_compiler(tmp_path):
    lines = ["#include <cstddef>", "#include <cstdio>", '#include "rt_abi.h"', "int main() {"]
    want = {}
    for name, (cls, size) in STRUCTS.items():
        assert ctypes.sizeof(cls) == size, name
        lines.append(f'    std::printf("{name} %zu\\n", sizeof({name}));')
        want[name] = size
        for field in c_fields(cls):
            lines.append(f'    std::printf("{name}.{field} %zu\\n", offsetof({name}, {field}));')
            want[f"{name}.{field}"] = getattr(cls, field).offset
    lines += ["    return 0;", "}"]
    source, program = tmp_path / "layouts.cpp", tmp_path / "layouts"
    source.write_text("\n".join(lines) + "\n")
    r = subprocess.run(["g++", "-std=c++17", "-I", os.path.dirname(HEADER), str(source), "-o", str(program)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.run([str(program)], capture_output=True, text=True, timeout=30, check=True).stdout
    got = {k: int(v) for k, v in (line.split() for line in out.splitlines())}
    assert got == want, {k: (got.get(k), want.get(k)) for k in set(got) | set(want) if got.get(k) != want.get(k)}


@pytest.mark.parametrize("name", sorted(STRUCTS))
def test_against_the_header_text(name):
    cls, size = STRUCTS[name]
    hsize, offsets, declared = T.header_layout(open(HEADER).read(), name)
    fields = c_fields(cls)
    assert ctypes.sizeof(cls) == size and hsize == (None if name in NO_STATIC_ASSERT else size), (hsize, size)
    assert declared == fields, (declared, fields)
    assert set(offsets) <= set(fields)
    if name in EVERY_OFFSET_PINNED:
        assert hsize == size and set(offsets) == set(fields)
    for k, off in offsets.items():
        assert getattr(cls, k).offset == off, k
