"""The refusals rt_render makes once it has asked the device about the caller's buffers and looked the scene up, by
the exact rt_last_error text and return value 1, on the smallest inputs that reach them: a caller-built box of a few
triangles (tests/scene_cases.py) uploaded through rt_scene_upload, a 64 x 64 frame, and no frame rendered at all.  The
single faults come in rt_render's order of checks, then rows with two faults at once that pin which check comes first.
The refusals before that point need no device: tests/test_render_errors_cpu.py.

A buffer that a row needs too short is an allocation of its own (rt_malloc), so the check sees exactly its size; the
others are torch tensors.  The refusal for a missing plugin runs in a child process, because this one has it loaded."""
import ctypes
import json
import os
import subprocess
import sys

import pytest
import torch

import rt_testlib as T
import scene_cases as C

pytestmark = pytest.mark.gpu
W = H = 64                   # 16 tiles, 4096 pixel slots, 64 waves
STATS, REF, FLAT, WAVEFRONT = 1, 2, 4, 8  # rt_render_params.flags
BOX = dict(C.BY_NAME["box_front"], width=W, height=H)

LANE = "lane_slots / lane_cost / refill_lanes need the production tracer on an rt_scene_upload scene"
PROBE = "lane_cost probes run without refill"
WF = ("the wavefront tracer needs an rt_scene_upload scene and no statistics / lane_cost / wave_clock / refill / lone "
      "frames")
WF_LIMITS = "the wavefront tracer needs spp <= 65535, bounces <= 255, spp x bounces <= 65536"
PLUGIN = ("this frame asks for an experimental render path (wavefront tracer, refill, lone-pixel kernel or an RT_TUNE "
          "A/B variant), which lives in librt_hip_exp.so -- load it first (rt.load_experimental())")
LONE_COUNT = "lone_count must be in [0, 2^28] with lone_slots"
LONE_NEEDS = ("lone_slots need lane_slots and the production tracer on an rt_scene_upload scene (no statistics / "
              "lane_cost / refill frames)")
TREELETS = "lone_slots need the scene's treelets (a BVH of depth <= 75 with an inner root)"
TUNE = "RT_TUNE occupancy override 1 (compiler's choice) is not built"

# A value that is a string names a buffer of `world`: the sound ones, and "short_<name>", one element short of what
# the frame needs.  (elements, bytes of one) of each:
BUFFERS = {"tiles": (16, 4), "clock": (64, 8), "lanes": (64, 4), "cost": (W * H, 4), "stats": (None, 8), "lone": (4, 4)}
LANES = dict(lane_slots="lanes", lane_slot_count=64)
LONE = dict(LANES, lone_slots="lone", lone_count=4)
# (scene, overrides of rt_render_params, message after "rt_render: ")
TABLE = [
    # the buffers, in the order they are checked
    ("box", dict(tile_list="short_tiles", tile_count=16), "tile_list too small"),
    ("box", dict(wave_clock="short_clock"), "wave_clock too small"),
    ("box", dict(lane_slots="short_lanes", lane_slot_count=64), "lane_slots too small"),
    ("box", dict(lane_cost="short_cost"), "lane_cost too small"),
    ("box", dict(flags=STATS, stats="short_stats"), "stats too small"),
    # lane_slots / lane_cost / refill_lanes off the production tracer
    ("box", dict(LANES, flags=REF), LANE), ("box", dict(lane_cost="cost", flags=REF), LANE),
    ("box", dict(refill_lanes=8, flags=REF), LANE),
    ("box", dict(LANES, flags=FLAT), LANE), ("box", dict(lane_cost="cost", flags=FLAT), LANE),
    ("box", dict(refill_lanes=8, flags=FLAT), LANE),
    ("box", dict(lane_cost="cost", refill_lanes=8), PROBE),
    # the wavefront tracer: each clause of its refusal, then its limits
    ("box", dict(flags=WAVEFRONT | REF), WF), ("box", dict(flags=WAVEFRONT | FLAT), WF),
    ("box", dict(flags=WAVEFRONT | STATS, stats="stats"), WF), ("box", dict(flags=WAVEFRONT, lane_cost="cost"), WF),
    ("box", dict(flags=WAVEFRONT, refill_lanes=8), WF), ("box", dict(flags=WAVEFRONT, wave_clock="clock"), WF),
    ("box", dict(flags=WAVEFRONT, lone_count=1), WF),
    ("box", dict(flags=WAVEFRONT, spp=65536), WF_LIMITS), ("box", dict(flags=WAVEFRONT, bounces=256), WF_LIMITS),
    ("box", dict(flags=WAVEFRONT, spp=300, bounces=300), WF_LIMITS),
    # the lone-pixel kernel
    ("box", dict(LANES, lone_count=4), LONE_COUNT), ("box", dict(LONE, lone_count=-1), LONE_COUNT),
    ("box", dict(LONE, lone_count=2 ** 28 + 1), LONE_COUNT),
    ("box", dict(lone_slots="lone", lone_count=4), LONE_NEEDS), ("box", dict(LONE, flags=FLAT), LANE),
    ("box", dict(LONE, flags=STATS, stats="stats"), LONE_NEEDS),
    ("leaf", LONE, TREELETS),
    ("box", dict(LONE, lone_slots="short_lone"), "lone_slots too small"),
    # two faults
    ("box", dict(tune=1 << 9, tile_list="short_tiles", tile_count=16), TUNE),
    ("box", dict(tile_list="short_tiles", tile_count=16, wave_clock="short_clock"), "tile_list too small"),
    ("box", dict(wave_clock="short_clock", lane_cost="short_cost"), "wave_clock too small"),  # (a lane map sets the waves)
    ("box", dict(lane_slots="short_lanes", lane_slot_count=64, lane_cost="short_cost"), "lane_slots too small"),
    ("box", dict(lane_cost="short_cost", flags=STATS, stats="short_stats"), "lane_cost too small"),
    ("box", dict(LANES, flags=REF | STATS, stats="short_stats"), "stats too small"),
    ("box", dict(lane_cost="cost", refill_lanes=8, flags=REF), LANE),
    ("box", dict(lane_cost="cost", refill_lanes=8, flags=WAVEFRONT), PROBE),
    ("box", dict(flags=WAVEFRONT | STATS, stats="stats", spp=65536), WF),
    ("box", dict(lone_slots="lone", lone_count=2 ** 28 + 1), LONE_COUNT),
    ("leaf", dict(lone_slots="lone", lone_count=4), LONE_NEEDS),
    ("leaf", dict(LONE, lone_slots="short_lone"), TREELETS),
]
# without the plugin: what asks for it, and the two checks on either side of that one
CHILD_TABLE = [
    (dict(flags=WAVEFRONT), PLUGIN), (dict(refill_lanes=8), PLUGIN), (dict(tune=4096), PLUGIN),
    (dict(lone_count=1), PLUGIN), (dict(flags=WAVEFRONT, spp=300, bounces=300), WF_LIMITS),
    (dict(lone_count=-1), LONE_COUNT),
]


def upload(rt, scene):
    rng = rt.alloc_rng(W * H)
    scene.set_viewport(W, H)
    scene.upload(rng.data_ptr())
    return scene, rng  # the states live as long as the scene


def render_code(rt, scene_ptr, surface, fields):
    """(rt_render's return value, rt_last_error) of a one-sample 64 x 64 frame with `fields` over it."""
    p = rt.RenderParams()
    p.surface, p.width, p.height, p.pitch, p.spp, p.bounces, p.shard_count = surface.data_ptr(), W, H, surface.shape[1] * 4, 1, 1, 1
    for k, v in fields.items():
        setattr(p, k, v)
    code = rt.lib().rt_render(ctypes.byref(p), scene_ptr, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    return code, rt.lib().rt_last_error().decode()


@pytest.fixture(scope="module")
def world():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    torch.cuda.set_device(0)
    rt = T.load_rt()
    rt.load_experimental()
    leaf = rt.Scene()  # one triangle: the BVH's root is a leaf, so the scene has no treelets
    leaf.add_triangle((-1.0, -1.0, 5.0), (1.0, -1.0, 5.0), (0.0, 1.0, 5.0), leaf.add_material(albedo=(0.5, 0.5, 0.5)))
    w = {"rt": rt, "box": upload(rt, C.apply_product(rt, BOX)), "leaf": upload(rt, leaf), "surface": rt.alloc_surface(W, H)}
    short = []
    for name, (n, size) in BUFFERS.items():
        n = n or rt.STAT_COUNT
        w[name] = torch.full((n * size // 4,), -1 if name in ("lanes", "lone") else 0, dtype=torch.int32, device="cuda")
        p = ctypes.c_void_p()
        assert rt.lib().rt_malloc(ctypes.byref(p), (n - 1) * size) == 0
        short.append(p)
        w["short_" + name] = p
    yield w
    torch.cuda.synchronize()
    for p in short:
        assert rt.lib().rt_free(p) == 0


def resolve(world, fields):
    """`fields` with the buffers' names replaced by their addresses."""
    at = lambda b: b.value if isinstance(b, ctypes.c_void_p) else b.data_ptr()
    return {k: at(world[v]) if isinstance(v, str) else v for k, v in fields.items()}


@pytest.mark.parametrize("scene, fields, message", TABLE, ids=lambda v: None if isinstance(v, dict) else v[:24])
def test_refusal(world, scene, fields, message):
    rt = world["rt"]
    code, error = render_code(rt, ctypes.cast(world[scene][0].gpu, ctypes.c_void_p), world["surface"], resolve(world, fields))
    assert (code, error) == (1, "rt_render: " + message), fields


def test_foreign_scene(world):
    """A GPUScene another host filled: lane_slots is refused with the production tracer's text while no mirror is
    installed (the reference layout would render the frame) and once one is (the frame is gated); the wavefront tracer
    likewise.  The refused calls have enqueued the frame's fingerprint all the same, and it matches the mirror's."""
    rt, (s, rng) = world["rt"], world["box"]
    ha, g = s.host_arrays(), s.gpu.contents
    sizes = {"gpu_bvh_nodes": ha["nodes"].nbytes, "gpu_bvh_face_indices": ha["face_indices"].nbytes,
             "gpu_vertices": ha["vertices"].nbytes, "gpu_faces": ha["faces"].nbytes, "gpu_spheres": 32 * g.sphere_count,
             "gpu_materials": 64 * g.material_count}
    f = rt.GPUScene()
    ctypes.pointer(f)[0] = g
    owned = {}
    try:
        for k, n in sizes.items():
            owned[k] = ctypes.c_void_p()
            assert rt.lib().rt_malloc(ctypes.byref(owned[k]), n) == 0
            assert rt.lib().rt_memcpy_d2d(owned[k], ctypes.c_void_p(getattr(g, k)), n) == 0
            setattr(f, k, owned[k].value)
        ptr = ctypes.cast(ctypes.pointer(f), ctypes.c_void_p)
        lanes = resolve(world, LANES)
        assert render_code(rt, ptr, world["surface"], lanes) == (1, "rt_render: " + LANE)
        assert rt.foreign_last_tracer(f) == -1  # no mirror yet
        rt.foreign_mirror_wait(f)
        assert render_code(rt, ptr, world["surface"], lanes) == (1, "rt_render: " + LANE)  # installs the mirror
        assert render_code(rt, ptr, world["surface"], dict(flags=WAVEFRONT)) == (1, "rt_render: " + WF)
        assert rt.foreign_last_tracer(f) == 1
    finally:
        torch.cuda.synchronize()
        for p in owned.values():
            rt.lib().rt_free(p)


CHILD = """
import ctypes, json, sys
sys.path.insert(0, %r)
import torch
import test_gpu_render_errors as E
torch.cuda.set_device(0)
rt = E.T.load_rt()
assert rt.lib().rt_experimental_loaded() == 0
s, rng = E.upload(rt, E.C.apply_product(rt, E.BOX))
surface = rt.alloc_surface(E.W, E.H)
out = [E.render_code(rt, ctypes.cast(s.gpu, ctypes.c_void_p), surface, fields) for fields, _ in E.CHILD_TABLE]
torch.cuda.synchronize()
print("RESULT " + json.dumps(out))
"""


def test_experimental_paths_before_the_plugin_is_loaded():
    r = subprocess.run([sys.executable, "-c", CHILD % os.path.join(T.ROOT, "tests")], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    got = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    assert got == [[1, "rt_render: " + m] for _, m in CHILD_TABLE]
