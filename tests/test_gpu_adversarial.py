"""The adversarial scenes and rays of tests/adversarial_cases.py through the production traversal on the GPU:
rt_trace_rays (rtfast::trace in the variants a production frame runs: the lean MODE 17 | 128 for scenes A and C,
whose big leaf has pair, quad and unit records, MODE 21 for scene B, whose big leaf has a leaf tree) against
tests/query_ref.py, and one rendered frame of scene A against the reference-layout tracer.  No tolerance: the
arithmetic is specified.  tests/test_adversarial_cpu.py shows on the host that the cases are what they claim.
"""
import numpy as np
import pytest
import torch

import adversarial_cases as AC
import query_ref as Q
import rt_testlib as T

pytestmark = pytest.mark.gpu

F32 = np.float32
SCENES = ["A", "B"] + ["C:" + v for v in AC.GATES]
WAVES = [0, 5, 6, 7]


@pytest.fixture(scope="module", params=SCENES)
def prepared(request):
    """One scene on the device, its rays, and the reference's records (computed once per scene, left unchanged)."""
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    torch.cuda.set_device(0)
    rt = T.load_rt()
    name = request.param
    with AC.build_options(rt, name == "B"):
        case = AC.build_case(rt, name)
        case.scene.upload(0)  # queries only: no RNG states
        _, tree, _ = case.scene.mirror(trees=True)
        quads, units = case.scene.mirror_twins()
    case.big_leaf()
    if name == "B":
        assert len(tree) > 0, "no leaf tree: this would not be the MODE 21 kernel"
    else:
        assert len(tree) == 0 and len(quads) > 0 and len(units) > 0, "no twin records: this would not be the lean kernel"
    rs = AC.ray_set(case)
    assert len(rs.rays) % 64 != 0
    return name, case, rs, torch.from_numpy(rs.rays).cuda()


def same_records(got, rs, what):
    """Integer words bytewise; float words bytewise where neither side is a NaN, NaN positions identical (a NaN's
    payload is the ISA's choice: the rule of test_gpu_lean.py)."""
    g = np.ascontiguousarray(got.detach().cpu().numpy(), F32).reshape(-1, 12)
    w = rs.want
    assert g.shape == w.shape, (what, g.shape, w.shape)
    gu, wu = g.view(np.uint32), w.view(np.uint32)
    floats = np.ones(12, dtype=bool)
    floats[1:4] = False  # kind, id, material
    nan_g, nan_w = np.isnan(g) & floats, np.isnan(w) & floats
    bad = (nan_g != nan_w) | ((gu != wu) & ~(nan_g & nan_w))
    rows = np.flatnonzero(bad.any(axis=1))
    if rows.size:
        i = int(rows[0])
        fams = sorted({AC.FAMILIES[int(f)] for f in rs.family[rows]})
        pytest.fail(f"{what}: {rows.size} of {len(g)} records differ (families {fams}); first: ray {i}, family "
                    f"{AC.FAMILIES[int(rs.family[i])]}\n ray  {rs.rays[i, :7]!r} (bits {rs.rays[i, :7].view(np.uint32)})\n"
                    f" got  {g[i]!r} kind/id/material {gu[i, 1:4]}\n want {w[i]!r} kind/id/material {wu[i, 1:4]}")


@pytest.mark.parametrize("waves", WAVES)
def test_adversarial_rays(prepared, waves):
    rt = T.load_rt()
    name, case, rs, dev = prepared
    got = rt.trace_rays(case.scene, dev, waves_per_simd=waves)
    torch.cuda.synchronize()
    assert got.shape == (len(rs.rays), 12) and got.dtype == torch.float32
    same_records(got, rs, f"scene {name} at {waves} waves per SIMD")


# --- one rendered frame of scene A: the lean body sees the same geometry through bounce rays ---------------------------
W, H, SPP, BOUNCES = 32, 18, 2, 6


def render(rt, wps=0, tracer="fast"):
    """(surface [H, W, 4] float32, final RNG states [H * W, 6] uint32) of one frame of scene A."""
    case = AC.build_case(rt, "A")
    s = case.scene
    s.set_viewport(W, H)
    rng = rt.alloc_rng(W * H)
    rt.init_rng_states(rng, W, H, T.SEED)
    s.upload(rng.data_ptr())
    a, b = rt.alloc_surface(W, H), rt.alloc_surface(W, H)
    rt.render(s, a, b, W, H, SPP, BOUNCES, waves_per_simd=wps, tracer=tracer)
    torch.cuda.synchronize()
    return (rt.surface_view(a, W).cpu().numpy().copy(), rng.view(-1, 12)[:, :6].cpu().numpy().view(np.uint32).copy())


@pytest.fixture(scope="module")
def frame_reference():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    torch.cuda.set_device(0)
    rt = T.load_rt()
    case = AC.build_case(rt, "A")
    quads, units = case.scene.mirror_twins()
    assert len(quads) > 0 and len(units) > 0, "scene A has no big-leaf records: the general kernel would render it"
    # the camera looks at the pinwheel: most pixel-centre rays end on one of its faces
    cam = np.frombuffer(bytes(case.scene.camera()), dtype=F32)
    hits, _, _ = Q.trace(case.arrays(), Q.camera_rays(cam, W, H))
    u = hits.view(np.uint32)
    seen = float(((u[:, 1] == 2) & (u[:, 2] < 2 * case.k)).mean())
    assert seen >= 0.25, seen
    return render(rt, tracer="ref")


@pytest.mark.parametrize("wps", [5, 6, 7])
def test_rendered_frame(frame_reference, wps):
    rt = T.load_rt()
    got, want = render(rt, wps), frame_reference
    what = f"scene A frame at {wps} waves"
    nan_g, nan_w = np.isnan(got[0]), np.isnan(want[0])
    assert np.array_equal(nan_g, nan_w), f"{what}: NaN positions differ"
    mism = int((got[0].view(np.uint32)[~nan_g] != want[0].view(np.uint32)[~nan_w]).sum())
    assert mism == 0, f"{what}: {mism} surface words differ"
    assert np.array_equal(got[1], want[1]), f"{what}: final RNG states differ"
