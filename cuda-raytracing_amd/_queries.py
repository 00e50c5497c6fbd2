"""Queries on an uploaded scene's BVH: closest hits, occlusion and ambient occlusion, closest points, hit lists,
radiance along caller-given rays, and the tensor code built on them (G-buffer, grids, containment, panoramas)."""
import ctypes

import numpy as np
import torch

from ._abi import (HIT_MISS, HITS_MAX, RAY_TMAX, REFERENCE_BOUNCES, REFERENCE_SPP, RT_HITS_COUNT_ALL, RT_HITS_CULL_BACK,
                   AoParams, ClosestParams, HitsParams, OcclusionParams, RadianceParams, RTError, TraceParams, _check,
                   _last_error, lib)
from ._args import (_allocating_on, _f3, _given_or_new, _is_hits, _is_rays, _is_rng, _is_tensor, _launch, _set_scratch,
                    alloc_rng, alloc_surface, surface_view)
from ._render import init_rng_states


def _trace(scene, rays, count, width, height, hits, stream, waves_per_simd):
    hits = _given_or_new(hits, stream, torch.empty, (count, 12), dtype=torch.float32,
                         device=rays.device if rays is not None else "cuda")
    assert _is_hits(hits, count)
    p = TraceParams(rays=rays.data_ptr() if rays is not None else None, count=count, width=width, height=height,
                    hits=hits.data_ptr(), waves_per_simd=int(waves_per_simd))
    _launch("rt_trace_rays", p, stream, scene)
    return hits


def trace_rays(scene, rays, hits=None, stream=None, waves_per_simd=0):
    """rt_trace_rays: the closest hit of every ray of a float32 CUDA tensor [N, 8] (rt_ray rows: origin,
    tmax, direction, a zero word) on `stream` (default: torch's current stream), as a float32 [N, 12]
    tensor of rt_hit rows (`hits`, or a new one; hit_fields gives typed views).  The scene must have
    been uploaded (Scene.upload; its RNG pointer may be 0 for a scene that is only queried)."""
    assert _is_rays(rays)
    return _trace(scene, rays, rays.shape[0], 0, 0, hits, stream, waves_per_simd)


def trace_camera(scene, width, height, hits=None, stream=None, waves_per_simd=0):
    """rt_trace_rays in camera mode: the rays through the pixel centres of the uploaded scene's camera
    (Scene.set_viewport before upload), row i = pixel (i % width, i // width); float32 [H*W, 12]."""
    return _trace(scene, None, int(width) * int(height), int(width), int(height), hits, stream, waves_per_simd)


def hit_fields(hits):
    """Typed views of a [N, 12] hit tensor (torch or numpy): t, kind / id / material (int32), normal [N, 3],
    position [N, 3], bx, by."""
    ints = hits.view(torch.int32) if isinstance(hits, torch.Tensor) else hits.view(np.int32)
    return {"t": hits[:, 0], "kind": ints[:, 1], "id": ints[:, 2], "material": ints[:, 3], "normal": hits[:, 4:7],
            "bx": hits[:, 7], "position": hits[:, 8:11], "by": hits[:, 11]}


def gbuffer(scene, width, height, stream=None, waves_per_simd=0):
    """First-hit images of an uploaded Scene's camera (rt_trace_rays in camera mode: the pixel centres, no
    jitter) as device tensors, rows bottom to top like the surface: depth [H, W] (t; inf on a miss),
    normal / position / albedo [H, W, 3] (0 on a miss; albedo is the hit material's), material, prim (-1 on
    a miss; sphere or face index) and kind [H, W] int32."""
    w, h = int(width), int(height)
    f = hit_fields(trace_camera(scene, w, h, stream=stream, waves_per_simd=waves_per_simd))
    hit = f["kind"] != HIT_MISS
    mats = torch.from_numpy(scene.materials()).to(hit.device)
    albedo = torch.zeros((w * h, 3), dtype=torch.float32, device=hit.device)
    if mats.shape[0]:
        albedo = torch.where(hit[:, None], mats[f["material"].long().clamp(0, mats.shape[0] - 1), :3], albedo)
    return {"depth": torch.where(hit, f["t"], torch.full_like(f["t"], float("inf"))).reshape(h, w),
            "normal": f["normal"].reshape(h, w, 3).clone(), "position": f["position"].reshape(h, w, 3).clone(),
            "albedo": albedo.reshape(h, w, 3), "material": f["material"].reshape(h, w).clone(),
            "prim": torch.where(hit, f["id"], torch.full_like(f["id"], -1)).reshape(h, w),
            "kind": f["kind"].reshape(h, w).clone()}


def occluded(scene, rays, out=None, stream=None, waves_per_simd=0):
    """rt_occluded: whether each ray of a float32 CUDA tensor [N, 8] (rt_ray rows, as trace_rays takes them) hits
    anything before its tmax, as a uint8 tensor [N] (`out`, or a new one): byte i is `kind != 0` of the record
    trace_rays gives for ray i, for every ray, at a fraction of the cost where the traversal may stop at the first
    occluder.  Stream-ordered on `stream` (default: torch's current stream)."""
    assert _is_rays(rays)
    n = rays.shape[0]
    out = _given_or_new(out, stream, torch.empty, (n,), dtype=torch.uint8, device=rays.device)
    assert _is_tensor(out, torch.uint8, 1, least=n)
    if n == 0:  # rt_occluded returns at once for count 0; an empty tensor has no address to pass
        return out
    p = OcclusionParams(rays=rays.data_ptr(), count=n, occluded=out.data_ptr(), waves_per_simd=int(waves_per_simd))
    _launch("rt_occluded", p, stream, scene)
    return out


def closest_points(scene, points, out=None, waves_per_simd=0, stream=None):
    """rt_closest_point: the nearest point of the scene's surface to every row of a float32 CUDA tensor [N, 4]
    (rt_point rows: position, search radius -- inf for none), as a float32 [N, 8] tensor of rt_nearest rows (`out`, or
    a new one; nearest_fields gives typed views): distance, kind, id, material, the point, the triangle's region.  A
    point with nothing within its radius gets a miss: its radius and zeros.  Exact and unsigned (rt_abi.h).
    Stream-ordered on `stream` (default: torch's current stream)."""
    assert _is_tensor(points, torch.float32, 2, (4,))
    n = points.shape[0]
    out = _given_or_new(out, stream, torch.empty, (n, 8), dtype=torch.float32, device=points.device)
    assert _is_tensor(out, torch.float32, 2, (8,), n)
    if n == 0:  # rt_closest_point returns at once for count 0; an empty tensor has no address to pass
        return out
    p = ClosestParams(points=points.data_ptr(), count=n, nearest=out.data_ptr(), waves_per_simd=int(waves_per_simd))
    _launch("rt_closest_point", p, stream, scene)
    return out


def nearest_fields(nearest):
    """Typed views of a [N, 8] record tensor (torch or numpy): distance, kind / id / material / region (int32),
    point [N, 3]."""
    ints = nearest.view(torch.int32) if isinstance(nearest, torch.Tensor) else nearest.view(np.int32)
    return {"distance": nearest[:, 0], "kind": ints[:, 1], "id": ints[:, 2], "material": ints[:, 3],
            "point": nearest[:, 4:7], "region": ints[:, 7]}


def closest_points_host(scene, points):
    """rt_closest_point_host: closest_points' records by brute force on the host (a built or uploaded Scene, a
    float32 numpy array [N, 4]) as a float32 numpy array [N, 8].  No BVH and no device: for checking."""
    pts = np.ascontiguousarray(points, dtype=np.float32)
    assert pts.ndim == 2 and pts.shape[1] == 4
    out = np.zeros((pts.shape[0], 8), dtype=np.float32)
    _check(lib().rt_closest_point_host(scene.handle, pts.ctypes.data, pts.shape[0], out.ctypes.data), "rt_closest_point_host")
    return out


def closest_bound_host(p, lo, hi):
    """closest.h box_bound on the host (rt_closest_bound_host): the kernel's lower bound on the computed squared
    distance from p to any face with its vertices in the box [lo, hi]; -1 = no bound."""
    return float(lib().rt_closest_bound_host(_f3(p), _f3(lo), _f3(hi)))


def _grid_axes(lo, hi, shape):
    """The cell centres of a (nz, ny, nx) grid over the box [lo, hi] as device tensors (z, y, x)."""
    axes = []
    for n, a, b in ((shape[0], lo[2], hi[2]), (shape[1], lo[1], hi[1]), (shape[2], lo[0], hi[0])):
        i = torch.arange(n, dtype=torch.float32, device="cuda")
        axes.append(float(a) + (i + 0.5) * ((float(b) - float(a)) / n))
    return axes


def distance_grid(scene, lo, hi, shape, radius=float("inf"), stream=None, waves_per_simd=0):
    """The unsigned distance from the centre of every cell of a regular grid to the scene's surface: `shape` =
    (nz, ny, nx) cells over the box [lo, hi] (x, y, z), as a float32 device tensor [nz, ny, nx].  A cell with nothing
    within `radius` holds `radius`.  Tensor code over closest_points."""
    nz, ny, nx = (int(s) for s in shape)
    with _allocating_on(stream):
        z, y, x = torch.meshgrid(*_grid_axes(lo, hi, (nz, ny, nx)), indexing="ij")
        pts = torch.stack([x, y, z, torch.full_like(x, float(radius))], dim=-1).reshape(-1, 4).contiguous()
    rec = closest_points(scene, pts, stream=stream, waves_per_simd=waves_per_simd)
    return rec[:, 0].reshape(nz, ny, nx).clone()


def _trace_hits(scene, rays, count, width, height, max_hits, flags, hits, counts, stream, waves_per_simd):
    k = int(max_hits)
    device = rays.device if rays is not None else "cuda"
    hits = _given_or_new(hits, stream, torch.empty, (count, k, 12), dtype=torch.float32, device=device)
    counts = _given_or_new(counts, stream, torch.empty, (count,), dtype=torch.int32, device=device)
    assert _is_tensor(hits, torch.float32, 3, (k, 12), count)
    if counts is False:  # none kept
        counts = None
    else:
        assert _is_tensor(counts, torch.int32, 1, least=count)
    if count == 0:  # rt_trace_hits returns at once for count 0; an empty tensor has no address to pass
        return hits, counts
    p = HitsParams(rays=rays.data_ptr() if rays is not None else None, count=count, width=width, height=height,
                   hits=hits.data_ptr(), counts=None if counts is None else counts.data_ptr(), max_hits=k,
                   flags=int(flags), waves_per_simd=int(waves_per_simd))
    _launch("rt_trace_hits", p, stream, scene)
    return hits, counts


def trace_hits(scene, rays, max_hits, flags=0, hits=None, counts=None, stream=None, waves_per_simd=0):
    """rt_trace_hits: the first `max_hits` (1..16) hits of every ray of a float32 CUDA tensor [N, 8] (rt_ray rows), in
    order of distance, as (hits, counts): a float32 [N, K, 12] tensor of rt_hit rows -- row k of a ray its k-th hit, the
    rows past the last a miss record (t = tmax, zeros) -- and an int32 [N] tensor of list lengths.  flags:
    RT_HITS_CULL_BACK / RT_HITS_CULL_FRONT keep one winding's triangles (on a loaded mesh: one record per crossing),
    RT_HITS_COUNT_ALL makes counts the number of all hits below tmax (it may exceed K).  `hits` / `counts`: tensors to
    fill in place (counts=False: none kept, None is returned for it).  Exact, as trace_rays (rt_abi.h); stream-ordered
    on `stream` (default: torch's current stream)."""
    assert _is_rays(rays)
    return _trace_hits(scene, rays, rays.shape[0], 0, 0, max_hits, flags, hits, counts, stream, waves_per_simd)


def trace_hits_camera(scene, width, height, max_hits, flags=0, hits=None, counts=None, stream=None, waves_per_simd=0):
    """rt_trace_hits in camera mode: trace_camera's rays (the pixel centres of the uploaded scene's camera), ray i =
    pixel (i % width, i // width); (hits [H*W, K, 12], counts [H*W])."""
    return _trace_hits(scene, None, int(width) * int(height), int(width), int(height), max_hits, flags, hits, counts, stream,
                       waves_per_simd)


def hit_list_host(t, payload, max_hits, tmax, count_all=False):
    """rt_hit_list_host: the kernel's list code (csrc/hit_list.h) on the host -- the pairs (t[j], payload[j]) offered in
    order to an empty list of `max_hits` entries under `tmax`.  Returns (t float32 [n], payload uint32 [n], total)."""
    t = np.ascontiguousarray(t, dtype=np.float32).reshape(-1)
    payload = np.ascontiguousarray(payload, dtype=np.uint32).reshape(-1)
    assert t.shape == payload.shape
    out_t, out_p = np.zeros(HITS_MAX, dtype=np.float32), np.zeros(HITS_MAX, dtype=np.uint32)
    total = ctypes.c_int64(0)
    n = lib().rt_hit_list_host(int(max_hits), float(tmax), 1 if count_all else 0, t.shape[0], t.ctypes.data, payload.ctypes.data,
                               out_t.ctypes.data, out_p.ctypes.data, ctypes.byref(total))
    if n < 0:
        raise RTError("rt_hit_list_host failed: " + _last_error())
    return out_t[:n].copy(), out_p[:n].copy(), int(total.value)


# contains(): three fixed unit directions in general position (no component 0, none parallel to a box face or diagonal)
CONTAINS_DIRECTIONS = ((0.36, 0.48, 0.8), (-0.6, 0.64, -0.48), (0.8, -0.36, 0.48))


def contains(scene, points, flags=RT_HITS_CULL_BACK, stream=None, waves_per_simd=0):
    """Whether each row of a float32 CUDA tensor [N, 3] lies inside a closed body of the scene, as a bool tensor [N]:
    the parity of the surface crossings along a ray to infinity, counted under one winding (rt_trace_hits with
    RT_HITS_COUNT_ALL | `flags`, so that a loaded mesh's twin faces count once), by majority over three fixed
    directions.  Meaningful for closed surfaces; spheres count as they are crossed (one distance each)."""
    assert _is_tensor(points, torch.float32, 2, (3,), contiguous=False)
    n = points.shape[0]
    with _allocating_on(stream):  # the tensor code here runs on the call's stream, like the kernels between it
        votes = torch.zeros((n,), dtype=torch.int32, device=points.device)
        rays = torch.zeros((n, 8), dtype=torch.float32, device=points.device)
        rays[:, 0:3] = points
        rays[:, 3] = RAY_TMAX
        hits = torch.empty((n, 1, 12), dtype=torch.float32, device=points.device)
        for d in CONTAINS_DIRECTIONS:
            rays[:, 4:7] = torch.tensor(d, dtype=torch.float32, device=points.device)
            _, counts = trace_hits(scene, rays, 1, flags=RT_HITS_COUNT_ALL | int(flags), hits=hits, stream=stream,
                                   waves_per_simd=waves_per_simd)
            votes += counts & 1
        return votes >= 2


def signed_distance_grid(scene, lo, hi, shape, radius=float("inf"), flags=RT_HITS_CULL_BACK, stream=None, waves_per_simd=0):
    """distance_grid with a sign: the same distances (bit for bit), negated at the cell centres `contains` finds inside."""
    nz, ny, nx = (int(s) for s in shape)
    dist = distance_grid(scene, lo, hi, shape, radius=radius, stream=stream, waves_per_simd=waves_per_simd)
    with _allocating_on(stream):
        z, y, x = torch.meshgrid(*_grid_axes(lo, hi, (nz, ny, nx)), indexing="ij")
        pts = torch.stack([x, y, z], dim=-1).reshape(-1, 3).contiguous()
        inside = contains(scene, pts, flags=flags, stream=stream).reshape(nz, ny, nx)
        return torch.where(inside, -dist, dist)


def radiance(scene, rays, rng, bounces=REFERENCE_BOUNCES, samples=1, out=None, stream=None, waves_per_simd=0):
    """rt_radiance: the path-traced radiance along every ray of a float32 CUDA tensor [N, 8] (rt_ray rows, as
    trace_rays takes them; tmax is not read) as a float32 [N, 4] tensor (`out`, or a new one): rgb = the mean of
    `samples` evaluations of the reference's ray_color along the ray, w = 1.  `rng`: an int32 CUDA tensor of N states
    (ray_rng, alloc_rng), state i read for ray i and written back advanced.  Pass unit directions unless the rays
    reproduce the reference's camera (rt_abi.h).  Stream-ordered on `stream` (default: torch's current stream)."""
    assert _is_rays(rays)
    n = rays.shape[0]
    assert _is_rng(rng, n)
    out = _given_or_new(out, stream, torch.empty, (n, 4), dtype=torch.float32, device=rays.device)
    assert _is_tensor(out, torch.float32, 2, (4,), n)
    if n == 0:  # rt_radiance returns at once for count 0; an empty tensor has no address to pass
        return out
    p = RadianceParams(rays=rays.data_ptr(), count=n, rng=rng.data_ptr(), radiance=out.data_ptr(), bounces=int(bounces),
                       samples=int(samples), waves_per_simd=int(waves_per_simd))
    _launch("rt_radiance", p, stream, scene)
    return out


def ray_rng(count, seed, device=None, stream=None):
    """`count` RNG states for radiance(): state i is curand_init(seed, i, 0) (alloc_rng + rt_init_rng of a count x 1
    frame), allocated and initialised on `stream` (default: torch's current stream)."""
    rng = _given_or_new(None, stream, alloc_rng, int(count), device=device)
    if int(count) > 0:
        init_rng_states(rng, int(count), 1, seed, stream=stream)
    return rng


def panorama_rays(origin, width, height):
    """A float32 [H*W, 8] numpy table of rt_ray rows: the equirectangular rays of a width x height panorama from
    `origin`.  Row y*W + x, rows bottom to top like the surface: longitude phi = 2 pi (x + 0.5) / W - pi, latitude
    theta = pi (y + 0.5) / H - pi / 2, direction (cos theta sin phi, sin theta, cos theta cos phi) -- the centre
    column looks along +z, x grows to the right of it -- computed in float64 and rounded; tmax = RAY_TMAX.  (The
    renderer's camera looking along +z has +x on its LEFT: shown as an image this map is the mirror image of what that
    camera sees; flip the columns for a view from inside.)"""
    w, h = int(width), int(height)
    phi = 2.0 * np.pi * (np.arange(w, dtype=np.float64) + 0.5) / w - np.pi
    theta = np.pi * (np.arange(h, dtype=np.float64) + 0.5) / h - 0.5 * np.pi
    ct, st = np.cos(theta)[:, None], np.sin(theta)[:, None]
    out = np.zeros((h, w, 8), dtype=np.float32)
    out[..., 0:3] = np.asarray(origin, dtype=np.float32).reshape(3)
    out[..., 3] = RAY_TMAX
    out[..., 4], out[..., 5], out[..., 6] = ct * np.sin(phi)[None, :], st * np.ones((1, w)), ct * np.cos(phi)[None, :]
    return out.reshape(h * w, 8)


def panorama(scene, width, height, origin=None, samples=REFERENCE_SPP, bounces=REFERENCE_BOUNCES, seed=0xDEADBEEF,
             device=None, stream=None):
    """A width x height equirectangular panorama of an uploaded Scene seen from `origin` (default: its camera's
    position) as a new pitched surface (alloc_surface layout, rows bottom to top): radiance() along panorama_rays()
    with the states ray_rng(width * height, seed).  The rays are uploaded with a synchronous copy; the rest is
    stream-ordered on `stream` (default: torch's current stream), where everything here is allocated."""
    w, h = int(width), int(height)
    if origin is None:
        origin = tuple(scene.camera().origin)
    with _allocating_on(stream):
        rays = torch.from_numpy(panorama_rays(origin, w, h)).to(device or "cuda")
        rng = ray_rng(w * h, seed, device=rays.device, stream=stream)
        rgba = radiance(scene, rays, rng, bounces=bounces, samples=samples, stream=stream)
        surface = alloc_surface(w, h, device=rays.device)
        surface_view(surface, w).copy_(rgba.view(h, w, 4))
    return surface


def ao_directions(count=256):
    """A [count, 4] float32 table of unit vectors for ambient_occlusion (w = 0): the Fibonacci sphere points
    z = 1 - (2k + 1) / count, azimuth k * pi * (3 - sqrt(5)), computed in float64 and rounded."""
    k = np.arange(int(count), dtype=np.float64)
    z = 1.0 - (2.0 * k + 1.0) / float(count)
    r = np.sqrt(np.maximum(0.0, 1.0 - z * z))
    phi = k * (np.pi * (3.0 - np.sqrt(5.0)))
    out = np.zeros((int(count), 4), dtype=np.float32)
    out[:, 0], out[:, 1], out[:, 2] = r * np.cos(phi), r * np.sin(phi), z
    return out


_ao_default_tables = {}  # device -> ao_directions(256) on it


def _ao_default_directions(device):
    """ao_directions(256) on `device`, built and uploaded once per device (a synchronous copy from pageable host
    memory: complete when it returns, so the table is safe to read on any stream)."""
    key = torch.device(device)
    if key.type == "cuda" and key.index is None:
        key = torch.device("cuda", torch.cuda.current_device())
    t = _ao_default_tables.get(key)
    if t is None:
        t = _ao_default_tables[key] = torch.from_numpy(ao_directions(256)).to(key)
    return t


def ao_scratch_bytes(width, height, samples):
    """rt_ao_scratch_bytes: bytes of scratch rt_ao needs."""
    return int(lib().rt_ao_scratch_bytes(int(width), int(height), int(samples)))


def ambient_occlusion(scene, hits, width, height, radius, samples=8, bias=0.001, directions=None, out=None, scratch=None,
                      stream=None, waves_per_simd=0):
    """rt_ao: the ambient-occlusion image [H, W] float32 (1 = open, 0 = closed; 1 where the camera ray missed) of an
    uploaded Scene from the first-hit records `hits` (float32 [H*W, 12], what trace_camera returns): per pixel,
    `samples` cosine-weighted rays of length `radius` from the hit point, offset along its normal by `bias` times the
    hit distance.  `directions`: a float32 [K, 4] table of unit vectors; default ao_directions(256), uploaded once
    per device and kept.  Stream-ordered on `stream` (default: torch's current stream) when `directions` is a CUDA
    tensor or the default; a numpy table is uploaded by this call with a synchronous copy.  What is allocated here
    is allocated on that stream."""
    w, h = int(width), int(height)
    assert _is_hits(hits, w * h)
    need = ao_scratch_bytes(w, h, samples)
    with _allocating_on(stream):
        if directions is None:
            directions = _ao_default_directions(hits.device)
        if not isinstance(directions, torch.Tensor):
            directions = torch.from_numpy(np.ascontiguousarray(directions, dtype=np.float32)).to(hits.device)
    out = _given_or_new(out, stream, torch.empty, (h, w), dtype=torch.float32, device=hits.device)
    assert _is_tensor(directions, torch.float32, 2, (4,)) and _is_tensor(out, torch.float32, least=w * h)
    p = AoParams(hits=hits.data_ptr(), width=w, height=h, directions=directions.data_ptr(),
                 direction_count=directions.shape[0], samples=int(samples), radius=float(radius), bias=float(bias),
                 ao=out.data_ptr(), waves_per_simd=int(waves_per_simd))
    scratch = _set_scratch(p, scratch, stream, need, hits.device)  # nothing is allocated when rt_ao needs none
    _launch("rt_ao", p, stream, scene)
    return out
