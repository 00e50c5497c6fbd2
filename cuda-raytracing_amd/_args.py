"""What every wrapper does to its arguments: pointers for the library, the checks on tensors, "given or new"
allocation on the call's stream, and the call line itself."""
import contextlib
import ctypes

import numpy as np
import torch

from ._abi import RNG_STATE_BYTES, GPUCamera, _check, lib

_INT16S = tuple(getattr(torch, n) for n in ("int16", "uint16") if hasattr(torch, n))  # the 2-byte integer dtypes


def _f3(v):
    return (ctypes.c_float * 3)(*[float(x) for x in v])


def _stream_ptr(stream=None):
    s = stream if stream is not None else torch.cuda.current_stream()
    return ctypes.c_void_p(s.cuda_stream)


def _scene_ptr(scene):
    """The GPUScene* of a Scene, or of a GPUScene filled by the caller."""
    return ctypes.cast(scene.gpu if hasattr(scene, "gpu") else ctypes.pointer(scene), ctypes.c_void_p)


def _launch(name, p, stream, scene=None):
    """The call line of a params-struct entry point: rt_x(&p, [scene,] stream), an error code raised as RTError."""
    args = (ctypes.byref(p), _stream_ptr(stream)) if scene is None else (ctypes.byref(p), _scene_ptr(scene), _stream_ptr(stream))
    _check(getattr(lib(), name)(*args), name)


def _allocating_on(stream):
    """Context in which torch allocates (and fills) on `stream`; None = torch's current stream, as it is."""
    return torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()


def _given_or_new(given, stream, new, *args, **kw):
    """`given`, or new(*args, **kw) allocated (and filled) on the call's stream: the kernels that write it run there, so
    a fill is ordered before them and the caching allocator does not hand the memory to another stream's work while
    they still run."""
    if given is not None:
        return given
    with _allocating_on(stream):
        return new(*args, **kw)


def _set_scratch(p, given, stream, need, device, check_size=False):
    """Fill p.scratch / p.scratch_bytes from `given` -- any contiguous CUDA tensor (of at least `need` bytes where the
    call checks that itself; the others leave it to the library) -- or from `need` new bytes on the call's stream.
    Returns the tensor, which the caller holds until the call is enqueued; None when nothing is given or needed."""
    if given is None and need:
        given = _given_or_new(None, stream, torch.empty, (need,), dtype=torch.uint8, device=device)
    if given is not None:
        p.scratch, p.scratch_bytes = given.data_ptr(), given.numel() * given.element_size()
        assert _is_tensor(given) and (not check_size or p.scratch_bytes >= need)
    return given


def _is_tensor(t, dtype=None, dim=None, tail=(), least=0, contiguous=True):
    """A CUDA tensor of `dtype` (one, a tuple of them, or None for any), contiguous unless the call never asked, of
    rank `dim` with the trailing sizes `tail` and at least `least` rows -- or, dim None, of at least `least` elements."""
    if dtype is not None and t.dtype not in (dtype if isinstance(dtype, tuple) else (dtype,)):
        return False
    if not t.is_cuda or (contiguous and not t.is_contiguous()):
        return False
    if dim is None:
        return t.numel() >= least
    return t.dim() == dim and tuple(t.shape[1:]) == tuple(tail) and t.shape[0] >= least


def _is_rays(t):
    """A float32 CUDA tensor [N, 8] of rt_ray rows."""
    return _is_tensor(t, torch.float32, 2, (8,))


def _is_hits(t, n):
    """A float32 CUDA tensor of at least n rt_hit rows [N, 12]."""
    return _is_tensor(t, torch.float32, 2, (12,), n)


def _is_history(t, w, h):
    return _is_tensor(t, torch.float32, least=w * h)


def _is_rng(t, count):
    """An int32 CUDA tensor of at least `count` RNG states (alloc_rng)."""
    return _is_tensor(t, torch.int32, least=count * (RNG_STATE_BYTES // 4))


def _is_surface(t, w, h, aligned=False):
    """A pitched float4 surface tensor (alloc_surface layout) of at least w x h; aligned: its pitch a multiple of 16 bytes."""
    return (t.dtype == torch.float32 and t.is_cuda and t.dim() == 2 and t.stride(1) == 1 and t.shape[0] >= h
            and t.shape[1] >= w * 4 and (not aligned or (t.stride(0) * 4) % 16 == 0))


def alloc_surface(width, height, device=None):
    """A pitched float4 surface (RGBA fp32), rows padded to a 256-byte pitch like cudaMallocPitch."""
    row_floats = ((width * 16 + 255) // 256) * 256 // 4
    return torch.zeros((height, row_floats), dtype=torch.float32, device=device or "cuda")


def surface_view(t, width):
    """[H, W, 4] view of a pitched surface tensor."""
    return t[:, : width * 4].reshape(t.shape[0], width, 4)


def alloc_rng(count, device=None):
    return torch.zeros((count * RNG_STATE_BYTES // 4,), dtype=torch.int32, device=device or "cuda")


def _materials_of(scene_or_materials):
    """(device pointer or None, count) of a Scene's, a GPUScene's or a float32 CUDA [M, 16] tensor's material table."""
    m = scene_or_materials
    if isinstance(m, torch.Tensor):
        assert _is_tensor(m, torch.float32, 2, (16,))
        return (m.data_ptr() if m.shape[0] else None), m.shape[0]
    gpu = m.gpu.contents if hasattr(m, "gpu") else m
    return gpu.gpu_materials, gpu.material_count


def _as_camera(camera):
    """A GPUCamera from a GPUCamera or 15 floats in its layout (origin, viewport size, aspect, horizontal,
    vertical, lower-left corner)."""
    if isinstance(camera, GPUCamera):
        return camera
    v = np.ascontiguousarray(camera, dtype=np.float32).reshape(-1)
    assert v.size == 15, "a camera is a GPUCamera or 15 floats"
    return GPUCamera.from_buffer_copy(v.tobytes())
