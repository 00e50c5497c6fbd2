"""The image-space calls on a rendered frame and its first-hit records: rt_denoise, rt_reproject, rt_moments,
rt_denoise_variance, rt_upsample, and the accumulators that chain them from frame to frame."""
import numpy as np
import torch

from ._abi import (DENOISE_DEFAULT, DENOISE_VARIANCE_DEFAULTS, REPROJECT_DEFAULT, REPROJECT_DEFAULTS, UPSAMPLE_DEFAULT,
                   DenoiseParams, DenoiseVarianceParams, MomentsParams, ReprojectParams, UpsampleParams, lib)
from ._args import (_allocating_on, _as_camera, _given_or_new, _is_hits, _is_history, _is_surface, _launch, _materials_of,
                    _set_scratch, alloc_surface)
from ._queries import trace_camera


def denoise_scratch_bytes(width, height):
    """rt_denoise_scratch_bytes: bytes of scratch rt_denoise needs for a width x height frame."""
    return int(lib().rt_denoise_scratch_bytes(int(width), int(height)))


def _denoise(surface, hits, materials, width, height, out, scratch, iterations, normal_power_log2, sigma_plane, sigma_color,
             stream):
    w, h = int(width), int(height)
    assert _is_surface(surface, w, h) and _is_hits(hits, w * h)
    out = _given_or_new(out, stream, alloc_surface, w, h, device=surface.device)
    assert _is_surface(out, w, h)
    p = DenoiseParams(surface=surface.data_ptr(), pitch=surface.stride(0) * 4, width=w, height=h, hits=hits.data_ptr(),
                      out=out.data_ptr(), out_pitch=out.stride(0) * 4, iterations=int(iterations),
                      normal_power_log2=int(normal_power_log2), sigma_plane=float(sigma_plane), sigma_color=float(sigma_color))
    p.materials, p.material_count = _materials_of(materials)
    scratch = _set_scratch(p, scratch, stream, denoise_scratch_bytes(w, h), surface.device)
    _launch("rt_denoise", p, stream)
    return out


def denoise_raw(surface, hits, materials, width, height, out=None, scratch=None, iterations=DENOISE_DEFAULT,
                normal_power_log2=DENOISE_DEFAULT, sigma_plane=DENOISE_DEFAULT, sigma_color=DENOISE_DEFAULT, stream=None):
    """rt_denoise on tensors only: `surface` a pitched float4 surface (alloc_surface), `hits` a float32 [H*W, 12]
    tensor of rt_hit rows (record y*W + x, what trace_camera returns), `materials` a float32 CUDA tensor [M, 16]
    of GPUMaterial rows (M may be 0).  Returns `out` (a new surface when None; `out is surface` is allowed).
    `scratch`: any contiguous CUDA tensor of at least denoise_scratch_bytes(width, height) bytes, contents
    irrelevant (allocated when None).  A filter parameter left at DENOISE_DEFAULT takes the library's default
    (DENOISE_DEFAULTS).  Stream-ordered on `stream` (default: torch's current stream); tensors allocated here are
    allocated on that stream, tensors passed in must be safe to use on it."""
    assert isinstance(materials, torch.Tensor)
    return _denoise(surface, hits, materials, width, height, out, scratch, iterations, normal_power_log2, sigma_plane,
                    sigma_color, stream)


def denoise(scene, surface, width, height, hits=None, out=None, scratch=None, iterations=DENOISE_DEFAULT,
            normal_power_log2=DENOISE_DEFAULT, sigma_plane=DENOISE_DEFAULT, sigma_color=DENOISE_DEFAULT, stream=None):
    """A viewable image from one low-sample frame of an uploaded Scene: rt_denoise guided by the camera's
    first-hit records (`hits`, or trace_camera(scene, width, height) when None) and the scene's materials.
    Returns `out` (a new surface when None).  Do not pass the tracer's last-frame surface as `out`: the
    progressive accumulation would then average filtered colours."""
    if hits is None:
        hits = trace_camera(scene, width, height, stream=stream)
    return _denoise(surface, hits, scene, width, height, out, scratch, iterations, normal_power_log2, sigma_plane,
                    sigma_color, stream)


def camera_floats(camera):
    """The 15 floats of a GPUCamera as a numpy float32 array."""
    return np.frombuffer(bytes(_as_camera(camera)), dtype=np.float32).copy()


def reproject_raw(surface, hits, camera, width, height, prev=None, out=None, out_history=None,
                  max_history=REPROJECT_DEFAULT, sigma_plane=REPROJECT_DEFAULT, normal_min=REPROJECT_DEFAULT, stream=None):
    """rt_reproject on tensors only: `surface` a pitched float4 surface holding a frame rendered with frame_index 0,
    `hits` the float32 [H*W, 12] records of trace_camera for `camera` (a GPUCamera, as Scene.camera() returns it after
    the upload, or its 15 floats).  `prev` = (prev_surface, prev_hits, prev_history, prev_camera): what the previous
    call returned and was given; None on the first frame.  Returns (out, out_history): the accumulated surface and
    the float32 [H, W] number of frames it holds per pixel (new tensors when None; `out is surface` is allowed,
    `out is prev_surface` is not).  A filter parameter left at REPROJECT_DEFAULT takes the library's default
    (REPROJECT_DEFAULTS).  Stream-ordered on `stream` (default: torch's current stream); tensors allocated here are
    allocated on that stream, tensors passed in must be safe to use on it."""
    w, h = int(width), int(height)
    assert _is_surface(surface, w, h) and _is_hits(hits, w * h)
    out = _given_or_new(out, stream, alloc_surface, w, h, device=surface.device)
    out_history = _given_or_new(out_history, stream, torch.zeros, (h, w), dtype=torch.float32, device=surface.device)
    assert _is_surface(out, w, h) and _is_history(out_history, w, h)
    p = ReprojectParams(surface=surface.data_ptr(), pitch=surface.stride(0) * 4, hits=hits.data_ptr(), out=out.data_ptr(),
                        out_pitch=out.stride(0) * 4, out_history=out_history.data_ptr(), camera=_as_camera(camera),
                        width=w, height=h, max_history=int(max_history), sigma_plane=float(sigma_plane),
                        normal_min=float(normal_min))
    if prev is not None:
        prev_surface, prev_hits, prev_history, prev_camera = prev
        assert _is_surface(prev_surface, w, h) and _is_hits(prev_hits, w * h) and _is_history(prev_history, w, h)
        p.prev_surface, p.prev_pitch = prev_surface.data_ptr(), prev_surface.stride(0) * 4
        p.prev_hits, p.prev_history = prev_hits.data_ptr(), prev_history.data_ptr()
        p.prev_camera = _as_camera(prev_camera)
    _launch("rt_reproject", p, stream)
    return out, out_history


class TemporalAccumulator:
    """Temporal accumulation of a moving camera's frames (rt_reproject): two accumulated surfaces, two histories
    and two hit buffers used in turn, plus the previous camera.  **filter_params are reproject_raw's max_history,
    sigma_plane and normal_min.  Static geometry only."""

    def __init__(self, width, height, **filter_params):
        assert not set(filter_params) - set(REPROJECT_DEFAULTS), sorted(set(filter_params) - set(REPROJECT_DEFAULTS))
        self.width, self.height = int(width), int(height)
        self.filter_params = dict(filter_params)
        self._slots = [None, None]  # (surface, hits, history), allocated at first use
        self.reset()

    def reset(self):
        """Forget the history: the next push starts a new accumulation."""
        self._latest = None  # index of the slot the last push wrote
        self._camera = None

    def push(self, scene, surface, hits=None, stream=None):
        """Accumulate `surface`, a frame of the uploaded `scene`'s current camera rendered with frame_index 0; `hits`:
        that camera's trace_camera records (traced here when None).  Returns the accumulated surface, which stays
        valid until the next-but-one push."""
        w, h = self.width, self.height
        camera = scene.camera()
        k = 0 if self._latest is None else 1 - self._latest
        with _allocating_on(stream):
            if self._slots[k] is None:
                self._slots[k] = (alloc_surface(w, h, device=surface.device),
                                  torch.empty((w * h, 12), dtype=torch.float32, device=surface.device),
                                  torch.zeros((h, w), dtype=torch.float32, device=surface.device))
            out, own_hits, history = self._slots[k]
            if hits is None:
                trace_camera(scene, w, h, hits=own_hits, stream=stream)
            else:
                assert _is_hits(hits, w * h)
                own_hits.copy_(hits[: w * h])
        prev = None if self._latest is None else (*self._slots[self._latest], self._camera)
        reproject_raw(surface, own_hits, camera, w, h, prev=prev, out=out, out_history=history, stream=stream,
                      **self.filter_params)
        self._latest, self._camera = k, camera
        return out

    @property
    def history(self):
        """[H, W] view of the latest history: the number of frames the latest accumulated surface holds per pixel
        (None before the first push)."""
        return None if self._latest is None else self._slots[self._latest][2]


def moments(scene_or_materials, surface, hits, width, height, out=None, stream=None):
    """rt_moments: the luminance moments (l, l*l, 0, alpha) of one frame, `surface`, divided by its first hits'
    albedo, as a pitched float4 surface -- what a second rt_reproject accumulates for rt_denoise_variance.
    `scene_or_materials`: an uploaded Scene (or GPUScene), or a float32 CUDA tensor [M, 16] of GPUMaterial rows.
    Returns `out` (a new surface when None; `out is surface` is refused).  Stream-ordered on `stream` (default:
    torch's current stream); a surface allocated here is allocated on that stream."""
    w, h = int(width), int(height)
    assert _is_surface(surface, w, h) and _is_hits(hits, w * h)
    out = _given_or_new(out, stream, alloc_surface, w, h, device=surface.device)
    assert _is_surface(out, w, h)
    p = MomentsParams(surface=surface.data_ptr(), pitch=surface.stride(0) * 4, width=w, height=h, hits=hits.data_ptr(),
                      out=out.data_ptr(), out_pitch=out.stride(0) * 4)
    p.materials, p.material_count = _materials_of(scene_or_materials)
    _launch("rt_moments", p, stream)
    return out


def denoise_variance_scratch_bytes(width, height):
    """rt_denoise_variance_scratch_bytes: bytes of scratch rt_denoise_variance needs for a width x height frame."""
    return int(lib().rt_denoise_variance_scratch_bytes(int(width), int(height)))


def _denoise_variance(surface, hits, materials, width, height, moments, history, out, out_variance, scratch, iterations,
                      normal_power_log2, sigma_plane, sigma_lum, min_history, stream):
    w, h = int(width), int(height)
    assert _is_surface(surface, w, h) and _is_hits(hits, w * h)
    assert (moments is None or _is_surface(moments, w, h)) and (history is None or _is_history(history, w, h))
    out = _given_or_new(out, stream, alloc_surface, w, h, device=surface.device)
    out_variance = _given_or_new(out_variance, stream, torch.zeros, (h, w), dtype=torch.float32, device=surface.device)
    assert _is_surface(out, w, h) and _is_history(out_variance, w, h)
    p = DenoiseVarianceParams(surface=surface.data_ptr(), pitch=surface.stride(0) * 4, width=w, height=h,
                              hits=hits.data_ptr(), out=out.data_ptr(), out_pitch=out.stride(0) * 4,
                              out_variance=out_variance.data_ptr(), iterations=int(iterations),
                              normal_power_log2=int(normal_power_log2), sigma_plane=float(sigma_plane),
                              sigma_lum=float(sigma_lum), min_history=float(min_history))
    p.materials, p.material_count = _materials_of(materials)
    if moments is not None:
        p.moments, p.moments_pitch = moments.data_ptr(), moments.stride(0) * 4
    if history is not None:
        p.history = history.data_ptr()
    scratch = _set_scratch(p, scratch, stream, denoise_variance_scratch_bytes(w, h), surface.device)
    _launch("rt_denoise_variance", p, stream)
    return out, out_variance


def denoise_variance_raw(surface, hits, materials, width, height, moments=None, history=None, out=None, out_variance=None,
                         scratch=None, iterations=DENOISE_DEFAULT, normal_power_log2=DENOISE_DEFAULT,
                         sigma_plane=DENOISE_DEFAULT, sigma_lum=DENOISE_DEFAULT, min_history=DENOISE_DEFAULT, stream=None):
    """rt_denoise_variance on tensors only: `surface` the accumulated image (a pitched float4 surface), `hits` the
    float32 [H*W, 12] records of trace_camera, `materials` a float32 CUDA tensor [M, 16] of GPUMaterial rows (M may
    be 0), `moments` the accumulated moments surface (moments() through reproject_raw) and `history` the colour's
    float32 [H, W] history, either or both None.  Returns (out, out_variance): the filtered surface (`out is surface`
    is allowed) and the float32 [H, W] filtered variance of the albedo-divided luminance (new tensors when None).
    `scratch`: any contiguous CUDA tensor of at least denoise_variance_scratch_bytes(width, height) bytes.  A filter
    parameter left at DENOISE_DEFAULT takes the library's default (DENOISE_VARIANCE_DEFAULTS).  Stream-ordered on
    `stream` (default: torch's current stream); tensors allocated here are allocated on that stream, tensors passed
    in must be safe to use on it."""
    assert isinstance(materials, torch.Tensor)
    return _denoise_variance(surface, hits, materials, width, height, moments, history, out, out_variance, scratch,
                             iterations, normal_power_log2, sigma_plane, sigma_lum, min_history, stream)


def denoise_variance(scene, surface, width, height, hits=None, moments=None, history=None, out=None, out_variance=None,
                     scratch=None, iterations=DENOISE_DEFAULT, normal_power_log2=DENOISE_DEFAULT,
                     sigma_plane=DENOISE_DEFAULT, sigma_lum=DENOISE_DEFAULT, min_history=DENOISE_DEFAULT, stream=None):
    """rt_denoise_variance for an uploaded Scene: guided by the camera's first-hit records (`hits`, or
    trace_camera(scene, width, height) when None) and the scene's materials; otherwise denoise_variance_raw.  Feed it
    the accumulated image with the history and moments that belong to it (VarianceAccumulator does all of it)."""
    if hits is None:
        hits = trace_camera(scene, width, height, stream=stream)
    return _denoise_variance(surface, hits, scene, width, height, moments, history, out, out_variance, scratch,
                             iterations, normal_power_log2, sigma_plane, sigma_lum, min_history, stream)


def upsample_scratch_bytes(low_width, low_height):
    """rt_upsample_scratch_bytes: bytes of scratch rt_upsample needs for a low frame of low_width x low_height pixels."""
    return int(lib().rt_upsample_scratch_bytes(int(low_width), int(low_height)))


def _upsample(low_surface, low_hits, hits, materials, low_width, low_height, scale, out, scratch, normal_power_log2,
              sigma_plane, stream):
    lw, lh, s = int(low_width), int(low_height), int(scale)
    w, h = lw * s, lh * s
    assert _is_surface(low_surface, lw, lh) and _is_hits(low_hits, lw * lh) and _is_hits(hits, w * h)
    out = _given_or_new(out, stream, alloc_surface, w, h, device=low_surface.device)
    assert _is_surface(out, w, h)
    p = UpsampleParams(low_surface=low_surface.data_ptr(), low_pitch=low_surface.stride(0) * 4, low_hits=low_hits.data_ptr(),
                       hits=hits.data_ptr(), low_width=lw, low_height=lh, scale=s, out=out.data_ptr(),
                       out_pitch=out.stride(0) * 4, normal_power_log2=int(normal_power_log2), sigma_plane=float(sigma_plane))
    p.materials, p.material_count = _materials_of(materials)
    scratch = _set_scratch(p, scratch, stream, upsample_scratch_bytes(lw, lh), low_surface.device)
    _launch("rt_upsample", p, stream)
    return out


def upsample_raw(low_surface, low_hits, hits, materials, low_width, low_height, scale, out=None, scratch=None,
                 normal_power_log2=UPSAMPLE_DEFAULT, sigma_plane=UPSAMPLE_DEFAULT, stream=None):
    """rt_upsample on tensors only: `low_surface` a pitched float4 surface of low_width x low_height pixels, `low_hits`
    and `hits` float32 [N, 12] tensors of rt_hit rows of one camera at the low size and at the output size
    (scale * low_width x scale * low_height; scale 2, 3 or 4), `materials` a float32 CUDA tensor [M, 16] of
    GPUMaterial rows (M may be 0).  Returns `out`, a surface of the output size (a new one when None; it may overlap
    none of the inputs).  `scratch`: any contiguous CUDA tensor of at least upsample_scratch_bytes(low_width,
    low_height) bytes, contents irrelevant (allocated when None).  A filter parameter left at UPSAMPLE_DEFAULT takes
    the library's default (UPSAMPLE_DEFAULTS).  Stream-ordered on `stream` (default: torch's current stream); tensors
    allocated here are allocated on that stream, tensors passed in must be safe to use on it."""
    assert isinstance(materials, torch.Tensor)
    return _upsample(low_surface, low_hits, hits, materials, low_width, low_height, scale, out, scratch,
                     normal_power_log2, sigma_plane, stream)


def upsample(scene, low_surface, low_width, low_height, scale, low_hits=None, hits=None, out=None, scratch=None,
             normal_power_log2=UPSAMPLE_DEFAULT, sigma_plane=UPSAMPLE_DEFAULT, stream=None):
    """A frame of scale * low_width x scale * low_height pixels from a frame of an uploaded Scene rendered at low_width x
    low_height: rt_upsample guided by the camera's first-hit records at both sizes (`low_hits`, `hits`; each traced
    with trace_camera on the call's stream when None -- the uploaded camera serves both sizes, its aspect being the
    same) and the scene's materials.  Returns `out` (a new surface when None)."""
    lw, lh, s = int(low_width), int(low_height), int(scale)
    if low_hits is None:
        low_hits = trace_camera(scene, lw, lh, stream=stream)
    if hits is None:
        hits = trace_camera(scene, lw * s, lh * s, stream=stream)
    return _upsample(low_surface, low_hits, hits, scene, lw, lh, s, out, scratch, normal_power_log2, sigma_plane, stream)


class VarianceAccumulator:
    """The per-frame chain of the variance-steered filter: rt_reproject on the colour (a TemporalAccumulator),
    rt_moments on the new frame, rt_reproject on the moments with a history of their own, rt_denoise_variance on
    the accumulated image.  **filter_params are denoise_variance_raw's iterations, normal_power_log2, sigma_plane,
    sigma_lum and min_history; `reproject_params` (a dict) are reproject_raw's max_history, sigma_plane and
    normal_min, used for both reprojections.  Static geometry only."""

    def __init__(self, width, height, reproject_params=None, **filter_params):
        unknown = set(filter_params) - set(DENOISE_VARIANCE_DEFAULTS)
        assert not unknown, sorted(unknown)
        self.width, self.height = int(width), int(height)
        self.filter_params = dict(filter_params)
        self._colour = TemporalAccumulator(width, height, **(reproject_params or {}))
        self._moment_slots = [None, None]  # (accumulated moments, their history)
        self._buffers = None               # (moments of the frame, filtered image, variance, scratch)
        self.reset()

    @property
    def reproject_params(self):
        return self._colour.filter_params

    def reset(self):
        """Forget the history: the next push starts a new accumulation."""
        self._colour.reset()
        self._pushed = False

    def push(self, scene, surface, hits=None, stream=None):
        """Accumulate `surface`, a frame of the uploaded `scene`'s current camera rendered with frame_index 0, and
        filter the accumulated image; `hits`: that camera's trace_camera records (traced here when None).  Returns
        the filtered surface, valid until the next push."""
        w, h = self.width, self.height
        before, prev_camera = self._colour._latest, self._colour._camera
        accumulated = self._colour.push(scene, surface, hits=hits, stream=stream)
        k = self._colour._latest
        _, own_hits, history = self._colour._slots[k]
        with _allocating_on(stream):
            if self._moment_slots[k] is None:
                self._moment_slots[k] = (alloc_surface(w, h, device=surface.device),
                                         torch.zeros((h, w), dtype=torch.float32, device=surface.device))
            if self._buffers is None:
                self._buffers = (alloc_surface(w, h, device=surface.device), alloc_surface(w, h, device=surface.device),
                                 torch.zeros((h, w), dtype=torch.float32, device=surface.device),
                                 torch.empty((denoise_variance_scratch_bytes(w, h) // 4,), dtype=torch.float32,
                                             device=surface.device))
        frame_moments, filtered, variance, scratch = self._buffers
        moments(scene, surface, own_hits, w, h, out=frame_moments, stream=stream)
        prev = None if before is None else (self._moment_slots[before][0], self._colour._slots[before][1],
                                            self._moment_slots[before][1], prev_camera)
        acc_moments, moments_history = self._moment_slots[k]
        reproject_raw(frame_moments, own_hits, self._colour._camera, w, h, prev=prev, out=acc_moments,
                      out_history=moments_history, stream=stream, **self._colour.filter_params)
        _denoise_variance(accumulated, own_hits, scene, w, h, acc_moments, history, filtered, variance, scratch,
                          stream=stream, **{**{k_: DENOISE_DEFAULT for k_ in DENOISE_VARIANCE_DEFAULTS}, **self.filter_params})
        self._pushed = True
        return filtered

    @property
    def accumulated(self):
        """The latest accumulated (unfiltered) surface (None before the first push)."""
        return None if not self._pushed else self._colour._slots[self._colour._latest][0]

    @property
    def history(self):
        """[H, W]: the number of frames the accumulated surface holds per pixel (None before the first push)."""
        return None if not self._pushed else self._colour.history

    @property
    def moments(self):
        """The latest accumulated moments surface (None before the first push)."""
        return None if not self._pushed else self._moment_slots[self._colour._latest][0]

    @property
    def variance(self):
        """[H, W]: the filtered variance of the albedo-divided luminance of the latest filtered image (None before
        the first push)."""
        return None if not self._pushed else self._buffers[2]
