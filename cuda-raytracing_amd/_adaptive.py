"""Adaptive sampling: rt_sample_pixels / rt_sample_priority / rt_sample_plan / rt_sample_resolve and the
AdaptiveSampler that runs them round after round.  Its surfaces need a pitch that is a multiple of 16 bytes."""
import torch

from ._abi import (REFERENCE_BOUNCES, SAMPLE_SCALE_DEFAULT, SamplePixelsParams, SamplePlanParams, SamplePriorityParams,
                   SampleResolveParams, lib)
from ._args import (_INT16S, _allocating_on, _given_or_new, _is_rng, _is_surface, _is_tensor, _launch, _set_scratch,
                    alloc_rng, alloc_surface, surface_view)
from ._render import init_rng_states


def sample_pixels(scene, width, height, samples, rng, accum, pixels=None, moments=None, bounces=REFERENCE_BOUNCES,
                  stream=None, waves_per_simd=0):
    """rt_sample_pixels: samples[i] more of the renderer's samples for pixel pixels[i] (= y * width + x; None: entry i
    is pixel i) of the uploaded Scene's camera, added to the undivided accumulator `accum` (a pitched surface: sum of
    rgb, sample count), to `moments` (float32 [H*W, 2], optional) and the pixel's state in `rng` (H*W states in the
    renderer's layout).  `samples`: int16 / uint16 CUDA tensor (read as uint16), one entry each; `pixels`: int32.
    Stream-ordered on `stream` (default: torch's current stream)."""
    w, h = int(width), int(height)
    assert _is_tensor(samples, _INT16S)
    n = samples.numel()
    assert _is_rng(rng, w * h) and _is_surface(accum, w, h, aligned=True)
    p = SamplePixelsParams()
    if pixels is not None:
        assert _is_tensor(pixels, torch.int32, least=n)
        p.pixels = pixels.data_ptr() if n else None
    if moments is not None:
        assert _is_tensor(moments, torch.float32, least=2 * w * h)
        p.moments = moments.data_ptr()
    if n == 0:  # rt_sample_pixels returns at once for count 0; an empty tensor has no address to pass
        return accum
    p.samples, p.count, p.rng = samples.data_ptr(), n, rng.data_ptr()
    p.accum, p.accum_pitch = accum.data_ptr(), accum.stride(0) * 4
    p.width, p.height, p.bounces, p.waves_per_simd = w, h, int(bounces), int(waves_per_simd)
    _launch("rt_sample_pixels", p, stream, scene)
    return accum


def sample_priority(accum, moments, width, height, out=None, stream=None):
    """rt_sample_priority: float32 [H*W] priorities (`out`, or a new tensor) from an accumulator and its moments: the
    relative variance of the mean, +inf where fewer than two samples are known."""
    w, h = int(width), int(height)
    assert _is_surface(accum, w, h, aligned=True) and _is_tensor(moments, torch.float32, least=2 * w * h)
    out = _given_or_new(out, stream, torch.empty, (w * h,), dtype=torch.float32, device=accum.device)
    assert _is_tensor(out, torch.float32, least=w * h)
    p = SamplePriorityParams(accum=accum.data_ptr(), accum_pitch=accum.stride(0) * 4, moments=moments.data_ptr(),
                             priority=out.data_ptr(), width=w, height=h)
    _launch("rt_sample_priority", p, stream)
    return out


def sample_plan_scratch_bytes(width, height):
    """rt_sample_plan_scratch_bytes (needs no GPU)."""
    return int(lib().rt_sample_plan_scratch_bytes(int(width), int(height)))


def sample_plan(priority, width, height, budget, min_samples=0, max_samples=64, scale=SAMPLE_SCALE_DEFAULT, pixels=None,
                samples=None, total=None, scratch=None, stream=None):
    """rt_sample_plan: the list of the next round from float32 [H*W] priorities and a total `budget` of samples.
    Returns (pixels int32 [H*W], samples int16 [H*W] holding uint16 counts, total int64 [1]): every pixel once, sorted
    by count descending, 8x8 sub-tile order inside a count.  Tensors not given are allocated on `stream`."""
    w, h = int(width), int(height)
    n = w * h
    assert _is_tensor(priority, torch.float32, least=n)
    device = priority.device
    pixels = _given_or_new(pixels, stream, torch.empty, (n,), dtype=torch.int32, device=device)
    samples = _given_or_new(samples, stream, torch.empty, (n,), dtype=torch.int16, device=device)
    total = _given_or_new(total, stream, torch.empty, (1,), dtype=torch.int64, device=device)
    assert _is_tensor(pixels, torch.int32, least=n) and _is_tensor(samples, _INT16S, least=n)
    assert _is_tensor(total, torch.int64, least=1, contiguous=False)
    p = SamplePlanParams(priority=priority.data_ptr(), width=w, height=h, budget=int(budget), min_samples=int(min_samples),
                         max_samples=int(max_samples), scale=float(scale), pixels=pixels.data_ptr(),
                         samples=samples.data_ptr(), total=total.data_ptr())
    scratch = _set_scratch(p, scratch, stream, sample_plan_scratch_bytes(w, h), device, check_size=True)
    _launch("rt_sample_plan", p, stream)
    return pixels, samples, total


def sample_resolve(accum, width, height, out=None, stream=None):
    """rt_sample_resolve: the mean image of an accumulator as a pitched surface (`out`, or a new one): rgb / count where
    count >= 1, else 0; alpha 1."""
    w, h = int(width), int(height)
    assert _is_surface(accum, w, h, aligned=True)
    out = _given_or_new(out, stream, alloc_surface, w, h, device=accum.device)
    assert _is_surface(out, w, h, aligned=True)
    p = SampleResolveParams(accum=accum.data_ptr(), accum_pitch=accum.stride(0) * 4, out=out.data_ptr(),
                            out_pitch=out.stride(0) * 4, width=w, height=h)
    _launch("rt_sample_resolve", p, stream)
    return out


class AdaptiveSampler:
    """Adaptive sampling of an uploaded Scene's camera at width x height (the scene's viewport): it owns the states
    (rt_init_rng(seed), the renderer's own), the undivided accumulator, the luminance moments, the list of the current
    round and the planner's scratch.  warmup(spp) gives every pixel spp samples; step(budget_spp) spends
    budget_spp * width * height samples where the relative variance of the mean is largest.  Every pixel always holds
    exactly what the renderer's first counts()[y, x] samples of that pixel sum to (rt_abi.h).  Everything runs on
    `stream` (default: torch's current stream at each call) without synchronisation."""

    def __init__(self, scene, width, height, bounces=REFERENCE_BOUNCES, seed=0xDEADBEEF, device=None, stream=None):
        self.scene, self.width, self.height, self.bounces, self.seed = scene, int(width), int(height), int(bounces), seed
        self.stream = stream
        n = self.width * self.height
        with _allocating_on(stream):
            self.rng = alloc_rng(n, device=device)
            self.accum = alloc_surface(self.width, self.height, device=self.rng.device)
            self.moments = torch.zeros((n, 2), dtype=torch.float32, device=self.rng.device)
            self.priority = torch.empty((n,), dtype=torch.float32, device=self.rng.device)
            self.pixels = torch.empty((n,), dtype=torch.int32, device=self.rng.device)
            self.samples = torch.empty((n,), dtype=torch.int16, device=self.rng.device)
            self.total = torch.zeros((1,), dtype=torch.int64, device=self.rng.device)
            self.scratch = torch.empty((sample_plan_scratch_bytes(self.width, self.height),), dtype=torch.uint8,
                                       device=self.rng.device)
        self.reset()

    def reset(self):
        """Forget every sample: zero accumulator and moments, the states of sample 0."""
        with _allocating_on(self.stream):
            self.accum.zero_()
            self.moments.zero_()
        init_rng_states(self.rng, self.width, self.height, self.seed, stream=self.stream)

    def warmup(self, spp):
        """A uniform round: spp samples for every pixel (pixels=None)."""
        with _allocating_on(self.stream):
            self.samples.fill_(int(spp))
        sample_pixels(self.scene, self.width, self.height, self.samples, self.rng, self.accum, moments=self.moments,
                      bounces=self.bounces, stream=self.stream)

    def step(self, budget_spp, min_samples=0, max_samples=64, scale=SAMPLE_SCALE_DEFAULT):
        """One adaptive round of at most budget_spp * width * height samples: priority, plan, sample.  `total`
        (device int64 [1]) then holds the samples the round spent."""
        budget = int(round(float(budget_spp) * self.width * self.height))
        sample_priority(self.accum, self.moments, self.width, self.height, out=self.priority, stream=self.stream)
        sample_plan(self.priority, self.width, self.height, budget, min_samples=min_samples, max_samples=max_samples,
                    scale=scale, pixels=self.pixels, samples=self.samples, total=self.total, scratch=self.scratch,
                    stream=self.stream)
        sample_pixels(self.scene, self.width, self.height, self.samples, self.rng, self.accum, pixels=self.pixels,
                      moments=self.moments, bounces=self.bounces, stream=self.stream)

    def image(self, out=None):
        """The mean image as a pitched surface (rt_sample_resolve)."""
        return sample_resolve(self.accum, self.width, self.height, out=out, stream=self.stream)

    def counts(self):
        """Samples per pixel so far: float32 [H, W], a view of the accumulator's alpha."""
        return surface_view(self.accum, self.width)[..., 3]
