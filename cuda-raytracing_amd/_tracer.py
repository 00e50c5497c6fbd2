"""RayTracer: the reference's CUDARayTracer, headless, with the queries and filters as methods on its scene."""
import torch

from . import _image  # its denoise() is called through the module: upsampled() has an argument of that name
from ._abi import DENOISE_VARIANCE_DEFAULTS, HIT_MISS, REFERENCE_BOUNCES, REFERENCE_SPP, REPROJECT_DEFAULTS
from ._adaptive import AdaptiveSampler
from ._args import _allocating_on, alloc_rng, alloc_surface, surface_view
from ._image import TemporalAccumulator, VarianceAccumulator, upsample
from ._queries import ambient_occlusion, closest_points, gbuffer, hit_fields, panorama, trace_camera, trace_hits_camera
from ._render import init_rng_states, render, tonemap, write_pfm, write_ppm
from ._scene import Scene


class RayTracer:
    """CUDARayTracer mirror (RayTracing/RayTracing.{h,cpp}), headless.

    ``process()`` = one progressive frame: lazy RNG init (fixed seed instead of the
    reference's time-based one), camera update + upload, render, copy to the last-frame
    surface, frame_index++ (RayTracing.cpp:205-234).
    """

    def __init__(self, width, height, scene="bunny", spp=REFERENCE_SPP, bounces=REFERENCE_BOUNCES, seed=0xDEADBEEF):
        self.spp, self.bounces, self.seed = spp, bounces, seed
        self.scene = Scene()
        self.scene.setup(scene)
        self.on_resize(width, height)

    def on_resize(self, width, height):
        self.width, self.height = width, height
        self.surface = alloc_surface(width, height)
        self.last_frame = alloc_surface(width, height)
        self.rng = None
        self.frame_index = 0
        self._accumulator = None           # reprojected()'s TemporalAccumulator
        self._variance_accumulator = None  # filtered()'s VarianceAccumulator

    def _upload(self):
        """The scene at the current size on the device, with the RNG states if there are any yet."""
        self.scene.set_viewport(self.width, self.height)
        self.scene.upload(self.rng.data_ptr() if self.rng is not None else 0)

    def process(self, stats=None):
        if self.rng is None:
            self.rng = alloc_rng(self.width * self.height)
            init_rng_states(self.rng, self.width, self.height, self.seed)
        self._upload()
        render(self.scene, self.surface, self.last_frame, self.width, self.height, self.spp, self.bounces,
               frame_index=self.frame_index, stats=stats)
        self.last_frame.copy_(self.surface)
        self.frame_index += 1
        return surface_view(self.surface, self.width)

    def gbuffer(self, stream=None, waves_per_simd=0):
        """First-hit images of the current camera and size (module-level gbuffer()).  Uploads the scene
        like process(); the frame index, the surfaces and the RNG states are left alone."""
        self._upload()
        return gbuffer(self.scene, self.width, self.height, stream=stream, waves_per_simd=waves_per_simd)

    def denoised(self, **kw):
        """A denoised copy of the current frame as a new pitched surface (module-level denoise(); **kw are its
        filter parameters, hits, scratch, stream).  Uploads the scene like process(); `surface`, `last_frame`,
        the RNG states and the frame index are left alone."""
        assert "out" not in kw, "RayTracer.denoised returns a new surface"
        self._upload()
        return _image.denoise(self.scene, self.surface, self.width, self.height, **kw)

    def upsampled(self, scale=2, denoise=False, **kw):
        """The current frame as a new pitched surface of scale * width x scale * height pixels (module-level
        upsample(); **kw are its filter parameters, low_hits, hits, scratch, stream).  With denoise=True the frame
        goes through rt_denoise (its defaults) first.  Uploads the scene like process(); `surface`, `last_frame`, the
        RNG states and the frame index are left alone."""
        assert "out" not in kw, "RayTracer.upsampled returns a new surface"
        self._upload()
        stream = kw.get("stream")
        if kw.get("low_hits") is None:
            kw["low_hits"] = trace_camera(self.scene, self.width, self.height, stream=stream)
        low = self.surface
        if denoise:
            low = _image.denoise(self.scene, low, self.width, self.height, hits=kw["low_hits"], stream=stream)
        return upsample(self.scene, low, self.width, self.height, scale, **kw)

    def ao(self, radius, **kw):
        """The ambient-occlusion image [H, W] of the current camera and size (module-level ambient_occlusion();
        **kw are its samples, bias, directions, hits, stream, ...).  Uploads the scene like process(); the frame
        index, the surfaces and the RNG states are left alone."""
        self._upload()
        hits = kw.pop("hits", None)
        if hits is None:
            hits = trace_camera(self.scene, self.width, self.height, stream=kw.get("stream"))
        return ambient_occlusion(self.scene, hits, self.width, self.height, radius, **kw)

    def closest_points(self, points, **kw):
        """The nearest surface point of every row of a [N, 4] point tensor (module-level closest_points(); **kw are
        its out, waves_per_simd, stream).  Uploads the scene like process() and works before any frame is rendered;
        the frame index, the surfaces and the RNG states are left alone."""
        self._upload()
        return closest_points(self.scene, points, **kw)

    def layers(self, max_hits, flags=0, stream=None, waves_per_simd=0):
        """The first `max_hits` surfaces behind every pixel (trace_hits_camera: the pixel centres, no jitter) as device
        tensors, rows bottom to top like the surface: depth [H, W, K] (t; inf past the last hit), prim (sphere or face
        index, -1 past the last hit) and kind [H, W, K] int32, and count [H, W] int32 (the list length, or with
        RT_HITS_COUNT_ALL in `flags` every hit below tmax).  Uploads the scene like process(); the frame index, the
        surfaces and the RNG states are left alone."""
        self._upload()
        w, h, k = self.width, self.height, int(max_hits)
        hits, counts = trace_hits_camera(self.scene, w, h, k, flags=flags, stream=stream, waves_per_simd=waves_per_simd)
        with _allocating_on(stream):
            f = hit_fields(hits.reshape(w * h * k, 12))
            hit = f["kind"] != HIT_MISS
            return {"depth": torch.where(hit, f["t"], torch.full_like(f["t"], float("inf"))).reshape(h, w, k),
                    "prim": torch.where(hit, f["id"], torch.full_like(f["id"], -1)).reshape(h, w, k),
                    "kind": f["kind"].reshape(h, w, k).clone(), "count": counts.reshape(h, w)}

    def panorama(self, width, height, origin=None, samples=None, bounces=None, seed=None, stream=None):
        """A width x height equirectangular panorama of the scene seen from `origin` (default: the camera's position),
        as a new pitched surface (alloc_surface layout, rows bottom to top): radiance() along panorama_rays(), `samples`
        paths per pixel (default: spp), `bounces` (default: the tracer's), states ray_rng(width * height, seed) (default:
        the tracer's seed).  Uploads the scene like process(); the frame index, the surfaces and the tracer's RNG states
        are left alone."""
        self._upload()
        return panorama(self.scene, int(width), int(height), origin=origin, samples=self.spp if samples is None else samples,
                        bounces=self.bounces if bounces is None else bounces, seed=self.seed if seed is None else seed,
                        device=self.surface.device, stream=stream)

    def adaptive(self, rounds, budget_spp, warmup=2, bounces=None, seed=None, stream=None, **kw):
        """An adaptively sampled image of the current camera and size: a new AdaptiveSampler, warmup(`warmup`), then
        `rounds` steps of budget_spp samples per pixel each (**kw are step()'s min_samples, max_samples, scale).
        Returns the sampler: image() is the picture, counts() the samples per pixel.  Uploads the scene like
        process(); the frame index, the surfaces and the tracer's RNG states are left alone."""
        self._upload()
        sampler = AdaptiveSampler(self.scene, self.width, self.height, bounces=self.bounces if bounces is None else bounces,
                                  seed=self.seed if seed is None else seed, device=self.surface.device, stream=stream)
        sampler.warmup(warmup)
        for _ in range(int(rounds)):
            sampler.step(budget_spp, **kw)
        return sampler

    def reprojected(self, **kw):
        """The current frame accumulated with the frames of earlier calls, whatever cameras they had (a lazily
        created TemporalAccumulator; **kw are its filter parameters, and push's hits and stream).  Meant for frames
        rendered with frame_index == 0: set ``tracer.frame_index = 0`` after moving the camera, as the reference's
        Process() does on its dirty flag, then process(), then this.  Returns the accumulated surface, valid until
        the next-but-one call.  Uploads the scene like process(); `surface`, `last_frame`, the RNG states and the
        frame index are left alone.  on_resize drops the accumulator."""
        self._upload()
        push_kw = {k: kw.pop(k) for k in ("hits", "stream") if k in kw}
        if self._accumulator is None:
            self._accumulator = TemporalAccumulator(self.width, self.height)
        assert not set(kw) - set(REPROJECT_DEFAULTS), sorted(set(kw) - set(REPROJECT_DEFAULTS))
        self._accumulator.filter_params.update(kw)
        return self._accumulator.push(self.scene, self.surface, **push_kw)

    def filtered(self, **kw):
        """The current frame accumulated with the frames of earlier calls and filtered by rt_denoise_variance (a
        lazily created VarianceAccumulator, kept apart from reprojected()'s accumulator; **kw are its filter
        parameters, `reproject_params`, and push's hits and stream).  Meant for frames rendered with frame_index == 0,
        like reprojected().  Returns the filtered surface, valid until the next call; the accumulator itself
        (accumulated image, history, variance) is `tracer.variance_accumulator`.  Uploads the scene like process();
        `surface`, `last_frame`, the RNG states and the frame index are left alone.  on_resize drops the accumulator."""
        self._upload()
        push_kw = {k: kw.pop(k) for k in ("hits", "stream") if k in kw}
        reproject_params = kw.pop("reproject_params", None)
        acc = self._variance_accumulator
        if acc is None or (acc.width, acc.height) != (self.width, self.height):
            acc = self._variance_accumulator = VarianceAccumulator(self.width, self.height)
        assert not set(kw) - set(DENOISE_VARIANCE_DEFAULTS), sorted(set(kw) - set(DENOISE_VARIANCE_DEFAULTS))
        acc.filter_params.update(kw)
        acc.reproject_params.update(reproject_params or {})
        return acc.push(self.scene, self.surface, **push_kw)

    @property
    def variance_accumulator(self):
        """filtered()'s VarianceAccumulator (None before the first call and after on_resize)."""
        return self._variance_accumulator

    def save(self, path):
        """The current frame: ``.pfm`` linear RGB, ``.ppm`` as the reference's viewer shows it
        (exposure 0.5, ACES film, sRGB; main.cpp:78-94, 438)."""
        if str(path).lower().endswith(".pfm"):
            write_pfm(path, self.surface, self.width, self.height)
        elif str(path).lower().endswith(".ppm"):
            write_ppm(path, tonemap(self.surface, self.width, self.height))
        else:
            raise ValueError("RayTracer.save: .pfm or .ppm")

