"""ctypes face of lib/libfjgpu.so (include/fjgpu.h): the HIP core."""
import ctypes as C

import numpy as np

from . import ffi

_lib = None


class GpuError(RuntimeError):
    pass


def lib():
    global _lib
    if _lib is None:
        L = ffi.load("libfjgpu.so")
        L.fjgpu_last_error.restype = C.c_char_p
        L.fjgpu_device_count.restype = C.c_int
        L.fjgpu_scene_create.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
        L.fjgpu_scene_destroy.argtypes = [C.c_void_p]
        L.fjgpu_scene_destroy.restype = None
        L.fjgpu_tile_count.argtypes = [C.POINTER(ffi.RenderDesc)]
        L.fjgpu_tile_rect.argtypes = [C.POINTER(ffi.RenderDesc), C.c_int, C.POINTER(C.c_int32)]
        L.fjgpu_render_tiles.argtypes = [C.c_void_p, C.POINTER(ffi.RenderDesc), C.c_void_p, C.c_int,
                                         C.c_void_p, C.c_void_p, C.POINTER(ffi.GpuStats)]
        L.fjgpu_render_tiles_variance.argtypes = ffi.RENDER_TILES_VARIANCE_ARGTYPES
        L.fjgpu_render_frame.argtypes = [C.c_void_p, C.POINTER(ffi.RenderDesc), C.c_void_p, C.POINTER(ffi.GpuStats)]
        L.fjgpu_trace.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.POINTER(ffi.GpuStats)]
        L.fjgpu_scene_create_multi.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_void_p)]
        L.fjgpu_render_frame_multi.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.POINTER(ffi.RenderDesc), C.c_void_p, C.c_int,
                                               C.c_void_p, C.POINTER(ffi.GpuStats)]
        L.fjgpu_pack_tiles.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.fjgpu_unpack_tiles.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.fjgpu_render_aov.argtypes = [C.c_void_p, C.POINTER(ffi.RenderDesc), C.c_void_p, C.c_int, C.POINTER(ffi.AovBuffers),
                                       C.c_void_p, C.POINTER(ffi.GpuStats)]
        L.fjgpu_render_aov_albedo.argtypes = [C.c_void_p, C.POINTER(ffi.RenderDesc), C.c_void_p, C.c_int, C.POINTER(ffi.AovBuffers),
                                              C.c_void_p, C.c_void_p, C.POINTER(ffi.GpuStats)]
        L.fjgpu_render_aov_matte.argtypes = ffi.RENDER_AOV_MATTE_ARGTYPES
        L.fjgpu_denoise_albedo.argtypes = [C.c_int, C.POINTER(ffi.DenoiseDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_float, C.c_void_p, C.c_void_p, C.POINTER(ffi.GpuStats)]
        L.fjgpu_denoise.argtypes = [C.c_int, C.POINTER(ffi.DenoiseDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.POINTER(ffi.GpuStats)]
        L.fjgpu_denoise_estimate_variance.argtypes = [C.c_int, C.POINTER(ffi.DenoiseDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                      C.c_void_p, C.c_void_p, C.POINTER(ffi.GpuStats)]
        L.fjgpu_denoise_variance.argtypes = [C.c_int, C.POINTER(ffi.DenoiseDesc), C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(ffi.GpuStats)]
        L.fjgpu_denoise_estimate_variance_albedo.argtypes = [C.c_int, C.POINTER(ffi.DenoiseDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                             C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.POINTER(ffi.GpuStats)]
        L.fjgpu_scene_get_camera.argtypes = [C.c_void_p, C.POINTER(ffi.CameraDesc)]
        L.fjgpu_scene_set_camera.argtypes = [C.c_void_p, C.POINTER(ffi.CameraDesc)]
        L.fjgpu_scene_view.argtypes = [C.c_void_p, C.POINTER(ffi.RenderDesc), C.POINTER(ffi.View)]
        L.fjgpu_denoise_temporal.argtypes = [C.c_int, C.POINTER(ffi.TemporalDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.POINTER(ffi.View), C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.POINTER(ffi.TemporalHistory), C.POINTER(ffi.TemporalHistory), C.c_void_p, C.c_void_p,
                                             C.POINTER(ffi.GpuStats)]
        _tp = list(L.fjgpu_denoise_temporal.argtypes)          # the clamp goes behind the description
        L.fjgpu_denoise_temporal_clamped.argtypes = _tp[:2] + [C.POINTER(ffi.TemporalClamp)] + _tp[2:]
        L.fjgpu_accumulate.argtypes = ffi.ACCUMULATE_ARGTYPES
        L.fjgpu_accumulate_tile_error.argtypes = ffi.ACCUMULATE_TILE_ERROR_ARGTYPES
        L.fjgpu_host_xorshift_f01_seeded.argtypes = [C.c_uint, C.c_int, C.c_void_p]
        L.fjgpu_host_xorshift_f01_seeded.restype = None
        L.fjgpu_host_seeded_tile_id.argtypes = [C.c_uint, C.c_int32]
        L.fjgpu_host_seeded_tile_id.restype = C.c_int32
        L.fjgpu_camera_samples.argtypes = [C.c_void_p, C.POINTER(ffi.RenderDesc), C.c_int, C.c_void_p, C.c_int]
        L.fjgpu_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_long]
        L.fjgpu_global_option.argtypes = [C.c_char_p, C.c_long]
        L.fjgpu_scene_query.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_double)]
        L.fjgpu_build_config.argtypes = [C.c_char_p, C.POINTER(C.c_double)]
        L.fjgpu_dev_rccl_selftest.argtypes = [C.c_int, C.c_int]
        L.fjgpu_dev_sort_pairs.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_double)]
        L.fjgpu_dev_slab32_batch.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.fjgpu_dev_quantize_nodes.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib = L
    return _lib


def _check(rc):
    if rc != 0:
        raise GpuError("fjgpu error %d: %s" % (rc, lib().fjgpu_last_error().decode("utf-8", "replace")))


def device_count():
    return lib().fjgpu_device_count()


AOV_NAMES = ("depth", "position", "normal", "uv", "ids", "coverage")       # the members of fjgpu_aov_buffers
AOV_ALL = AOV_NAMES + ("albedo",)                                           # ... and the buffer of fjgpu_render_aov_albedo (Scene.render_aov_albedo)
AOV_CHANNELS = {"depth": 1, "position": 3, "normal": 3, "uv": 2, "ids": 4, "coverage": 1, "albedo": 3}


MATTE_NAMES = ("ids", "coverage", "rest", "distinct")                      # the members of fjgpu_matte_buffers


def matte_select(ids, coverage, keys):
    """One matte out of the ranked ones (Scene.render_matte / Scene._render_matte_device): ids, coverage [H, W, ranks] (numpy arrays or
    torch tensors) and the keys that make up the object -> [H, W] float32 of the same kind: per pixel the sum, rank by rank, of the
    coverage of the ranks whose id is in `keys`.  Plumbing, no kernel."""
    keys = [int(k) for k in np.atleast_1d(keys)]
    if isinstance(ids, np.ndarray):
        sel = np.isin(ids, np.asarray(keys, dtype=ids.dtype))
        out = np.zeros(ids.shape[:2], dtype=np.float32)
        for r in range(ids.shape[2]):
            out += np.where(sel[:, :, r], coverage[:, :, r], np.float32(0))
        return out
    import torch
    sel = torch.isin(ids, torch.tensor(keys, dtype=ids.dtype, device=ids.device))
    out = torch.zeros(ids.shape[:2], dtype=torch.float32, device=ids.device)
    for r in range(ids.shape[2]):
        out += torch.where(sel[:, :, r], coverage[:, :, r], torch.zeros((), dtype=torch.float32, device=ids.device))
    return out


class Scene(object):
    """Device-resident scene (BLAS, instances, lights, shaders, textures)."""

    def __init__(self, scene_desc_ptr, device=0):
        self._h = C.c_void_p()
        self._device = device
        _check(lib().fjgpu_scene_create(scene_desc_ptr, device, C.byref(self._h)))

    def close(self):
        if self._h:
            lib().fjgpu_scene_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def query(self, name):
        v = C.c_double(0)
        _check(lib().fjgpu_scene_query(self._h, name.encode(), C.byref(v)))
        return v.value

    def set_option(self, name, value):
        _check(lib().fjgpu_set_option(self._h, name.encode(), int(value)))

    def render_frame(self, render):
        """All tiles -> numpy [H, W, 4] float32 plus GpuStats."""
        fb = np.zeros((render.yres, render.xres, 4), dtype=np.float32)
        st = ffi.GpuStats()
        _check(lib().fjgpu_render_frame(self._h, C.byref(render), fb.ctypes.data_as(C.c_void_p), C.byref(st)))
        return fb, st

    def render_tiles(self, render, tile_ids, d_framebuffer_ptr, stream=None, variance=None, albedo=None, albedo_floor=None):
        """Listed tiles into a DEVICE framebuffer (raw pointer, e.g. torch data_ptr()).  variance: a raw pointer to a DEVICE [H, W]
        float32 buffer that takes the sample variance of the listed tiles' pixels (include/fjgpu.h: fjgpu_render_tiles_variance), under
        the DEVICE [H, W, 3] float32 `albedo` (raw pointer) where one is given; albedo_floor None: ALBEDO_FLOOR.  Without `variance` the
        call is fjgpu_render_tiles."""
        st = ffi.GpuStats()
        if tile_ids is None:
            ids_p, n = None, 0
        else:
            ids = np.ascontiguousarray(tile_ids, dtype=np.int32)
            ids_p, n = ids.ctypes.data_as(C.c_void_p), len(ids)
        if variance is None:
            if albedo is not None:
                raise ValueError("albedo is the variance output's: pass variance too")
            _check(lib().fjgpu_render_tiles(self._h, C.byref(render), ids_p, n, C.c_void_p(d_framebuffer_ptr),
                                            C.c_void_p(stream or 0), C.byref(st)))
        else:
            floor = ALBEDO_FLOOR if albedo_floor is None else albedo_floor
            _check(lib().fjgpu_render_tiles_variance(self._h, C.byref(render), ids_p, n, C.c_void_p(d_framebuffer_ptr),
                                                     C.c_void_p(albedo or 0), C.c_float(float(floor)), C.c_void_p(variance),
                                                     C.c_void_p(stream or 0), C.byref(st)))
        return st

    def render_frame_variance(self, render, albedo=None, albedo_floor=None):
        """All tiles with the sample variance (include/fjgpu.h: fjgpu_render_tiles_variance) -> numpy [H, W, 4] float32, numpy [H, W]
        float32, GpuStats.  albedo: [H, W, 3] (numpy or device tensor, Scene.render_aov_albedo's): the variance is that of the luminance
        of the samples divided by max(albedo, albedo_floor) of their pixel; albedo_floor None: ALBEDO_FLOOR."""
        import torch
        dev = torch.device("cuda", self._device)
        hw = (render.yres, render.xres)
        fb = torch.zeros(hw + (4,), dtype=torch.float32, device=dev)
        var = torch.zeros(hw, dtype=torch.float32, device=dev)
        a = _device_tensor(albedo, "albedo", torch.float32, 3, dev, hw)
        torch.cuda.synchronize(dev)          # uploads and fills ran on torch's stream
        st = self.render_tiles(render, None, fb.data_ptr(), variance=var.data_ptr(), albedo=None if a is None else a.data_ptr(),
                               albedo_floor=albedo_floor)
        return fb.cpu().numpy(), var.cpu().numpy(), st

    def trace(self, group, rays):
        """Closest hits of rays [n, 8] (orig, dir, tmin, tmax) -> t [n], ids [n, 2], uv [n, 2], stats."""
        rays = np.ascontiguousarray(rays, dtype=np.float64)
        n = rays.shape[0]
        t = np.empty(n, dtype=np.float64)
        ids = np.empty((n, 2), dtype=np.int32)
        uv = np.empty((n, 2), dtype=np.float64)
        st = ffi.GpuStats()
        _check(lib().fjgpu_trace(self._h, group, n, rays.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p),
                                 ids.ctypes.data_as(C.c_void_p), uv.ctypes.data_as(C.c_void_p), C.byref(st)))
        return t, ids, uv, st

    def render_aov(self, render, tile_ids=None, want=AOV_NAMES, prefill=None, stream=None):
        """First-hit AOV pass (include/fjgpu.h: fjgpu_render_aov) of the listed tiles (None = all tiles of the render region):
        the nearest of every pixel's own samples.  -> ({name: numpy array [H, W, channels]}, GpuStats) for the names in `want`:
        depth [1] f32, position [3], normal [3], uv [2], ids [4] int32 (instance, primitive, shading group, shader index),
        coverage [1].  The buffers are torch tensors on the scene's device; `prefill` (a number, or {name: number}) sets every
        element beforehand, so that the pixels of tiles not listed can be told from those written (default 0)."""
        tensors, st = self._render_aov_device(render, tile_ids, want, prefill, stream)
        return {name: t.cpu().numpy() for name, t in tensors.items()}, st

    def render_aov_albedo(self, render, tile_ids=None, want=AOV_ALL, prefill=None, stream=None):
        """render_aov through the entry point that also knows "albedo" [3] f32 (include/fjgpu.h: fjgpu_render_aov_albedo): the mean
        over the pixel's own samples of the surface colour without light, from the same camera rays and the same walk as the six
        geometry buffers.  `want` takes any of AOV_ALL, ("albedo",) alone included; everything else is render_aov's."""
        tensors, st = self._render_aov_device(render, tile_ids, want, prefill, stream, names=AOV_ALL)
        return {name: t.cpu().numpy() for name, t in tensors.items()}, st

    def _render_aov_device(self, render, tile_ids=None, want=AOV_NAMES, prefill=None, stream=None, names=AOV_NAMES):
        """render_aov (names=AOV_ALL: render_aov_albedo) with the buffers left where the pass wrote them ->
        ({name: torch tensor on the scene's device}, GpuStats)"""
        import torch
        want = tuple(want)
        for name in want:
            if name not in names:
                raise ValueError("unknown AOV %r (one of %s)" % (name, ", ".join(names)))
        dev = torch.device("cuda", self._device)
        bufs = ffi.AovBuffers()
        tensors = {}
        for name in want:
            dtype = torch.int32 if name == "ids" else torch.float32
            fill = prefill.get(name, 0) if isinstance(prefill, dict) else (0 if prefill is None else prefill)
            tensors[name] = torch.full((render.yres, render.xres, AOV_CHANNELS[name]), fill, dtype=dtype, device=dev)
            if name != "albedo":
                setattr(bufs, name, tensors[name].data_ptr())
        torch.cuda.synchronize(dev)          # the fills ran on torch's stream
        st = ffi.GpuStats()
        if tile_ids is None:
            ids_p, n = None, 0
        else:
            ids = np.ascontiguousarray(tile_ids, dtype=np.int32)
            ids_p, n = ids.ctypes.data_as(C.c_void_p), len(ids)
        if names is AOV_ALL:
            albedo = tensors["albedo"].data_ptr() if "albedo" in tensors else None
            _check(lib().fjgpu_render_aov_albedo(self._h, C.byref(render), ids_p, n, C.byref(bufs), C.c_void_p(albedo),
                                                 C.c_void_p(stream or 0), C.byref(st)))
        else:
            _check(lib().fjgpu_render_aov(self._h, C.byref(render), ids_p, n, C.byref(bufs), C.c_void_p(stream or 0), C.byref(st)))
        return tensors, st

    def render_matte(self, render, key="instance", ranks=4, filtered=True, tile_ids=None, prefill=None, stream=None):
        """Ranked id/coverage mattes (include/fjgpu.h: fjgpu_render_aov_matte) of the listed tiles (None = all tiles of the render
        region): per pixel the `ranks` keys with the greatest share of the pixel and those shares.  key: "instance" or "shader" (or the
        number of a FJGPU_MATTE_KEY_*); filtered: the shares of the beauty pixel's filter window under its weights (True) or of the
        pixel's own samples (False).  -> ({"ids": [H, W, ranks] int32 (-1: empty rank), "coverage": [H, W, ranks] f32, "rest": [H, W, 1]
        f32 (the share of the hit keys that did not fit), "distinct": [H, W, 1] int32}, GpuStats), numpy arrays; `prefill` as in
        render_aov.  matte_select() turns a set of keys into one matte."""
        tensors, st = self._render_matte_device(render, key, ranks, filtered, tile_ids, prefill, stream)
        return {name: t.cpu().numpy() for name, t in tensors.items()}, st

    def _render_matte_device(self, render, key="instance", ranks=4, filtered=True, tile_ids=None, prefill=None, stream=None):
        """render_matte with the buffers left where the pass wrote them -> ({name: torch tensor on the scene's device}, GpuStats)"""
        import torch
        if isinstance(key, str):
            if key not in ffi.MATTE_KEYS:
                raise ValueError("unknown matte key %r (one of %s)" % (key, ", ".join(sorted(ffi.MATTE_KEYS))))
            key = ffi.MATTE_KEYS[key]
        desc = ffi.MatteDesc(int(key), int(ranks), 1 if filtered else 0, 0)
        dev = torch.device("cuda", self._device)
        k = max(1, min(int(ranks), ffi.MATTE_MAX_RANKS))      # (a refused rank count still gets buffers: the refusal is the library's)
        bufs = ffi.MatteBuffers()
        tensors = {}
        for name in MATTE_NAMES:
            dtype = torch.float32 if name in ("coverage", "rest") else torch.int32
            fill = prefill.get(name, 0) if isinstance(prefill, dict) else (0 if prefill is None else prefill)
            tensors[name] = torch.full((render.yres, render.xres, k if name in ("ids", "coverage") else 1), fill, dtype=dtype, device=dev)
            setattr(bufs, name, tensors[name].data_ptr())
        torch.cuda.synchronize(dev)          # the fills ran on torch's stream
        st = ffi.GpuStats()
        if tile_ids is None:
            ids_p, n = None, 0
        else:
            ids = np.ascontiguousarray(tile_ids, dtype=np.int32)
            ids_p, n = ids.ctypes.data_as(C.c_void_p), len(ids)
        _check(lib().fjgpu_render_aov_matte(self._h, C.byref(render), ids_p, n, C.byref(desc), C.byref(bufs), C.c_void_p(stream or 0),
                                            C.byref(st)))
        return tensors, st

    def render_denoised(self, render, keep_inputs=False, stream=None, demodulate=False, variance_guided=False, variance="spatial", **kw):
        """A beauty frame, its feature buffers and the denoiser (include/fjgpu.h: fjgpu_denoise) in one go, everything on the device:
        render_tiles into a device framebuffer, render_aov(want=("position", "normal", "ids")), denoise over the render region; the
        only copy to the host is the result's.  -> (numpy [H, W, 4] float32, info) with info["beauty_stats"], info["aov_stats"],
        info["denoise_stats"] (GpuStats), info["sigma_position"] (the value used) and, with keep_inputs, info["beauty"] and
        info["aov"] (numpy copies of what the filter read).  `kw` are denoise()'s parameters.  Where sigma_position is not given it
        is SIGMA_POSITION_FRACTION of the diagonal of the bounding box of the finite positions of the foreground pixels (ids[0] >= 0)
        of the region; a frame without foreground switches the term off.  The AOV pass's refusals (adaptive sampler, time-sampled
        camera, scene with motion) pass through unchanged.  demodulate=True adds "albedo" to the one AOV call (render_aov_albedo's) and filters the
        frame divided by it (fjgpu_denoise_albedo: textures are kept out of the filter); info["aov"] then holds the albedo too and
        info["albedo_floor"] is the value used (denoise()'s albedo_floor).  variance_guided=True filters with denoise_variance()
        (include/fjgpu.h: fjgpu_denoise_variance, the variance estimated from the frame; `kw` are then its parameters) in place of
        denoise(); it combines with demodulate, and the derived sigma_position is SIGMA_POSITION_FRACTION_VARIANCE of the diagonal.  info["sigma_luminance"] is the value used and, with keep_inputs, info["variance"] the
        [H, W] variance of the last iteration.  variance="samples" (with variance_guided): the filter's input variance is the beauty pass's
        sample variance (include/fjgpu.h: fjgpu_render_tiles_variance) in place of the spatial estimate -- the AOV call then runs BEFORE
        the beauty pass, so that with demodulate the variance is taken under the albedo; with keep_inputs info["variance_in"] is that
        [H, W] variance.  variance="spatial", the default, is the path described above."""
        import torch
        dev = torch.device("cuda", self._device)
        region = tuple(int(v) for v in render.region)
        if "region" in kw:
            raise ValueError("render_denoised filters the render region of `render`")
        if variance not in ("spatial", "samples"):
            raise ValueError("variance is \"spatial\" or \"samples\", not %r" % (variance,))
        if variance == "samples" and not variance_guided:
            raise ValueError("variance=\"samples\" is the variance-guided filter's input: variance_guided=True")
        fb = torch.zeros((render.yres, render.xres, 4), dtype=torch.float32, device=dev)
        torch.cuda.synchronize(dev)          # the fill ran on torch's stream
        want = ("position", "normal", "ids") + (("albedo",) if demodulate else ())
        var_in = None
        if variance == "samples":
            aov, st_aov = self._render_aov_device(render, want=want, stream=stream, names=AOV_ALL if demodulate else AOV_NAMES)
            var_in = torch.zeros((render.yres, render.xres), dtype=torch.float32, device=dev)
            torch.cuda.synchronize(dev)
            st_beauty = self.render_tiles(render, None, fb.data_ptr(), stream=stream, variance=var_in.data_ptr(),
                                          albedo=aov["albedo"].data_ptr() if demodulate else None,
                                          albedo_floor=kw.get("albedo_floor", ALBEDO_FLOOR))
        else:
            st_beauty = self.render_tiles(render, None, fb.data_ptr(), stream=stream)
            aov, st_aov = self._render_aov_device(render, want=want, stream=stream, names=AOV_ALL if demodulate else AOV_NAMES)
        if kw.get("sigma_position") is None:
            x0, y0, x1, y1 = region
            pos = aov["position"][y0:y1, x0:x1].reshape(-1, 3)
            keep = (aov["ids"][y0:y1, x0:x1, 0].reshape(-1) >= 0) & torch.isfinite(pos).all(dim=1)
            if bool(keep.any()):
                p = pos[keep].double()
                fraction = SIGMA_POSITION_FRACTION_VARIANCE if variance_guided else SIGMA_POSITION_FRACTION
                kw["sigma_position"] = fraction * float(torch.linalg.norm(p.max(dim=0).values - p.min(dim=0).values))
            else:
                kw["sigma_position"] = 0.0
        info = dict(beauty_stats=st_beauty, aov_stats=st_aov, sigma_position=kw["sigma_position"])
        if keep_inputs:
            info["beauty"] = fb.cpu().numpy()
            info["aov"] = {name: t.cpu().numpy() for name, t in aov.items()}
        if demodulate:
            kw["albedo"] = aov["albedo"]
            info["albedo_floor"] = kw.setdefault("albedo_floor", ALBEDO_FLOOR)
        elif "albedo" in kw or "albedo_floor" in kw:
            raise ValueError("render_denoised takes the albedo from its own AOV pass: demodulate=True")
        if variance_guided:
            info["sigma_luminance"] = kw.setdefault("sigma_luminance", SIGMA_LUMINANCE)
            if "variance" in kw or "return_variance" in kw or "variance_out" in kw:
                raise ValueError("render_denoised estimates the variance from its own frame")
            if var_in is not None:
                kw["variance"] = var_in
                if keep_inputs:
                    info["variance_in"] = var_in.cpu().numpy()
            res = denoise_variance(fb, aov["normal"], aov["position"], aov["ids"], region=region, device=self._device, stream=stream,
                                   out=fb, return_variance=bool(keep_inputs), **kw)
            if keep_inputs:
                info["variance"] = res[1]
            info["denoise_stats"] = res[-1]
            return res[0], info
        out, info["denoise_stats"] = denoise(fb, aov["normal"], aov["position"], aov["ids"], region=region, device=self._device,
                                             stream=stream, out=fb, **kw)
        return out, info

    def get_camera(self):
        """the camera the scene renders with (include/fjgpu.h: fjgpu_scene_get_camera) -> ffi.CameraDesc, a copy"""
        cam = ffi.CameraDesc()
        _check(lib().fjgpu_scene_get_camera(self._h, C.byref(cam)))
        return cam

    def set_camera(self, camera=None, translate=None, rotate=None, fov=None):
        """Move the camera of the resident scene (include/fjgpu.h: fjgpu_scene_set_camera): host state only, no device work, no BLAS
        build; every later render, trace and AOV call gives what a scene created with that camera gives.  camera: an ffi.CameraDesc
        (None: the current one); translate / rotate (three numbers each) and fov then override its first sample.  Static cameras
        only.  -> the ffi.CameraDesc that was set."""
        cam = self.get_camera() if camera is None else camera.copy()
        if translate is not None:
            cam.xform.translate[0].v[:] = tuple(float(v) for v in translate)
        if rotate is not None:
            cam.xform.rotate[0].v[:] = tuple(float(v) for v in rotate)
        if fov is not None:
            cam.fov = float(fov)
        _check(lib().fjgpu_scene_set_camera(self._h, C.byref(cam)))
        return cam

    def view(self, render):
        """what it takes to find a world point in the frame the current camera renders with `render` (include/fjgpu.h: fjgpu_scene_view;
        the projection is written out there) -> ffi.View"""
        v = ffi.View()
        _check(lib().fjgpu_scene_view(self._h, C.byref(render), C.byref(v)))
        return v

    def render_progressive(self, render, passes, target_error=None, first_seed=1, lum_floor=None, keep_state=False, stream=None):
        """Refine one frame by rendering it again under other sampler seeds (include/fjgpu.h: option "sampler_seed", fjgpu_accumulate,
        fjgpu_accumulate_tile_error), everything on the device.  Pass i = 0 .. passes-1 sets seed first_seed + i (1..65535), renders the
        still-active tiles into a scratch framebuffer with render_tiles, accumulates those tiles' rectangles and, where target_error is
        set, reads their errors and drops the tiles at or below it; a pass without active tiles ends the loop.  The scene's seed is put
        back on exit, also on an exception.  No framebuffer crosses to the host between passes: per pass the tile list goes down and,
        with target_error, one float per active tile comes up.  lum_floor None: LUM_FLOOR.
        -> (mean, info): mean numpy [H, W, 4] float32, the mean frame; info["count"] [H, W] (frames accumulated per pixel),
        info["variance"] [H, W] (of the mean: denoise_variance's `variance`), info["active"] (per pass the tile ids rendered),
        info["errors"] (per pass the float32 array of those tiles' errors, or None without target_error), info["rays"] (ffi.RayCounts,
        summed over the passes), info["stats"] (per pass the beauty GpuStats) and, with keep_state, info["state"] (the device tensors
        mean, m2, count) and info["variance_device"]."""
        import torch
        dev = torch.device("cuda", self._device)
        floor = LUM_FLOOR if lum_floor is None else float(lum_floor)
        hw = (render.yres, render.xres)
        rects = np.array([tile_rect(render, t) for t in range(tile_count(render))], dtype=np.int32).reshape(-1, 4)
        fb = torch.zeros(hw + (4,), dtype=torch.float32, device=dev)
        state = new_accum_state(hw, self._device)
        var = torch.zeros(hw, dtype=torch.float32, device=dev)
        torch.cuda.synchronize(dev)          # the fills ran on torch's stream
        active = list(range(len(rects)))
        info = dict(active=[], errors=[], stats=[], rays=ffi.RayCounts())
        seed_before = int(self.query("sampler_seed"))
        try:
            for i in range(int(passes)):
                if not active:
                    break
                self.set_option("sampler_seed", int(first_seed) + i)
                ids = np.array(active, dtype=np.int32)
                st = self.render_tiles(render, ids, fb.data_ptr(), stream=stream)
                accumulate(fb, state, rects=rects[ids], variance_out=var, device=self._device, stream=stream)
                errs = None
                if target_error is not None:
                    errs, _ = tile_errors(state, rects=rects[ids], lum_floor=floor, device=self._device, stream=stream)
                    active = [t for t, e in zip(active, errs) if not e <= target_error]
                info["active"].append([int(t) for t in ids])
                info["errors"].append(errs)
                info["stats"].append(st)
                for name, _ in ffi.RayCounts._fields_:
                    setattr(info["rays"], name, getattr(info["rays"], name) + getattr(st.rays, name))
        finally:
            self.set_option("sampler_seed", seed_before)
        info["count"] = state["count"].cpu().numpy()
        info["variance"] = var.cpu().numpy()
        if keep_state:
            info["state"], info["variance_device"] = state, var
        return state["mean"].cpu().numpy(), info

    def camera_samples(self, render, tile_id):
        """the camera rays of one tile as the AOV and beauty passes trace them (include/fjgpu.h: fjgpu_camera_samples) ->
        ndarray [n, 8] = orig, dir, znear, zfar in sample order k = y * nx + x, margin samples included: what trace() takes"""
        n = lib().fjgpu_camera_samples(self._h, C.byref(render), int(tile_id), None, 0)
        if n < 0:
            _check(n)
        rays = np.empty((n, 8), dtype=np.float64)
        m = lib().fjgpu_camera_samples(self._h, C.byref(render), int(tile_id), rays.ctypes.data_as(C.c_void_p), n)
        if m < 0:
            _check(m)
        return rays


class MultiScene(object):
    """The same scene resident on several devices (fjgpu_scene_create_multi): one host-side
    build, one upload per entry of `devices` (an index may repeat: two replicas on one device
    exercise the multi-device path on a single GPU)."""

    def __init__(self, scene_desc_ptr, devices):
        self.n = len(devices)
        self._h = (C.c_void_p * self.n)()
        devs = (C.c_int * self.n)(*devices)
        _check(lib().fjgpu_scene_create_multi(scene_desc_ptr, devs, self.n, self._h))

    def close(self):
        for k in range(self.n):
            if self._h[k]:
                lib().fjgpu_scene_destroy(self._h[k])
                self._h[k] = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def render_frame(self, render, tile_ids=None):
        """Tile k of the list on replica k % n, slabs gathered on the first device ->
        numpy [H, W, 4] float32 plus one GpuStats per replica."""
        fb = np.zeros((render.yres, render.xres, 4), dtype=np.float32)
        st = (ffi.GpuStats * self.n)()
        if tile_ids is None:
            ids_p, n = None, 0
        else:
            ids = np.ascontiguousarray(tile_ids, dtype=np.int32)
            ids_p, n = ids.ctypes.data_as(C.c_void_p), len(ids)
        _check(lib().fjgpu_render_frame_multi(self._h, self.n, C.byref(render), ids_p, n, fb.ctypes.data_as(C.c_void_p), st))
        return fb, list(st)


def host_instance_level(scene_desc_ptr, group):
    """(inst [n], skip [n], box [n, 6]) of the group's instance level as the host builder lays it out; no device needed"""
    L = lib()
    L.fjgpu_host_instance_level.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    L.fjgpu_host_instance_level.restype = C.c_int
    n = L.fjgpu_host_instance_level(scene_desc_ptr, group, None, None, None, 0)
    if n < 0:
        _check(n)
    inst = np.zeros(n, dtype=np.int32)
    skip = np.zeros(n, dtype=np.int32)
    box = np.zeros((n, 6), dtype=np.float64)
    _check(min(0, L.fjgpu_host_instance_level(scene_desc_ptr, group, inst.ctypes.data_as(C.c_void_p), skip.ctypes.data_as(C.c_void_p),
                                              box.ctypes.data_as(C.c_void_p), n)))
    return inst, skip, box


LIGHT_HULL = np.dtype([("n", np.float64, (6, 3)), ("reach", np.float64), ("count", np.int32), ("pad", np.int32)])


def host_light_hulls(scene_desc_ptr, group):
    """(records [n_light_samples] of LIGHT_HULL, Pl [n_light_samples, 3], M [3, 4]): the hull cones of the single-instance group as scene
    creation builds them (count 0: no record), the light samples' positions and the instance's object-to-world matrix; no device needed"""
    L = lib()
    L.fjgpu_host_light_hulls.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.fjgpu_host_light_hulls.restype = C.c_int
    n = L.fjgpu_host_light_hulls(scene_desc_ptr, group, None, None, 0, None)
    if n < 0:
        _check(n)
    rec = np.zeros(n, dtype=LIGHT_HULL)
    Pl = np.zeros((n, 3), dtype=np.float64)
    M = np.zeros((3, 4), dtype=np.float64)
    _check(min(0, L.fjgpu_host_light_hulls(scene_desc_ptr, group, rec.ctypes.data_as(C.c_void_p), Pl.ctypes.data_as(C.c_void_p), n,
                                           M.ctypes.data_as(C.c_void_p))))
    return rec, Pl, M


def host_curve_blas(scene_desc_ptr, curve_set):
    """the BLAS over a curve set as scene creation builds it on the host (include/fjgpu.h: fjgpu_host_curve_blas; reads
    FJGPU_CURVE_SEGDEPTH when called) -> dict(curve [n] int32, A [n, 3], B [n, 3], reach [n] (f32), depth [n] int32, box [n, 6] f32
    (min xyz, max xyz), grid_n [3], grid_cell [3], bounds [6]), n = BLAS slots; no device needed"""
    L = lib()
    L.fjgpu_host_curve_blas.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                        C.c_void_p]
    L.fjgpu_host_curve_blas.restype = C.c_int
    n = L.fjgpu_host_curve_blas(scene_desc_ptr, curve_set, None, None, None, None, 0, None, None, None)
    if n < 0:
        _check(n)
    curve = np.zeros(n, dtype=np.int32)
    cap = np.zeros((n, 7), dtype=np.float32)
    depth = np.zeros(n, dtype=np.int32)
    box = np.zeros((n, 6), dtype=np.float32)
    grid_n = np.zeros(3, dtype=np.int32)
    grid_cell = np.zeros(3, dtype=np.float64)
    bounds = np.zeros(6, dtype=np.float64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    _check(min(0, L.fjgpu_host_curve_blas(scene_desc_ptr, curve_set, p(curve), p(cap), p(depth), p(box), n, p(grid_n), p(grid_cell), p(bounds))))
    return dict(curve=curve, A=cap[:, 0:3].copy(), B=cap[:, 3:6].copy(), reach=cap[:, 6].copy(), depth=depth, box=box, grid_n=grid_n,
                grid_cell=grid_cell, bounds=bounds)


# the denoiser's defaults: of the grid in profiles/denoise_pass.txt (the 64 x 48 Cornell box at 2 x 2 spp against a 12 x 12 spp frame, CPU
# oracle and numpy model) the setting with the smallest mean squared error among those that stop at instance ids
DENOISE_ITERATIONS = 5
SIGMA_COLOR = 3.0
SIGMA_NORMAL = 1.0
SIGMA_POSITION_FRACTION = 0.1       # of the diagonal of the foreground's bounding box (Scene.render_denoised)
# the smallest albedo a beauty frame is divided by (fjgpu_denoise_albedo): of the grid in profiles/albedo_pass.txt the floor with the smallest
# mean squared error on the textured scene
ALBEDO_FLOOR = 1e-4


def _device_tensor(a, name, dtype, channels, dev, shape=None):
    import torch
    if a is None:
        return None
    t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
    t = t.to(device=dev, dtype=dtype).contiguous()
    if t.dim() != 3 or t.shape[2] != channels or (shape is not None and tuple(t.shape[:2]) != tuple(shape)):
        raise ValueError("%s must be [H, W, %d]%s, not %s" % (name, channels, "" if shape is None else " with H, W = %d, %d" % tuple(shape),
                                                             tuple(t.shape)))
    return t


def denoise(color, normal=None, position=None, ids=None, iterations=DENOISE_ITERATIONS, sigma_color=SIGMA_COLOR,
            sigma_normal=SIGMA_NORMAL, sigma_position=None, stop_at_ids=True, region=None, device=0, stream=None, out=None,
            albedo=None, albedo_floor=ALBEDO_FLOOR):
    """Edge-avoiding a-trous filter of a beauty frame (include/fjgpu.h: fjgpu_denoise) -> (numpy [H, W, 4] float32, GpuStats).
    color [H, W, 4] RGBA, normal / position [H, W, 3], ids [H, W, 4] int32 (the buffers of Scene.render_aov): numpy arrays, which
    are uploaded, or torch tensors on the device, which are used where they are.  A sigma <= 0 or +inf switches its term off;
    sigma_position is in world units (None: off -- Scene.render_denoised derives one from the scene's size).  region = (xmin, ymin,
    xmax, ymax), None = the frame; pixels outside it are the input's.  out: a float32 device tensor [H, W, 4] to write instead of
    a new one -- it may be `color` itself (in place) -- whose pixels outside the region are left as they are.  albedo [H, W, 3] f32
    (Scene.render_aov_albedo's "albedo"): the filter runs on colour / max(albedo, albedo_floor) and the result is multiplied by it again
    (include/fjgpu.h: fjgpu_denoise_albedo); None: no demodulation."""
    import torch
    dev = torch.device("cuda", device)
    c = _device_tensor(color, "color", torch.float32, 4, dev)
    hw = tuple(c.shape[:2])
    n = _device_tensor(normal, "normal", torch.float32, 3, dev, hw)
    p = _device_tensor(position, "position", torch.float32, 3, dev, hw)
    i = _device_tensor(ids, "ids", torch.int32, 4, dev, hw)
    a = _device_tensor(albedo, "albedo", torch.float32, 3, dev, hw)
    if out is None:
        out = c.clone()
    elif not (torch.is_tensor(out) and out.device == dev and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == tuple(c.shape)):
        raise ValueError("out must be a contiguous float32 tensor of color's shape on the device")
    d = ffi.DenoiseDesc()
    d.yres, d.xres = hw
    d.region[:] = (0, 0, d.xres, d.yres) if region is None else tuple(int(v) for v in region)
    d.iterations = int(iterations)
    d.sigma_color, d.sigma_normal = float(sigma_color), float(sigma_normal)
    d.sigma_position = 0.0 if sigma_position is None else float(sigma_position)
    d.stop_at_ids = 1 if stop_at_ids else 0
    torch.cuda.synchronize(dev)          # uploads and copies ran on torch's stream
    st = ffi.GpuStats()
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    if a is not None:
        _check(lib().fjgpu_denoise_albedo(device, C.byref(d), ptr(c), ptr(n), ptr(p), ptr(i), ptr(a), C.c_float(float(albedo_floor)), ptr(out),
                                          C.c_void_p(stream or 0), C.byref(st)))
    else:
        _check(lib().fjgpu_denoise(device, C.byref(d), ptr(c), ptr(n), ptr(p), ptr(i), ptr(out), C.c_void_p(stream or 0), C.byref(st)))
    return out.cpu().numpy(), st


# the luminance sigma of denoise_variance(), in units of the local standard deviation: of the grid in profiles/denoise_variance.txt (the frames
# and the method of the grid above, scripts/denoise_variance_grid.py) the setting with the smallest mean squared error: sigma_luminance 4,
# sigma_normal 1, sigma_position 0.03 of the diagonal.  The position term is tighter than the plain filter's: the estimate's 7 x 7 window
# must not straddle an illumination edge, which it would take for variance.
SIGMA_LUMINANCE = 4.0
SIGMA_POSITION_FRACTION_VARIANCE = 0.03       # of the diagonal of the foreground's bounding box (Scene.render_denoised(variance_guided=True))


def _variance_tensor(v, name, dev, hw):
    import torch
    if v is None:
        return None
    t = v if torch.is_tensor(v) else torch.from_numpy(np.ascontiguousarray(v))
    t = t.to(device=dev, dtype=torch.float32).contiguous()
    if tuple(t.shape) != tuple(hw):
        raise ValueError("%s must be [H, W] = %d, %d, not %s" % ((name,) + tuple(hw) + (tuple(t.shape),)))
    return t


def _denoise_desc(hw, region, iterations, sigma_normal, sigma_position, stop_at_ids):
    d = ffi.DenoiseDesc()
    d.yres, d.xres = hw
    d.region[:] = (0, 0, d.xres, d.yres) if region is None else tuple(int(v) for v in region)
    d.iterations = int(iterations)
    d.sigma_color, d.sigma_normal = 0.0, float(sigma_normal)
    d.sigma_position = 0.0 if sigma_position is None else float(sigma_position)
    d.stop_at_ids = 1 if stop_at_ids else 0
    return d


def estimate_variance(color, normal=None, position=None, ids=None, region=None, sigma_normal=SIGMA_NORMAL, sigma_position=None,
                      stop_at_ids=True, device=0, stream=None):
    """Spatial variance estimate of a beauty frame's luminance under the AOV guides (include/fjgpu.h: fjgpu_denoise_estimate_variance)
    -> (numpy [H, W] float32, GpuStats).  The inputs and the sigmas are denoise()'s; pixels outside the region are 0."""
    import torch
    dev = torch.device("cuda", device)
    c = _device_tensor(color, "color", torch.float32, 4, dev)
    hw = tuple(c.shape[:2])
    n = _device_tensor(normal, "normal", torch.float32, 3, dev, hw)
    p = _device_tensor(position, "position", torch.float32, 3, dev, hw)
    i = _device_tensor(ids, "ids", torch.int32, 4, dev, hw)
    var = torch.zeros(hw, dtype=torch.float32, device=dev)
    d = _denoise_desc(hw, region, 1, sigma_normal, sigma_position, stop_at_ids)
    torch.cuda.synchronize(dev)          # uploads and the fill ran on torch's stream
    st = ffi.GpuStats()
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    _check(lib().fjgpu_denoise_estimate_variance(device, C.byref(d), ptr(c), ptr(n), ptr(p), ptr(i), ptr(var), C.c_void_p(stream or 0),
                                                 C.byref(st)))
    return var.cpu().numpy(), st


def denoise_variance(color, normal=None, position=None, ids=None, albedo=None, variance=None, sigma_luminance=SIGMA_LUMINANCE,
                     iterations=DENOISE_ITERATIONS, sigma_normal=SIGMA_NORMAL, sigma_position=None, stop_at_ids=True, region=None,
                     device=0, stream=None, out=None, albedo_floor=ALBEDO_FLOOR, return_variance=False, variance_out=None):
    """Variance-guided a-trous filter of a beauty frame (include/fjgpu.h: fjgpu_denoise_variance) -> (numpy [H, W, 4] float32, GpuStats),
    or with return_variance (numpy [H, W, 4], numpy [H, W] variance of the last iteration, GpuStats).  The inputs, region, out, albedo
    and albedo_floor are denoise()'s; there is no colour sigma: sigma_luminance is in units of the local standard deviation (<= 0 or
    +inf: off).  variance [H, W] f32 (numpy or device tensor, finite and >= 0): the variance of the frame's luminance -- of the
    demodulated frame's where there is an albedo; None: estimated as estimate_variance() does.  variance_out: a float32 device tensor
    [H, W] to take the last iteration's variance (implies return_variance); its pixels outside the region are left as they are."""
    import torch
    dev = torch.device("cuda", device)
    c = _device_tensor(color, "color", torch.float32, 4, dev)
    hw = tuple(c.shape[:2])
    n = _device_tensor(normal, "normal", torch.float32, 3, dev, hw)
    p = _device_tensor(position, "position", torch.float32, 3, dev, hw)
    i = _device_tensor(ids, "ids", torch.int32, 4, dev, hw)
    a = _device_tensor(albedo, "albedo", torch.float32, 3, dev, hw)
    v = _variance_tensor(variance, "variance", dev, hw)
    if out is None:
        out = c.clone()
    elif not (torch.is_tensor(out) and out.device == dev and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == tuple(c.shape)):
        raise ValueError("out must be a contiguous float32 tensor of color's shape on the device")
    if variance_out is not None:
        if not (torch.is_tensor(variance_out) and variance_out.device == dev and variance_out.dtype == torch.float32 and
                variance_out.is_contiguous() and tuple(variance_out.shape) == hw):
            raise ValueError("variance_out must be a contiguous float32 tensor [H, W] on the device")
        return_variance = True
    elif return_variance:
        variance_out = torch.zeros(hw, dtype=torch.float32, device=dev)
    d = _denoise_desc(hw, region, iterations, sigma_normal, sigma_position, stop_at_ids)
    torch.cuda.synchronize(dev)          # uploads and copies ran on torch's stream
    st = ffi.GpuStats()
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    _check(lib().fjgpu_denoise_variance(device, C.byref(d), C.c_float(float(sigma_luminance)), ptr(c), ptr(n), ptr(p), ptr(i), ptr(a),
                                        C.c_float(float(albedo_floor)), ptr(v), ptr(out), ptr(variance_out), C.c_void_p(stream or 0),
                                        C.byref(st)))
    if return_variance:
        return out.cpu().numpy(), variance_out.cpu().numpy(), st
    return out.cpu().numpy(), st


def _estimate_variance_device(color, normal, position, ids, albedo, albedo_floor, region, sigma_normal, sigma_position, stop_at_ids, device,
                              stream):
    """estimate_variance() of device tensors with the result left on the device, of colour / albedo where there is an albedo
    (include/fjgpu.h: fjgpu_denoise_estimate_variance_albedo) -> (float32 tensor [H, W], GpuStats)"""
    import torch
    dev = torch.device("cuda", device)
    hw = tuple(color.shape[:2])
    var = torch.zeros(hw, dtype=torch.float32, device=dev)
    d = _denoise_desc(hw, region, 1, sigma_normal, sigma_position, stop_at_ids)
    torch.cuda.synchronize(dev)          # the fill ran on torch's stream
    st = ffi.GpuStats()
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    _check(lib().fjgpu_denoise_estimate_variance_albedo(device, C.byref(d), ptr(color), ptr(normal), ptr(position), ptr(ids), ptr(albedo),
                                                        C.c_float(float(albedo_floor)), ptr(var), C.c_void_p(stream or 0), C.byref(st)))
    return var, st


def estimate_variance_albedo(color, albedo, normal=None, position=None, ids=None, albedo_floor=ALBEDO_FLOOR, region=None,
                             sigma_normal=SIGMA_NORMAL, sigma_position=None, stop_at_ids=True, device=0, stream=None):
    """estimate_variance() of colour / max(albedo, albedo_floor) (include/fjgpu.h: fjgpu_denoise_estimate_variance_albedo): the variance
    of the demodulated luminance, what temporal_accumulate() takes as variance_spatial next to an albedo -> (numpy [H, W] float32, GpuStats)"""
    import torch
    dev = torch.device("cuda", device)
    c = _device_tensor(color, "color", torch.float32, 4, dev)
    hw = tuple(c.shape[:2])
    var, st = _estimate_variance_device(c, _device_tensor(normal, "normal", torch.float32, 3, dev, hw),
                                        _device_tensor(position, "position", torch.float32, 3, dev, hw),
                                        _device_tensor(ids, "ids", torch.int32, 4, dev, hw), _device_tensor(albedo, "albedo", torch.float32, 3, dev, hw),
                                        albedo_floor, region, sigma_normal, sigma_position, stop_at_ids, device, stream)
    return var.cpu().numpy(), st


# the defaults of temporal_accumulate() and TemporalDenoiser: of the grid in profiles/temporal_pass.txt (a six-frame sub-pixel pan of the
# 64 x 48 Cornell box at 2 x 2 spp against a 12 x 12 spp frame of the last camera, CPU oracle and numpy model, scripts/temporal_grid.py)
# the setting with the smallest mean squared error of the last frame (demodulated chain) among those that keep a history on at least 90 %
# of the foreground: the position tolerance has to span a pixel of a surface seen at a grazing angle (0.02 of the diagonal keeps 84 %, 0.05
# keeps 99 %).  Six frames reach neither 1 / ALPHA_MIN nor MAX_HISTORY.  MIN_HISTORY_VARIANCE is SVGF's: shorter histories take the spatial
# estimate.  What accumulation does NOT buy on that frame without a colour clamp and a sampler seed is written out in the same file.
ALPHA_MIN = 0.1
MAX_HISTORY = 32.0
MIN_HISTORY_VARIANCE = 4.0
COS_NORMAL = 0.97
TOL_POSITION_FRACTION = 0.05        # of the diagonal of the foreground's bounding box (TemporalDenoiser)

# the clamp of temporal_accumulate(clamp=...) and TemporalDenoiser(clamp=...) that the grid of profiles/temporal_clamp.txt picks
# (scripts/temporal_clamp_grid.py: the same pan, the cell with the smallest filtered error of the chain that is not demodulated: 0.186
# against 0.249 unclamped -- and against 0.066 for the last frame filtered alone, which no cell reaches).  Neither call uses them unasked.
CLAMP_RADIUS = 1
CLAMP_GAMMA = 0.75
CLAMP_STOP_AT_IDS = False

# the luminance below which a tile's error (tile_errors, Scene.render_progressive) is measured against the floor instead of the pixel's own
# mean: the relative error of a black pixel means nothing.  1e-3 of a frame whose white is 1.
LUM_FLOOR = 1e-3

ACCUM_NAMES = ("mean", "m2", "count")


def new_accum_state(hw, device=0):
    """the zeroed state of accumulate() for frames [H, W]: {"mean": [H, W, 4], "m2": [H, W], "count": [H, W]} float32 tensors on the device"""
    import torch
    dev = torch.device("cuda", device)
    hw = tuple(int(v) for v in hw)
    return {n: torch.zeros(hw + ((4,) if n == "mean" else ()), dtype=torch.float32, device=dev) for n in ACCUM_NAMES}


def _accum_args(state, rects, dev, hw):
    import torch
    for n in ACCUM_NAMES:
        t, want = state[n], hw + ((4,) if n == "mean" else ())
        if not (torch.is_tensor(t) and t.device == dev and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == want):
            raise ValueError("state[%r] must be a contiguous float32 tensor %s on the device" % (n, want))
    s = ffi.AccumState()
    for n in ACCUM_NAMES:
        setattr(s, n, state[n].data_ptr())
    if rects is None:
        return s, None, None, 0
    r = np.ascontiguousarray(rects, dtype=np.int32).reshape(-1, 4)
    return s, r, r.ctypes.data_as(C.c_void_p), len(r)


def accumulate(color, state=None, rects=None, reset=False, variance_out=None, device=0, stream=None):
    """One more frame into the running mean (include/fjgpu.h: fjgpu_accumulate) -> (state, variance_out, GpuStats), device tensors in
    and out.  color: float32 device tensor [H, W, 4] (numpy arrays are uploaded); state: new_accum_state()'s dict, updated in place (None:
    a new one); rects: [n, 4] ints xmin ymin xmax ymax (tile_rect's; None: the whole frame) -- pixels outside them are not touched;
    reset: the state read counts as zero; variance_out: a contiguous float32 device tensor [H, W] that takes the variance of the MEAN of
    the listed pixels (what denoise_variance takes as `variance`), or None: none is written, and None is returned in its place."""
    import torch
    dev = torch.device("cuda", device)
    c = _device_tensor(color, "color", torch.float32, 4, dev)
    hw = tuple(c.shape[:2])
    if state is None:
        state = new_accum_state(hw, device)
    s, _keep, rects_p, n = _accum_args(state, rects, dev, hw)
    if variance_out is not None and not (torch.is_tensor(variance_out) and variance_out.device == dev and variance_out.dtype == torch.float32 and
                                         variance_out.is_contiguous() and tuple(variance_out.shape) == hw):
        raise ValueError("variance_out must be a contiguous float32 tensor [H, W] on the device")
    torch.cuda.synchronize(dev)          # uploads and fills ran on torch's stream
    st = ffi.GpuStats()
    _check(lib().fjgpu_accumulate(device, hw[1], hw[0], rects_p, n, C.c_void_p(c.data_ptr()), C.byref(s), 1 if reset else 0,
                                  None if variance_out is None else C.c_void_p(variance_out.data_ptr()), C.c_void_p(stream or 0), C.byref(st)))
    return state, variance_out, st


def tile_errors(state, rects=None, lum_floor=LUM_FLOOR, device=0, stream=None):
    """The error of the accumulated mean per rectangle (include/fjgpu.h: fjgpu_accumulate_tile_error): the mean over its pixels of the
    standard deviation of the mean relative to max(luminance, lum_floor); +inf where a pixel holds fewer than two frames.  state: the
    device tensors of accumulate(); rects as there.  -> (numpy float32 [n], GpuStats): the n floats are all that crosses to the host."""
    import torch
    dev = torch.device("cuda", device)
    hw = tuple(state["count"].shape)
    s, _keep, rects_p, n = _accum_args(state, rects, dev, hw)
    out = np.zeros(1 if rects is None else n, dtype=np.float32)
    torch.cuda.synchronize(dev)
    st = ffi.GpuStats()
    _check(lib().fjgpu_accumulate_tile_error(device, hw[1], hw[0], rects_p, n, C.byref(s), C.c_float(float(lum_floor)),
                                             out.ctypes.data_as(C.c_void_p), C.c_void_p(stream or 0), C.byref(st)))
    return out, st


HISTORY_NAMES = ("color", "moments", "length")
HISTORY_CHANNELS = {"color": 4, "moments": 2, "length": 1}


def _history_tensors(h, name, dev, hw, fresh):
    """{name: device tensor} of a history given as a dict of numpy arrays or tensors (length as [H, W] or [H, W, 1]); fresh: new zeroed ones"""
    import torch
    if fresh:
        return {n: torch.zeros(hw + ((HISTORY_CHANNELS[n],) if n != "length" else ()), dtype=torch.float32, device=dev) for n in HISTORY_NAMES}
    out = {}
    for n in HISTORY_NAMES:
        if n == "length":
            out[n] = _variance_tensor(h[n], "%s['length']" % name, dev, hw)
        else:
            out[n] = _device_tensor(h[n], "%s[%r]" % (name, n), torch.float32, HISTORY_CHANNELS[n], dev, hw)
    return out


def _history_struct(t):
    h = ffi.TemporalHistory()
    for n in HISTORY_NAMES:
        setattr(h, n, t[n].data_ptr())
    return h


def _temporal_clamp(clamp):
    """ffi.TemporalClamp (without an amount) of temporal_accumulate's `clamp`, or None"""
    if clamp is None:
        return None
    if isinstance(clamp, dict):
        unknown = sorted(set(clamp) - {"radius", "gamma", "stop_at_ids"})
        if unknown or "radius" not in clamp or "gamma" not in clamp:
            raise ValueError("clamp is a (radius, gamma) pair or a dict with radius, gamma and optionally stop_at_ids")
        radius, gamma, stop = clamp["radius"], clamp["gamma"], clamp.get("stop_at_ids", CLAMP_STOP_AT_IDS)
    else:
        radius, gamma = clamp
        stop = CLAMP_STOP_AT_IDS
    cl = ffi.TemporalClamp()
    cl.radius, cl.gamma, cl.stop_at_ids = int(radius), float(gamma), 1 if stop else 0
    return cl


def temporal_accumulate(color, position, normal, ids, albedo=None, variance_spatial=None, prev_view=None, prev_position=None,
                        prev_normal=None, prev_ids=None, prev=None, next=None, region=None, alpha_min=ALPHA_MIN, max_history=MAX_HISTORY,
                        tol_position=None, cos_normal=COS_NORMAL, min_history_variance=MIN_HISTORY_VARIANCE, albedo_floor=ALBEDO_FLOOR,
                        device=0, stream=None, variance_out=None, to_host=True, clamp=None, clamp_amount=None):
    """Temporal accumulation of a beauty frame (include/fjgpu.h: fjgpu_denoise_temporal) -> (history, variance, GpuStats): history =
    {"color": [H, W, 4], "moments": [H, W, 2], "length": [H, W]}, variance [H, W], as numpy arrays -- or, with to_host=False, as the
    float32 tensors on the device the call wrote.  color [H, W, 4], position / normal [H, W, 3], ids [H, W, 4] int32 (Scene.render_aov's)
    and the optional albedo [H, W, 3] and variance_spatial [H, W] describe the current frame; prev_view (Scene.view of the previous
    camera), prev_position, prev_normal, prev_ids and prev (a history as returned) the previous one -- prev None: the first frame of a
    sequence.  numpy arrays are uploaded, device tensors used where they are.  next / variance_out: a history of contiguous float32
    device tensors / a tensor [H, W] to write instead of new ones (pixels outside the region are left as they are; new ones are 0
    there); they must not be prev's or an input's.  tol_position is in world units (None, <= 0 or +inf: off), cos_normal <= -1: off.
    clamp: None, or a (radius, gamma) pair or a dict with "radius", "gamma" and optionally "stop_at_ids" (default CLAMP_STOP_AT_IDS):
    the history is clipped to the box of the current frame's window before the blend (fjgpu_denoise_temporal_clamped); clamp_amount: a
    contiguous float32 device tensor [H, W] that receives how far each pixel's history was moved (it needs a clamp)."""
    import torch
    dev = torch.device("cuda", device)
    c = _device_tensor(color, "color", torch.float32, 4, dev)
    hw = tuple(c.shape[:2])
    p = _device_tensor(position, "position", torch.float32, 3, dev, hw)
    n = _device_tensor(normal, "normal", torch.float32, 3, dev, hw)
    i = _device_tensor(ids, "ids", torch.int32, 4, dev, hw)
    a = _device_tensor(albedo, "albedo", torch.float32, 3, dev, hw)
    vs = _variance_tensor(variance_spatial, "variance_spatial", dev, hw)
    pp = _device_tensor(prev_position, "prev_position", torch.float32, 3, dev, hw)
    pn = _device_tensor(prev_normal, "prev_normal", torch.float32, 3, dev, hw)
    pi = _device_tensor(prev_ids, "prev_ids", torch.int32, 4, dev, hw)
    hp = None if prev is None else _history_tensors(prev, "prev", dev, hw, False)
    if next is None:
        hn = _history_tensors(None, "next", dev, hw, True)
    else:
        hn = {k: next[k] for k in HISTORY_NAMES}
        for k, t in hn.items():
            want = hw + ((HISTORY_CHANNELS[k],) if k != "length" else ())
            if not (torch.is_tensor(t) and t.device == dev and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == want):
                raise ValueError("next[%r] must be a contiguous float32 tensor %s on the device" % (k, want))
    if variance_out is None:
        variance_out = torch.zeros(hw, dtype=torch.float32, device=dev)
    elif not (torch.is_tensor(variance_out) and variance_out.device == dev and variance_out.dtype == torch.float32 and
              variance_out.is_contiguous() and tuple(variance_out.shape) == hw):
        raise ValueError("variance_out must be a contiguous float32 tensor [H, W] on the device")
    cl = _temporal_clamp(clamp)
    if clamp_amount is not None:
        if cl is None:
            raise ValueError("clamp_amount needs a clamp")
        if not (torch.is_tensor(clamp_amount) and clamp_amount.device == dev and clamp_amount.dtype == torch.float32 and
                clamp_amount.is_contiguous() and tuple(clamp_amount.shape) == hw):
            raise ValueError("clamp_amount must be a contiguous float32 tensor [H, W] on the device")
        cl.amount = clamp_amount.data_ptr()
    d = ffi.TemporalDesc()
    d.yres, d.xres = hw
    d.region[:] = (0, 0, d.xres, d.yres) if region is None else tuple(int(v) for v in region)
    d.alpha_min, d.max_history = float(alpha_min), float(max_history)
    d.tol_position = 0.0 if tol_position is None else float(tol_position)
    d.cos_normal, d.min_history_variance, d.albedo_floor = float(cos_normal), float(min_history_variance), float(albedo_floor)
    torch.cuda.synchronize(dev)          # uploads and fills ran on torch's stream
    st = ffi.GpuStats()
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    h_prev = None if hp is None else C.byref(_history_struct(hp))
    h_next = _history_struct(hn)
    args = (ptr(c), ptr(p), ptr(n), ptr(i), ptr(a), ptr(vs), None if prev_view is None else C.byref(prev_view), ptr(pp), ptr(pn), ptr(pi),
            h_prev, C.byref(h_next), ptr(variance_out), C.c_void_p(stream or 0), C.byref(st))
    if cl is None:
        _check(lib().fjgpu_denoise_temporal(device, C.byref(d), *args))
    else:
        _check(lib().fjgpu_denoise_temporal_clamped(device, C.byref(d), C.byref(cl), *args))
    if to_host:
        return {k: t.cpu().numpy() for k, t in hn.items()}, variance_out.cpu().numpy(), st
    return hn, variance_out, st


class TemporalDenoiser(object):
    """A sequence of frames of one resident scene -- a turntable, a fly-through of a static set -- denoised with the history of the frames
    before (include/fjgpu.h: fjgpu_denoise_temporal in front of fjgpu_denoise_variance).  render(camera) runs, with every buffer on the
    device: Scene.set_camera; the beauty pass into a device framebuffer; one AOV call (position, normal, ids and, with demodulate, albedo);
    the spatial variance estimate of the current frame; temporal_accumulate against the previous frame's guides, view and history (the
    histories ping-pong between two sets of buffers); denoise_variance(variance=the temporal variance) on the accumulated colour.  The
    only copy to the host is the result's.  `params` are temporal_accumulate's alpha_min, max_history, tol_position, cos_normal,
    min_history_variance and denoise_variance's sigma_luminance, iterations, sigma_normal, sigma_position, stop_at_ids, albedo_floor.
    tol_position / sigma_position not given: TOL_POSITION_FRACTION / SIGMA_POSITION_FRACTION_VARIANCE of the diagonal of the bounding
    box of the first frame's foreground (a frame without foreground switches the terms off).  variance="samples": the beauty pass's sample
    variance (Scene.render_tiles(variance=...), the AOV call in front of it) is temporal_accumulate's variance_spatial -- the fallback for
    short histories -- and the spatial estimate is not run (info["estimate_stats"] is None); "spatial", the default, estimates it from
    the frame.  clamp: temporal_accumulate's -- None, the default, or e.g. (CLAMP_RADIUS, CLAMP_GAMMA): the history is clipped to the
    current frame's neighbourhood before the blend.  The limits are the entry's: static scene,
    static camera per frame, fixed-grid sampler.  reseed=False, the default: the scene's "sampler_seed" is left alone, and frames from one and
    the same camera are identical and gain nothing; reseed=True: frame k of the sequence renders (beauty and AOV pass) under seed
    1 + (k mod 65535) and the scene's own seed is put back after it, so that the frames of a standing camera are independent draws.
    The AOV pass's position is the hit of the pixel's nearest own sample, 0.28 pixels from the pixel's centre on average, and a seed moves
    it about; projected as it is, even a camera that stands fetches its history beside the pixel it came from and resamples it every
    frame.  So under reseed, and for any frame whose camera has not moved since the frame before, the point that is reprojected is slid
    at its own depth onto the ray through the pixel's centre (info["aov"]["position"] is the point used), and for a camera that has not
    moved the fetch is keyed by the pixel, so that every pixel's history is its own: a repeated frame leaves the accumulated colour as
    it is, and reseeded frames average.  The Cornell box from one camera, mse against 12 x 12 spp: 0.177 at frame 1, 0.033 at frame 8
    under reseed; 0.181 at every frame without.  A camera that moves every frame without reseed is the pass as it always was."""

    _TEMPORAL = ("alpha_min", "max_history", "tol_position", "cos_normal", "min_history_variance")
    _FILTER = ("sigma_luminance", "iterations", "sigma_normal", "sigma_position", "stop_at_ids")

    def __init__(self, scene, render, demodulate=True, stream=None, variance="spatial", clamp=None, reseed=False, **params):
        for k in params:
            if k not in self._TEMPORAL + self._FILTER + ("albedo_floor",):
                raise ValueError("unknown parameter %r" % k)
        if variance not in ("spatial", "samples"):
            raise ValueError("variance is \"spatial\" or \"samples\", not %r" % (variance,))
        self.variance = variance
        _temporal_clamp(clamp)               # (refuses what temporal_accumulate would)
        self.clamp = clamp
        self.reseed = bool(reseed)
        self.scene, self.render_desc, self.demodulate, self.stream = scene, render.copy(), bool(demodulate), stream
        self.params = dict(params)
        self.albedo_floor = float(self.params.pop("albedo_floor", ALBEDO_FLOOR))
        self.frames = 0
        self._prev = None            # (view, aov tensors, history tensors) of the frame before
        self._spare = None           # the history buffers the next frame writes

    @staticmethod
    def _centre_position(position, ids, view):
        """`position` [H, W, 3] moved to the pixel's centre: every foreground pixel's point slid, at its own depth in camera space, onto
        the ray through (x + .5, y + .5) -- the inverse of the projection written out at fjgpu_scene_view (include/fjgpu.h), in f64,
        rounded to f32 once.  The point moves by less than a pixel's footprint and projects through `view` onto its own pixel."""
        import torch
        dev = position.device
        M = torch.tensor(list(view.world_to_camera), dtype=torch.float64, device=dev).reshape(3, 4)
        R, t = M[:, :3], M[:, 3]
        c = position.double() @ R.T + t
        d = -c[..., 2]
        H, W = position.shape[:2]
        x = (torch.arange(W, dtype=torch.float64, device=dev) + .5) / view.xres
        y = (torch.arange(H, dtype=torch.float64, device=dev) + .5) / view.yres
        cx = (x[None, :] - .5) * view.uv_size[0] * d
        cy = (.5 - y[:, None]) * view.uv_size[1] * d
        moved = ((torch.stack([cx, cy, c[..., 2]], dim=-1) - t) @ torch.linalg.inv(R).T).float()
        ok = (ids[..., :1] >= 0) & (d > 0)[..., None] & torch.isfinite(moved).all(dim=-1, keepdim=True)
        return torch.where(ok, moved, position)

    def reset(self):
        """drop the history: the next frame is the first of a sequence"""
        self._prev = None
        self.frames = 0

    def render(self, camera=None, keep_inputs=False):
        """one frame -> (numpy [H, W, 4] float32, info).  camera: an ffi.CameraDesc, or a dict of Scene.set_camera's overrides, or None
        (the scene's current camera).  info: "beauty_stats", "aov_stats", "estimate_stats", "temporal_stats", "denoise_stats" (GpuStats),
        "tol_position", "sigma_position" (the values used), "frame" (0 for the first of a sequence) and, with keep_inputs, "beauty",
        "aov", "variance_spatial" [H, W] (the temporal pass's fallback: the estimate, or the sample variance), "accumulated",
        "history_length" [H, W] and "variance" [H, W] (the temporal pass's) and, with a clamp, "clamp_amount" [H, W] as numpy copies."""
        import torch
        sc, r = self.scene, self.render_desc
        dev = torch.device("cuda", sc._device)
        region = tuple(int(v) for v in r.region)
        if camera is not None:
            sc.set_camera(**camera) if isinstance(camera, dict) else sc.set_camera(camera)
        view = sc.view(r)            # (the refusals of the AOV pass, before anything is rendered)
        fb = torch.zeros((r.yres, r.xres, 4), dtype=torch.float32, device=dev)
        torch.cuda.synchronize(dev)          # the fill ran on torch's stream
        want = ("position", "normal", "ids") + (("albedo",) if self.demodulate else ())
        var_s = None
        seed_before = int(sc.query("sampler_seed")) if self.reseed else None
        try:
            if self.reseed:
                sc.set_option("sampler_seed", 1 + self.frames % 65535)
            if self.variance == "samples":       # (the AOV call first: the sample variance is taken under its albedo)
                aov, st_aov = sc._render_aov_device(r, want=want, stream=self.stream, names=AOV_ALL if self.demodulate else AOV_NAMES)
                var_s = torch.zeros((r.yres, r.xres), dtype=torch.float32, device=dev)
                torch.cuda.synchronize(dev)
                st_beauty = sc.render_tiles(r, None, fb.data_ptr(), stream=self.stream, variance=var_s.data_ptr(),
                                            albedo=aov["albedo"].data_ptr() if self.demodulate else None, albedo_floor=self.albedo_floor)
            else:
                st_beauty = sc.render_tiles(r, None, fb.data_ptr(), stream=self.stream)
                aov, st_aov = sc._render_aov_device(r, want=want, stream=self.stream, names=AOV_ALL if self.demodulate else AOV_NAMES)
            standing = self._prev is not None and bytes(view) == bytes(self._prev[0])
            if self.reseed or standing:
                # the position that is reprojected lies on the ray through the pixel's CENTRE.  The AOV pass's position is the nearest own
                # sample's, 0.28 pixels from the centre on average: a camera that stands would fetch its history beside the pixel it came
                # from, every frame, and a seed moves that sample about from frame to frame
                aov["position"] = self._centre_position(aov["position"], aov["ids"], view)
        finally:
            if self.reseed:
                sc.set_option("sampler_seed", seed_before)
        p = self.params
        if "tol_position" not in p or p.get("sigma_position") is None:
            x0, y0, x1, y1 = region
            pos = aov["position"][y0:y1, x0:x1].reshape(-1, 3)
            keep = (aov["ids"][y0:y1, x0:x1, 0].reshape(-1) >= 0) & torch.isfinite(pos).all(dim=1)
            diag = 0.0
            if bool(keep.any()):
                q = pos[keep].double()
                diag = float(torch.linalg.norm(q.max(dim=0).values - q.min(dim=0).values))
            p.setdefault("tol_position", TOL_POSITION_FRACTION * diag)
            if p.get("sigma_position") is None:
                p["sigma_position"] = SIGMA_POSITION_FRACTION_VARIANCE * diag
        tkw = {k: p[k] for k in self._TEMPORAL if k in p}
        fkw = {k: p[k] for k in self._FILTER if k in p}
        albedo = aov.get("albedo")
        st_est = None                        # (variance="samples": no estimate, the beauty pass wrote var_s)
        if var_s is None:
            var_s, st_est = _estimate_variance_device(fb, aov["normal"], aov["position"], aov["ids"], albedo, self.albedo_floor, region,
                                                      fkw.get("sigma_normal", SIGMA_NORMAL), fkw["sigma_position"], fkw.get("stop_at_ids", True),
                                                      sc._device, self.stream)
        prev = self._prev
        amount = torch.zeros((r.yres, r.xres), dtype=torch.float32, device=dev) if (self.clamp is not None and keep_inputs) else None
        ids_t, prev_ids_t = aov["ids"], prev[1]["ids"] if prev else None
        clamp_stops = isinstance(self.clamp, dict) and self.clamp.get("stop_at_ids", CLAMP_STOP_AT_IDS)
        if standing and not clamp_stops:
            # a camera that has not moved reprojects every pixel onto ITSELF.  The slid position lands there up to f32's rounding of the
            # point, some 2e-6 pixels, and a neighbour tap of that weight still leaks into a dark pixel beside a bright one (measured:
            # 2e-3 relative per frame).  So the fetch is keyed by the pixel: where both frames show the same instance the id the pass
            # compares is the pixel's index, and only the pixel's own tap counts.  The guides that are kept and filtered are the true ones.
            own = aov["ids"][..., 0]
            index = torch.arange(own.numel(), dtype=torch.int32, device=dev).reshape(own.shape)
            ids_t, prev_ids_t = aov["ids"].clone(), prev[1]["ids"].clone()
            ids_t[..., 0] = torch.where(own >= 0, index, own)
            prev_ids_t[..., 0] = torch.where((own >= 0) & (prev[1]["ids"][..., 0] == own), index, torch.full_like(own, -2))
        hist, var_t, st_tmp = temporal_accumulate(
            fb, aov["position"], aov["normal"], ids_t, albedo=albedo, variance_spatial=var_s,
            prev_view=prev[0] if prev else None, prev_position=prev[1]["position"] if prev else None,
            prev_normal=prev[1]["normal"] if prev else None, prev_ids=prev_ids_t, prev=prev[2] if prev else None,
            next=self._spare, region=region, albedo_floor=self.albedo_floor, device=sc._device, stream=self.stream, to_host=False,
            clamp=self.clamp, clamp_amount=amount, **tkw)
        out = torch.zeros_like(fb)
        res, st_dn = denoise_variance(hist["color"], aov["normal"], aov["position"], aov["ids"], albedo=albedo, variance=var_t, region=region,
                                      device=sc._device, stream=self.stream, out=out, albedo_floor=self.albedo_floor, **fkw)
        info = dict(beauty_stats=st_beauty, aov_stats=st_aov, estimate_stats=st_est, temporal_stats=st_tmp, denoise_stats=st_dn,
                    tol_position=p["tol_position"], sigma_position=p["sigma_position"], frame=self.frames)
        if keep_inputs:
            info["beauty"] = fb.cpu().numpy()
            info["aov"] = {name: t.cpu().numpy() for name, t in aov.items()}
            info["variance_spatial"] = var_s.cpu().numpy()
            info["accumulated"] = hist["color"].cpu().numpy()
            info["history_length"] = hist["length"].cpu().numpy()
            info["variance"] = var_t.cpu().numpy()
            if amount is not None:
                info["clamp_amount"] = amount.cpu().numpy()
        # ping-pong: what this frame read is what the next one writes
        self._spare = prev[2] if prev else None
        self._prev = (view, aov, hist)
        self.frames += 1
        return res, info


def build_config(name):
    """what the loaded library was compiled with (fjgpu_build_config): "stack_lds*", "*_validate"; no device needed"""
    v = C.c_double(0)
    _check(lib().fjgpu_build_config(name.encode(), C.byref(v)))
    return v.value


def global_option(name, value):
    """process-wide option of the core, e.g. global_option("device_build", 1)"""
    _check(lib().fjgpu_global_option(name.encode(), int(value)))


def host_xorshift_f01_seeded(seed, n):
    """the first n draws of the jitter / time stream under option "sampler_seed" = seed (include/fjgpu.h); no device needed"""
    out = np.zeros(max(int(n), 0), dtype=np.float64)
    lib().fjgpu_host_xorshift_f01_seeded(int(seed), int(n), out.ctypes.data_as(C.c_void_p))
    return out


def tile_count(render):
    return lib().fjgpu_tile_count(C.byref(render))


def rccl_selftest(device=0, n_floats=1 << 20):
    """RCCL bring-up on one device through the core's own loader (include/fjgpu.h: fjgpu_dev_rccl_selftest)"""
    _check(lib().fjgpu_dev_rccl_selftest(device, n_floats))


def sort_pairs(keys, key_bits, device=0, repeats=1):
    """the ray-queue sort on its own (include/fjgpu.h: fjgpu_dev_sort_pairs): (keys[i], i) pairs, stable, over the low key_bits
    bits -> (sorted keys, perm, milliseconds of the fastest of `repeats` device-side runs)"""
    keys = np.ascontiguousarray(keys, dtype=np.uint32)
    out, perm = np.empty_like(keys), np.empty_like(keys)
    ms = C.c_double(0)
    _check(lib().fjgpu_dev_sort_pairs(device, keys.ctypes.data_as(C.c_void_p), int(keys.size), int(key_bits),
                                      out.ctypes.data_as(C.c_void_p), perm.ctypes.data_as(C.c_void_p), int(repeats), C.byref(ms)))
    return out, perm, ms.value


def slab32_batch(rays, grid, words, device=0):
    """the walks' slab tests on their own (include/fjgpu.h: fjgpu_dev_slab32_batch): rays [n, 8] (o, d, tmin, tmax), grid [n, 6], words [n, 3]
    -> [n] 128-byte records as uint8 [n, 128] (Slab32Probe of csrc/device/fjgpu_slab32.h)"""
    rays = np.ascontiguousarray(rays, dtype=np.float64)
    grid = np.ascontiguousarray(grid, dtype=np.float64)
    words = np.ascontiguousarray(words, dtype=np.uint32)
    n = int(rays.shape[0])
    assert rays.shape == (n, 8) and grid.shape == (n, 6) and words.shape == (n, 3)
    out = np.zeros((n, 128), np.uint8)
    _check(lib().fjgpu_dev_slab32_batch(device, n, rays.ctypes.data_as(C.c_void_p), grid.ctypes.data_as(C.c_void_p),
                                        words.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)))
    return out


def quantize_nodes(nodes, origin, cell, device=0):
    """k_quantize_nodes on its own (include/fjgpu.h: fjgpu_dev_quantize_nodes): nodes = [n] 128-byte DNode records (any dtype of that size)
    -> uint8 [n, 64] (DNodeQ records)"""
    nodes = np.ascontiguousarray(nodes)
    assert nodes.dtype.itemsize == 128 and nodes.ndim == 1
    origin = np.ascontiguousarray(origin, dtype=np.float64)
    cell = np.ascontiguousarray(cell, dtype=np.float64)
    out = np.zeros((len(nodes), 64), np.uint8)
    _check(lib().fjgpu_dev_quantize_nodes(device, int(len(nodes)), nodes.ctypes.data_as(C.c_void_p), origin.ctypes.data_as(C.c_void_p),
                                          cell.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)))
    return out


def tile_rect(render, tile_id):
    r = (C.c_int32 * 4)()
    _check(lib().fjgpu_tile_rect(C.byref(render), tile_id, r))
    return tuple(r)


def pack_tiles(fb_ptr, xres, rects_ptr, n_tiles, tile_px, slab_ptr, stream=None):
    """device framebuffer -> tile slab (include/fjgpu.h: fjgpu_pack_tiles); raw device pointers"""
    _check(lib().fjgpu_pack_tiles(fb_ptr, xres, rects_ptr, n_tiles, tile_px, slab_ptr, stream))


def unpack_tiles(fb_ptr, xres, rects_ptr, n_tiles, tile_px, slab_ptr, stream=None):
    _check(lib().fjgpu_unpack_tiles(fb_ptr, xres, rects_ptr, n_tiles, tile_px, slab_ptr, stream))
