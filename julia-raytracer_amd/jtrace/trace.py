"""Trace module host mirror — src/trace.jl's public surface over the HIP C-ABI.

    make_trace_lights(scene)        src/trace.jl:117   -> jt_make_lights
    make_scene_bvh(scene, hq)       src/bvh.jl:66      -> jt_build_scene_bvh
    TraceState / make_trace_state   src/trace.jl:87,189 -> jt_create (device context)
    trace_samples(state)            src/trace.jl:215   -> jt_trace_samples (one batch)
    get_image(state)                src/trace.jl:676   -> jt_get_image
    state.denoise() / denoise_image / denoise_defaults (the build's own) -> jt_denoise, jt_get_denoised,
                                                       jt_denoise_image, jt_denoise_defaults
    state.variance() / state.noise() (the build's own) -> jt_get_variance, jt_get_noise
    state.denoise_guided() / denoise_guided_image / denoise_guided_defaults (the build's own)
                                                       -> jt_denoise_guided, jt_denoise_guided_image,
                                                       jt_denoise_guided_defaults
    state.adapt() / state.sample_counts() (the build's own) -> jt_adapt, jt_get_sample_counts
    state.intersect() / state.occluded()   src/bvh.jl:306 -> jt_intersect, jt_occluded (and their
                                                       device-pointer variants for torch tensors)

There is no CPU fallback anywhere in this module: every call goes through libjtrace_hip.so.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import abi


class SceneBvh:
    """Owns a jt_scene_bvh built by the library (make_scene_bvh, src/bvh.jl:66-88)."""

    def __init__(self, scene_abi: abi.SceneABI, high_quality: bool = False, lib=None):
        self.lib = lib or abi.load_library()
        self.struct = abi.jt_scene_bvh()
        abi.check(self.lib, self.lib.jt_build_scene_bvh(scene_abi.ref, int(high_quality), C.byref(self.struct)))

    @property
    def ref(self):
        return C.byref(self.struct)

    def tree(self, which: int = -1):
        """(nodes structured array, primitives) of the TLAS (which=-1) or BLAS `which`."""
        t = self.struct.tlas if which < 0 else self.struct.blas[which]
        nodes = np.ctypeslib.as_array(C.cast(t.nodes, C.POINTER(C.c_uint8)), shape=(t.nnodes * 32,))
        dt = np.dtype([("bmin", "<f4", 3), ("bmax", "<f4", 3), ("start", "<i4"), ("num", "<i2"),
                       ("axis", "i1"), ("internal", "i1")])
        prims = np.ctypeslib.as_array(t.primitives, shape=(t.nprimitives,)) if t.nprimitives else np.zeros(0, np.int32)
        return nodes.view(dt).copy(), prims.copy()

    def __del__(self):
        if getattr(self, "lib", None) is not None and getattr(self, "struct", None) is not None:
            self.lib.jt_free_scene_bvh(C.byref(self.struct))


class TraceLights:
    """Owns a jt_lights built by the library (make_trace_lights, src/trace.jl:117-187)."""

    def __init__(self, scene_abi: abi.SceneABI, lib=None):
        self.lib = lib or abi.load_library()
        self.struct = abi.jt_lights()
        abi.check(self.lib, self.lib.jt_make_lights(scene_abi.ref, C.byref(self.struct)))

    @property
    def ref(self):
        return C.byref(self.struct)

    def cdfs(self):
        out = []
        for k in range(self.struct.nlights):
            light = self.struct.lights[k]
            out.append((light.instance, light.environment,
                        np.ctypeslib.as_array(light.cdf, shape=(light.ncdf,)).copy()))
        return out

    def __del__(self):
        if getattr(self, "lib", None) is not None and getattr(self, "struct", None) is not None:
            self.lib.jt_free_lights(C.byref(self.struct))


def make_scene_bvh(scene_abi, high_quality=False, lib=None) -> SceneBvh:
    return SceneBvh(scene_abi, high_quality, lib)


def make_trace_lights(scene_abi, lib=None) -> TraceLights:
    return TraceLights(scene_abi, lib)


def image_size(scene_abi, params: abi.jt_params, lib=None):
    lib = lib or abi.load_library()
    w, h = C.c_int32(), C.c_int32()
    abi.check(lib, lib.jt_image_size(scene_abi.ref, C.byref(params), C.byref(w), C.byref(h)))
    return w.value, h.value


class TraceState:
    """Device-resident TraceState (src/trace.jl:87-100): running-mean image/albedo/normal/hits."""

    def __init__(self, scene_abi, bvh: SceneBvh, lights: TraceLights, params: abi.jt_params, lib=None,
                 devices=None):
        """devices: None for one context on params.device (jt_create), or a list of HIP
        ordinals for one context over those GPUs (jt_create_multi: every batch sharded across
        them, the running means reduced with RCCL when read)."""
        self.lib = lib or abi.load_library()
        self._keep = (scene_abi, bvh, lights)
        self.params = params
        h = C.c_void_p()
        if devices is None:
            abi.check(self.lib, self.lib.jt_create(scene_abi.ref, bvh.ref, lights.ref, C.byref(params), C.byref(h)))
        else:
            devs = (C.c_int32 * len(devices))(*devices)
            abi.check(self.lib, self.lib.jt_create_multi(scene_abi.ref, bvh.ref, lights.ref, C.byref(params), devs,
                                                         len(devices), C.byref(h)))
        self.devices = devices
        self.handle = h
        w, hh = C.c_int32(), C.c_int32()
        abi.check(self.lib, self.lib.jt_get_size(self.handle, C.byref(w), C.byref(hh)))
        self.width, self.height = w.value, hh.value

    # --- trace.jl surface
    def trace_samples(self):
        abi.check(self.lib, self.lib.jt_trace_samples(self.handle))

    def trace_range(self, s0: int, s1: int):
        abi.check(self.lib, self.lib.jt_trace_range(self.handle, int(s0), int(s1)))

    @property
    def samples(self) -> int:
        n = C.c_int32()
        abi.check(self.lib, self.lib.jt_get_samples(self.handle, C.byref(n)))
        return n.value

    @property
    def streams(self) -> int:
        """Sample streams per pixel k (jt_get_streams): local sample t goes to stream t mod k, and
        the image is the streams' running means combined in stream order (include/jtrace.h)."""
        n = C.c_int32()
        abi.check(self.lib, self.lib.jt_get_streams(self.handle, C.byref(n)))
        return n.value

    def get_image(self) -> np.ndarray:
        out = np.empty((self.height, self.width, 4), np.float32)
        abi.check(self.lib, self.lib.jt_get_image(self.handle, out.ctypes.data_as(abi.f32p)))
        return out

    def get_aovs(self):
        n = self.width * self.height
        alb = np.empty((self.height, self.width, 3), np.float32)
        nrm = np.empty((self.height, self.width, 3), np.float32)
        hits = np.empty((self.height, self.width), np.int64)
        abi.check(self.lib, self.lib.jt_get_aovs(self.handle, alb.ctypes.data_as(abi.f32p),
                                                 nrm.ctypes.data_as(abi.f32p),
                                                 hits.ctypes.data_as(C.POINTER(C.c_int64))))
        del n
        return alb, nrm, hits

    def _denoised(self, entry: str, params, defaults, overrides) -> np.ndarray:
        """The context filter `entry` (jt_denoise or jt_denoise_guided), then jt_get_denoised."""
        if overrides and params is None:
            params = defaults()
        params = _with_overrides(params, overrides)
        abi.check(self.lib, getattr(self.lib, entry)(self.handle, None if params is None else C.byref(params)))
        out = np.empty((self.height, self.width, 4), np.float32)
        abi.check(self.lib, self.lib.jt_get_denoised(self.handle, out.ctypes.data_as(abi.f32p)))
        return out

    def denoise(self, params: abi.jt_denoise_params | None = None, **overrides) -> np.ndarray:
        """jt_denoise then jt_get_denoised: the (H, W, 4) float32 a-trous filter of the running
        means (include/jtrace.h). params None: the defaults for the samples traced so far;
        overrides replace single fields (iterations, sigma_color, ...) of either."""
        return self._denoised("jt_denoise", params, lambda: denoise_defaults(self.samples, self.lib), overrides)

    def denoise_guided(self, params: abi.jt_denoise_guided_params | None = None, **overrides) -> np.ndarray:
        """jt_denoise_guided then jt_get_denoised: the (H, W, 4) float32 variance-guided a-trous
        filter of the running means, its colour tolerance the per-pixel variance of
        jt_get_variance (include/jtrace.h). Needs k > 1 streams and two samples. params None: the
        defaults; overrides replace single fields (iterations, sigma_variance, ...) of either."""
        return self._denoised("jt_denoise_guided", params, lambda: denoise_guided_defaults(self.lib), overrides)

    def variance(self) -> np.ndarray:
        """jt_get_variance: the (H, W, 4) float32 variance of the image per channel (of the mean,
        not of one sample), from the spread of the sample streams' means. Needs k > 1 streams
        and two samples (include/jtrace.h)."""
        out = np.empty((self.height, self.width, 4), np.float32)
        abi.check(self.lib, self.lib.jt_get_variance(self.handle, out.ctypes.data_as(abi.f32p)))
        return out

    def noise(self) -> float:
        """jt_get_noise: the image's relative RMS error, sqrt(mean channel variance) / mean
        channel value over the pixels this context traces."""
        v = C.c_double()
        abi.check(self.lib, self.lib.jt_get_noise(self.handle, C.byref(v)))
        return v.value

    def adapt(self, noise_target: float) -> int:
        """jt_adapt: freezes the 8x8 tiles whose error estimate meets the image-level noise target
        (later trace calls skip them) and returns the traced tiles still active. Needs k > 1
        streams and a sample count that is a multiple of k (include/jtrace.h)."""
        n = C.c_int32()
        abi.check(self.lib, self.lib.jt_adapt(self.handle, float(noise_target), C.byref(n)))
        return n.value

    @property
    def adaptive(self):
        """(active, traced) tiles of jt_describe's adaptive= field; None before the first adapt()."""
        for tok in self.describe().split():
            if tok.startswith("adaptive="):
                a, t = tok.split("=", 1)[1].split("/")
                return int(a), int(t)
        return None

    def sample_counts(self) -> np.ndarray:
        """jt_get_sample_counts: (H, W) int32, the samples behind every pixel: the count at which
        its tile froze, the context's samples for an active tile, 0 outside a tile share."""
        out = np.empty((self.height, self.width), np.int32)
        abi.check(self.lib, self.lib.jt_get_sample_counts(self.handle, out.ctypes.data_as(abi.i32p)))
        return out

    # --- ray queries (jt_intersect, jt_occluded: include/jtrace.h)
    def _device_rays(self, rays, instance=None):
        """A torch tensor of rays (and of instance ids) checked for the zero-copy path: (torch, n)."""
        import torch
        dev = int(self.params.device)
        if self.devices is not None:
            raise abi.JTError(-2, "ray queries are not available on a multi-device context")
        for name, t, dtype, shape in (("rays", rays, torch.float32, (len(rays), 6)),
                                      ("instance", instance, torch.int32, (len(rays),))):
            if t is None:
                continue
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.device.index == dev and t.dtype == dtype
                    and tuple(t.shape) == shape and t.is_contiguous()):
                raise ValueError(f"{name}: expected a contiguous {dtype} tensor of shape {shape} on cuda:{dev}")
        # the library reads on the context's own stream: what produced the tensors must be done
        torch.cuda.current_stream(dev).synchronize()
        return torch, len(rays)

    def _bounds(self, rays, tmax):
        """tmax of a bounded query, a scalar or (n,), as what the library reads: a float32 (n,) numpy
        array for numpy rays, a contiguous float32 tensor on the rays' device for torch rays."""
        n = len(rays)
        if hasattr(rays, "data_ptr"):
            import torch
            if isinstance(tmax, torch.Tensor):
                t = tmax.to(device=rays.device, dtype=torch.float32)
            else:
                t = torch.as_tensor(np.asarray(tmax, np.float32), device=rays.device)
            t = t.expand(n).contiguous() if t.dim() == 0 else t.contiguous()
            torch.cuda.current_stream(rays.device.index).synchronize()
        else:
            if hasattr(tmax, "data_ptr"):
                tmax = tmax.cpu().numpy()
            t = np.asarray(tmax, np.float32)
            t = np.full(n, t, np.float32) if t.ndim == 0 else np.ascontiguousarray(t)
        if tuple(t.shape) != (n,):
            raise ValueError(f"tmax: expected a scalar or shape ({n},), got {tuple(t.shape)}")
        return t

    def intersect(self, rays, instance=None, tmax=None):
        """jt_intersect: the closest hit of every ray (n, 6) = (origin, direction) on the context's
        scene, in the context's traversal; instance: None, or per ray -1 (the scene) or an
        instance id (that instance only). A float32 numpy array gives a structured array with
        jt_hit's fields (abi.HIT_DTYPE); a torch tensor on the context's device goes zero-copy
        through jt_intersect_device and gives an int32 (n, 6) tensor of the records (split_hits
        names the fields). tmax (a scalar or (n,)): jt_intersect_bounded, the query of the ray
        that ends at t = tmax, a hit exactly there included; None: unbounded."""
        if tmax is not None:
            return self._intersect_bounded(rays, instance, self._bounds(rays, tmax))
        if hasattr(rays, "data_ptr"):
            torch, n = self._device_rays(rays, instance)
            out = torch.empty((n, 6), dtype=torch.int32, device=rays.device)
            abi.check(self.lib, self.lib.jt_intersect_device(self.handle, n, rays.data_ptr(),
                                                             None if instance is None else instance.data_ptr(),
                                                             out.data_ptr()))
            return out
        rays = _host_rays(rays)
        n = len(rays)
        ip = None
        if instance is not None:
            instance = np.ascontiguousarray(instance, np.int32)
            if instance.shape != (n,):
                raise ValueError(f"instance: expected shape ({n},), got {instance.shape}")
            ip = instance.ctypes.data_as(abi.i32p)
        out = np.empty(n, abi.HIT_DTYPE)
        abi.check(self.lib, self.lib.jt_intersect(self.handle, n, rays.ctypes.data_as(abi.f32p), ip,
                                                  out.ctypes.data_as(C.POINTER(abi.jt_hit))))
        return out

    def _intersect_bounded(self, rays, instance, tmax):
        if hasattr(rays, "data_ptr"):
            torch, n = self._device_rays(rays, instance)
            out = torch.empty((n, 6), dtype=torch.int32, device=rays.device)
            abi.check(self.lib, self.lib.jt_intersect_bounded_device(self.handle, n, rays.data_ptr(), tmax.data_ptr(),
                                                                     None if instance is None else instance.data_ptr(),
                                                                     out.data_ptr()))
            return out
        rays = _host_rays(rays)
        n = len(rays)
        ip = None
        if instance is not None:
            instance = np.ascontiguousarray(instance, np.int32)
            if instance.shape != (n,):
                raise ValueError(f"instance: expected shape ({n},), got {instance.shape}")
            ip = instance.ctypes.data_as(abi.i32p)
        out = np.empty(n, abi.HIT_DTYPE)
        abi.check(self.lib, self.lib.jt_intersect_bounded(self.handle, n, rays.ctypes.data_as(abi.f32p),
                                                          tmax.ctypes.data_as(abi.f32p), ip,
                                                          out.ctypes.data_as(C.POINTER(abi.jt_hit))))
        return out

    def occluded(self, rays, tmax=None):
        """jt_occluded: bool (n,), whether anything is hit along each ray (a numpy array, or for a
        torch tensor on the context's device a torch.bool tensor there, zero-copy). tmax (a scalar
        or (n,)): jt_occluded_bounded, anything within t <= tmax; None: unbounded."""
        if tmax is not None:
            tmax = self._bounds(rays, tmax)
            if hasattr(rays, "data_ptr"):
                torch, n = self._device_rays(rays)
                out = torch.empty(n, dtype=torch.uint8, device=rays.device)
                abi.check(self.lib, self.lib.jt_occluded_bounded_device(self.handle, n, rays.data_ptr(), tmax.data_ptr(),
                                                                        out.data_ptr()))
                return out != 0
            rays = _host_rays(rays)
            out = np.empty(len(rays), np.uint8)
            abi.check(self.lib, self.lib.jt_occluded_bounded(self.handle, len(rays), rays.ctypes.data_as(abi.f32p),
                                                             tmax.ctypes.data_as(abi.f32p), out.ctypes.data_as(abi.u8p)))
            return out != 0
        if hasattr(rays, "data_ptr"):
            torch, n = self._device_rays(rays)
            out = torch.empty(n, dtype=torch.uint8, device=rays.device)
            abi.check(self.lib, self.lib.jt_occluded_device(self.handle, n, rays.data_ptr(), out.data_ptr()))
            return out != 0
        rays = _host_rays(rays)
        out = np.empty(len(rays), np.uint8)
        abi.check(self.lib, self.lib.jt_occluded(self.handle, len(rays), rays.ctypes.data_as(abi.f32p),
                                                 out.ctypes.data_as(abi.u8p)))
        return out != 0

    def visible(self, segments):
        """jt_visible: bool (n,), whether nothing lies between the two ends of each segment (n, 6) =
        (a, b): 1 - occluded of the ray (a, b - a) bounded by 1 - ray_eps, so a surface through
        either end does not hide it. numpy gives numpy, a torch tensor on the context's device a
        torch.bool tensor there."""
        if hasattr(segments, "data_ptr"):
            torch, n = self._device_rays(segments)
            out = torch.empty(n, dtype=torch.uint8, device=segments.device)
            abi.check(self.lib, self.lib.jt_visible_device(self.handle, n, segments.data_ptr(), out.data_ptr()))
            return out != 0
        segments = _host_rays(segments)
        out = np.empty(len(segments), np.uint8)
        abi.check(self.lib, self.lib.jt_visible(self.handle, len(segments), segments.ctypes.data_as(abi.f32p),
                                                out.ctypes.data_as(abi.u8p)))
        return out != 0

    # --- all hits along a ray (jt_intersect_multi, jt_count_hits: include/jtrace.h)
    def _host_instance(self, instance, n):
        if instance is None:
            return None, None
        instance = np.ascontiguousarray(instance, np.int32)
        if instance.shape != (n,):
            raise ValueError(f"instance: expected shape ({n},), got {instance.shape}")
        return instance, instance.ctypes.data_as(abi.i32p)

    def intersect_multi(self, rays, k, instance=None, tmax=None):
        """jt_intersect_multi: the k nearest hits of every ray (n, 6), ordered by (t, instance,
        element), in one traversal: (records, counts). numpy rays give records (n, k) of abi.HIT_DTYPE
        (slots counts[i] .. k - 1 hold the miss record) and counts (n,) int32; a torch tensor on the
        context's device goes zero-copy through jt_intersect_multi_device and gives an int32
        (n, k, 6) tensor and an int32 (n,) tensor. instance and tmax as intersect's."""
        k = int(k)
        if tmax is not None:
            tmax = self._bounds(rays, tmax)
        if hasattr(rays, "data_ptr"):
            torch, n = self._device_rays(rays, instance)
            if not 1 <= k <= abi.MULTI_MAX_HITS:
                raise ValueError(f"k: expected 1 .. {abi.MULTI_MAX_HITS}, got {k}")
            out = torch.empty((n, k, 6), dtype=torch.int32, device=rays.device)
            counts = torch.empty(n, dtype=torch.int32, device=rays.device)
            abi.check(self.lib, self.lib.jt_intersect_multi_device(self.handle, n, rays.data_ptr(),
                                                                   None if tmax is None else tmax.data_ptr(),
                                                                   None if instance is None else instance.data_ptr(), k,
                                                                   out.data_ptr(), counts.data_ptr()))
            return out, counts
        rays = _host_rays(rays)
        n = len(rays)
        instance, ip = self._host_instance(instance, n)
        out = np.empty((n, max(k, 0)), abi.HIT_DTYPE)
        counts = np.empty(n, np.int32)
        abi.check(self.lib, self.lib.jt_intersect_multi(self.handle, n, rays.ctypes.data_as(abi.f32p),
                                                        None if tmax is None else tmax.ctypes.data_as(abi.f32p), ip, k,
                                                        out.ctypes.data_as(C.POINTER(abi.jt_hit)), counts.ctypes.data_as(abi.i32p)))
        return out, counts

    def count_hits(self, rays, tmax=None, instance=None):
        """jt_count_hits: int32 (n,), the primitives every ray crosses within ray_eps <= t <= tmax
        (None: unbounded), tmax held throughout; an odd count from outside a closed mesh means the
        origin is inside it. numpy gives numpy, a torch tensor on the context's device a tensor there."""
        if tmax is not None:
            tmax = self._bounds(rays, tmax)
        if hasattr(rays, "data_ptr"):
            torch, n = self._device_rays(rays, instance)
            counts = torch.empty(n, dtype=torch.int32, device=rays.device)
            abi.check(self.lib, self.lib.jt_count_hits_device(self.handle, n, rays.data_ptr(),
                                                              None if tmax is None else tmax.data_ptr(),
                                                              None if instance is None else instance.data_ptr(), counts.data_ptr()))
            return counts
        rays = _host_rays(rays)
        n = len(rays)
        instance, ip = self._host_instance(instance, n)
        counts = np.empty(n, np.int32)
        abi.check(self.lib, self.lib.jt_count_hits(self.handle, n, rays.ctypes.data_as(abi.f32p),
                                                   None if tmax is None else tmax.ctypes.data_as(abi.f32p), ip,
                                                   counts.ctypes.data_as(abi.i32p)))
        return counts

    def transmittance(self, rays, tmax=None, k: int = 8):
        """(T, complete): T = the product of (1 - opacity) over a ray's first k hits, nearest first,
        in float32, from surfaces() of intersect_multi's records; complete = counts < k, the list
        holds every hit of the ray. The opacity-aware visibility that the first-hit queries
        (occluded, visible, gbuffer) do not give. Python only: two library calls."""
        recs, counts = self.intersect_multi(rays, k, tmax=tmax)
        if hasattr(rays, "data_ptr"):
            n = len(rays)
            surf = split_surfaces(self.surfaces(rays.repeat_interleave(k, dim=0).contiguous(), recs.reshape(n * k, 6)))
            through = 1 - surf["opacity"].reshape(n, k)
            through[recs[:, :, 5] == 0] = 1
            T = through[:, 0].clone()
        else:
            rays = _host_rays(rays)
            surf = self.surfaces(np.repeat(rays, k, axis=0), recs.reshape(-1))
            through = np.where(recs["hit"] != 0, np.float32(1) - surf["opacity"].reshape(len(rays), k), np.float32(1)).astype(np.float32)
            T = through[:, 0].copy()
        for j in range(1, k):
            T = T * through[:, j]
        return T, counts < k

    # --- the surface at a hit (jt_eval_hits, jt_camera_rays, jt_gbuffer: include/jtrace.h)
    def _torch_device(self):
        """torch and the context's device, for the calls that return device tensors."""
        import torch
        if self.devices is not None:
            raise abi.JTError(-2, "surface evaluation and camera rays are not available on a multi-device context")
        dev = int(self.params.device)
        torch.cuda.current_stream(dev).synchronize()
        return torch, torch.device("cuda", dev)

    def camera_rays(self, sample: int = -1, device: bool = False):
        """jt_camera_rays: the (W*H, 6) float32 camera rays (origin, direction), row-major pixels.
        sample >= 0: the ray the integrator traces for (pixel, sample), bit for bit; -1: the
        deterministic ray through the pixel centre. device=True gives a torch tensor on the
        context's device (jt_camera_rays_device), else a numpy array."""
        n = self.width * self.height
        if device:
            torch, dev = self._torch_device()
            out = torch.empty((n, 6), dtype=torch.float32, device=dev)
            abi.check(self.lib, self.lib.jt_camera_rays_device(self.handle, int(sample), out.data_ptr()))
            return out
        out = np.empty((n, 6), np.float32)
        abi.check(self.lib, self.lib.jt_camera_rays(self.handle, int(sample), out.ctypes.data_as(abi.f32p)))
        return out

    def surfaces(self, rays, hits):
        """jt_eval_hits: the surface each hit record names, as seen along its ray: position,
        shading and element normal, texture coordinates, the material point. numpy rays (n, 6)
        and hits (abi.HIT_DTYPE) give a structured array (abi.SURFACE_DTYPE); torch tensors on the
        context's device (rays float32 (n, 6), hits int32 (n, 6) as intersect returns them) go
        zero-copy through jt_eval_hits_device and give a float32 (n, 24) tensor of the records
        (split_surfaces names the fields)."""
        if hasattr(rays, "data_ptr"):
            torch, n = self._device_rays(rays)
            if not (isinstance(hits, torch.Tensor) and hits.device == rays.device and hits.dtype == torch.int32
                    and tuple(hits.shape) == (n, 6) and hits.is_contiguous()):
                raise ValueError(f"hits: expected a contiguous int32 tensor of shape ({n}, 6) on {rays.device}")
            out = torch.empty((n, 24), dtype=torch.float32, device=rays.device)
            abi.check(self.lib, self.lib.jt_eval_hits_device(self.handle, n, rays.data_ptr(), hits.data_ptr(), out.data_ptr()))
            return out
        rays = _host_rays(rays)
        n = len(rays)
        hits = np.ascontiguousarray(hits)
        if hits.dtype != abi.HIT_DTYPE or hits.shape != (n,):
            raise ValueError(f"hits: expected shape ({n},) of abi.HIT_DTYPE, got {hits.shape} of {hits.dtype}")
        out = np.empty(n, abi.SURFACE_DTYPE)
        abi.check(self.lib, self.lib.jt_eval_hits(self.handle, n, rays.ctypes.data_as(abi.f32p),
                                                  hits.ctypes.data_as(C.POINTER(abi.jt_hit)),
                                                  out.ctypes.data_as(C.POINTER(abi.jt_surface))))
        return out

    def gbuffer(self, sample: int = -1, device: bool = False):
        """jt_gbuffer: (rays, hits, surfaces) of every pixel, row-major — camera_rays(sample), their
        closest hits in the context's traversal, and the surfaces there, with the bits of those
        three calls. The first geometric hit is reported: a surface with opacity < 1 is never
        passed through. device=True gives torch tensors on the context's device."""
        n = self.width * self.height
        if device:
            torch, dev = self._torch_device()
            rays = torch.empty((n, 6), dtype=torch.float32, device=dev)
            hits = torch.empty((n, 6), dtype=torch.int32, device=dev)
            surf = torch.empty((n, 24), dtype=torch.float32, device=dev)
            abi.check(self.lib, self.lib.jt_gbuffer_device(self.handle, int(sample), rays.data_ptr(), hits.data_ptr(),
                                                           surf.data_ptr()))
            return rays, hits, surf
        rays = np.empty((n, 6), np.float32)
        hits = np.empty(n, abi.HIT_DTYPE)
        surf = np.empty(n, abi.SURFACE_DTYPE)
        abi.check(self.lib, self.lib.jt_gbuffer(self.handle, int(sample), rays.ctypes.data_as(abi.f32p),
                                                hits.ctypes.data_as(C.POINTER(abi.jt_hit)),
                                                surf.ctypes.data_as(C.POINTER(abi.jt_surface))))
        return rays, hits, surf

    # --- radiance along the caller's rays (jt_radiance: include/jtrace.h)
    def radiance(self, rays, sample_begin: int = 0, sample_end: int = 1, stream_base: int = 0):
        """jt_radiance: the integrator's running mean of samples [sample_begin, sample_end) along
        every ray (n, 6) = (origin, unit direction), ray i drawing from the random stream of pixel
        stream_base + i: (n, 4) float32 rgba. A numpy array gives a numpy array; a torch tensor on
        the context's device goes zero-copy through jt_radiance_device and gives a tensor there.
        With camera_rays(s), the range [s, s + 1) and stream_base 0 it is the image of a context
        whose only sample is s, bit for bit. The context's image and counters are untouched."""
        if hasattr(rays, "data_ptr"):
            torch, n = self._device_rays(rays)
            out = torch.empty((n, 4), dtype=torch.float32, device=rays.device)
            abi.check(self.lib, self.lib.jt_radiance_device(self.handle, n, rays.data_ptr(), int(stream_base),
                                                            int(sample_begin), int(sample_end), out.data_ptr()))
            return out
        rays = _host_rays(rays)
        out = np.empty((len(rays), 4), np.float32)
        abi.check(self.lib, self.lib.jt_radiance(self.handle, len(rays), rays.ctypes.data_as(abi.f32p), int(stream_base),
                                                 int(sample_begin), int(sample_end), out.ctypes.data_as(abi.f32p)))
        return out

    # --- cosine-weighted gathers at the caller's points (jt_irradiance, jt_hemisphere_rays: include/jtrace.h)
    def irradiance(self, points, sample_begin: int = 0, sample_end: int = 1, stream_base: int = 0):
        """jt_irradiance: at every point (n, 6) = (position, normal) the integrator's running mean of
        samples [sample_begin, sample_end), each along a direction of its own drawn cosine-weighted
        about the normal from the stream of pixel stream_base + i: (n, 4) float32. pi * rgb is the
        irradiance, albedo * rgb what a matte surface there sends out, alpha the share of gather
        rays that met a surface or a visible environment. numpy gives numpy; a torch tensor on the
        context's device goes zero-copy through jt_irradiance_device and gives a tensor there. One
        sample s has the bits of radiance(hemisphere_rays(points, s), s, s + 1)."""
        if hasattr(points, "data_ptr"):
            torch, n = self._device_rays(points)
            out = torch.empty((n, 4), dtype=torch.float32, device=points.device)
            abi.check(self.lib, self.lib.jt_irradiance_device(self.handle, n, points.data_ptr(), int(stream_base),
                                                              int(sample_begin), int(sample_end), out.data_ptr()))
            return out
        points = _host_rays(points)
        out = np.empty((len(points), 4), np.float32)
        abi.check(self.lib, self.lib.jt_irradiance(self.handle, len(points), points.ctypes.data_as(abi.f32p), int(stream_base),
                                                   int(sample_begin), int(sample_end), out.ctypes.data_as(abi.f32p)))
        return out

    def hemisphere_rays(self, points, sample: int, stream_base: int = 0):
        """jt_hemisphere_rays: the (n, 6) float32 rays (origin, direction) irradiance starts sample
        `sample` of every point with: the position's bits and the cosine-weighted direction about
        the normal. numpy gives numpy, a torch tensor on the context's device a tensor there."""
        if hasattr(points, "data_ptr"):
            torch, n = self._device_rays(points)
            out = torch.empty((n, 6), dtype=torch.float32, device=points.device)
            abi.check(self.lib, self.lib.jt_hemisphere_rays_device(self.handle, n, points.data_ptr(), int(stream_base), int(sample),
                                                                   out.data_ptr()))
            return out
        points = _host_rays(points)
        out = np.empty((len(points), 6), np.float32)
        abi.check(self.lib, self.lib.jt_hemisphere_rays(self.handle, len(points), points.ctypes.data_as(abi.f32p), int(stream_base),
                                                        int(sample), out.ctypes.data_as(abi.f32p)))
        return out

    def ambient_occlusion(self, points, radius, sample_begin: int = 0, sample_end: int = 1, stream_base: int = 0):
        """jt_ambient_occlusion: at every point (n, 6) = (position, normal) the share of samples
        [sample_begin, sample_end) whose hemisphere_rays ray meets nothing within `radius` (> 0,
        inf: unbounded): (n,) float32 in [0, 1], 1 fully open. numpy gives numpy; a torch tensor on
        the context's device goes zero-copy through jt_ambient_occlusion_device and gives a tensor
        there. One sample s is 1 - occluded(hemisphere_rays(points, s), tmax=radius)."""
        if hasattr(points, "data_ptr"):
            torch, n = self._device_rays(points)
            out = torch.empty(n, dtype=torch.float32, device=points.device)
            abi.check(self.lib, self.lib.jt_ambient_occlusion_device(self.handle, n, points.data_ptr(), int(stream_base),
                                                                     int(sample_begin), int(sample_end), float(radius),
                                                                     out.data_ptr()))
            return out
        points = _host_rays(points)
        out = np.empty(len(points), np.float32)
        abi.check(self.lib, self.lib.jt_ambient_occlusion(self.handle, len(points), points.ctypes.data_as(abi.f32p), int(stream_base),
                                                          int(sample_begin), int(sample_end), float(radius),
                                                          out.ctypes.data_as(abi.f32p)))
        return out

    # --- spherical-harmonic radiance probes (jt_probe_sh, jt_sphere_rays: include/jtrace.h)
    def _device_points(self, points):
        """A torch tensor of (n, 3) positions checked for the zero-copy path: (torch, n)."""
        import torch
        dev = int(self.params.device)
        if self.devices is not None:
            raise abi.JTError(-2, "probes are not available on a multi-device context")
        if not (isinstance(points, torch.Tensor) and points.is_cuda and points.device.index == dev and points.dtype == torch.float32
                and tuple(points.shape) == (len(points), 3) and points.is_contiguous()):
            raise ValueError(f"points: expected a contiguous torch.float32 tensor of shape ({len(points)}, 3) on cuda:{dev}")
        torch.cuda.current_stream(dev).synchronize()
        return torch, len(points)

    def probe_sh(self, points, sample_begin: int = 0, sample_end: int = 1, stream_base: int = 0):
        """jt_probe_sh: at every point (n, 3) the running mean over samples [sample_begin,
        sample_end) of the integrator's rgba target along a uniform direction over the sphere, times
        the nine real spherical harmonics of bands 0..2 at that direction: (n, 9, 4) float32.
        jtrace.sh turns it into radiance coefficients (4 pi rgb) and irradiance. numpy gives numpy;
        a torch tensor on the context's device goes zero-copy through jt_probe_sh_device and gives a
        tensor there. One sample s is the fold step 0 * 0 + (radiance(sphere_rays(points, s), s,
        s + 1) * sh_basis(d)) * 1 in every bit."""
        if hasattr(points, "data_ptr"):
            torch, n = self._device_points(points)
            out = torch.empty((n, 9, 4), dtype=torch.float32, device=points.device)
            abi.check(self.lib, self.lib.jt_probe_sh_device(self.handle, n, points.data_ptr(), int(stream_base),
                                                            int(sample_begin), int(sample_end), out.data_ptr()))
            return out
        points = _host_points(points)
        out = np.empty((len(points), 9, 4), np.float32)
        abi.check(self.lib, self.lib.jt_probe_sh(self.handle, len(points), points.ctypes.data_as(abi.f32p), int(stream_base),
                                                 int(sample_begin), int(sample_end), out.ctypes.data_as(abi.f32p)))
        return out

    def sphere_rays(self, points, sample: int, stream_base: int = 0):
        """jt_sphere_rays: the (n, 6) float32 rays (origin, direction) probe_sh starts sample
        `sample` of every point (n, 3) with: the position's bits and the uniform direction over the
        sphere. numpy gives numpy, a torch tensor on the context's device a tensor there."""
        if hasattr(points, "data_ptr"):
            torch, n = self._device_points(points)
            out = torch.empty((n, 6), dtype=torch.float32, device=points.device)
            abi.check(self.lib, self.lib.jt_sphere_rays_device(self.handle, n, points.data_ptr(), int(stream_base), int(sample),
                                                               out.data_ptr()))
            return out
        points = _host_points(points)
        out = np.empty((len(points), 6), np.float32)
        abi.check(self.lib, self.lib.jt_sphere_rays(self.handle, len(points), points.ctypes.data_as(abi.f32p), int(stream_base),
                                                    int(sample), out.ctypes.data_as(abi.f32p)))
        return out

    def counters(self) -> dict:
        c = abi.jt_counters()
        abi.check(self.lib, self.lib.jt_get_counters(self.handle, C.byref(c)))
        return c.as_dict()

    def device_buffers(self) -> abi.jt_device_buffers:
        b = abi.jt_device_buffers()
        abi.check(self.lib, self.lib.jt_get_device_buffers(self.handle, C.byref(b)))
        return b

    def set_counters(self, level: int):
        abi.check(self.lib, self.lib.jt_set_counters(self.handle, int(level)))

    def describe(self) -> str:
        """Launch configuration of the next trace_range (kernel instance, scene mode, grid)."""
        buf = C.create_string_buffer(1024)
        abi.check(self.lib, self.lib.jt_describe(self.handle, buf, 1024))
        return buf.value.decode()

    @property
    def traversal(self) -> str:
        """The BVH traversal this context runs ("reference", "near" or "wide"): jt_params.traversal,
        with "auto" resolved by the library (wide for a scene in HBM mode with a stack bound above 32, near otherwise)."""
        for tok in self.describe().split():
            if tok.startswith("traversal="):
                return tok.split("=", 1)[1]
        raise RuntimeError("jt_describe reports no traversal")

    def reset(self):
        abi.check(self.lib, self.lib.jt_reset(self.handle))

    def synchronize(self):
        abi.check(self.lib, self.lib.jt_synchronize(self.handle))

    def close(self):
        if getattr(self, "handle", None):
            self.lib.jt_destroy(self.handle)
            self.handle = None

    def __del__(self):
        self.close()


def make_trace_state(scene_abi, bvh, lights, params, lib=None, devices=None) -> TraceState:
    return TraceState(scene_abi, bvh, lights, params, lib, devices)


def trace_samples(state: TraceState):
    state.trace_samples()


def get_image(state: TraceState) -> np.ndarray:
    return state.get_image()


def _host_rays(rays) -> np.ndarray:
    rays = np.ascontiguousarray(rays, np.float32)
    if rays.ndim != 2 or rays.shape[1] != 6:
        raise ValueError(f"rays: expected shape (n, 6) = (origin, direction), got {rays.shape}")
    return rays


def _host_points(points) -> np.ndarray:
    points = np.ascontiguousarray(points, np.float32)
    if points.ndim != 2 or points.shape[1] != 3:
        raise ValueError(f"points: expected shape (n, 3) = position, got {points.shape}")
    return points


def split_hits(records) -> dict:
    """The fields of TraceState.intersect's records, by name: a structured numpy array, or the
    int32 (n, 6) torch tensor of the device path (u, v, t reinterpreted as float32, no copy)."""
    if isinstance(records, np.ndarray):
        return {name: records[name] for name in abi.HIT_DTYPE.names}
    import torch
    return {name: records[:, k].view(torch.float32) if name in ("u", "v", "t") else records[:, k]
            for k, name in enumerate(abi.HIT_DTYPE.names)}


def split_surfaces(records) -> dict:
    """The fields of TraceState.surfaces' records, by name: a structured numpy array, or the
    float32 (n, 24) torch tensor of the device path (material, type and hit reinterpreted as
    int32, vectors as (n, 3) / (n, 2) column ranges, no copy)."""
    if isinstance(records, np.ndarray):
        return {name: records[name] for name in abi.SURFACE_DTYPE.names}
    import torch
    out, k = {}, 0
    for name in abi.SURFACE_DTYPE.names:
        dt, shape = abi.SURFACE_DTYPE[name].base, abi.SURFACE_DTYPE[name].shape
        w = shape[0] if shape else 1
        col = records[:, k:k + w] if shape else records[:, k]
        out[name] = col.view(torch.int32) if dt.kind == "i" else col
        k += w
    return out


def _with_overrides(params, overrides):
    if not overrides:
        return params
    p = type(params).from_buffer_copy(params)  # jt_denoise_params or jt_denoise_guided_params
    names = [name for name, _ in p._fields_]
    for name, value in overrides.items():
        if name not in names:
            raise TypeError(f"unknown denoise parameter {name!r} (one of {', '.join(names)})")
        setattr(p, name, value)
    return p


def denoise_defaults(samples: int, lib=None) -> abi.jt_denoise_params:
    """jt_denoise_defaults: the denoiser's parameters for a render of `samples` samples per pixel."""
    lib = lib or abi.load_library()
    p = abi.jt_denoise_params()
    abi.check(lib, lib.jt_denoise_defaults(int(samples), C.byref(p)))
    return p


def _filter_host_arrays(lib, entry: str, arrays, channels, device, params, defaults, overrides) -> np.ndarray:
    """The host-array filter `entry` (jt_denoise_image or jt_denoise_guided_image) on `arrays`,
    the first the image and all in the entry's argument order, (H, W, n) for the n of `channels`."""
    arrays = [np.ascontiguousarray(a, np.float32) for a in arrays]
    rgba = arrays[0]
    if rgba.ndim != 3 or any(a.shape != rgba.shape[:2] + (n,) for a, n in zip(arrays, channels)):
        raise ValueError(f"expected {', '.join(f'(H, W, {n})' for n in channels)} arrays, "
                         f"got {', '.join(str(a.shape) for a in arrays)}")
    p = _with_overrides(params if params is not None else defaults(), overrides)
    out = np.empty_like(rgba)
    abi.check(lib, getattr(lib, entry)(*(a.ctypes.data_as(abi.f32p) for a in arrays), rgba.shape[1], rgba.shape[0],
                                       C.byref(p), int(device), out.ctypes.data_as(abi.f32p)))
    return out


def denoise_image(rgba, albedo, normal, device: int = 0, params: abi.jt_denoise_params | None = None, samples: int = 1,
                  lib=None, **overrides) -> np.ndarray:
    """jt_denoise_image: the denoiser on host arrays (H, W, 4), (H, W, 3), (H, W, 3) -> (H, W, 4)
    float32, on HIP device `device`. params None: the defaults for `samples` samples per pixel;
    overrides replace single fields."""
    lib = lib or abi.load_library()
    return _filter_host_arrays(lib, "jt_denoise_image", (rgba, albedo, normal), (4, 3, 3), device, params,
                               lambda: denoise_defaults(samples, lib), overrides)


def denoise_guided_defaults(lib=None) -> abi.jt_denoise_guided_params:
    """jt_denoise_guided_defaults: the variance-guided denoiser's parameters (the same for every
    sample count: the variance carries it)."""
    lib = lib or abi.load_library()
    p = abi.jt_denoise_guided_params()
    abi.check(lib, lib.jt_denoise_guided_defaults(C.byref(p)))
    return p


def denoise_guided_image(rgba, variance, albedo, normal, device: int = 0,
                         params: abi.jt_denoise_guided_params | None = None, lib=None, **overrides) -> np.ndarray:
    """jt_denoise_guided_image: the variance-guided denoiser on host arrays (H, W, 4), (H, W, 4),
    (H, W, 3), (H, W, 3) -> (H, W, 4) float32, on HIP device `device`; variance as
    TraceState.variance() returns it. params None: the defaults; overrides replace single fields."""
    lib = lib or abi.load_library()
    return _filter_host_arrays(lib, "jt_denoise_guided_image", (rgba, variance, albedo, normal), (4, 4, 3, 3), device,
                               params, lambda: denoise_guided_defaults(lib), overrides)
