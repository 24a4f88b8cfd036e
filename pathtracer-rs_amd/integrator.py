"""Host mirror of the reference's integrator API over the HIP library.

Mirrors (reference file:line):
  SamplerBuilder::new(log, spp, &sample_bounds)          src/pathtracer/sampler/sobol.rs:35-60
  PathIntegrator::{new, preprocess, render,
                   render_single_pixel}                  src/pathtracer/integrator.rs:230,250,536,505
Construction matches src/main.rs:103-110:
    integrator = PathIntegrator(SamplerBuilder(spp, camera.film.get_sample_bounds()), max_depth)
    integrator.preprocess(scene); integrator.render(camera, scene)
render() accumulates into camera.film like the reference (callers clear() first for a fresh image).
"""
import ctypes as C
import os
import warnings

import numpy as np

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


class PtrsError(RuntimeError):
    pass


def load_library():
    """Loads libptrs_hip.so (built in-tree by build.py).  Fails loudly when it is missing."""
    global _LIB
    if _LIB is not None:
        return _LIB
    so = os.environ.get("PTRS_LIB") or os.path.join(_HERE, "libptrs_hip.so")  # PTRS_LIB: A/B builds of the same library
    if not os.path.exists(so):
        raise PtrsError("HIP library %s is missing: run `python -c 'import __graft_entry__ as g; g.build()'`. "
                        "There is no CPU fallback for the render path." % so)
    L = C.CDLL(so)
    L.ptrs_last_error.restype = C.c_char_p
    L.ptrs_build_id.restype = C.c_char_p
    if L.ptrs_abi_version() != 4:
        raise PtrsError("ABI version mismatch")
    structs = [abi.PtrsTexture, abi.PtrsMaterial, abi.PtrsMesh, abi.PtrsLight, abi.PtrsBvhNode, abi.PtrsSceneDesc, abi.PtrsCamera,
               abi.PtrsRenderParams, abi.PtrsStats, abi.PtrsHit]
    for i, s in enumerate(structs):
        if L.ptrs_abi_sizeof(i) != C.sizeof(s):
            raise PtrsError("ABI struct %s: library %d bytes, binding %d bytes" % (s.__name__, L.ptrs_abi_sizeof(i), C.sizeof(s)))
    if L.ptrs_abi_sizeof(11) != C.sizeof(abi.PtrsDenoiseParams):
        raise PtrsError("ABI struct PtrsDenoiseParams: library %d bytes, binding %d bytes" % (L.ptrs_abi_sizeof(11), C.sizeof(abi.PtrsDenoiseParams)))
    for i, s in ((12, abi.PtrsTileError), (13, abi.PtrsFilmErrorSummary), (14, abi.PtrsConvergeResult), (15, abi.PtrsAdaptiveCheck), (16, abi.PtrsAdaptiveResult)):
        if L.ptrs_abi_sizeof(i) != C.sizeof(s):
            raise PtrsError("ABI struct %s: library %d bytes, binding %d bytes" % (s.__name__, L.ptrs_abi_sizeof(i), C.sizeof(s)))
    L.ptrs_render_range.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ptrs_render_range_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ptrs_film_error.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ptrs_film_error_device.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ptrs_converge_schedule.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    L.ptrs_render_converged.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ptrs_render_tiles.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ptrs_render_tiles_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ptrs_render_adaptive.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ptrs_adaptive_freeze.argtypes = [C.c_void_p, C.c_uint32, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
    vp, u32 = C.c_void_p, C.c_uint32
    L.ptrs_render_aov_range.argtypes = [vp, vp, vp, u32, u32, u32, vp, vp, vp]
    L.ptrs_render_aov_range_device.argtypes = [vp, vp, vp, u32, u32, u32, vp, vp, vp, vp]
    L.ptrs_render_aov_tiles.argtypes = [vp, vp, vp, u32, u32, vp, u32, vp, vp, vp]
    L.ptrs_render_aov_tiles_device.argtypes = [vp, vp, vp, u32, u32, vp, u32, vp, vp, vp, vp]
    L.ptrs_render_aov_adaptive.argtypes = [vp, vp, vp, u32, vp, u32, vp, vp]
    L.ptrs_render_aov_adaptive_device.argtypes = [vp, vp, vp, u32, vp, u32, vp, vp, vp]
    L.ptrs_set_option.argtypes = [C.c_char_p, C.c_int64]
    L.ptrs_scene_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
    L.ptrs_get_option.argtypes = [C.c_char_p, C.POINTER(C.c_int64)]
    _LIB = L
    # A/B convenience of this Python host only (the library itself reads no environment): PTRS_OPT_<NAME>=<int>
    for k, v in os.environ.items():
        if k.startswith("PTRS_OPT_"):
            set_option(k[len("PTRS_OPT_"):].lower(), int(v))
    return L


def set_option(name, value):
    """ptrs_set_option: process-wide tuning knob (lanes, refill, refill_connect, vote, stack_lds, grid_mult, node_form,
    workspace_pct); none of them changes a result."""
    _check(load_library().ptrs_set_option(name.encode(), int(value)))


def get_option(name):
    v = C.c_int64()
    _check(load_library().ptrs_get_option(name.encode(), C.byref(v)))
    return v.value


class options:
    """Context manager: `with options(lanes=1, refill=0): ...` sets knobs and restores the previous values."""

    def __init__(self, **kw):
        self.kw, self.old = kw, {}

    def __enter__(self):
        for k, v in self.kw.items():
            self.old[k] = get_option(k)
            set_option(k, v)
        return self

    def __exit__(self, *a):
        for k, v in self.old.items():
            set_option(k, v)
        return False


def _check(rc):
    if rc != 0:
        raise PtrsError("ptrs error %d: %s" % (rc, _LIB.ptrs_last_error().decode() if _LIB is not None else "library not loaded"))


def round_up_pow2(v):
    return 1 << max(0, (int(v) - 1).bit_length())


class SamplerBuilder:
    """SobolSamplerBuilder (sobol.rs:25-78): spp is rounded up to a power of two with a warning."""

    def __init__(self, samples_per_pixel, sample_bounds):
        self.samples_per_pixel = round_up_pow2(samples_per_pixel)
        if self.samples_per_pixel != samples_per_pixel:
            warnings.warn("non power-of-two sample count rounded up to %d for sobol sampler" % self.samples_per_pixel)
        self.sample_bounds = tuple(sample_bounds)
        ext = max(self.sample_bounds[2] - self.sample_bounds[0], self.sample_bounds[3] - self.sample_bounds[1])
        self.resolution = round_up_pow2(ext)
        self.log_2_resolution = self.resolution.bit_length() - 1

    def with_seed(self, _seed):  # sobol.rs:75-77: a no-op in the reference as well
        return self


class StratifiedSamplerBuilder:
    """StratifiedSamplerBuilder::new(log, dim_pixel_samples, n_sampled_dimensions) (sampler/stratified.rs:22-36): spp =
    dim_pixel_samples^2, jittered.  The reference compiles this sampler but never builds one (sampler/mod.rs:169-170); here
    it selects PtrsRenderParams.sampler = PTRS_SAMPLER_STRATIFIED.  with_seed is applied per tile by render (integrator.rs:553)."""

    def __init__(self, dim_pixel_samples, n_sampled_dimensions):
        self.dim_pixel_samples = int(dim_pixel_samples)
        self.n_sampled_dimensions = int(n_sampled_dimensions)
        self.samples_per_pixel = self.dim_pixel_samples * self.dim_pixel_samples

    def with_seed(self, _seed):
        return self


class _DeviceScene:
    def __init__(self, render_scene, device=0, bvh=None):
        self.handle = C.c_void_p()
        self.device = device
        desc = render_scene.desc(bvh)
        _check(load_library().ptrs_scene_create(C.byref(desc), int(device), C.byref(self.handle)))

    def info(self):
        n, d, t = C.c_uint64(), C.c_uint64(), C.c_uint64()
        _check(load_library().ptrs_scene_info(self.handle, C.byref(n), C.byref(d), C.byref(t)))
        return dict(bvh_nodes=n.value, bvh_max_depth=d.value, n_tris=t.value)

    def set_option(self, name, value):
        """ptrs_scene_set_option: this scene's renders take `value` for the knob instead of the process-wide setting."""
        _check(load_library().ptrs_scene_set_option(self.handle, name.encode(), C.c_int64(int(value))))

    def close(self):
        if self.handle:
            load_library().ptrs_scene_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _device_scene(render_scene, device=0, bvh=None):
    key = "_ptrs_dev_%d" % device
    ds = getattr(render_scene, key, None)
    if ds is None or bvh is not None:
        ds = _DeviceScene(render_scene, device, bvh)
        setattr(render_scene, key, ds)
    return ds


class PathIntegrator:
    """PathIntegrator (integrator.rs:219-246): rr_threshold 1.0, rr_start_depth 3, rr_enable true."""

    def __init__(self, sampler_builder, max_depth, show_progress_bar=False, device=0, paths_per_pass=0):
        self.sampler_builder = sampler_builder
        self.max_depth = int(max_depth)
        self.rr_threshold, self.rr_start_depth, self.rr_enable = 1.0, 3, True
        self.show_progress_bar = show_progress_bar
        self.device = device
        self.paths_per_pass = paths_per_pass
        self.last_stats = None

    def preprocess(self, scene):  # integrator.rs:250-258
        if len(scene.lights) > 16:
            warnings.warn("scene contains too many lights for path integrator to handle well")

    def toggle_progress_bar(self):  # integrator.rs:260-262
        self.show_progress_bar = not self.show_progress_bar

    def params(self, camera, row_begin=0, row_end=0, flags=0):
        p = abi.PtrsRenderParams()
        p.width, p.height = camera.film.width, camera.film.height
        p.spp, p.max_depth = self.sampler_builder.samples_per_pixel, self.max_depth
        p.rr_threshold, p.rr_start_depth, p.rr_enable = self.rr_threshold, self.rr_start_depth, int(self.rr_enable)
        p.row_begin, p.row_end = row_begin, (row_end if row_end else camera.film.height)
        p.device, p.paths_per_pass, p.flags = self.device, self.paths_per_pass, flags
        if getattr(camera, "lens_radius", 0.0) > 0.0:  # camera.to_abi() is then a PtrsCameraLens
            p.flags |= abi.FLAG_THIN_LENS
        if isinstance(self.sampler_builder, StratifiedSamplerBuilder):
            p.sampler, p.n_sampled_dimensions = abi.SAMPLER_STRATIFIED, self.sampler_builder.n_sampled_dimensions
        return p

    def render(self, camera, scene, row_begin=0, row_end=0, flags=0, want_samples=False):
        """integrator.rs:536-642 on the GPU; accumulates into camera.film.pixels (host memory)."""
        ds = _device_scene(scene, self.device)
        p = self.params(camera, row_begin, row_end, flags)
        cam = camera.to_abi()
        stats = abi.PtrsStats()
        film = camera.film.pixels
        samples = None
        if want_samples:
            samples = np.zeros((p.height + 4, p.width + 4, p.spp if p.sampler == abi.SAMPLER_STRATIFIED else round_up_pow2(p.spp), 3), dtype=np.float32)
        _check(load_library().ptrs_render_samples(ds.handle, C.byref(cam), C.byref(p), C.c_void_p(film.ctypes.data),
                                                  C.c_void_p(samples.ctypes.data) if want_samples else None, C.byref(stats)))
        self.last_stats = stats
        return samples if want_samples else None

    def render_device(self, camera, scene, film_device_ptr, stream=0, row_begin=0, row_end=0, flags=0):
        """Same, film accumulators in device memory (film_device_ptr: width*height*16 bytes)."""
        ds = _device_scene(scene, self.device)
        p = self.params(camera, row_begin, row_end, flags)
        cam = camera.to_abi()
        stats = abi.PtrsStats()
        _check(load_library().ptrs_render_device(ds.handle, C.byref(cam), C.byref(p), C.c_void_p(int(film_device_ptr)), C.c_void_p(int(stream)), C.byref(stats)))
        self.last_stats = stats
        return stats

    def render_aov(self, camera, scene, planes=("albedo", "normal", "depth"), row_begin=0, row_end=0, want_samples=False, into=None):
        """ptrs_render_aov: the first-hit feature planes of this integrator's view, filtered onto the film by the samples and weights
        of render() (max_depth plays no part).  Returns a dict name -> (H, W) FILM_DTYPE array of accumulated sums (resolve_aov turns
        them into displayable values); planes given in `into` are accumulated into, the others start from zero.  With want_samples
        returns (planes, samples), samples of shape (H + 4, W + 4, spp, 12): albedo, coverage, normal, depth, position, triangle id bits."""
        ds = _device_scene(scene, self.device)
        p = self.params(camera, row_begin, row_end)
        cam = camera.to_abi()
        stats = abi.PtrsStats()
        mask, out = _aov_mask(planes), {}
        ptrs = (C.c_void_p * abi.PtrsAovPlanes)()
        for k, name in enumerate(abi.PtrsAovNames):
            if mask & (1 << k):
                a = into.get(name) if into else None
                if a is None:
                    a = np.zeros((p.height, p.width), dtype=abi.FILM_DTYPE)
                if a.dtype != abi.FILM_DTYPE or a.shape != (p.height, p.width) or not a.flags.c_contiguous:
                    raise PtrsError("render_aov: plane %s must be a contiguous (H, W) FILM_DTYPE array" % name)
                out[name] = a
                ptrs[k] = a.ctypes.data
        samples = None
        if want_samples:
            samples = np.zeros((p.height + 4, p.width + 4, p.spp if p.sampler == abi.SAMPLER_STRATIFIED else round_up_pow2(p.spp), abi.PtrsAovSampleFloats), dtype=np.float32)
        _check(load_library().ptrs_render_aov(ds.handle, C.byref(cam), C.byref(p), C.c_uint32(mask), ptrs,
                                              C.c_void_p(samples.ctypes.data) if want_samples else None, C.byref(stats)))
        self.last_stats = stats
        return (out, samples) if want_samples else out

    def render_aov_device(self, camera, scene, plane_device_ptrs, planes=("albedo", "normal", "depth"), stream=0, row_begin=0, row_end=0, flags=0, samples_device_ptr=0):
        """Same, the planes' accumulators in device memory: plane_device_ptrs maps a plane's name to the address of width*height*16 bytes."""
        ds = _device_scene(scene, self.device)
        p = self.params(camera, row_begin, row_end, flags)
        cam = camera.to_abi()
        stats = abi.PtrsStats()
        mask = _aov_mask(planes)
        ptrs = (C.c_void_p * abi.PtrsAovPlanes)()
        for k, name in enumerate(abi.PtrsAovNames):
            if mask & (1 << k) and plane_device_ptrs.get(name):
                ptrs[k] = int(plane_device_ptrs[name])
        _check(load_library().ptrs_render_aov_device(ds.handle, C.byref(cam), C.byref(p), C.c_uint32(mask), ptrs,
                                                     C.c_void_p(int(samples_device_ptr)) if samples_device_ptr else None, C.c_void_p(int(stream)), C.byref(stats)))
        self.last_stats = stats
        return stats

    def render_range(self, camera, scene, sample_begin, sample_end, half=None, row_begin=0, row_end=0, flags=0, samples=None):
        """ptrs_render_range: samples [sample_begin, sample_end) of this integrator's render (the sampler's spp stays the whole render's
        count) accumulated into camera.film.pixels and, when given, into `half` (an (H, W) FILM_DTYPE array).  samples: None, or the
        (H + 4, W + 4, spp, 3) float32 array of render(want_samples=True), of which only the range's entries are written.  With a pass
        plan that keeps the band's rows in one pass, successive ranges that tile [0, spp) give render()'s film bit for bit."""
        ds = _device_scene(scene, self.device)
        p = self.params(camera, row_begin, row_end, flags)
        cam = camera.to_abi()
        stats = abi.PtrsStats()
        film = camera.film.pixels
        if half is not None and (half.dtype != abi.FILM_DTYPE or half.shape != film.shape or not half.flags.c_contiguous):
            raise PtrsError("render_range: half must be a contiguous (H, W) FILM_DTYPE array")
        if samples is not None:
            spp = p.spp if p.sampler == abi.SAMPLER_STRATIFIED else round_up_pow2(p.spp)
            if samples.dtype != np.float32 or samples.shape != (p.height + 4, p.width + 4, spp, 3) or not samples.flags.c_contiguous:
                raise PtrsError("render_range: samples must be a contiguous (H + 4, W + 4, spp, 3) float32 array")
        _check(load_library().ptrs_render_range(ds.handle, C.addressof(cam), C.addressof(p), int(sample_begin), int(sample_end), film.ctypes.data,
                                                half.ctypes.data if half is not None else None, samples.ctypes.data if samples is not None else None, C.addressof(stats)))
        self.last_stats = stats
        return stats

    def render_range_device(self, camera, scene, sample_begin, sample_end, film_device_ptr, half_device_ptr=0, stream=0, row_begin=0, row_end=0, flags=0):
        """Same, the film (and the half film, 0: none) in device memory (width*height*16 bytes each)."""
        ds = _device_scene(scene, self.device)
        p = self.params(camera, row_begin, row_end, flags)
        cam = camera.to_abi()
        stats = abi.PtrsStats()
        _check(load_library().ptrs_render_range_device(ds.handle, C.addressof(cam), C.addressof(p), int(sample_begin), int(sample_end), int(film_device_ptr),
                                                       int(half_device_ptr) or None, int(stream) or None, C.addressof(stats)))
        self.last_stats = stats
        return stats

    def render_converged(self, camera, scene, target_error, min_spp=8, want_half=False):
        """ptrs_render_converged: renders blocks of samples (converge_schedule: min_spp, then doubling up to the sampler's spp, the
        ceiling) into camera.film.pixels until film_error's max_tile_error is below target_error.  The films stay on the device between
        the blocks.  Returns a dict: spp_done, converged, history = [(spp, max_tile_error) per check], worst_tile, and with want_half
        the half film the last check was made against.  The film is render_range(0, spp_done)'s; at the ceiling it is render()'s."""
        ds = _device_scene(scene, self.device)
        p = self.params(camera)
        cam = camera.to_abi()
        stats = abi.PtrsStats()
        res = abi.PtrsConvergeResult()
        film = camera.film.pixels
        half = np.zeros_like(film) if want_half else None
        _check(load_library().ptrs_render_converged(ds.handle, C.addressof(cam), C.addressof(p), float(target_error), int(min_spp), film.ctypes.data,
                                                    half.ctypes.data if want_half else None, C.addressof(res), C.addressof(stats)))
        self.last_stats = stats
        out = dict(spp_done=int(res.spp_done), converged=bool(res.converged), worst_tile=int(res.worst_tile),
                   history=[(int(res.history[k].spp), float(res.history[k].max_tile_error)) for k in range(res.n_checks)])
        if want_half:
            out["half"] = half
        return out

    def _tile_flags(self, p, tiles, what):
        T = abi.PtrsErrorTile
        shape = ((p.height + T - 1) // T, (p.width + T - 1) // T)
        flags = np.ascontiguousarray(np.asarray(tiles) != 0, dtype=np.uint8)
        if flags.size != shape[0] * shape[1]:
            raise PtrsError("%s: tiles must have tiles_y x tiles_x = %d x %d entries" % (what, shape[0], shape[1]))
        return flags

    def render_tiles(self, camera, scene, sample_begin, sample_end, tiles, half=None, samples=None, flags=0):
        """ptrs_render_tiles: render_range restricted to the active tiles -- `tiles` is a (tiles_y, tiles_x) array over the 16 x 16
        tiles of film_error, non-zero = active.  Only the sample pixels within the filter radius of an active tile are traced; the
        pixels of the active tiles end with render_range's bits, all others keep theirs; of `samples` only the entries of the
        active sample pixels are written.  Returns the stats (samples = active sample pixels x the range)."""
        p = self.params(camera, 0, 0, flags)
        tf = self._tile_flags(p, tiles, "render_tiles")
        ds = _device_scene(scene, self.device)
        cam = camera.to_abi()
        stats = abi.PtrsStats()
        film = camera.film.pixels
        if half is not None and (half.dtype != abi.FILM_DTYPE or half.shape != film.shape or not half.flags.c_contiguous):
            raise PtrsError("render_tiles: half must be a contiguous (H, W) FILM_DTYPE array")
        if samples is not None:
            spp = p.spp if p.sampler == abi.SAMPLER_STRATIFIED else round_up_pow2(p.spp)
            if samples.dtype != np.float32 or samples.shape != (p.height + 4, p.width + 4, spp, 3) or not samples.flags.c_contiguous:
                raise PtrsError("render_tiles: samples must be a contiguous (H + 4, W + 4, spp, 3) float32 array")
        _check(load_library().ptrs_render_tiles(ds.handle, C.addressof(cam), C.addressof(p), int(sample_begin), int(sample_end), tf.ctypes.data, film.ctypes.data,
                                                half.ctypes.data if half is not None else None, samples.ctypes.data if samples is not None else None, C.addressof(stats)))
        self.last_stats = stats
        return stats

    def render_tiles_device(self, camera, scene, sample_begin, sample_end, tiles, film_device_ptr, half_device_ptr=0, stream=0, flags=0):
        """Same, the film (and the half film, 0: none) in device memory (width*height*16 bytes each); `tiles` stays a host array."""
        p = self.params(camera, 0, 0, flags)
        tf = self._tile_flags(p, tiles, "render_tiles_device")
        ds = _device_scene(scene, self.device)
        cam = camera.to_abi()
        stats = abi.PtrsStats()
        _check(load_library().ptrs_render_tiles_device(ds.handle, C.addressof(cam), C.addressof(p), int(sample_begin), int(sample_end), tf.ctypes.data, int(film_device_ptr),
                                                       int(half_device_ptr) or None, int(stream) or None, C.addressof(stats)))
        self.last_stats = stats
        return stats

    def render_adaptive(self, camera, scene, target_error, min_spp=8, want_half=False):
        """ptrs_render_adaptive: render_converged's schedule, every block on the tiles whose error has not been below target_error yet
        (a tile below it is frozen: never rendered again).  Stops when no tile is active or at the sampler's spp.  Returns a dict:
        spp_done, converged, worst_tile, tile_spp (a (tiles_y, tiles_x) array: the samples each tile's pixels hold), history =
        [(spp, tiles_active, max_tile_error) per check], and with want_half the half film.  Tile t of the film is tile t of
        render_range(0, tile_spp[t])."""
        ds = _device_scene(scene, self.device)
        p = self.params(camera)
        cam = camera.to_abi()
        stats = abi.PtrsStats()
        res = abi.PtrsAdaptiveResult()
        film = camera.film.pixels
        half = np.zeros_like(film) if want_half else None
        T = abi.PtrsErrorTile
        tile_spp = np.zeros(((p.height + T - 1) // T, (p.width + T - 1) // T), dtype=np.uint32)
        _check(load_library().ptrs_render_adaptive(ds.handle, C.addressof(cam), C.addressof(p), float(target_error), int(min_spp), film.ctypes.data,
                                                   half.ctypes.data if want_half else None, tile_spp.ctypes.data, C.addressof(res), C.addressof(stats)))
        self.last_stats = stats
        out = dict(spp_done=int(res.spp_done), converged=bool(res.converged), worst_tile=int(res.worst_tile), tile_spp=tile_spp,
                   history=[(int(res.history[k].spp), int(res.history[k].tiles_active), float(res.history[k].max_tile_error)) for k in range(res.n_checks)])
        if want_half:
            out["half"] = half
        return out

    def _aov_host_planes(self, p, planes, into, what):
        """The planes asked for as host arrays (those given in `into`, else zeros) and the pointer array of the ptrs_render_aov_* calls."""
        mask, out = _aov_mask(planes), {}
        ptrs = (C.c_void_p * abi.PtrsAovPlanes)()
        for k, name in enumerate(abi.PtrsAovNames):
            if mask & (1 << k):
                a = into.get(name) if into else None
                if a is None:
                    a = np.zeros((p.height, p.width), dtype=abi.FILM_DTYPE)
                if a.dtype != abi.FILM_DTYPE or a.shape != (p.height, p.width) or not a.flags.c_contiguous:
                    raise PtrsError("%s: plane %s must be a contiguous (H, W) FILM_DTYPE array" % (what, name))
                out[name] = a
                ptrs[k] = a.ctypes.data
        return mask, out, ptrs

    @staticmethod
    def _aov_device_planes(planes, plane_device_ptrs):
        mask = _aov_mask(planes)
        ptrs = (C.c_void_p * abi.PtrsAovPlanes)()
        for k, name in enumerate(abi.PtrsAovNames):
            if mask & (1 << k) and plane_device_ptrs.get(name):
                ptrs[k] = int(plane_device_ptrs[name])
        return mask, ptrs

    def _aov_samples_arg(self, p, samples, what):
        if samples is None:
            return None
        spp = p.spp if p.sampler == abi.SAMPLER_STRATIFIED else round_up_pow2(p.spp)
        if samples.dtype != np.float32 or samples.shape != (p.height + 4, p.width + 4, spp, abi.PtrsAovSampleFloats) or not samples.flags.c_contiguous:
            raise PtrsError("%s: samples must be a contiguous (H + 4, W + 4, spp, 12) float32 array" % what)
        return samples.ctypes.data

    def render_aov_range(self, camera, scene, sample_begin, sample_end, planes=("albedo", "normal", "depth"), row_begin=0, row_end=0, samples=None, into=None):
        """ptrs_render_aov_range: samples [sample_begin, sample_end) of render_aov's call (the sampler's spp stays the whole render's
        count), accumulated into the planes of `into` (absent ones start from zero).  samples: None, or the (H + 4, W + 4, spp, 12)
        array of render_aov(want_samples=True), of which only the range's entries are written.  Ranges that tile [0, spp) in order give
        render_aov's planes and samples bit for bit under every pass plan.  Returns the dict of planes."""
        ds = _device_scene(scene, self.device)
        p = self.params(camera, row_begin, row_end)
        cam = camera.to_abi()
        stats = abi.PtrsStats()
        mask, out, ptrs = self._aov_host_planes(p, planes, into, "render_aov_range")
        _check(load_library().ptrs_render_aov_range(ds.handle, C.addressof(cam), C.addressof(p), int(sample_begin), int(sample_end), mask, ptrs,
                                                    self._aov_samples_arg(p, samples, "render_aov_range"), C.addressof(stats)))
        self.last_stats = stats
        return out

    def render_aov_range_device(self, camera, scene, sample_begin, sample_end, plane_device_ptrs, planes=("albedo", "normal", "depth"), stream=0, row_begin=0, row_end=0,
                                samples_device_ptr=0):
        """Same, the planes (and the sample export, 0: none) in device memory."""
        ds = _device_scene(scene, self.device)
        p = self.params(camera, row_begin, row_end)
        cam = camera.to_abi()
        stats = abi.PtrsStats()
        mask, ptrs = self._aov_device_planes(planes, plane_device_ptrs)
        _check(load_library().ptrs_render_aov_range_device(ds.handle, C.addressof(cam), C.addressof(p), int(sample_begin), int(sample_end), mask, ptrs,
                                                           int(samples_device_ptr) or None, int(stream) or None, C.addressof(stats)))
        self.last_stats = stats
        return stats

    def render_aov_tiles(self, camera, scene, sample_begin, sample_end, tiles, planes=("albedo", "normal", "depth"), samples=None, into=None):
        """ptrs_render_aov_tiles: render_aov_range restricted to the active tiles (`tiles` as in render_tiles, the same dilation rule).
        The pixels of the active tiles end with render_aov_range's bits in every plane asked for, all others keep theirs; of `samples`
        only the range's entries of the active sample pixels are written.  Returns the dict of planes."""
        p = self.params(camera, 0, 0)
        tf = self._tile_flags(p, tiles, "render_aov_tiles")
        ds = _device_scene(scene, self.device)
        cam = camera.to_abi()
        stats = abi.PtrsStats()
        mask, out, ptrs = self._aov_host_planes(p, planes, into, "render_aov_tiles")
        _check(load_library().ptrs_render_aov_tiles(ds.handle, C.addressof(cam), C.addressof(p), int(sample_begin), int(sample_end), tf.ctypes.data, mask, ptrs,
                                                    self._aov_samples_arg(p, samples, "render_aov_tiles"), C.addressof(stats)))
        self.last_stats = stats
        return out

    def render_aov_tiles_device(self, camera, scene, sample_begin, sample_end, tiles, plane_device_ptrs, planes=("albedo", "normal", "depth"), stream=0, samples_device_ptr=0):
        """Same, the planes (and the sample export, 0: none) in device memory; `tiles` stays a host array."""
        p = self.params(camera, 0, 0)
        tf = self._tile_flags(p, tiles, "render_aov_tiles_device")
        ds = _device_scene(scene, self.device)
        cam = camera.to_abi()
        stats = abi.PtrsStats()
        mask, ptrs = self._aov_device_planes(planes, plane_device_ptrs)
        _check(load_library().ptrs_render_aov_tiles_device(ds.handle, C.addressof(cam), C.addressof(p), int(sample_begin), int(sample_end), tf.ctypes.data, mask, ptrs,
                                                           int(samples_device_ptr) or None, int(stream) or None, C.addressof(stats)))
        self.last_stats = stats
        return stats

    def _tile_spp_arg(self, p, tile_spp, what):
        T = abi.PtrsErrorTile
        shape = ((p.height + T - 1) // T, (p.width + T - 1) // T)
        ts = np.ascontiguousarray(tile_spp, dtype=np.uint32)
        if ts.size != shape[0] * shape[1]:
            raise PtrsError("%s: tile_spp must have tiles_y x tiles_x = %d x %d entries" % (what, shape[0], shape[1]))
        return ts

    def render_aov_adaptive(self, camera, scene, tile_spp, min_spp=8, planes=("albedo", "normal", "depth"), into=None):
        """ptrs_render_aov_adaptive: the planes of a film whose tile t holds tile_spp[t] samples of converge_schedule(spp, min_spp) --
        render_adaptive's tile_spp.  Tile t of every plane is tile t of render_aov_range(0, tile_spp[t]); a tile with 0 keeps its bits;
        from cleared planes the weights equal those of the render_adaptive film that produced tile_spp.  Returns the dict of planes."""
        p = self.params(camera, 0, 0)
        ts = self._tile_spp_arg(p, tile_spp, "render_aov_adaptive")
        ds = _device_scene(scene, self.device)
        cam = camera.to_abi()
        stats = abi.PtrsStats()
        mask, out, ptrs = self._aov_host_planes(p, planes, into, "render_aov_adaptive")
        _check(load_library().ptrs_render_aov_adaptive(ds.handle, C.addressof(cam), C.addressof(p), int(min_spp), ts.ctypes.data, mask, ptrs, C.addressof(stats)))
        self.last_stats = stats
        return out

    def render_aov_adaptive_device(self, camera, scene, tile_spp, plane_device_ptrs, min_spp=8, planes=("albedo", "normal", "depth"), stream=0):
        """Same, the planes in device memory; tile_spp stays a host array."""
        p = self.params(camera, 0, 0)
        ts = self._tile_spp_arg(p, tile_spp, "render_aov_adaptive_device")
        ds = _device_scene(scene, self.device)
        cam = camera.to_abi()
        stats = abi.PtrsStats()
        mask, ptrs = self._aov_device_planes(planes, plane_device_ptrs)
        _check(load_library().ptrs_render_aov_adaptive_device(ds.handle, C.addressof(cam), C.addressof(p), int(min_spp), ts.ctypes.data, mask, ptrs, int(stream) or None, C.addressof(stats)))
        self.last_stats = stats
        return stats

    def render_denoised(self, camera, scene, target_error=None, min_spp=8, adaptive=False, **params):
        """render, then render_aov, then Denoiser.denoise (params: iterations, sigma_color, sigma_normal, sigma_depth, demodulate).  The
        noisy film stays in camera.film; returns the denoised (H, W) FILM_DTYPE pixels (rgb = colour, weight = 1).  With target_error:
        render_converged (adaptive: render_adaptive) in place of render, and planes that hold exactly the film's samples --
        render_aov_range(0, spp_done), or render_aov_adaptive on the tile_spp the render returned; the render's result is kept in
        self.last_converge."""
        if target_error is not None:
            if adaptive:
                res = self.render_adaptive(camera, scene, target_error, min_spp)
                planes = self.render_aov_adaptive(camera, scene, res["tile_spp"], min_spp)
            else:
                res = self.render_converged(camera, scene, target_error, min_spp)
                planes = self.render_aov_range(camera, scene, 0, res["spp_done"])
            self.last_converge = res
            dn = Denoiser(camera.film.width, camera.film.height, self.device)
            try:
                return dn.denoise(camera.film.pixels, planes, **params)
            finally:
                dn.close()
        self.render(camera, scene)
        planes = self.render_aov(camera, scene)
        dn = Denoiser(camera.film.width, camera.film.height, self.device)
        try:
            return dn.denoise(camera.film.pixels, planes, **params)
        finally:
            dn.close()

    def render_progressive(self, camera, scene, on_pass, row_begin=0, row_end=0):
        """ptrs_render_progressive: like render(), and after every pass of the pipeline the rows it touched are copied into
        camera.film.pixels and on_pass(passes_done, passes_total, row_begin, row_end) is called (the preview hook the
        reference's headless front-end gets by polling its film, headless.rs:197-214)."""
        ds = _device_scene(scene, self.device)
        p = self.params(camera, row_begin, row_end)
        cam = camera.to_abi()
        stats = abi.PtrsStats()
        cb_t = C.CFUNCTYPE(None, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int32, C.c_int32)
        cb = cb_t(lambda _u, done, total, y0, y1: on_pass(done, total, y0, y1))
        _check(load_library().ptrs_render_progressive(ds.handle, C.byref(cam), C.byref(p), C.c_void_p(camera.film.pixels.ctypes.data), cb, None, C.byref(stats)))
        self.last_stats = stats
        return stats

    def set_scene_option(self, scene, name, value):
        """A tuning knob for this scene on this integrator's device only (ptrs_scene_set_option)."""
        _device_scene(scene, self.device).set_option(name, value)

    def render_multi(self, camera, scene, devices, bounds=None, row_cost=None, film_is_zero=False, scene_options=None):
        """ptrs_render_multi: the frame's rows split over `devices` (one PtrsScene per entry, one host thread each, bands
        gathered on the first device); bounds = n+1 row numbers, or planned by ptrs_plan_bands (weighted by row_cost when
        given).  Accumulates into camera.film.pixels; returns (bounds, [PtrsStats per device])."""
        L = load_library()
        n = len(devices)
        scenes = [_DeviceScene(scene, d) for d in devices]  # fresh replicas, also when several share a device
        try:
            for k, v in (scene_options or {}).items():
                for sc_ in scenes:
                    sc_.set_option(k, v)
            p = self.params(camera, flags=abi.FLAG_FILM_ZERO if film_is_zero else 0)
            cam = camera.to_abi()
            b = (C.c_int32 * (n + 1))()
            if bounds is None:
                rc = None if row_cost is None else np.ascontiguousarray(row_cost, dtype=np.float32)
                _check(L.ptrs_plan_bands(p.height, n, C.c_void_p(rc.ctypes.data) if rc is not None else None, b))
            else:
                b[:] = [int(v) for v in bounds]
            handles = (C.c_void_p * n)(*[s.handle for s in scenes])
            stats = (abi.PtrsStats * n)()
            _check(L.ptrs_render_multi(handles, n, C.byref(cam), C.byref(p), b, C.c_void_p(camera.film.pixels.ctypes.data), stats))
            return list(b), list(stats)
        finally:
            for s in scenes:
                s.close()

    def render_single_pixel(self, camera, pixel, scene):  # integrator.rs:505-534
        ds = _device_scene(scene, self.device)
        p = self.params(camera)
        cam = camera.to_abi()
        out = np.zeros((round_up_pow2(p.spp), 3), dtype=np.float32)
        self.last_single_pixel_paths = round_up_pow2(p.spp)
        _check(load_library().ptrs_render_single_pixel(ds.handle, C.byref(cam), C.byref(p), int(pixel[0]), int(pixel[1]), C.c_void_p(out.ctypes.data)))
        return out


def denoise_params(iterations=None, sigma_color=None, sigma_normal=None, sigma_depth=None, demodulate=None, timing=False):
    """PtrsDenoiseParams: ptrs_denoise_default_params (5 iterations, sigmas 0.25 / 0.3 / 0.1, demodulation on) with the given fields replaced."""
    p = abi.PtrsDenoiseParams()
    load_library().ptrs_denoise_default_params(C.byref(p))
    if iterations is not None:
        p.iterations = int(iterations)
    if sigma_color is not None:
        p.sigma_color = float(sigma_color)
    if sigma_normal is not None:
        p.sigma_normal = float(sigma_normal)
    if sigma_depth is not None:
        p.sigma_depth = float(sigma_depth)
    if demodulate is not None:
        p.flags = (p.flags & ~abi.PtrsDenoiseDemodulate) | (abi.PtrsDenoiseDemodulate if demodulate else 0)
    if timing:  # the call's PtrsStats.debug then holds nanoseconds per launch: [0] prepare, [1 + i] iteration i, [9] finish
        p.flags |= abi.PtrsDenoiseTiming
    return p


class Denoiser:
    """PtrsDenoiser: the a-trous denoiser's workspace of one device for one width x height.  One call at a time."""

    def __init__(self, width, height, device=0):
        self.width, self.height, self.device = int(width), int(height), int(device)
        self.handle = C.c_void_p()
        self.last_stats = None
        _check(load_library().ptrs_denoiser_create(self.device, self.width, self.height, C.byref(self.handle)))

    def denoise(self, film_pixels, planes, **params):
        """ptrs_denoise: film_pixels (the beauty film) and planes["albedo" | "normal" | "depth"] (render_aov's dict), all (H, W)
        FILM_DTYPE accumulated sums in host memory -> the denoised (H, W) FILM_DTYPE array (rgb = colour, weight = 1; zeros where the
        beauty film has no weight).  The inputs are not written."""
        films = [film_pixels] + [planes[k] for k in abi.PtrsAovNames]
        for f in films:
            if f.dtype != abi.FILM_DTYPE or f.shape != (self.height, self.width) or not f.flags.c_contiguous:
                raise PtrsError("denoise: every film must be a contiguous (%d, %d) FILM_DTYPE array" % (self.height, self.width))
        out = np.zeros((self.height, self.width), dtype=abi.FILM_DTYPE)
        p = denoise_params(**params)
        ptrs = (C.c_void_p * abi.PtrsAovPlanes)(*[f.ctypes.data for f in films[1:]])
        stats = abi.PtrsStats()
        _check(load_library().ptrs_denoise(self.handle, C.byref(p), C.c_void_p(films[0].ctypes.data), ptrs, C.c_void_p(out.ctypes.data), C.byref(stats)))
        self.last_stats = stats
        return out

    def denoise_device(self, beauty_device_ptr, plane_device_ptrs, out_device_ptr, stream=0, **params):
        """ptrs_denoise_device: the films in device memory (width*height*16 bytes each; plane_device_ptrs maps a plane's name to its
        address), the work queued on `stream`; returns the call's PtrsStats after the stream has drained."""
        p = denoise_params(**params)
        ptrs = (C.c_void_p * abi.PtrsAovPlanes)(*[int(plane_device_ptrs[k]) for k in abi.PtrsAovNames])
        stats = abi.PtrsStats()
        _check(load_library().ptrs_denoise_device(self.handle, C.byref(p), C.c_void_p(int(beauty_device_ptr)), ptrs, C.c_void_p(int(out_device_ptr)), C.c_void_p(int(stream)), C.byref(stats)))
        self.last_stats = stats
        return stats

    def close(self):
        if self.handle:
            load_library().ptrs_denoiser_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def film_error(film, half, device=0, want_tiles=True):
    """ptrs_film_error: two (H, W) FILM_DTYPE films in host memory, `half` holding half of `film`'s samples -> (tiles, summary): the
    (tiles_y, tiles_x) TILE_DTYPE records of the 16 x 16 tiles (None without want_tiles) and the PtrsFilmErrorSummary."""
    if film.dtype != abi.FILM_DTYPE or half.dtype != abi.FILM_DTYPE or film.ndim != 2 or half.shape != film.shape or not film.flags.c_contiguous or not half.flags.c_contiguous:
        raise PtrsError("film_error: film and half must be contiguous (H, W) FILM_DTYPE arrays of one shape")
    H, W = film.shape
    tiles = np.zeros(((H + abi.PtrsErrorTile - 1) // abi.PtrsErrorTile, (W + abi.PtrsErrorTile - 1) // abi.PtrsErrorTile), dtype=abi.TILE_DTYPE) if want_tiles else None
    s = abi.PtrsFilmErrorSummary()
    _check(load_library().ptrs_film_error(int(device), W, H, film.ctypes.data, half.ctypes.data, tiles.ctypes.data if want_tiles else None, C.addressof(s)))
    return tiles, s


def film_error_device(width, height, film_device_ptr, half_device_ptr, tiles_device_ptr, device=0, stream=0):
    """ptrs_film_error_device: the films and the tile records (tiles_x * tiles_y * 8 bytes) in device memory -> the summary."""
    s = abi.PtrsFilmErrorSummary()
    _check(load_library().ptrs_film_error_device(int(device), int(width), int(height), int(film_device_ptr) or None, int(half_device_ptr) or None,
                                                 int(tiles_device_ptr) or None, int(stream) or None, C.addressof(s)))
    return s


def converge_schedule(spp, min_spp):
    """ptrs_converge_schedule (a pure function, no device): the blocks of render_converged as (begin, middle, end) -- [begin, middle)
    goes to the film and the half film, [middle, end) to the film only; an error check follows every block."""
    b = np.zeros((abi.PtrsConvergeMaxChecks, 3), dtype=np.uint32)
    n = C.c_uint32(0)
    _check(load_library().ptrs_converge_schedule(int(spp), int(min_spp), b.ctypes.data, C.addressof(n)))
    return [tuple(int(v) for v in r) for r in b[: n.value]]


def _aov_mask(planes):
    mask = 0
    for name in planes:
        if name not in abi.PtrsAovNames:
            raise PtrsError("unknown AOV plane %r (albedo, normal, depth)" % (name,))
        mask |= 1 << abi.PtrsAovNames.index(name)
    return mask


def resolve_aov(planes):
    """The accumulated planes of render_aov as displayable float64 arrays: albedo = rgb / weight; normal = rgb / weight, renormalised
    where non-zero; depth = r / g of the depth plane (mean depth over the covered weight, 0 where nothing is covered); alpha = g / weight
    of the depth plane.  Pixels without weight give 0."""
    def ratio(num, den):
        num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
        return np.divide(num, den, out=np.zeros_like(num), where=den != 0)
    out = {}
    if "albedo" in planes:
        a = planes["albedo"]
        out["albedo"] = ratio(a["rgb"], a["weight"][..., None] * np.ones(3))
    if "normal" in planes:
        a = planes["normal"]
        n = ratio(a["rgb"], a["weight"][..., None] * np.ones(3))
        l = np.sqrt((n * n).sum(axis=-1, keepdims=True))
        out["normal"] = ratio(n, l * np.ones(3))
    if "depth" in planes:
        a = planes["depth"]
        out["depth"] = ratio(a["rgb"][..., 0], a["rgb"][..., 1])
        out["alpha"] = ratio(a["rgb"][..., 1], a["weight"])
    return out


def trace_rays(scene, rays, any_hit=False, device=0, bvh=None):
    """RenderScene::intersect / intersect_p (pathtracer/mod.rs:92-98) for a batch of rays
    (n x 7: o, d, t_max) through the traversal kernel."""
    ds = _device_scene(scene, device, bvh)
    rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 7)
    hits = np.zeros(rays.shape[0], dtype=abi.HIT_DTYPE)
    stats = abi.PtrsStats()
    _check(load_library().ptrs_trace_rays(ds.handle, rays.shape[0], C.c_void_p(rays.ctypes.data), int(any_hit), C.c_void_p(hits.ctypes.data), C.byref(stats)))
    return hits, stats


def focus_distance(camera, scene, raster_xy, device=0):
    """ptrs_camera_focus_distance: the depth along the view axis of what the pinhole ray of raster point `raster_xy` hits -- the
    focal_distance that puts it in focus (Camera.with_lens); inf on a miss."""
    ds = _device_scene(scene, device)
    L = load_library()
    L.ptrs_camera_focus_distance.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_void_p]
    cam = camera.with_lens(0.0, 0.0).to_abi()
    out = C.c_float(0.0)
    _check(L.ptrs_camera_focus_distance(ds.handle, C.byref(cam), float(raster_xy[0]), float(raster_xy[1]), C.byref(out)))
    return float(out.value)


def dump_rays(integrator, camera, scene, round_no, max_rays):
    """ptrs_render_dump_rays: the extension rays of round `round_no` of the first pass of `integrator`'s render (n x 7: o, d, t_max)."""
    ds = _device_scene(scene, integrator.device)
    p = integrator.params(camera)
    cam = camera.to_abi()
    out = np.zeros((int(max_rays), 7), dtype=np.float32)
    n = C.c_uint32(0)
    _check(load_library().ptrs_render_dump_rays(ds.handle, C.byref(cam), C.byref(p), int(round_no), int(max_rays), C.c_void_p(out.ctypes.data), C.byref(n)))
    return out[: n.value].copy()


def trace_bench(scene, rays, repeats=5, device=0, want_hits=False):
    """ptrs_trace_bench: closest-hit traversal of `rays` with the frame's extension kernel, `repeats` timed launches.  Returns
    (stats, hits or None); stats.ms_trace is the sum of the timed launches, nodes_visited / tris_tested belong to one launch."""
    ds = _device_scene(scene, device)
    rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 7)
    hits = np.zeros(rays.shape[0], dtype=abi.HIT_DTYPE) if want_hits else None
    stats = abi.PtrsStats()
    _check(load_library().ptrs_trace_bench(ds.handle, rays.shape[0], C.c_void_p(rays.ctypes.data), int(repeats), C.c_void_p(hits.ctypes.data) if want_hits else None, C.byref(stats)))
    return stats, hits


def sobol_samples(params, px, py, sample_nums, dims):
    """SobolSampler::sample_dimension (sobol.rs:177-193) for arbitrary (pixel, sample, dimension)."""
    px = np.ascontiguousarray(px, dtype=np.int32)
    py = np.ascontiguousarray(py, dtype=np.int32)
    sn = np.ascontiguousarray(sample_nums, dtype=np.uint64)
    dm = np.ascontiguousarray(dims, dtype=np.uint32)
    out = np.zeros(px.shape[0], dtype=np.float32)
    idx = np.zeros(px.shape[0], dtype=np.uint64)
    _check(load_library().ptrs_sobol_samples(C.byref(params), px.shape[0], C.c_void_p(px.ctypes.data), C.c_void_p(py.ctypes.data), C.c_void_p(sn.ctypes.data),
                                             C.c_void_p(dm.ctypes.data), C.c_void_p(out.ctypes.data), C.c_void_p(idx.ctypes.data)))
    return out, idx


def selftest_div3(mode, n_sets, seed=1, device=0):
    """ptrs_selftest_div3: the device code's shared-divisor division against the compiler's IEEE division over ~n_sets generated operand
    sets.  Returns (mismatches, sets that took the fast path, first mismatch as 10 uint32 words: a0 a1 a2 b | got x3 | want x3)."""
    L = load_library()
    L.ptrs_selftest_div3.argtypes = [C.c_int32, C.c_uint32, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_void_p]
    bad, fast = C.c_uint64(0), C.c_uint64(0)
    first = np.zeros(10, dtype=np.uint32)
    _check(L.ptrs_selftest_div3(int(device), int(mode), int(n_sets), int(seed), C.byref(bad), C.byref(fast), C.c_void_p(first.ctypes.data)))
    return int(bad.value), int(fast.value), first


def probe_bsdf(scene, material, frame, rows, device=0):
    """ptrs_probe_bsdf: material `material` of `scene` at a hit with frame (ng, ns, dpdu), rows (n x 8: wo, wi, u) ->
    (n x 16): f(wo, wi).rgb, pdf(wo, wi), sample_f(wo, u) f.rgb, pdf, wi.xyz, flags, has-BSDF, 0 x 3 (csrc/pt_probe.h)."""
    ds = _device_scene(scene, device)
    L = load_library()
    L.ptrs_probe_bsdf.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    fr = np.ascontiguousarray(frame, dtype=np.float32).reshape(9)
    rows = np.ascontiguousarray(rows, dtype=np.float32).reshape(-1, 8)
    out = np.zeros((rows.shape[0], 16), dtype=np.float32)
    _check(L.ptrs_probe_bsdf(ds.handle, int(material), C.c_void_p(fr.ctypes.data), rows.shape[0], C.c_void_p(rows.ctypes.data), C.c_void_p(out.ctypes.data)))
    return out


def probe_light(scene, light, ref, rows, device=0):
    """ptrs_probe_light: light `light` of `scene` (area or environment) from ref (p, n), rows (n x 5: u, w) -> (n x 16):
    sample_li(u) wi.xyz, pdf, Li.rgb, ok; pdf_li(w); le(w).rgb; 0 x 4 (csrc/pt_probe.h)."""
    ds = _device_scene(scene, device)
    L = load_library()
    L.ptrs_probe_light.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    rf = np.ascontiguousarray(ref, dtype=np.float32).reshape(6)
    rows = np.ascontiguousarray(rows, dtype=np.float32).reshape(-1, 5)
    out = np.zeros((rows.shape[0], 16), dtype=np.float32)
    _check(L.ptrs_probe_light(ds.handle, int(light), C.c_void_p(rf.ctypes.data), rows.shape[0], C.c_void_p(rows.ctypes.data), C.c_void_p(out.ctypes.data)))
    return out


def probe_texture(scene, tex, rows, device=0):
    """ptrs_probe_texture: texture `tex` of `scene`, rows (n x 6: uv, dudx, dvdx, dudy, dvdy) -> (n x 8): rgb, then (image textures)
    the MIP level computed from the width, 1 for the zero-footprint shortcut, mapped st, 0 (csrc/pt_probe.h)."""
    ds = _device_scene(scene, device)
    L = load_library()
    L.ptrs_probe_texture.argtypes = [C.c_void_p, C.c_int32, C.c_uint32, C.c_void_p, C.c_void_p]
    rows = np.ascontiguousarray(rows, dtype=np.float32).reshape(-1, 6)
    out = np.zeros((rows.shape[0], 8), dtype=np.float32)
    _check(L.ptrs_probe_texture(ds.handle, int(tex), rows.shape[0], C.c_void_p(rows.ctypes.data), C.c_void_p(out.ctypes.data)))
    return out


def probe_surface(scene, prim, rows, device=0):
    """ptrs_probe_surface: triangle `prim` of `scene`, rows (n x 16: o, d, t_max, rx_d, ry_d, w) -> (n x 64): both leaf forms' hit, t,
    b0-b2, then the hit surface, spawn points and normal-mapping steps in the layout of csrc/pt_probe.h surface_probe_row."""
    ds = _device_scene(scene, device)
    L = load_library()
    L.ptrs_probe_surface.argtypes = [C.c_void_p, C.c_int32, C.c_uint32, C.c_void_p, C.c_void_p]
    rows = np.ascontiguousarray(rows, dtype=np.float32).reshape(-1, 16)
    out = np.zeros((rows.shape[0], 64), dtype=np.float32)
    _check(L.ptrs_probe_surface(ds.handle, int(prim), rows.shape[0], C.c_void_p(rows.ctypes.data), C.c_void_p(out.ctypes.data)))
    return out


def probe_math(op, rows, device=0):
    """ptrs_probe_math: op `op` (abi.MATH_*) of the arithmetic substrate on every row (n x 16 floats) -> (n x 16) raw results in the
    layout of csrc/pt_probe.h math_probe_row; integers travel as bit patterns."""
    L = load_library()
    L.ptrs_probe_math.argtypes = abi.PROBE_MATH_ARGTYPES
    rows = np.ascontiguousarray(rows, dtype=np.float32).reshape(-1, abi.PROBE_MATH_WIDTH)
    out = np.zeros((rows.shape[0], abi.PROBE_MATH_WIDTH), dtype=np.float32)
    _check(L.ptrs_probe_math(int(device), int(op), rows.shape[0], C.c_void_p(rows.ctypes.data), C.c_void_p(out.ctypes.data)))
    return out


def probe_shade_tables(scene, params, it, op, rows, device=0):
    """ptrs_probe_shade_tables: the shade kernels' LDS tables staged as round `it` of a render of `scene` with `params`
    (a PtrsRenderParams, e.g. PathIntegrator.params(camera)) stages them, then `rows` (n x 12 uint32; floats travel as bit patterns)
    through that context.  op abi.PROBE_SHADE_SOBOL: row = index lo, index hi, scramble, N, N dimensions -> the N values' bits, column
    8 the route (abi.SOB_ROUTE_*).  op abi.PROBE_SHADE_ENV: row = u.x, u.y, light -> wi.xyz, pdf, Li.rgb, ok, staged-marginal flag.
    Returns (header dict with the fields abi.PROBE_SHADE_HEADER, out n x 12 uint32)."""
    ds = _device_scene(scene, device)
    L = load_library()
    L.ptrs_probe_shade_tables.argtypes = abi.PROBE_SHADE_ARGTYPES
    rows = np.ascontiguousarray(rows, dtype=np.uint32).reshape(-1, abi.PROBE_SHADE_WIDTH)
    out = np.zeros((rows.shape[0], abi.PROBE_SHADE_WIDTH), dtype=np.uint32)
    header = np.zeros(12, dtype=np.uint32)
    _check(L.ptrs_probe_shade_tables(ds.handle, C.byref(params), int(it), int(op), rows.shape[0], C.c_void_p(rows.ctypes.data), C.c_void_p(out.ctypes.data), C.c_void_p(header.ctypes.data)))
    return {k: int(header[i]) for i, k in enumerate(abi.PROBE_SHADE_HEADER)}, out


def build_id():
    """ptrs_build_id: hash of the kernel sources and compiler flags the loaded library was built from (build.source_hash)."""
    return load_library().ptrs_build_id().decode()
