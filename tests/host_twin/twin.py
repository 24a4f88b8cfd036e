"""HOST TWIN binding -- TEST INFRASTRUCTURE ONLY (see twin.cpp)."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(os.path.dirname(_HERE))
abi = importlib.import_module("pathtracer-rs_amd.abi")
_lib = None


def lib():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-s", "-C", _HERE])
        L = C.CDLL(os.path.join(_HERE, "libtwin.so"))
        L.twin_last_error.restype = C.c_char_p
        if L.twin_load_tables(os.path.join(_ROOT, "data", "sobol_tables.bin").encode()) != 0:
            raise RuntimeError("twin: cannot load sobol tables")
        _lib = L
    return _lib


def _check(rc):
    if rc != 0:
        raise RuntimeError("twin error %d: %s" % (rc, lib().twin_last_error().decode()))


def round_up_pow2(v):
    return 1 << max(0, (int(v) - 1).bit_length())


class TwinScene:
    def __init__(self, render_scene, bvh=None, node_form=0):
        """node_form: the library's option of that name (0 = by size, 2 = quad nodes whatever the size)."""
        self._h = C.c_void_p()
        desc = render_scene.desc(bvh)
        _check(lib().twin_scene_create_form(C.byref(desc), C.c_int32(int(node_form)), C.byref(self._h)))

    def __del__(self):
        try:
            if self._h:
                lib().twin_scene_destroy(self._h)
        except Exception:
            pass

    def info(self):
        """twin_scene_info: max_depth, stack_bound (what the device sizes its stack columns from), the node count of the traversal
        form, and which form that is."""
        d, b, n = C.c_uint32(), C.c_uint32(), C.c_uint32()
        q = lib().twin_scene_info(self._h, C.byref(d), C.byref(b), C.byref(n))
        return dict(max_depth=d.value, stack_bound=b.value, n_nodes=n.value, quad=bool(q))

    def render(self, camera, params, want_samples=False, film=None):
        W, H = params.width, params.height
        if film is None:
            film = np.zeros((H, W), dtype=abi.FILM_DTYPE)
        spp = params.spp if params.sampler == abi.SAMPLER_STRATIFIED else round_up_pow2(params.spp)
        samples = np.zeros((H + 4, W + 4, spp, 3), dtype=np.float32) if want_samples else None
        stats = abi.PtrsStats()
        cam = camera.to_abi()
        _check(lib().twin_render(self._h, C.byref(cam), C.byref(params), C.c_void_p(film.ctypes.data),
                                 C.c_void_p(samples.ctypes.data) if want_samples else None, C.byref(stats)))
        return film, samples, stats

    def trace_rays(self, rays, any_hit=False):
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 7)
        hits = np.zeros(rays.shape[0], dtype=abi.HIT_DTYPE)
        stats = abi.PtrsStats()
        _check(lib().twin_trace_rays(self._h, rays.shape[0], C.c_void_p(rays.ctypes.data), int(any_hit), C.c_void_p(hits.ctypes.data), C.byref(stats)))
        return hits, stats


def peak_stack():
    """twin_peak_stack: the most entries any ray of the last trace_rays call had on its traversal stack (a push past the scene's
    stack_bound makes that call fail instead)."""
    L = lib()
    L.twin_peak_stack.restype = C.c_uint32
    return int(L.twin_peak_stack())


def sobol_samples(params, px, py, sample_nums, dims):
    px = np.ascontiguousarray(px, dtype=np.int32)
    py = np.ascontiguousarray(py, dtype=np.int32)
    sn = np.ascontiguousarray(sample_nums, dtype=np.uint64)
    dm = np.ascontiguousarray(dims, dtype=np.uint32)
    out = np.zeros(px.shape[0], dtype=np.float32)
    idx = np.zeros(px.shape[0], dtype=np.uint64)
    _check(lib().twin_sobol_samples(C.byref(params), px.shape[0], C.c_void_p(px.ctypes.data), C.c_void_p(py.ctypes.data), C.c_void_p(sn.ctypes.data),
                                    C.c_void_p(dm.ctypes.data), C.c_void_p(out.ctypes.data), C.c_void_p(idx.ctypes.data)))
    return out, idx


def bsdf_probe(scene, material, frame, rows):
    """twin_bsdf_probe: ptrs_probe_bsdf's rows on the CPU (scene: a TwinScene)."""
    L = lib()
    L.twin_bsdf_probe.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    fr = np.ascontiguousarray(frame, dtype=np.float32).reshape(9)
    rows = np.ascontiguousarray(rows, dtype=np.float32).reshape(-1, 8)
    out = np.zeros((rows.shape[0], 16), dtype=np.float32)
    _check(L.twin_bsdf_probe(scene._h, int(material), C.c_void_p(fr.ctypes.data), rows.shape[0], C.c_void_p(rows.ctypes.data), C.c_void_p(out.ctypes.data)))
    return out


def light_probe(scene, light, ref, rows):
    """twin_light_probe: ptrs_probe_light's rows on the CPU (scene: a TwinScene)."""
    L = lib()
    L.twin_light_probe.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    rf = np.ascontiguousarray(ref, dtype=np.float32).reshape(6)
    rows = np.ascontiguousarray(rows, dtype=np.float32).reshape(-1, 5)
    out = np.zeros((rows.shape[0], 16), dtype=np.float32)
    _check(L.twin_light_probe(scene._h, int(light), C.c_void_p(rf.ctypes.data), rows.shape[0], C.c_void_p(rows.ctypes.data), C.c_void_p(out.ctypes.data)))
    return out


def texture_probe(scene, tex, rows):
    """twin_texture_probe: ptrs_probe_texture's rows on the CPU (scene: a TwinScene)."""
    L = lib()
    L.twin_texture_probe.argtypes = [C.c_void_p, C.c_int32, C.c_uint32, C.c_void_p, C.c_void_p]
    rows = np.ascontiguousarray(rows, dtype=np.float32).reshape(-1, 6)
    out = np.zeros((rows.shape[0], 8), dtype=np.float32)
    _check(L.twin_texture_probe(scene._h, int(tex), rows.shape[0], C.c_void_p(rows.ctypes.data), C.c_void_p(out.ctypes.data)))
    return out


def surface_probe(scene, prim, rows):
    """twin_surface_probe: ptrs_probe_surface's rows on the CPU (scene: a TwinScene)."""
    L = lib()
    L.twin_surface_probe.argtypes = [C.c_void_p, C.c_int32, C.c_uint32, C.c_void_p, C.c_void_p]
    rows = np.ascontiguousarray(rows, dtype=np.float32).reshape(-1, 16)
    out = np.zeros((rows.shape[0], 64), dtype=np.float32)
    _check(L.twin_surface_probe(scene._h, int(prim), rows.shape[0], C.c_void_p(rows.ctypes.data), C.c_void_p(out.ctypes.data)))
    return out


def math_probe(op, rows):
    """twin_math_probe: ptrs_probe_math's rows on the CPU (n x 16 in, n x 16 out; csrc/pt_probe.h math_probe_row)."""
    L = lib()
    L.twin_math_probe.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    rows = np.ascontiguousarray(rows, dtype=np.float32).reshape(-1, 16)
    out = np.zeros((rows.shape[0], 16), dtype=np.float32)
    _check(L.twin_math_probe(int(op), rows.shape[0], C.c_void_p(rows.ctypes.data), C.c_void_p(out.ctypes.data)))
    return out


def camera_rays(camera, diff_scale, pfilm):
    """twin_camera_rays: pt::camera_ray for every p_film row (n x 2) -> (n x 12): o, d, rx_d, ry_d."""
    L = lib()
    L.twin_camera_rays.argtypes = [C.c_void_p, C.c_float, C.c_uint32, C.c_void_p, C.c_void_p]
    cam = camera.to_abi()
    pf = np.ascontiguousarray(pfilm, dtype=np.float32).reshape(-1, 2)
    out = np.zeros((pf.shape[0], 12), dtype=np.float32)
    _check(L.twin_camera_rays(C.byref(cam), float(diff_scale), pf.shape[0], C.c_void_p(pf.ctypes.data), C.c_void_p(out.ctypes.data)))
    return out


def plan_passes(band_rows, nx, ns, capacity, n_lanes, paths_per_pass_given):
    """twin_plan_passes: pt::plan_passes -> (rows per pass, samples per pass, paths of the largest pass); RuntimeError: pass too large."""
    L = lib()
    L.twin_plan_passes.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_int32, C.c_void_p]
    out = np.zeros(3, dtype=np.uint64)
    _check(L.twin_plan_passes(int(band_rows), int(nx), int(ns), int(capacity), int(n_lanes), int(bool(paths_per_pass_given)), C.c_void_p(out.ctypes.data)))
    return tuple(int(v) for v in out)
