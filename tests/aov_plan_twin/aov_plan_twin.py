"""AOV PLAN TWIN binding -- TEST INFRASTRUCTURE ONLY (see aov_plan_twin.cpp)."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(os.path.dirname(_HERE))
abi = importlib.import_module("pathtracer-rs_amd.abi")
_lib = None
ALL_PLANES = 7


def lib():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-s", "-C", _HERE])
        L = C.CDLL(os.path.join(_HERE, "libaovplantwin.so"))
        L.aov_plan_twin_last_error.restype = C.c_char_p
        L.aov_plan_twin_render.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.aov_plan_twin_render_adaptive.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        L.twin_scene_create.argtypes = [C.c_void_p, C.c_void_p]
        L.twin_scene_destroy.argtypes = [C.c_void_p]
        if L.twin_load_tables(os.path.join(_ROOT, "data", "sobol_tables.bin").encode()) != 0:
            raise RuntimeError("aov plan twin: cannot load sobol tables")
        _lib = L
    return _lib


def _check(rc):
    if rc != 0:
        raise RuntimeError("aov plan twin error %d: %s" % (rc, lib().aov_plan_twin_last_error().decode()))


def _plane_ptrs(planes, films):
    """films: (3, H, W) FILM_DTYPE, plane k = films[k]; the pointer array render_aov_impl's callers pass."""
    assert films.dtype == abi.FILM_DTYPE and films.shape[0] == 3 and films.flags.c_contiguous
    return (C.c_void_p * 3)(*[films[k].ctypes.data if planes & (1 << k) else None for k in range(3)])


class AovScene:
    """A host-twin scene for render_aov_impl on the CPU."""

    def __init__(self, render_scene):
        self._h = C.c_void_p()
        desc = render_scene.desc(None)
        rc = lib().twin_scene_create(C.addressof(desc), C.addressof(self._h))
        if rc != 0:
            raise RuntimeError("aov plan twin: scene error %d" % rc)

    def __del__(self):
        try:
            if self._h:
                lib().twin_scene_destroy(self._h)
        except Exception:
            pass

    def render(self, camera, params, films, sample_range=None, tiles=None, samples=None, planes=ALL_PLANES):
        """The twin of ptrs_render_aov (no range), ptrs_render_aov_range (no tiles) and ptrs_render_aov_tiles: accumulates into films
        (3, H, W); samples (NY, NX, spp, 12) float32 or None.  Returns the stats."""
        stats = abi.PtrsStats()
        cam = camera.to_abi()
        ptrs = _plane_ptrs(planes, films)
        if tiles is not None:
            tiles = np.ascontiguousarray(tiles, dtype=np.uint8)
            assert tiles.size == ((params.height + 15) // 16) * ((params.width + 15) // 16)
        b, e = sample_range if sample_range is not None else (0, 0)
        _check(lib().aov_plan_twin_render(self._h, C.addressof(cam), C.addressof(params), 0 if sample_range is None else 1, int(b), int(e),
                                          tiles.ctypes.data if tiles is not None else None, int(planes), C.addressof(ptrs),
                                          samples.ctypes.data if samples is not None else None, C.addressof(stats)))
        return stats

    def render_adaptive(self, camera, params, min_spp, tile_spp, films, planes=ALL_PLANES):
        """The twin of ptrs_render_aov_adaptive.  Returns the samples traced."""
        tile_spp = np.ascontiguousarray(tile_spp, dtype=np.uint32)
        assert tile_spp.size == ((params.height + 15) // 16) * ((params.width + 15) // 16)
        cam = camera.to_abi()
        ptrs = _plane_ptrs(planes, films)
        n = C.c_uint64()
        _check(lib().aov_plan_twin_render_adaptive(self._h, C.addressof(cam), C.addressof(params), int(min_spp), tile_spp.ctypes.data, int(planes), C.addressof(ptrs), C.addressof(n)))
        return int(n.value)
